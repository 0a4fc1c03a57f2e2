// Softmax + sparse categorical cross-entropy at vocabulary width: the loss of a language
// model's [tokens, vocab] logits (ops.softmax_cross_entropy on [..., C], Keras
// SparseCategoricalCrossentropy on sequences).  bf16 or fp32 logits, fp32 math, any C >= 1,
// any N >= 1, rows with a pitch ldz >= C (a padded head's [:, :C] view is read in place).
//
// xent.hip gives a wave to each row and walks it three times with 2-byte loads: right for a
// 1000-way head, 512 sequential wave loads per pass at C = 32768.  Here a row belongs to a
// whole workgroup of G = 256 / 512 / 1024 lanes:
//
//  * resident form (xent_vocab_kernel): lane t holds the 16-byte vectors at columns
//    E*(t + G*i), i < NV, of its row in registers as loaded (E = 8 bf16 or 4 fp32, NV <= 8:
//    32 VGPRs at most), so the row is read from memory ONCE.  Max / arg-max, then sum-exp,
//    the sum of the logits and the label's logit, then the gradient, all from those registers.
//    Resident limits: 8 * 1024 * 8 = 65536 columns of bf16, 4 * 1024 * 8 = 32768 of fp32.
//  * streaming form (xent_vocab_stream_kernel) above those: one read with an online
//    (max, sum) per lane, a second read for the gradient; 64-bit column arithmetic, any C
//    that fits an int.
//
// Per row: loss (the formula of xent_kernel, label smoothing included), the correct flag
// (arg-max ties go to the SMALLEST index, within a lane by walking columns upwards with a
// strict compare, across lanes and waves by comparing indices), and
// dz = (softmax - target) * scale into a contiguous [N, C] tensor of the logits' dtype.  A
// label outside [0, C) makes the row ignored: loss 0, correct 0, a gradient row of exact
// zeros (the logits of such a row are not read at all).  `scale` comes by value, or from
// scale_dev[1] when the launcher is given a device buffer (the valid-token mean: see
// xent_count_kernel) -- no host sync.
//
// Memory access: 16 bytes per lane.  With an odd pitch or an odd C the rows of z and dz start
// on 2-byte (bf16) / 4-byte (fp32) boundaries; the vector types carry that alignment, as in
// layernorm.hip.  The last, partial vector of a row goes element by element under a bound
// check: nothing is read past column C of a row, nothing is written past N*C of dz.
//
// Cross-wave reductions meet in LDS and are combined in wave order by every lane; the
// count and finalise kernels are one block each with a fixed order.  No atomics: results are
// bitwise reproducible.
#include "ca_common.h"

namespace {

typedef us8 us8u __attribute__((aligned(2)));
typedef f4 f4u __attribute__((aligned(4)));

// One 16-byte vector of a row: E elements, kept as loaded.
template <typename T> struct Vec;
template <> struct Vec<bf16_t> {
  static constexpr int E = 8;
  typedef us8 reg;
  typedef us8u mem;
  static __device__ __forceinline__ float get(const reg& r, int j) { return bf2f(r[j]); }
  static __device__ __forceinline__ bf16_t cvt(float f) { return f2bf(f); }
  static __device__ __forceinline__ bf16_t ninf() { return (bf16_t)0xff80; }
};
template <> struct Vec<float> {
  static constexpr int E = 4;
  typedef f4 reg;
  typedef f4u mem;
  static __device__ __forceinline__ float get(const reg& r, int j) { return r[j]; }
  static __device__ __forceinline__ float cvt(float f) { return f; }
  static __device__ __forceinline__ float ninf() { return -INFINITY; }
};

// columns c .. c+E-1 of a row; columns >= C are not touched and read as -inf (they lose every
// max and add exp(-inf) = 0 to the sum; the plain sum of the logits checks the bound itself)
template <typename T>
__device__ __forceinline__ typename Vec<T>::reg ldv(const T* __restrict__ row, long c, long C) {
  typedef Vec<T> V;
  typename V::reg r;
  if (c + V::E <= C) {
    r = *reinterpret_cast<const typename V::mem*>(row + c);
  } else {
#pragma unroll
    for (int j = 0; j < V::E; ++j) r[j] = c + j < C ? row[c + j] : V::ninf();
  }
  return r;
}

template <typename T>
__device__ __forceinline__ void stv(T* __restrict__ row, long c, long C, const float* o) {
  typedef Vec<T> V;
  if (c + V::E <= C) {
    typename V::reg r;
#pragma unroll
    for (int j = 0; j < V::E; ++j) r[j] = V::cvt(o[j]);
    *reinterpret_cast<typename V::mem*>(row + c) = r;
  } else {
#pragma unroll
    for (int j = 0; j < V::E; ++j)
      if (c + j < C) row[c + j] = V::cvt(o[j]);
  }
}

// an ignored row: exact zeros
template <typename T, int G>
__device__ __forceinline__ void zero_row(T* __restrict__ dr, long C) {
  typedef Vec<T> V;
  float o[V::E];
#pragma unroll
  for (int j = 0; j < V::E; ++j) o[j] = 0.f;
  for (long c = (long)V::E * threadIdx.x; c < C; c += (long)V::E * G) stv<T>(dr, c, C, o);
}

// (max, arg-max) over the G lanes of the block, ties to the smallest index; every lane gets it.
template <int G>
__device__ __forceinline__ void group_argmax(float& m, int& am, float* sm, int* sa) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x >> 6] = m;
    sa[threadIdx.x >> 6] = am;
  }
  __syncthreads();
  m = sm[0];
  am = sa[0];
#pragma unroll
  for (int w = 1; w < G / 64; ++w) {
    const float om = sm[w];
    const int oa = sa[w];
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
}

// three sums over the G lanes of the block, added in wave order; every lane gets them.
template <int G>
__device__ __forceinline__ void group_sum3(float& a, float& b, float& c, float (*slot)[16]) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    slot[0][threadIdx.x >> 6] = a;
    slot[1][threadIdx.x >> 6] = b;
    slot[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  a = b = c = 0.f;
#pragma unroll
  for (int w = 0; w < G / 64; ++w) {
    a += slot[0][w];
    b += slot[1][w];
    c += slot[2][w];
  }
}

// 64 columns per lane (bf16, NV = 8): the compiler would carry the 64 converted values of one
// pass, or their exponentials, over to the next beside the 32 registers of the row, past the 128
// VGPRs of a 16-wave block, and spill.  The row is made opaque between the passes there, so
// that each pass converts it again.
template <typename T, int NV>
__device__ __forceinline__ void forget(typename Vec<T>::reg* v) {
  if constexpr (NV * Vec<T>::E > 32) {
#pragma unroll
    for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(v[i]));
  }
}

// the row's loss and correct flag (the formula of xent_kernel)
__device__ __forceinline__ void row_out(float m, int am, float s, float sz, float zl, long lab, int C, float eps,
                                        long row, float* __restrict__ loss, float* __restrict__ correct) {
  const float lse = m + __logf(s);
  loss[row] = (1.f - eps) * (lse - zl) + eps * (lse - sz / (float)C);
  correct[row] = am == lab ? 1.f : 0.f;
}

// Resident form: one row per block of G lanes, lane t holds columns E*(t + G*i) + j.
template <typename T, int G, int NV>
__global__ void __launch_bounds__(G) xent_vocab_kernel(const T* __restrict__ z, long ldz,
                                                       const int64_t* __restrict__ labels, int C, float scale,
                                                       const float* __restrict__ scale_dev, float eps,
                                                       float* __restrict__ loss, float* __restrict__ correct,
                                                       T* __restrict__ dz) {
  typedef Vec<T> V;
  constexpr int E = V::E;
  __shared__ float sm[16];
  __shared__ int sa[16];
  __shared__ float red[3][16];
  const int t = threadIdx.x;
  const long row = blockIdx.x;
  const long lab = labels[row];
  T* dr = dz + row * C;
  if (lab < 0 || lab >= C) {  // the whole block: no barrier is skipped by a part of it
    zero_row<T, G>(dr, C);
    if (t == 0) loss[row] = correct[row] = 0.f;
    return;
  }
  const T* zr = z + row * ldz;
  const int li = (int)lab;  // 0 <= lab < C: 32-bit column compares
  typename V::reg v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = E * (t + G * i);
    if (c < C) {
      v[i] = ldv<T>(zr, c, C);
    } else {
#pragma unroll
      for (int j = 0; j < E; ++j) v[i][j] = V::ninf();
    }
  }
  float m = -INFINITY;
  int am = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = E * (t + G * i);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float x = V::get(v[i], j);
      if (x > m) { m = x; am = c + j; }
    }
  }
  group_argmax<G>(m, am, sm, sa);
  forget<T, NV>(v);
  float s = 0.f, sz = 0.f, zl = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = E * (t + G * i);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float x = V::get(v[i], j);
      s += __expf(x - m);
      sz += c + j < C ? x : 0.f;
      zl += c + j == li ? x : 0.f;  // one lane adds the label's logit, every other one zeros
    }
  }
  group_sum3<G>(s, sz, zl, red);
  if (t == 0) row_out(m, am, s, sz, zl, lab, C, eps, row, loss, correct);
  const float gs = scale_dev ? scale_dev[1] : scale;
  const float inv_s = 1.f / s, tu = eps / (float)C;
  forget<T, NV>(v);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = E * (t + G * i);
    if (c >= C) continue;
    float o[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float p = __expf(V::get(v[i], j) - m) * inv_s;
      const float tg = (c + j == li ? 1.f - eps : 0.f) + tu;
      o[j] = (p - tg) * gs;
    }
    stv<T>(dr, c, C, o);
  }
}

// Streaming form for rows wider than the registers of a 1024-lane block: an online
// (max, sum) per lane over the first read, the gradient from a second one.
constexpr int XV_SG = 1024;

template <typename T>
__global__ void __launch_bounds__(XV_SG) xent_vocab_stream_kernel(const T* __restrict__ z, long ldz,
                                                                  const int64_t* __restrict__ labels, int C,
                                                                  float scale, const float* __restrict__ scale_dev,
                                                                  float eps, float* __restrict__ loss,
                                                                  float* __restrict__ correct, T* __restrict__ dz) {
  typedef Vec<T> V;
  constexpr int E = V::E, G = XV_SG;
  __shared__ float sm[16];
  __shared__ int sa[16];
  __shared__ float red[3][16];
  const int t = threadIdx.x;
  const long row = blockIdx.x;
  const long lab = labels[row];
  const long Cl = C;
  T* dr = dz + row * Cl;
  if (lab < 0 || lab >= Cl) {
    zero_row<T, G>(dr, Cl);
    if (t == 0) loss[row] = correct[row] = 0.f;
    return;
  }
  const T* zr = z + row * ldz;
  float lm = -INFINITY, s = 0.f, sz = 0.f, zl = 0.f;  // lm: this lane's running max
  int am = 0x7fffffff;
#pragma unroll 2
  for (long c = (long)E * t; c < Cl; c += (long)E * G) {
    const typename V::reg r = ldv<T>(zr, c, Cl);
    float x[E];
    float vm = -INFINITY;
    int vj = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      x[j] = V::get(r, j);
      if (x[j] > vm) { vm = x[j]; vj = j; }
      sz += c + j < Cl ? x[j] : 0.f;
      zl += c + j == lab ? x[j] : 0.f;
    }
    if (vm == -INFINITY) continue;  // nothing but -inf here: adds 0 to the sum, wins no max
    if (vm > lm) {                  // columns go upwards: a later equal value does not win
      s *= __expf(lm - vm);         // lm = -inf the first time: s = 0 * 0
      lm = vm;
      am = (int)(c + vj);
    }
#pragma unroll
    for (int j = 0; j < E; ++j) s += __expf(x[j] - lm);
  }
  float m = lm;
  group_argmax<G>(m, am, sm, sa);
  s = lm == -INFINITY ? 0.f : s * __expf(lm - m);
  group_sum3<G>(s, sz, zl, red);
  if (t == 0) row_out(m, am, s, sz, zl, lab, C, eps, row, loss, correct);
  const float gs = scale_dev ? scale_dev[1] : scale;
  const float inv_s = 1.f / s, tu = eps / (float)C;
#pragma unroll 2
  for (long c = (long)E * t; c < Cl; c += (long)E * G) {
    const typename V::reg r = ldv<T>(zr, c, Cl);
    float o[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float p = __expf(V::get(r, j) - m) * inv_s;
      const float tg = (c + j == lab ? 1.f - eps : 0.f) + tu;
      o[j] = (p - tg) * gs;
    }
    stv<T>(dr, c, Cl, o);
  }
}

// out[0] = number of labels inside [0, C), out[1] = 1 / max(that, 1): the scale of the mean
// over the valid rows, left on the device for the main and the finalise kernel.  One block;
// the counts are integers, so the result does not depend on an order anyway.
__global__ void __launch_bounds__(1024) xent_count_kernel(const int64_t* __restrict__ labels, long N, int C,
                                                          float* __restrict__ out) {
  __shared__ unsigned cnt[16];
  unsigned n = 0;
  for (long i = threadIdx.x; i < N; i += 1024) {
    const long lab = labels[i];
    n += lab >= 0 && lab < C ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
    for (int w = 0; w < 16; ++w) tot += cnt[w];
    out[0] = (float)tot;
    out[1] = 1.f / (float)(tot > 0 ? tot : 1u);
  }
}

// mean_out = sum(loss) * scale; acc += [sum loss, sum correct, rows] * acc_w.  One block: lane
// t sums rows t, t + 1024, .. upwards, the lanes of a wave meet in wave_sum, the waves in LDS
// in wave order.  cnt (the count kernel's buffer) given: scale = cnt[1], rows = cnt[0].
__global__ void __launch_bounds__(1024) xent_finalize_kernel(const float* __restrict__ loss,
                                                             const float* __restrict__ correct, long N, float scale,
                                                             const float* __restrict__ cnt,
                                                             float* __restrict__ mean_out, float* __restrict__ acc,
                                                             float acc_w) {
  __shared__ float red[2][16];
  float l = 0.f, k = 0.f;
  for (long i = threadIdx.x; i < N; i += 1024) {
    l += loss[i];
    k += correct[i];
  }
  l = wave_sum(l);
  k = wave_sum(k);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = l;
    red[1][threadIdx.x >> 6] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tl = 0.f, tc = 0.f;
    for (int w = 0; w < 16; ++w) {
      tl += red[0][w];
      tc += red[1][w];
    }
    mean_out[0] = tl * (cnt ? cnt[1] : scale);
    if (acc) {
      acc[0] += tl * acc_w;
      acc[1] += tc * acc_w;
      acc[2] += (cnt ? cnt[0] : (float)N) * acc_w;
    }
  }
}

template <typename T, int G, int NV>
void resident_launch(const void* z, long ldz, const int64_t* labels, long N, int C, float scale,
                     const float* scale_dev, float eps, float* loss, float* correct, void* dz, hipStream_t s) {
  xent_vocab_kernel<T, G, NV><<<(unsigned)N, G, 0, s>>>((const T*)z, ldz, labels, C, scale, scale_dev, eps, loss,
                                                        correct, (T*)dz);
}

// One (G, NV) per width in 16-byte vectors, G * NV >= vectors; above 1024 * 8 the streaming form.
template <typename T>
void vocab_launch(const void* z, long ldz, const int64_t* labels, long N, int C, float scale, const float* scale_dev,
                  float eps, float* loss, float* correct, void* dz, hipStream_t s) {
  const long nv = ((long)C + Vec<T>::E - 1) / Vec<T>::E;
#define XV_ARGS z, ldz, labels, N, C, scale, scale_dev, eps, loss, correct, dz, s
  if (nv <= 256) resident_launch<T, 256, 1>(XV_ARGS);
  else if (nv <= 512) resident_launch<T, 256, 2>(XV_ARGS);
  else if (nv <= 1024) resident_launch<T, 512, 2>(XV_ARGS);
  else if (nv <= 2048) resident_launch<T, 512, 4>(XV_ARGS);
  else if (nv <= 4096) resident_launch<T, 1024, 4>(XV_ARGS);
  else if (nv <= 8192) resident_launch<T, 1024, 8>(XV_ARGS);
  else
    xent_vocab_stream_kernel<T><<<(unsigned)N, XV_SG, 0, s>>>((const T*)z, ldz, labels, C, scale, scale_dev, eps,
                                                              loss, correct, (T*)dz);
#undef XV_ARGS
}

}  // namespace

extern "C" {

// widest row the resident form takes (wider ones stream)
int ca_xent_vocab_resident_max(int is_bf16) { return is_bf16 ? 8 * 1024 * 8 : 4 * 1024 * 8; }

// loss[N], correct[N], dlogits[N, C] (contiguous) from logits[N, :C] with row pitch ldz.
// scale_dev != nullptr: the gradient scale is scale_dev[1] (ca_xent_vocab_count's buffer).
int ca_xent_vocab(const void* logits, long ldz, int is_bf16, const int64_t* labels, long N, int C, float scale,
                  const float* scale_dev, float label_smoothing, float* loss, float* correct, void* dlogits,
                  hipStream_t s) {
  if (N <= 0 || N > 0x7fffffffL || C <= 0 || ldz < C) return -1;
  if (is_bf16)
    vocab_launch<bf16_t>(logits, ldz, labels, N, C, scale, scale_dev, label_smoothing, loss, correct, dlogits, s);
  else
    vocab_launch<float>(logits, ldz, labels, N, C, scale, scale_dev, label_smoothing, loss, correct, dlogits, s);
  CA_LAUNCH_CHECK();
  return 0;
}

// out[0] = labels inside [0, C), out[1] = 1 / max(out[0], 1)
int ca_xent_vocab_count(const int64_t* labels, long N, int C, float* out, hipStream_t s) {
  if (N <= 0 || C <= 0) return -1;
  xent_count_kernel<<<1, 1024, 0, s>>>(labels, N, C, out);
  CA_LAUNCH_CHECK();
  return 0;
}

// mean_out[0] = sum(loss) * scale (cnt: * cnt[1]); acc (optional) += [sum loss, sum correct, rows] * acc_w
int ca_xent_vocab_finalize(const float* loss, const float* correct, long N, float scale, const float* cnt,
                           float* mean_out, float* acc, float acc_w, hipStream_t s) {
  if (N <= 0) return -1;
  xent_finalize_kernel<<<1, 1024, 0, s>>>(loss, correct, N, scale, cnt, mean_out, acc, acc_w);
  CA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
