// LayerNorm at any width (ops.layer_norm, Keras LayerNormalization): 1 <= C <= 16384, any
// M >= 1, C not necessarily a multiple of anything, any 2-byte-aligned base pointer.
// bf16 activations / gradients, fp32 gamma / beta / row statistics, fp32 math.
//
//  * forward:   h = x (+ residual);  y = LN(h) * gamma + beta;  mean[M], rstd[M]
//    (h is written only with a residual).  Two-pass statistics over the row held in
//    registers: the mean first, then the centred sum of squares.
//  * backward:  dh = rstd * (g*dy - mean_c(g*dy) - xhat * mean_c(g*dy*xhat))  (row pass, xhat
//    re-centred: see the kernel), and
//    per-chunk [dgamma | dbeta] column partials (column pass) that the fixed-order column
//    finalisation of gradfin.hip sums: no atomics, bitwise reproducible.
//
// The BERT path's ln_fwd / ln_bwd (rowops.hip) keep a row in one wave and the column
// partials of a whole block in 12*C floats of LDS, which ends at C = 2048 / 1344.  Here a
// row belongs to a GROUP of G lanes -- one wave (C <= 1024), a 256-lane block (C <= 4096), a
// 512- or 1024-lane block above -- so a lane holds at most 16 columns of a tensor (32 in the
// forward above 8192), and the column sums are a
// pass of their own over 256-column tiles whose registers and 16 KB of LDS do not depend on C.
//
// Memory access: a lane moves 8 consecutive bf16 (16 B) of a row at columns 8k .. 8k+7.
// With an odd C (or a sliced base) those 16 bytes start on any 2-byte boundary; the vector
// types below carry that alignment, and global memory takes such accesses as they are.  The
// last, partial vector of a row (C % 8 columns) goes element by element under a bound check,
// so nothing is read or written past M*C elements.
#include "ca_common.h"

namespace {

typedef us8 us8u __attribute__((aligned(2)));
typedef f4 f4u __attribute__((aligned(4)));

// columns c .. c+7 of a row as fp32; columns >= C read as 0 and are not touched
__device__ __forceinline__ void ld8(const bf16_t* __restrict__ row, int c, int C, float* v) {
  if (c + 8 <= C) {
    const us8 u = *reinterpret_cast<const us8u*>(row + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(u[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c + j < C ? bf2f(row[c + j]) : 0.f;
  }
}

__device__ __forceinline__ void st8(bf16_t* __restrict__ row, int c, int C, const float* v) {
  if (c + 8 <= C) {
    us8 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = f2bf(v[j]);
    *reinterpret_cast<us8u*>(row + c) = u;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c + j < C) row[c + j] = f2bf(v[j]);
  }
}

// gamma / beta: fp32 [C], 4-byte aligned
__device__ __forceinline__ void ldf8(const float* __restrict__ p, int c, int C, float* v) {
  if (c + 8 <= C) {
    const f4 a = *reinterpret_cast<const f4u*>(p + c), b = *reinterpret_cast<const f4u*>(p + c + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = a[j];
      v[4 + j] = b[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c + j < C ? p[c + j] : 0.f;
  }
}

// Sum over the G lanes that share a row, every lane gets it.  G = 64: the wave.  G > 64: the
// whole block (one row per block); the waves' sums meet in `slot` and are added in wave
// order.  Every reduction of a kernel has a slot of its own, so one barrier each is enough.
template <int G>
__device__ __forceinline__ float group_sum(float v, float* slot) {
  v = wave_sum(v);
  if constexpr (G == 64) {
    return v;
  } else {
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < G / 64; ++w) t += slot[w];
    return t;
  }
}

template <int G>
constexpr int ln_block() {
  return G == 64 ? 256 : G;  // G = 64: four rows (waves) per block
}

// lane `t` of its group holds columns 8*(t + G*i) + j, i < NV, j < 8
template <int G, int NV>
__global__ void __launch_bounds__(ln_block<G>()) ln_any_fwd_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ res, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16_t* __restrict__ y, bf16_t* __restrict__ h_out, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, long M, int C, float eps) {
  __shared__ float red[2][16];
  const int t = G == 64 ? (threadIdx.x & 63) : threadIdx.x;
  const long row = G == 64 ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x;
  if (row >= M) return;  // a whole wave (G = 64); never taken for G > 64 (grid = M)
  const long base = row * C;
  float v[NV][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 8 * (t + G * i);
    ld8(x + base, c, C, v[i]);
    if (res) {
      float r[8];
      ld8(res + base, c, C, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] += r[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[i][j];
  }
  const float mean = group_sum<G>(s, red[0]) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 8 * (t + G * i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = v[i][j] - mean;
      q += c + j < C ? d * d : 0.f;
    }
  }
  const float rstd = rsqrtf(group_sum<G>(q, red[1]) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 8 * (t + G * i);
    if (c >= C) continue;
    if (h_out) st8(h_out + base, c, C, v[i]);
    float g[8], b[8], o[8];
    ldf8(gamma, c, C, g);
    ldf8(beta, c, C, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + b[j];
    st8(y + base, c, C, o);
  }
  if (t == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

// Row pass of the backward: dh, and xm[M], the row means of the rebuilt xhat (below), which
// the column pass takes out as well.
template <int G, int NV>
__global__ void __launch_bounds__(ln_block<G>()) ln_any_bwd_dh_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ h, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, bf16_t* __restrict__ dh,
    float* __restrict__ xm, long M, int C) {
  __shared__ float red[3][16];
  const int t = G == 64 ? (threadIdx.x & 63) : threadIdx.x;
  const long row = G == 64 ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x;
  if (row >= M) return;
  const long base = row * C;
  const float mu = mean[row], rs = rstd[row];
  float gd[NV][8], xh[NV][8];
  float sa = 0.f, sb = 0.f, sx = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 8 * (t + G * i);
    float g[8];
    ld8(dy + base, c, C, gd[i]);
    ld8(h + base, c, C, xh[i]);
    ldf8(gamma, c, C, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // past C: dy and gamma read as 0, so the (meaningless) xh there adds nothing to sa, sb
      // (one rounded product, the same in the column pass: no contraction into an fma)
      xh[i][j] = __fmul_rn(xh[i][j] - mu, rs);
      gd[i][j] *= g[j];
      sa += gd[i][j];
      sb += gd[i][j] * xh[i][j];
      sx += c + j < C ? xh[i][j] : 0.f;
    }
  }
  // The statistics are those of the fp32 sum x + residual, h is that sum rounded to bf16: the
  // xhat rebuilt from h has a row mean m of the size of that rounding, not 0.  It is taken out
  // (xhat - m, and b with it), which keeps dh exactly orthogonal to a constant shift of the
  // row -- for C = 1 exactly 0 -- also where rstd is large against the rounding (var << eps).
  const float invC = 1.f / (float)C;
  const float m = group_sum<G>(sx, red[2]) * invC;
  const float a = group_sum<G>(sa, red[0]) * invC, b = group_sum<G>(sb, red[1]) * invC - m * a;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = 8 * (t + G * i);
    if (c >= C) continue;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = rs * (gd[i][j] - a - (xh[i][j] - m) * b);
    st8(dh + base, c, C, o);
  }
  if (t == 0) xm[row] = m;
}

// Column pass of the backward.  Block (bx, by): columns 256*bx .. +255, rows of chunk by.
// Lane (ty, tx) = (threadIdx.x / 32, threadIdx.x % 32) walks the chunk's rows ty, ty + 8, ..
// with columns 256*bx + 8*tx + j in registers; the eight row lanes meet in LDS in a fixed
// order.  part[by][0][C] = sum dy * (xhat - xm), part[by][1][C] = sum dy over the chunk's rows.
constexpr int LN_CT = 256;  // columns per block
constexpr int LN_RL = 8;    // row lanes per block

__global__ void __launch_bounds__(256) ln_any_bwd_cols_kernel(const bf16_t* __restrict__ dy,
                                                              const bf16_t* __restrict__ h,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ xm,
                                                              float* __restrict__ part, long M, int C, long rpc) {
  __shared__ __attribute__((aligned(16))) float red[LN_RL][2][LN_CT];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = blockIdx.x * LN_CT + 8 * tx;
  const long r0 = (long)blockIdx.y * rpc;
  const long r1 = r0 + rpc < M ? r0 + rpc : M;
  float ag[8], ab[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ag[j] = ab[j] = 0.f;
  if (c < C) {
#pragma unroll 2
    for (long r = r0 + ty; r < r1; r += LN_RL) {
      float d[8], xv[8];
      ld8(dy + r * C, c, C, d);
      ld8(h + r * C, c, C, xv);
      const float mu = mean[r], rs = rstd[r], m = xm[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ag[j] += d[j] * (__fmul_rn(xv[j] - mu, rs) - m);
        ab[j] += d[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[ty][0][8 * tx + j] = ag[j];
    red[ty][1][8 * tx + j] = ab[j];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int col = blockIdx.x * LN_CT + threadIdx.x;
    if (col >= C) continue;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LN_RL; ++w) s += red[w][k][threadIdx.x];
    part[((long)blockIdx.y * 2 + k) * C + col] = s;
  }
}

template <int G, int NV>
void fwd_launch(const bf16_t* x, const bf16_t* res, const float* g, const float* b, bf16_t* y, bf16_t* h, float* mu,
                float* rs, long M, int C, float eps, hipStream_t s) {
  const long blocks = G == 64 ? (M + 3) / 4 : M;
  ln_any_fwd_kernel<G, NV><<<(unsigned)blocks, ln_block<G>(), 0, s>>>(x, res, g, b, y, h, mu, rs, M, C, eps);
}

template <int G, int NV>
void dh_launch(const bf16_t* dy, const bf16_t* h, const float* mu, const float* rs, const float* g, bf16_t* dh,
               float* xm, long M, int C, hipStream_t s) {
  const long blocks = G == 64 ? (M + 3) / 4 : M;
  ln_any_bwd_dh_kernel<G, NV><<<(unsigned)blocks, ln_block<G>(), 0, s>>>(dy, h, mu, rs, g, dh, xm, M, C);
}

// One (G, NV) per width, 8 * G * NV >= C; WIDE is the group of the rows above 8192 columns.
// 512 lanes with NV = 4 is the faster forward there (17.7 against 19.9 us at 1024 x 16384), but
// the backward's row pass then needs 170 VGPRs (two waves per SIMD) and loses (25.1 against
// 23.2 us), so that one keeps 1024 lanes with NV = 2.  At C <= 8192, 512 lanes x 2 beat 1024
// lanes x 1 in both directions (15.7 / 19.9 against 17.9 / 20.8 us at 2048 x 8192).
#define LN_ANY_DISPATCH(F, WIDE, ...)                            \
  do {                                                           \
    if (C <= 512) F<64, 1>(__VA_ARGS__);                         \
    else if (C <= 1024) F<64, 2>(__VA_ARGS__);                   \
    else if (C <= 2048) F<256, 1>(__VA_ARGS__);                  \
    else if (C <= 4096) F<256, 2>(__VA_ARGS__);                  \
    else if (C <= 8192) F<512, 2>(__VA_ARGS__);                  \
    else F<WIDE, 16384 / 8 / WIDE>(__VA_ARGS__);                 \
  } while (0)

bool ln_any_shape_ok(long M, int C) { return C >= 1 && C <= 16384 && M >= 1 && M <= 0x7fffffffL; }

// row chunks of the column pass: at least 32 rows each (4 per row lane), at most ~2048 blocks
long ln_any_rows_per_chunk(long M, int C) {
  const long tiles = ca_cdiv(C, LN_CT);
  long maxp = 2048 / tiles;
  if (maxp < 1) maxp = 1;
  long p = (M + 31) / 32;
  if (p > maxp) p = maxp;
  return (M + p - 1) / p;
}

}  // namespace

extern "C" {

// y = LN(x (+ res)) * gamma + beta; h_out (with res only) keeps the pre-norm sum.
int ca_layer_norm_fwd(const bf16_t* x, const bf16_t* res, const float* gamma, const float* beta, bf16_t* y,
                      bf16_t* h_out, float* mean, float* rstd, long M, int C, float eps, hipStream_t s) {
  if (!ln_any_shape_ok(M, C)) return -1;
  LN_ANY_DISPATCH(fwd_launch, 512, x, res, gamma, beta, y, h_out, mean, rstd, M, C, eps, s);
  CA_LAUNCH_CHECK();
  return 0;
}

// partial rows the backward leaves at the start of ws
long ca_layer_norm_bwd_parts(long M, int C) {
  if (!ln_any_shape_ok(M, C)) return 0;
  const long rpc = ln_any_rows_per_chunk(M, C);
  return (M + rpc - 1) / rpc;
}

// ws: [parts][2][C] partials, then the M row means xm that the row pass hands to the column pass
long ca_layer_norm_bwd_workspace_floats(long M, int C) { return ca_layer_norm_bwd_parts(M, C) * 2 * C + M; }

// dh = LN'(dy); ws[parts][2][C] = per-chunk [dgamma | dbeta] partials, to be summed over
// `parts` in a fixed order by the caller (column finalisation of gradfin.hip).
int ca_layer_norm_bwd(const bf16_t* dy, const bf16_t* h, const float* mean, const float* rstd, const float* gamma,
                      bf16_t* dh, float* ws, long M, int C, hipStream_t s) {
  if (!ln_any_shape_ok(M, C)) return -1;
  const long rpc = ln_any_rows_per_chunk(M, C);
  const long parts = (M + rpc - 1) / rpc;
  float* xm = ws + parts * 2 * C;
  LN_ANY_DISPATCH(dh_launch, 1024, dy, h, mean, rstd, gamma, dh, xm, M, C, s);
  CA_LAUNCH_CHECK();
  const dim3 grid(ca_cdiv(C, LN_CT), (unsigned)parts);
  ln_any_bwd_cols_kernel<<<grid, 256, 0, s>>>(dy, h, mean, rstd, xm, ws, M, C, rpc);
  CA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
