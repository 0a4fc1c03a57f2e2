// Depthwise convolution (ops.depthwise_conv2d, Keras DepthwiseConv2D / SeparableConv2D):
// NHWC bf16 activations, weight [KH, KW, Cin, DM] bf16 (the Keras layout; flattened it is
// [KH*KW, Cout] with Cout = Cin * DM, and output channel o = c * DM + m reads input channel
// c), fp32 math.  One input channel per output channel leaves the MFMA tile no reduction
// dimension, and the operation moves ~1 byte per FLOP: these are streaming kernels.
//
// One geometry (DwGeom) for the three passes.  OH / OW are given, not derived; only the top /
// left padding is carried, and a tap outside the image contributes zero -- TF's asymmetric
// SAME split (extra row / column at the bottom / right) needs no padded copy.
// KH, KW in 1..7, strides in 1..4, any Cin >= 1, any DM >= 1, dilation 1.
//
// Every kernel exists in two widths (template VW):
//   VW = 8  a lane moves 8 consecutive channels as one 16-byte vector; taken when DM == 1,
//           Cin % 8 == 0 and every bf16 base pointer is 16-byte aligned.  Neighbouring lanes
//           take neighbouring channel vectors, so a wave reads contiguous NHWC memory;
//   VW = 1  a lane moves one channel (any Cin, any DM, any 2-byte-aligned base).
//
//  * forward   y = act(dwconv(x, w) + bias): a thread owns VW output channels of a strip of
//    DW_TW = 4 output pixels along W.  Per tap it loads the weight vector once for the strip and
//    the input vector of each strip pixel; input columns shared by neighbouring outputs are
//    re-read from L1, not kept in registers (strides are run-time values).  The 3x3 filter has
//    its own instantiation with unrolled tap loops (forward: one filter row at a time; dgrad: all).  fp32
//    bias and the activation (the GEMM epilogue's codes) at the store; with `pre` the bf16
//    pre-activation is stored too (GELU' needs it).
//  * dgrad     gather form, one thread per VW channels of one dx pixel: for each tap the one
//    output pixel oy = (iy + pad_top - ky) / sh that reads it, where the division is exact
//    and in range.  No atomics; an input pixel that no output reads gets exactly 0.
//  * wgrad     two launches, deterministic, no float atomics.  A workgroup takes a fixed chunk
//    of output pixels (blockIdx.z), <= 64 channel vectors (blockIdx.x) and a group of <= 9
//    taps (blockIdx.y: 3x3 is one group, 7x7 six).  Its 256 threads are [PR pixel rows][CVB
//    channel vectors]; a thread walks the chunk's pixels pr, pr + PR, ..., loads dy once per
//    pixel and x once per tap, and keeps 9 x VW fp32 sums.  The PR rows are added through LDS
//    in row order into the [chunks][KH*KW][Cout] fp32 workspace; dw_wgrad_reduce_kernel then
//    adds the chunks in a fixed order (four quarter sums in chunk order, combined 0..3) and
//    overwrites or accumulates into the [KH, KW, Cin, DM] fp32 result.
//
// All element offsets are 64-bit (thread and pixel counts are 32-bit; the launchers refuse
// more).  A halo load is clamped to a pixel inside its image and its value replaced by zero;
// nothing outside N*H*W*Cin / N*OH*OW*Cout / KH*KW*Cout elements is touched.
#include "ca_common.h"
#include "ca_mfma_core.h"

namespace {

struct DwGeom {
  int N, H, W, Cin, DM, KH, KW, sh, sw, pad_top, pad_left, OH, OW;
};

constexpr int DW_TW = 4;    // forward: output pixels per thread along W
constexpr int DW_TPG = 9;   // wgrad: taps per workgroup
constexpr int DW_CVB = 64;  // wgrad: channel vectors per workgroup (at most)

template <int VW>
__device__ __forceinline__ void dw_ld(const bf16_t* __restrict__ p, float (&f)[VW]) {
  if constexpr (VW == 8) {
    const us8 u = *reinterpret_cast<const us8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f(u[j]);
  } else {
    f[0] = bf2f(*p);
  }
}

template <int VW>
__device__ __forceinline__ void dw_st(bf16_t* __restrict__ p, const float (&f)[VW]) {
  if constexpr (VW == 8) {
    us8 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = f2bf(f[j]);
    *reinterpret_cast<us8*>(p) = u;
  } else {
    *p = f2bf(f[0]);
  }
}

// t / s for a stride s in 1..4; true when t >= 0 and the division is exact
__device__ __forceinline__ bool dw_div(int t, int s, int& q) {
  if (s == 1) {
    q = t;
    return t >= 0;
  }
  if (s == 2) {
    q = t >> 1;
    return t >= 0 && !(t & 1);
  }
  q = t / s;
  return t >= 0 && q * s == t;
}

// KT = 3: the 3x3 filter with compile-time tap loops (fully unrolled); KT = 0: KH / KW from
// the geometry.  Halo loads are branch-free: the address of a tap outside the image is clamped
// to pixel (row 0 / column 0) of the same image and its value replaced by zero, so the
// compiler issues a strip's loads together instead of waiting for each behind its own branch.
template <int VW, int KT>
__global__ void __launch_bounds__(256) dw_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                    const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                    bf16_t* __restrict__ pre, DwGeom g, int act) {
  const int KH = KT ? KT : g.KH, KW = KT ? KT : g.KW;
  constexpr int UNR = KT ? KT : 1;  // tap loops: unrolled for the compile-time filter only
  const int Cout = g.Cin * g.DM;
  const uint32_t CT = Cout / VW;
  const uint32_t strips = (g.OW + DW_TW - 1) / DW_TW;
  const uint32_t total = (uint32_t)g.N * g.OH * strips * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int ox0 = (int)(r % strips) * DW_TW;
    r /= strips;
    const int oy = (int)(r % (uint32_t)g.OH);
    const int n = (int)(r / (uint32_t)g.OH);
    const int o0 = vc * VW;
    const int c0 = VW == 8 ? o0 : o0 / g.DM;  // VW == 8 runs with DM == 1 only
    float acc[DW_TW][VW];
#pragma unroll
    for (int q = 0; q < DW_TW; ++q)
#pragma unroll
      for (int j = 0; j < VW; ++j) acc[q][j] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < KH; ++ky) {
      const int iy = oy * g.sh - g.pad_top + ky;
      const bool oky = (unsigned)iy < (unsigned)g.H;
      const bf16_t* xr = x + ((long)n * g.H + (oky ? iy : 0)) * g.W * g.Cin + c0;
#pragma unroll UNR
      for (int kx = 0; kx < KW; ++kx) {
        float wv[VW];
        dw_ld<VW>(w + (long)(ky * KW + kx) * Cout + o0, wv);
#pragma unroll
        for (int q = 0; q < DW_TW; ++q) {
          // a strip pixel past OW reads a valid (clamped) address and is never stored
          const int ix = (ox0 + q) * g.sw - g.pad_left + kx;
          const bool ok = oky && (unsigned)ix < (unsigned)g.W;
          float xv[VW];
          dw_ld<VW>(xr + (ok ? (long)ix * g.Cin : 0L), xv);
#pragma unroll
          for (int j = 0; j < VW; ++j) acc[q][j] = fmaf(ok ? xv[j] : 0.f, wv[j], acc[q][j]);
        }
      }
    }
    float b[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) b[j] = bias ? bias[o0 + j] : 0.f;
#pragma unroll
    for (int q = 0; q < DW_TW; ++q) {
      if (ox0 + q >= g.OW) continue;
      const long off = (((long)n * g.OH + oy) * g.OW + ox0 + q) * Cout + o0;
      float v[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) v[j] = acc[q][j] + b[j];
      if (pre) dw_st<VW>(pre + off, v);
      if (act != ca::ACT_NONE) {
#pragma unroll
        for (int j = 0; j < VW; ++j) v[j] = ca::act_fwd(act, v[j]);
      }
      dw_st<VW>(y + off, v);
    }
  }
}

template <int VW, int KT>
__global__ void __launch_bounds__(256) dw_dgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                      bf16_t* __restrict__ dx, DwGeom g) {
  const int KH = KT ? KT : g.KH, KW = KT ? KT : g.KW;
  constexpr int UNR = KT ? KT : 1;  // tap loops: unrolled for the compile-time filter only
  const int Cout = g.Cin * g.DM;
  const uint32_t CT = g.Cin / VW;
  const uint32_t total = (uint32_t)g.N * g.H * g.W * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int ix = (int)(r % (uint32_t)g.W);
    r /= (uint32_t)g.W;
    const int iy = (int)(r % (uint32_t)g.H);
    const int n = (int)(r / (uint32_t)g.H);
    const int c0 = vc * VW;
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
#pragma unroll UNR
    for (int ky = 0; ky < KH; ++ky) {
      int oy;
      const bool oky = dw_div(iy + g.pad_top - ky, g.sh, oy) && oy < g.OH;
      const bf16_t* gr = dy + ((long)n * g.OH + (oky ? oy : 0)) * g.OW * Cout + (long)c0 * g.DM;
#pragma unroll UNR
      for (int kx = 0; kx < KW; ++kx) {
        int ox;
        const bool ok = dw_div(ix + g.pad_left - kx, g.sw, ox) && ox < g.OW && oky;
        const bf16_t* gp = gr + (ok ? (long)ox * Cout : 0L);  // clamped: pixel (0, 0) of the image
        const bf16_t* wp = w + (long)(ky * KW + kx) * Cout + (long)c0 * g.DM;
        for (int m = 0; m < g.DM; ++m) {  // VW == 8: DM == 1, one trip
          float gv[VW], wv[VW];
          dw_ld<VW>(gp + m, gv);
          dw_ld<VW>(wp + m, wv);
#pragma unroll
          for (int j = 0; j < VW; ++j) acc[j] = fmaf(ok ? gv[j] : 0.f, wv[j], acc[j]);
        }
      }
    }
    dw_st<VW>(dx + (((long)n * g.H + iy) * g.W + ix) * g.Cin + c0, acc);
  }
}

// ws[chunk][tap][o] = sum over the chunk's output pixels of dy[p, o] * x[pixel of tap, c(o)]
template <int VW>
__global__ void __launch_bounds__(256) dw_wgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                      float* __restrict__ ws, DwGeom g, int CVB, int PR,
                                                      int chunk, int P) {
  __shared__ float red[256 * VW];
  const int Cout = g.Cin * g.DM;
  const int CT = Cout / VW;
  const int ntap = g.KH * g.KW;
  const int t = threadIdx.x;
  const int vcl = t % CVB, pr = t / CVB;
  const int vc = blockIdx.x * CVB + vcl;
  const bool active = pr < PR && vc < CT;
  const int o0 = vc * VW;
  const int c0 = VW == 8 ? o0 : o0 / g.DM;
  const int tap0 = blockIdx.y * DW_TPG;
  int dky[DW_TPG], dkx[DW_TPG];
#pragma unroll
  for (int j = 0; j < DW_TPG; ++j) {
    const int tap = tap0 + j < ntap ? tap0 + j : ntap - 1;
    dky[j] = tap / g.KW - g.pad_top;
    dkx[j] = tap % g.KW - g.pad_left;
  }
  float acc[DW_TPG][VW];
#pragma unroll
  for (int j = 0; j < DW_TPG; ++j)
#pragma unroll
    for (int k = 0; k < VW; ++k) acc[j][k] = 0.f;
  const int p0 = blockIdx.z * chunk;  // P < 2^31: checked by the launcher
  const int p1 = p0 + chunk < P ? p0 + chunk : P;
  if (active) {
    for (int p = p0 + pr; p < p1; p += PR) {
      const int ox = (int)((uint32_t)p % (uint32_t)g.OW);
      const uint32_t r = (uint32_t)p / (uint32_t)g.OW;
      const int oy = (int)(r % (uint32_t)g.OH);
      const int n = (int)(r / (uint32_t)g.OH);
      float gv[VW];
      dw_ld<VW>(dy + (long)p * Cout + o0, gv);
      const bf16_t* xn = x + (long)n * g.H * g.W * g.Cin + c0;
#pragma unroll
      for (int j = 0; j < DW_TPG; ++j) {
        // branch-free: a tap outside the image (or past the filter) reads pixel (0, 0) as zero
        const int iy = oy * g.sh + dky[j], ix = ox * g.sw + dkx[j];
        const bool ok = tap0 + j < ntap && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
        float xv[VW];
        dw_ld<VW>(xn + (ok ? ((long)iy * g.W + ix) * g.Cin : 0L), xv);
#pragma unroll
        for (int k = 0; k < VW; ++k) acc[j][k] = fmaf(gv[k], ok ? xv[k] : 0.f, acc[j][k]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < DW_TPG; ++j) {
    const int tap = tap0 + j;
    if (tap >= ntap) break;  // uniform over the workgroup
#pragma unroll
    for (int k = 0; k < VW; ++k) red[t * VW + k] = acc[j][k];  // inactive threads hold zeros
    __syncthreads();
    for (int e = t; e < CVB * VW; e += 256) {
      const int v2 = e / VW, k = e % VW;
      const int vc2 = blockIdx.x * CVB + v2;
      if (vc2 < CT) {
        float s = 0.f;
        for (int q = 0; q < PR; ++q) s += red[(q * CVB + v2) * VW + k];
        ws[((long)blockIdx.z * ntap + tap) * Cout + vc2 * VW + k] = s;
      }
    }
    __syncthreads();
  }
}

// out[i] (+)= sum over chunks of ws[chunk][i], i < n = KH*KW*Cout.  256 threads = 4 quarters
// of the chunk range x 64 columns; a quarter adds its chunks in order, then 0 + 1 + 2 + 3.
__global__ void __launch_bounds__(256) dw_wgrad_reduce_kernel(const float* __restrict__ ws, int nchunks, long n,
                                                             float* __restrict__ out, int accumulate) {
  __shared__ float part[4][64];
  const int col = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const int per = (nchunks + 3) / 4;
  const int c0 = q * per, c1 = c0 + per < nchunks ? c0 + per : nchunks;
  float s = 0.f;
  if (i < n)
    for (int c = c0; c < c1; ++c) s += ws[(long)c * n + i];
  part[q][col] = s;
  __syncthreads();
  if (q == 0 && i < n) {
    const float tot = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
    out[i] = accumulate ? out[i] + tot : tot;
  }
}

bool dw_geom_ok(const DwGeom& g) {
  return g.N >= 1 && g.H >= 1 && g.W >= 1 && g.Cin >= 1 && g.DM >= 1 && g.KH >= 1 && g.KH <= 7 && g.KW >= 1 &&
         g.KW <= 7 && g.sh >= 1 && g.sh <= 4 && g.sw >= 1 && g.sw <= 4 && g.pad_top >= 0 && g.pad_left >= 0 &&
         g.OH >= 1 && g.OW >= 1 && (long)g.Cin * g.DM < (1L << 30);
}

bool dw_aligned16(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

bool dw_vec_ok(const DwGeom& g) { return g.DM == 1 && g.Cin % 8 == 0; }

long dw_chunk(long P) {
  const long c = (P + 511) / 512;
  return c < 64 ? 64 : c;
}

}  // namespace

extern "C" {

int ca_dwconv_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, bf16_t* pre, int N, int H, int W,
                  int Cin, int DM, int KH, int KW, int sh, int sw, int pad_top, int pad_left, int OH, int OW, int act,
                  hipStream_t st) {
  const DwGeom g{N, H, W, Cin, DM, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!dw_geom_ok(g) || !x || !w || !y || act < 0 || act > ca::ACT_ELU) return -1;
  const long strips = (long)N * OH * ((OW + DW_TW - 1) / DW_TW);
  if (strips * Cin * DM >= (1L << 31)) return -1;  // 32-bit thread indices
  if (dw_vec_ok(g) && dw_aligned16(x, w, y, pre)) {
    const int grid = ca_stream_grid(strips * (Cin / 8), 256);
    if (KH == 3 && KW == 3) dw_fwd_kernel<8, 3><<<grid, 256, 0, st>>>(x, w, bias, y, pre, g, act);
    else dw_fwd_kernel<8, 0><<<grid, 256, 0, st>>>(x, w, bias, y, pre, g, act);
  } else {
    dw_fwd_kernel<1, 0><<<ca_stream_grid(strips * Cin * DM, 256), 256, 0, st>>>(x, w, bias, y, pre, g, act);
  }
  CA_LAUNCH_CHECK();
  return 0;
}

int ca_dwconv_dgrad(const bf16_t* dy, const bf16_t* w, bf16_t* dx, int N, int H, int W, int Cin, int DM, int KH,
                    int KW, int sh, int sw, int pad_top, int pad_left, int OH, int OW, hipStream_t st) {
  const DwGeom g{N, H, W, Cin, DM, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!dw_geom_ok(g) || !dy || !w || !dx) return -1;
  const long pix = (long)N * H * W;
  if (pix * Cin >= (1L << 31)) return -1;  // 32-bit thread indices
  if (dw_vec_ok(g) && dw_aligned16(dy, w, dx)) {
    const int grid = ca_stream_grid(pix * (Cin / 8), 256);
    if (KH == 3 && KW == 3) dw_dgrad_kernel<8, 3><<<grid, 256, 0, st>>>(dy, w, dx, g);
    else dw_dgrad_kernel<8, 0><<<grid, 256, 0, st>>>(dy, w, dx, g);
  } else {
    dw_dgrad_kernel<1, 0><<<ca_stream_grid(pix * Cin, 256), 256, 0, st>>>(dy, w, dx, g);
  }
  CA_LAUNCH_CHECK();
  return 0;
}

// chunks of output pixels the weight gradient is split into (rows of its workspace)
long ca_dwconv_wgrad_chunks(int N, int OH, int OW) {
  const long P = (long)N * OH * OW;
  if (P < 1) return 0;
  const long c = dw_chunk(P);
  return (P + c - 1) / c;
}

// dw [KH, KW, Cin, DM] fp32 = (accumulate ? dw : 0) + sum dy * x; ws: chunks * KH*KW * Cout floats
int ca_dwconv_wgrad(const bf16_t* dy, const bf16_t* x, float* dw, int accumulate, float* ws, int N, int H, int W,
                    int Cin, int DM, int KH, int KW, int sh, int sw, int pad_top, int pad_left, int OH, int OW,
                    hipStream_t st) {
  const DwGeom g{N, H, W, Cin, DM, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!dw_geom_ok(g) || !dy || !x || !dw || !ws) return -1;
  const long P = (long)N * OH * OW;
  if (P >= (1L << 31)) return -1;  // 32-bit pixel indices
  const long chunk = dw_chunk(P);
  const int nchunks = (int)((P + chunk - 1) / chunk);
  const int Cout = Cin * DM, ntap = KH * KW;
  const bool vec = dw_vec_ok(g) && dw_aligned16(dy, x, nullptr);
  const int CT = vec ? Cout / 8 : Cout;
  const int CVB = CT < DW_CVB ? CT : DW_CVB;
  const int PR = 256 / CVB;
  const dim3 grid((unsigned)((CT + CVB - 1) / CVB), (unsigned)((ntap + DW_TPG - 1) / DW_TPG), (unsigned)nchunks);
  if (vec) dw_wgrad_kernel<8><<<grid, 256, 0, st>>>(dy, x, ws, g, CVB, PR, (int)chunk, (int)P);
  else dw_wgrad_kernel<1><<<grid, 256, 0, st>>>(dy, x, ws, g, CVB, PR, (int)chunk, (int)P);
  CA_LAUNCH_CHECK();
  const long n = (long)ntap * Cout;
  dw_wgrad_reduce_kernel<<<(unsigned)((n + 63) / 64), 256, 0, st>>>(ws, nchunks, n, dw, accumulate);
  CA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
