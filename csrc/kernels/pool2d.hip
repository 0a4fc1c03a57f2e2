// Windowed max / average pooling at any window (ops.max_pool2d_nhwc, ops.avg_pool2d_nhwc, Keras
// MaxPooling2D / AveragePooling2D and their 1D forms): NHWC bf16 activations, fp32 math.
// pool.hip keeps the square, symmetric-pad, C % 8 == 0 max pool of the ResNet path.
//
// One geometry (PoolGeom) for the four passes, modelled on DwGeom (dwconv.hip).  OH / OW are
// given, not derived; only the top / left padding is carried, and a tap outside the image is
// skipped -- TF's asymmetric SAME split (extra row / column at the bottom / right) needs no
// padded copy.  The launchers refuse a geometry in which a window holds no in-image tap, so
// every window's clipped tap range [k0, k1) is non-empty.
//
// Every kernel exists in two widths (template VW):
//   VW = 8  a lane moves 8 consecutive channels as one 16-byte vector (and 8 argmax bytes as one
//           8-byte word); taken when C % 8 == 0 and every base pointer is 16-byte aligned;
//   VW = 1  a lane moves one channel (any C >= 1, any 2-byte-aligned base).
//
//  * max forward    a thread owns VW channels of one output pixel.  It scans the in-image taps in
//    row-major order and keeps the first that attains the maximum (strict '>'); the argmax byte
//    kh * KW + kw starts at the first in-image tap, so a window of -inf only still points at a
//    real pixel.
//  * max backward   gather form, one thread per VW channels of one dx pixel (h, w): the windows
//    oh in [ceil((h + pad_top - KH + 1) / sh), floor((h + pad_top) / sh)] clipped to [0, OH - 1]
//    (ow likewise) are the ones that read it; dy is added where the window's argmax byte names
//    this pixel's tap.  Row-major window order, no atomics; an unread pixel gets exactly 0.
//  * avg forward    y = (sum of the in-image taps) / (their number): padding is excluded from
//    the divisor (TF's AveragePooling2D).  The number is the product of the two clipped extents.
//  * avg backward   the same window walk: dx = sum over covering windows of dy / count, the
//    count recomputed from the geometry; nothing is saved by the forward.
//
// All element offsets are 64-bit (thread counts are 32-bit; the launchers refuse more).  Loads
// and stores stay inside N*H*W*C / N*OH*OW*C elements: taps are clipped to the image before any
// address is formed.  Streaming kernels: no LDS, no atomics.
#include "ca_common.h"

namespace {

struct PoolGeom {
  int N, H, W, C, KH, KW, sh, sw, pad_top, pad_left, OH, OW;
};

template <int VW>
__device__ __forceinline__ void pl_ld(const bf16_t* __restrict__ p, float (&f)[VW]) {
  if constexpr (VW == 8) {
    const us8 u = *reinterpret_cast<const us8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f(u[j]);
  } else {
    f[0] = bf2f(*p);
  }
}

template <int VW>
__device__ __forceinline__ void pl_st(bf16_t* __restrict__ p, const float (&f)[VW]) {
  if constexpr (VW == 8) {
    us8 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = f2bf(f[j]);
    *reinterpret_cast<us8*>(p) = u;
  } else {
    *p = f2bf(f[0]);
  }
}

// in-image taps [k0, k1) of the window that starts at pixel `start` (may be negative) on an
// axis of n pixels with a k-tap window; non-empty for every window the launchers accept
__device__ __forceinline__ void pl_clip(int start, int k, int n, int& k0, int& k1) {
  k0 = start < 0 ? -start : 0;
  k1 = n - start < k ? n - start : k;
}

// windows [o0, o1] that read pixel i: o * s - pad <= i <= o * s - pad + k - 1, within [0, on - 1].
// The ceil's numerator is negative near the top / left edge: clamped to window 0 before dividing.
__device__ __forceinline__ void pl_cover(int i, int pad, int k, int s, int on, int& o0, int& o1) {
  const int a = i + pad - k + 1;
  o0 = a <= 0 ? 0 : (a + s - 1) / s;
  o1 = (i + pad) / s;  // i + pad >= 0
  if (o1 > on - 1) o1 = on - 1;
}

template <int VW>
__global__ void __launch_bounds__(256) pool_max_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                          uint8_t* __restrict__ idx, PoolGeom g) {
  const uint32_t CT = g.C / VW;
  const uint32_t total = (uint32_t)g.N * g.OH * g.OW * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int ow = (int)(r % (uint32_t)g.OW);
    r /= (uint32_t)g.OW;
    const int oh = (int)(r % (uint32_t)g.OH);
    const int n = (int)(r / (uint32_t)g.OH);
    const int h0 = oh * g.sh - g.pad_top, w0 = ow * g.sw - g.pad_left;
    int kh0, kh1, kw0, kw1;
    pl_clip(h0, g.KH, g.H, kh0, kh1);
    pl_clip(w0, g.KW, g.W, kw0, kw1);
    float best[VW];
    int bi[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      best[j] = -INFINITY;
      bi[j] = kh0 * g.KW + kw0;  // the first in-image tap
    }
    for (int kh = kh0; kh < kh1; ++kh) {
      const bf16_t* xr = x + ((long)n * g.H + (h0 + kh)) * g.W * g.C + vc * VW;
      for (int kw = kw0; kw < kw1; ++kw) {
        float v[VW];
        pl_ld<VW>(xr + (long)(w0 + kw) * g.C, v);
        const int tap = kh * g.KW + kw;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          if (v[j] > best[j]) {
            best[j] = v[j];
            bi[j] = tap;
          }
        }
      }
    }
    const long oo = (long)t * VW;  // t enumerates (n, oh, ow, vc) in storage order
    pl_st<VW>(y + oo, best);
    if constexpr (VW == 8) {
      uint64_t packed = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) packed |= (uint64_t)bi[j] << (8 * j);
      *reinterpret_cast<uint64_t*>(idx + oo) = packed;
    } else {
      idx[oo] = (uint8_t)bi[0];
    }
  }
}

template <int VW>
__global__ void __launch_bounds__(256) pool_max_bwd_kernel(const bf16_t* __restrict__ dy,
                                                          const uint8_t* __restrict__ idx, bf16_t* __restrict__ dx,
                                                          PoolGeom g) {
  const uint32_t CT = g.C / VW;
  const uint32_t total = (uint32_t)g.N * g.H * g.W * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int w = (int)(r % (uint32_t)g.W);
    r /= (uint32_t)g.W;
    const int h = (int)(r % (uint32_t)g.H);
    const int n = (int)(r / (uint32_t)g.H);
    int oh0, oh1, ow0, ow1;
    pl_cover(h, g.pad_top, g.KH, g.sh, g.OH, oh0, oh1);
    pl_cover(w, g.pad_left, g.KW, g.sw, g.OW, ow0, ow1);
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh) {
      const int kh = h + g.pad_top - oh * g.sh;  // in [0, KH)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int kw = w + g.pad_left - ow * g.sw;  // in [0, KW)
        const uint32_t want = (uint32_t)(kh * g.KW + kw);
        const long oo = (((long)n * g.OH + oh) * g.OW + ow) * g.C + vc * VW;
        float gv[VW];
        pl_ld<VW>(dy + oo, gv);
        if constexpr (VW == 8) {
          const uint64_t b = *reinterpret_cast<const uint64_t*>(idx + oo);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if ((uint32_t)((b >> (8 * j)) & 0xff) == want) acc[j] += gv[j];
        } else {
          if ((uint32_t)idx[oo] == want) acc[0] += gv[0];
        }
      }
    }
    pl_st<VW>(dx + (long)t * VW, acc);  // t enumerates (n, h, w, vc) in storage order
  }
}

template <int VW>
__global__ void __launch_bounds__(256) pool_avg_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                          PoolGeom g) {
  const uint32_t CT = g.C / VW;
  const uint32_t total = (uint32_t)g.N * g.OH * g.OW * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int ow = (int)(r % (uint32_t)g.OW);
    r /= (uint32_t)g.OW;
    const int oh = (int)(r % (uint32_t)g.OH);
    const int n = (int)(r / (uint32_t)g.OH);
    const int h0 = oh * g.sh - g.pad_top, w0 = ow * g.sw - g.pad_left;
    int kh0, kh1, kw0, kw1;
    pl_clip(h0, g.KH, g.H, kh0, kh1);
    pl_clip(w0, g.KW, g.W, kw0, kw1);
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
    for (int kh = kh0; kh < kh1; ++kh) {
      const bf16_t* xr = x + ((long)n * g.H + (h0 + kh)) * g.W * g.C + vc * VW;
      for (int kw = kw0; kw < kw1; ++kw) {
        float v[VW];
        pl_ld<VW>(xr + (long)(w0 + kw) * g.C, v);
#pragma unroll
        for (int j = 0; j < VW; ++j) acc[j] += v[j];
      }
    }
    const float inv = 1.f / (float)((kh1 - kh0) * (kw1 - kw0));  // >= 1 tap
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] *= inv;
    pl_st<VW>(y + (long)t * VW, acc);
  }
}

template <int VW>
__global__ void __launch_bounds__(256) pool_avg_bwd_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                                                          PoolGeom g) {
  const uint32_t CT = g.C / VW;
  const uint32_t total = (uint32_t)g.N * g.H * g.W * CT;  // < 2^31: checked by the launcher
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int vc = (int)(t % CT);
    uint32_t r = t / CT;
    const int w = (int)(r % (uint32_t)g.W);
    r /= (uint32_t)g.W;
    const int h = (int)(r % (uint32_t)g.H);
    const int n = (int)(r / (uint32_t)g.H);
    int oh0, oh1, ow0, ow1;
    pl_cover(h, g.pad_top, g.KH, g.sh, g.OH, oh0, oh1);
    pl_cover(w, g.pad_left, g.KW, g.sw, g.OW, ow0, ow1);
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh) {
      int k0, k1;
      pl_clip(oh * g.sh - g.pad_top, g.KH, g.H, k0, k1);
      const int rows = k1 - k0;
      const bf16_t* gr = dy + (((long)n * g.OH + oh) * g.OW) * g.C + vc * VW;
      for (int ow = ow0; ow <= ow1; ++ow) {
        pl_clip(ow * g.sw - g.pad_left, g.KW, g.W, k0, k1);
        const float inv = 1.f / (float)(rows * (k1 - k0));  // the window reads (h, w): >= 1 tap
        float gv[VW];
        pl_ld<VW>(gr + (long)ow * g.C, gv);
#pragma unroll
        for (int j = 0; j < VW; ++j) acc[j] = fmaf(gv[j], inv, acc[j]);
      }
    }
    pl_st<VW>(dx + (long)t * VW, acc);
  }
}

// every condition the kernels rely on; nothing is launched unless it holds
bool pool_geom_ok(const PoolGeom& g) {
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.C < 1 || g.OH < 1 || g.OW < 1) return false;
  if (g.KH < 1 || g.KW < 1 || g.KH > 255 || g.KW > 255 || g.KH * g.KW > 255) return false;  // the argmax byte
  if (g.sh < 1 || g.sw < 1) return false;
  if (g.pad_top < 0 || g.pad_top >= g.KH || g.pad_left < 0 || g.pad_left >= g.KW) return false;
  // the last window starts inside the image, so every window holds an in-image tap
  if ((long)(g.OH - 1) * g.sh - g.pad_top > g.H - 1 || (long)(g.OW - 1) * g.sw - g.pad_left > g.W - 1) return false;
  // 32-bit thread and pixel indices in both directions
  return (long)g.N * g.H * g.W * g.C < (1L << 31) && (long)g.N * g.OH * g.OW * g.C < (1L << 31);
}

bool pool_vec(const PoolGeom& g, const void* a, const void* b, const void* c = nullptr) {
  return g.C % 8 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                           reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace

extern "C" {

int ca_pool2d_max_fwd(const bf16_t* x, bf16_t* y, uint8_t* idx, int N, int H, int W, int C, int KH, int KW, int sh,
                      int sw, int pad_top, int pad_left, int OH, int OW, hipStream_t st) {
  const PoolGeom g{N, H, W, C, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!pool_geom_ok(g) || !x || !y || !idx) return -1;
  const long out = (long)N * OH * OW * C;
  if (pool_vec(g, x, y, idx)) pool_max_fwd_kernel<8><<<ca_stream_grid(out / 8, 256), 256, 0, st>>>(x, y, idx, g);
  else pool_max_fwd_kernel<1><<<ca_stream_grid(out, 256), 256, 0, st>>>(x, y, idx, g);
  CA_LAUNCH_CHECK();
  return 0;
}

int ca_pool2d_max_bwd(const bf16_t* dy, const uint8_t* idx, bf16_t* dx, int N, int H, int W, int C, int KH, int KW,
                      int sh, int sw, int pad_top, int pad_left, int OH, int OW, hipStream_t st) {
  const PoolGeom g{N, H, W, C, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!pool_geom_ok(g) || !dy || !idx || !dx) return -1;
  const long in = (long)N * H * W * C;
  if (pool_vec(g, dy, dx, idx)) pool_max_bwd_kernel<8><<<ca_stream_grid(in / 8, 256), 256, 0, st>>>(dy, idx, dx, g);
  else pool_max_bwd_kernel<1><<<ca_stream_grid(in, 256), 256, 0, st>>>(dy, idx, dx, g);
  CA_LAUNCH_CHECK();
  return 0;
}

int ca_pool2d_avg_fwd(const bf16_t* x, bf16_t* y, int N, int H, int W, int C, int KH, int KW, int sh, int sw,
                      int pad_top, int pad_left, int OH, int OW, hipStream_t st) {
  const PoolGeom g{N, H, W, C, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!pool_geom_ok(g) || !x || !y) return -1;
  const long out = (long)N * OH * OW * C;
  if (pool_vec(g, x, y)) pool_avg_fwd_kernel<8><<<ca_stream_grid(out / 8, 256), 256, 0, st>>>(x, y, g);
  else pool_avg_fwd_kernel<1><<<ca_stream_grid(out, 256), 256, 0, st>>>(x, y, g);
  CA_LAUNCH_CHECK();
  return 0;
}

int ca_pool2d_avg_bwd(const bf16_t* dy, bf16_t* dx, int N, int H, int W, int C, int KH, int KW, int sh, int sw,
                      int pad_top, int pad_left, int OH, int OW, hipStream_t st) {
  const PoolGeom g{N, H, W, C, KH, KW, sh, sw, pad_top, pad_left, OH, OW};
  if (!pool_geom_ok(g) || !dy || !dx) return -1;
  const long in = (long)N * H * W * C;
  if (pool_vec(g, dy, dx)) pool_avg_bwd_kernel<8><<<ca_stream_grid(in / 8, 256), 256, 0, st>>>(dy, dx, g);
  else pool_avg_bwd_kernel<1><<<ca_stream_grid(in, 256), 256, 0, st>>>(dy, dx, g);
  CA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
