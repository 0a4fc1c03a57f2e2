// Patch-fed implicit GEMM for stride-1 / pad-1 3x3 convolutions (forward and input gradient)
// with a 64-multiple gathered channel count and W <= PATCH_MAXW.
//
// The single-stage LDS-DMA core (mfma_gemm_glds, 128 x 128 tile, 2 x 2 waves) fetches the A
// tile of every K step, i.e. 16 KiB per (tap, 64-channel chunk): the same input rows nine
// times over, once per tap.  For a tile of 128 consecutive output pixels m0 .. m0 + 127
// (flattened (n, y, x); input and output share H x W) tap (kh, kw) reads the CONTIGUOUS input
// row range shifted by (kh - 1) * W + (kw - 1), so one dense copy of rows
//   [m0 - W - 1, m0 + 127 + W + 1]          ("the patch", 128 + 2 W + 2 rows x 128 B)
// per 64-channel chunk serves all nine taps.  The K order becomes (chunk outer, tap inner);
// the B loaders are stateless in k0 and take the reordered k0 unchanged.
//
//   per tile and chunk:  9 x (16 + 16) KiB = 288 KiB of LDS fill   (tap-gathered A)
//                        patch (<= 24 KiB) + 9 x 16 KiB <= 168 KiB   (this core)
//
// Loop shape, threads, LDS stage count are those of mfma_gemm_glds: DMA -> s_waitcnt vmcnt(0)
// -> barrier -> 32 MFMAs per wave -> barrier; at most 40 KiB of LDS (24 KiB patch at W <= 28,
// 20 KiB at W <= 14, plus 16 KiB B; the epilogue staging aliases them) keeps four workgroups
// per CU.
//
// Patch image: row-major [row][64] bf16 with the 16-B chunk slot XOR-swizzled by row & 7, as
// the K-contiguous tiles of the glds core -- ds_read_b128 fragment reads of 16 consecutive
// rows stay conflict-free at any row shift.  The DMA goes through a buffer resource whose
// span is the tensor: rows before its start or past its end read as zeros, and so do the
// rows past the patch (>= 128 + 2 W + 2), whose lanes are given an out-of-range offset; the
// first of those is the ZERO ROW.  Border handling: a per-lane 9-bit mask per fragment row
// (tap inside the image, row < M), computed once per tile; a fragment read of an invalid
// (row, tap) is redirected to the zero row.  The data is never multiplied by zero: the rows
// that a border tap would otherwise pick up are real pixels of the neighbouring image row or
// image and may hold NaN / Inf.
#pragma once
#include "ca_mfma_core.h"

namespace ca {

constexpr int PATCH_MAXW = 28;
// LDS rows of the patch image for width W: the 128 + 2 W + 2 pixel rows and the zero row, in
// whole 32-row DMA groups (192 rows = 24 KiB up to W = 28, 160 rows = 20 KiB up to W = 14)
constexpr int patch_rows(int W) { return (128 + 2 * W + 2) / 32 * 32 + 32; }

// DGRAD = false: forward, A = X, tap (kh, kw) of output pixel m reads input row m + (kh-1) W + (kw-1)
// DGRAD = true : input gradient, A = dY, tap (kh, kw) of input pixel m reads dY row m + (1-kh) W + (1-kw)
// P.A is the gathered tensor [Nb, H, W, C], C = P.K / 9 (a multiple of BK), host-checked:
// 3x3 / s1 / p1, patch_rows(W) <= PATCH_ROWS, Nb * H * W * C * 2 < BUF_CAP.
template <int PATCH_ROWS, bool DGRAD, template <int, int, int> class LBT, int EPI, int EPF = 1>
__device__ __forceinline__ void conv_patch_gemm(const CoreParams& P) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2, NT = 256, FM = 4, FN = 4;
  constexpr int A_ELEMS = PATCH_ROWS * BK, B_ELEMS = BN * BK;
  constexpr int SMEM = A_ELEMS + B_ELEMS;
  constexpr int CPB = B_ELEMS / 8 / NT;
  constexpr int MAX_ISSUE = PATCH_ROWS / (NT / 8);
  static_assert(SMEM >= BM * EpiLayout<BN>::LD, "the epilogue staging must fit the K stage");
  static_assert(PATCH_ROWS % (NT / 8) == 0 && PATCH_ROWS <= patch_rows(PATCH_MAXW), "patch rows");
  using LB = LBT<BN, CPB, NT>;
  constexpr bool B_KC = LB::KC;
  __shared__ __attribute__((aligned(16))) short smem[SMEM];
  short* const Bs = smem + A_ELEMS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (P.N + BN - 1) / BN;
  const BlkPos bp = blk_pos(P);
  const int tm = bp.tile / tiles_n, tn = bp.tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int W = P.W, H = P.H;
  const int C = P.K / 9;  // gathered channels
  const int need = BM + 2 * W + 2;        // patch rows that hold pixels; row `need` is the zero row
  const int n_issue = need / (NT / 8) + 1;  // 32 rows per workgroup DMA; covers the zero row

  LB lb(P, false, n0, tid);
  const auto rb = loader_rsrc(lb);
  // A: the whole gathered tensor behind one resource
  const uint32_t a_span = buf_span((long)P.M * C * 2);
  const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(P.A), (short)0, (int)a_span, 0x00020000);

  // patch DMA: lane -> (row_t + 32 i, swizzled chunk); row & 7 is the same for every i
  const int row_t = tid >> 3;
  const int pcol = ((tid & 7) ^ (row_t & 7)) << 3;
  const long pix0 = (long)m0 - W - 1 + row_t;  // pixel of patch row row_t
  auto issue_patch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < MAX_ISSUE; ++i) {
      if (i < n_issue) {
        const long pix = pix0 + i * (NT / 8);
        const bool ok = pix >= 0 && pix < (long)P.M && (row_t + i * (NT / 8)) < need;
        const uint32_t o = ok ? (uint32_t)((pix * C + c0 + pcol) * 2) : a_span;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(smem + (i * NT + wave * 64) * 8), 16, o, 0, 0, 0);
      }
    }
  };
  auto issue_b = [&](int k0) {
#pragma unroll
    for (int i = 0; i < CPB; ++i) CA_DMA_CHUNK(LB, lb, rb, i, k0, Bs + (i * NT + wave * 64) * 8);
  };

  // per-lane border masks of the four fragment rows: bit kh * 3 + kw set = tap inside the image
  const int frow0 = wm * (BM / WM) + (lane & 15);
  uint32_t vmask[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + frow0 + i * 16;
    uint32_t mask = 0;
    if (m < P.M) {
      const uint32_t t = fdiv((uint32_t)m, P.div_w);
      const int x = m - (int)t * W;
      const int y = (int)t - (int)fdiv(t, P.div_h) * H;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int yy = DGRAD ? y + 1 - kh : y + kh - 1, xx = DGRAD ? x + 1 - kw : x + kw - 1;
          if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) mask |= 1u << (kh * 3 + kw);
        }
    }
    vmask[i] = mask;
  }
  const int zoff = need * BK;  // zero row (shorts)
  const int g = lane >> 4;

  f4v acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f4v{0.f, 0.f, 0.f, 0.f};

  // one tap: A fragments from patch rows frow + shift, B fragments as in mfma_gemm_glds
  auto compute = [&](int tap, int shift) {
    const int pr0 = frow0 + shift;
    const int sw = pr0 & 7;  // rows 16 apart share row & 7
#pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      bf16x8 af[FM], bfr[FN];
      const int base = pr0 * BK + ((((kk >> 3) + g) ^ sw) << 3);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int a = ((vmask[i] >> tap) & 1u) ? base + i * 16 * BK : zoff;
        af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const s8v*>(smem + a));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) bfr[j] = read_frag_sw<BN, B_KC>(Bs, wn * (BN / WN) + j * 16, kk, lane);
      mfma_acc<FM, FN>(acc, af, bfr);
    }
  };

  // (A second B stage -- the B tile of step s + 1 in flight under the MFMAs of step s, one
  // barrier per step -- costs 16 KiB, i.e. three workgroups per CU: measured equal forward and
  // 7-14 % slower on the input gradient at W = 14 / 7, docs/performance.md, and removed.)
  for (int c0 = 0; c0 < C; c0 += BK) {
    int kh = 0, kw = 0;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      if (tap == 0) issue_patch(c0);
      issue_b(tap * C + c0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      compute(tap, DGRAD ? (2 - kh) * W + (2 - kw) : kh * W + kw);
      __syncthreads();
      if (++kw == 3) {
        kw = 0;
        ++kh;
      }
    }
  }
  gemm_epilogue<BM, BN, WM, WN, EPI, SMEM, EPF, FM, FN>(P, acc, smem, m0, n0, tm, tid);
}

}  // namespace ca
