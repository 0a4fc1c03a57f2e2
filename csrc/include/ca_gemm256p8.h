// 256 x 256 x 64 MFMA GEMM core over a double-buffered LDS-DMA image, two staggered wave
// groups, counted vmcnt (gfx950 / CDNA4).
//
//   C[M,N] = sum_k A(m,k) * B(k,n)     bf16 operands, fp32 accumulation
//
// Geometry: one 512-thread workgroup per CU (2 waves per SIMD), K tile 64 deep.  The LDS
// holds two K tiles, each as four 16 KB half tiles: A top / bottom (128 rows x 64 k) and
// B left / right (128 columns x 64 k) -- 128 KB.  Waves are 2 (M) x 4 (N); every phase is
// {fragment reads; s_waitcnt lgkmcnt(0); LDS-DMA of restaged half tiles (2 pieces per thread
// each); counted vmcnt} barrier {MFMAs at s_setprio 1} barrier, and waves 4-7 run one barrier
// behind waves 0-3, so on every SIMD one wave multiplies while its partner reads LDS and
// issues DMA (MI355X_MICROARCH.md "Two waves per SIMD").  Because each phase retires its own
// LDS reads before its first barrier, a half tile is restaged ONE phase after its last read;
// a half tile's data is waited for (counted vmcnt) before the first barrier of a phase that
// precedes the phase reading it (cdna_hip_programming.md section 5, RAW / WAR rules with the
// stagger).  The loop never drains vmcnt to 0.
//
// Two phases per K tile: one C HALF per phase, 32 MFMAs per wave between barriers.
//   K tile t, buffer b = t & 1     reads (buffer b)                 DMA issued
//     P1 top half    (qm 0)        A top, B left, B right           A bottom of t+1 (buffer b^1)
//     P2 bottom half (qm 1)        A bottom (B held in registers)   A top, B left, B right of t+2
//                                                                   (buffer b); vmcnt(6) -> t+1 complete
//
// Measured on MI355X, one process, random operands (bin/gemm_bench, profiles/r4_gemm/):
// 1,178-1,228 TF/s at 4096^3 and 1,245-1,260 at 8192^3 (MFMA busy 0.70); a four-phase schedule
// (one C quadrant, 16 MFMAs, per phase) reached 1,050-1,110 / 1,168-1,190 (busy 0.61) and the
// earlier 256 x 256 ring core 1,097-1,158 / 1,172-1,183 (busy 0.65) -- both removed, numbers in
// docs/performance.md.  Variants that waited for each half tile one phase before it is
// read (four half tiles in flight) or rotated A bottom over three slots (144 KB) gave the
// half-tile loads more latency budget and were NOT faster: the barrier count per MFMA, not the
// load latency, is what the extra MFMAs per phase buy back.  Epilogue: the shared
// gemm_epilogue with the quadrant fragment mapping (QUAD).
#pragma once
#include "ca_mfma_core.h"

namespace ca {

// The two-phase K loop for ONE 256 x 256 tile at (m0, n0) over K elements [kbeg, kend), into
// `acc` (zeroed here), on the 128-KB operand image `smem`.  Returns with both wave groups
// re-aligned and every LDS read retired (__syncthreads): the caller may reuse the LDS.
// (A static member, not a free function template: as a free function the host pass of gemm.hip
// finds no viable candidate for the call below, while gemm_bench.hip compiles either way.)
template <template <int, int, int> class LAT, template <int, int, int> class LBT>
struct P8Loop {
__device__ static __forceinline__ void run(const CoreParams& P, int m0, int n0, int kbeg, int kend, short* smem,
                                           f4v (&acc)[8][4]) {
  constexpr int NT = 512, HR = 128;
  constexpr int HT = HR * BK;  // shorts per half tile
  using LA = LAT<HR, 2, NT>;
  using LB = LBT<HR, 2, NT>;
  static_assert(!loader_stateful<LA>::value && !loader_stateful<LB>::value, "stateless loaders only");
  constexpr bool A_KC = LA::KC, B_KC = LB::KC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / 4, wn = wave % 4;
  const int grp = __builtin_amdgcn_readfirstlane(wave) >> 2;
  const int nk = (kend - kbeg + BK - 1) / BK;

  const LA la0(P, true, m0, tid), la1(P, true, m0 + HR, tid);
  const LB lb0(P, false, n0, tid), lb1(P, false, n0 + HR, tid);
  const auto ra0 = loader_rsrc(la0), ra1 = loader_rsrc(la1);
  const auto rb0 = loader_rsrc(lb0), rb1 = loader_rsrc(lb1);

  // half tile h of buffer b: 0 A top, 1 A bottom, 2 B left, 3 B right
  auto region = [&](int b, int h) { return smem + (b * 4 + h) * HT; };
  auto dma = [&](int t, int h) {
    const int k0 = kbeg + t * BK;
    short* dst = region(t & 1, h);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      short* d = dst + (i * NT + wave * 64) * 8;
      if (h == 0) CA_DMA_CHUNK(LA, la0, ra0, i, k0, d);
      else if (h == 1) CA_DMA_CHUNK(LA, la1, ra1, i, k0, d);
      else if (h == 2) CA_DMA_CHUNK(LB, lb0, rb0, i, k0, d);
      else CA_DMA_CHUNK(LB, lb1, rb1, i, k0, d);
    }
  };
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4v{0.f, 0.f, 0.f, 0.f};
  // fragments: A 4 rows x 2 k halves of one A half tile; B 2 cols x 2 k halves of the left
  // (bfl) and right (bfr) B half tiles
  bf16x8 af[4][2], bfl[2][2], bfr[2][2];
  auto read_a = [&](const short* half) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) af[i][kk] = read_frag_sw<HR, A_KC>(half, wm * 64 + i * 16, kk * 32, lane);
  };
  auto read_b = [&](bf16x8 (&f)[2][2], const short* half) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) f[j][kk] = read_frag_sw<HR, B_KC>(half, wn * 32 + j * 16, kk * 32, lane);
  };
  // C half qm (quadrants (qm,0), (qm,1)) from af, bfl and bfr: 32 MFMAs
  auto mfma_h = [&](int qm) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[qm * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(j < 2 ? bfl[j][kk] : bfr[j - 2][kk], af[i][kk],
                                                                       acc[qm * 4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // prologue: K tile 0, and tile 1's A top / B left / B right (what "P2 of tile -1" issues)
  if (nk > 0) {
    dma(0, 0);
    dma(0, 2);
    dma(0, 3);
    dma(0, 1);
  }
  if (nk > 1) {
    dma(1, 0);
    dma(1, 2);
    dma(1, 3);
    vm_wait<6>();
  } else {
    vm_wait<0>();
  }
  bar256();
  if (grp == 1) bar256();
  for (int t = 0; t < nk; ++t) {
    const int b = t & 1;
    // P1: top C half
    read_a(region(b, 0));
    read_b(bfl, region(b, 2));
    read_b(bfr, region(b, 3));
    lgkm_wait0();
    if (t + 1 < nk) dma(t + 1, 1);
    bar256();
    mfma_h(0);
    bar256();
    // P2: bottom C half; K tile t+1 must be complete before the next P1 reads it
    read_a(region(b, 1));
    lgkm_wait0();
    if (t + 2 < nk) {
      dma(t + 2, 0);
      dma(t + 2, 2);
      dma(t + 2, 3);
      vm_wait<6>();
    } else {
      vm_wait<0>();
    }
    bar256();
    mfma_h(1);
    bar256();
  }
  if (grp == 0) bar256();
  __syncthreads();
}
};

template <template <int, int, int> class LAT, template <int, int, int> class LBT, int EPI>
__device__ __forceinline__ void mfma_gemm_256p8(const CoreParams& P) {
  constexpr int BM = 256, BN = 256, HR = 128;
  constexpr int SMEM = 8 * HR * BK;  // 2 buffers x 4 half tiles = 128 KB
  static_assert(SMEM >= BM * EpiLayout<BN>::LD, "C staging must fit the operand image");
  constexpr int FM = 8, FN = 4;  // accumulator fragments per wave (2 x 2 quadrants of 4 x 2)
  __shared__ __attribute__((aligned(16))) short smem[SMEM];

  const int tid = threadIdx.x;
  const int tiles_m = (P.M + BM - 1) / BM, tiles_n = (P.N + BN - 1) / BN;
  const BlkPos bp = blk_pos(P);
  int tm, tn;
  tile256_coords(bp.tile, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = bp.split * P.k_per_split;
  int kend = kbeg + P.k_per_split;
  if (kend > P.K) kend = P.K;

  f4v acc[FM][FN];
  P8Loop<LAT, LBT>::run(P, m0, n0, kbeg, kend, smem, acc);
  gemm_epilogue<BM, BN, 2, 4, EPI, SMEM, 1, FM, FN, true>(P, acc, smem, m0, n0, tm, tid);
}

}  // namespace ca
