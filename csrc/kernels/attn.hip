// Fused multi-head attention (K13 in SURVEY.md 2.7) for head_dim D = 32, 64 or 128 on MFMA.
//
// Layout: the QKV projection output qkv[B*S][3*H*D] (Q | K | V, head h at
// columns h*D inside each third) is consumed in place -- no head split /
// transpose copies; the context is written to ctx[B*S][H*D].
//
// Forward (one workgroup = 64 queries of one (batch, head), 4 waves x 16 rows):
//   S = Q K^T * scale over 64-key blocks, online softmax in registers (exp2
//   domain), key-padding mask from key_len[b], attention-probability dropout
//   from the stateless hash (ca_rng.h), O += P V; P goes C-layout -> LDS -> A
//   fragments (one 2.3 KB slab per wave).  Log-sum-exp per row is kept for
//   the backward.  Q fragments are loaded straight from HBM into registers.
//
// Backward = three kernels, no atomics:
//   prep : Dv[q] = rowsum(dO * O)
//   dKV  : per 64-key block, loop over query blocks: S^T, P^T, dV += Pd^T dO,
//          dP^T = V dO^T, dS^T = P^T (dP^T*mask - Dv), dK += dS^T Q
//   dQ   : per 64-query block, loop over key blocks: dQ += dS K
// MFMA: v_mfma_f32_16x16x32_bf16; K-contiguous operands via ds_read_b128,
// N-contiguous ones (V / dO / Q / K as B with k along rows) via ds_read_b64_tr_b16.
//
// Kernels: one generic family (forward, dK/dV, dQ; templates on TAIL, MASK, CAUSAL; see GenArgs)
// that serves self-attention on the packed qkv and cross-attention on separate q and kv, two
// one-workgroup kernels for self-attention at S = 64 / 128 (below), and the prep kernel.
//
// Head dim: a compile-time parameter HD of the generic family and of the prep kernel.  Query and
// key blocks are 64 x 64 at every HD, so masks, causal skipping, block_x, the tail rules and the
// dropout element index do not depend on it.  What scales: the contractions over the head dim
// (Q K^T, V dO^T) take HD / 32 MFMA steps in ascending order, the outputs (P V, dV, dK, dQ) have
// HD / 16 tiles, the 64-row LDS tiles are 64 x HD at pitch HD + 8, and the outputs are staged
// through the per-wave 16 x 72 slabs in 64-column halves at HD = 128.  The HD = 64 instantiations
// are, instruction for instruction, the code from before the parameter existed; the one-workgroup
// kernels are HD = 64 only.
//
// Shapes: any S; self-attention with D = 64 at S = 64 / 128 takes the one-workgroup kernels, every
// other call the generic ones on ceil(S / 64) blocks.  S % 64 != 0 runs their TAIL instantiation, which
// only masks: fragment rows >= S are clamped to row S - 1, tile rows >= S are zero-filled in LDS,
// lse / Dv of queries >= S are not read (dKV: p = dS = 0 for those columns), and only rows
// < S are stored.
//
// Causal mode (CAUSAL, a compile-time parameter of the generic and the one-workgroup kernels; the
// non-causal instantiations are the code without it): key j is visible to query i iff j <= i and
// j < key_len[b], so key 0 is visible to every query and no row is fully masked.  The generic
// kernels skip the 64x64 blocks that lie entirely in the future -- forward and dQ stop after the
// diagonal key block, dK/dV starts at the diagonal query block, all bounds workgroup-uniform --
// and test key <= q per element in the diagonal block only.  The one-workgroup kernels mask per
// element; the forward one also skips the MFMA steps that are entirely in the future of a wave's
// rows, the fused backward does not (at S = 128 it sits at its 128-register budget, and every
// wave-dependent skip tried there spilled).  A masked element is exactly p = 0, dS = 0.  The
// dropout element index is the same in both modes.
//
// Cross-attention (queries and keys / values in separate tensors, own lengths and row pitches)
// runs on the generic kernels as well: see GenArgs.  They also take an arbitrary byte mask (MASK,
// a compile-time parameter like TAIL), non-causal only; masked self-attention comes in through the
// cross-attention entry points, on the Q and K | V column views of the packed qkv.
#include "ca_mfma_core.h"
#include "ca_rng.h"

namespace {
using namespace ca;

constexpr int D = 64;     // head dim of the one-workgroup kernels (the generic ones: template HD)
constexpr int QB = 64;    // queries per workgroup
constexpr int KB = 64;    // keys per block
constexpr int LDT = 72;   // LDS row pitch (64 + 8 pad) of every 64x64 tile
constexpr int PLD = 72;   // per-wave P / dS slab pitch
constexpr float LOG2E = 1.4426950408889634f;

// TAIL (S % 64 != 0): only the first `nrows` (>= 1) rows exist; the others are zero-filled in
// LDS, not read -- they are MFMA operands, and 0 x (whatever lies behind the tensor) may be NaN.
template <bool TAIL, int HD>
__device__ __forceinline__ void tile_load(short* lds, const bf16_t* g, long ld, int tid, int nrows) {
  // 64 rows x HD bf16 (HD / 8 chunks of 16 B per row) at pitch HD + 8: 8 HD chunks, HD / 32 per thread
  constexpr int CPR = HD / 8, CSH = HD == 32 ? 2 : (HD == 64 ? 3 : 4), LDH = HD + 8;
#pragma unroll
  for (int i = 0; i < HD / 32; ++i) {
    const int c = tid + i * 256;
    const int r = c >> CSH, col = (c & (CPR - 1)) * 8;
    if constexpr (TAIL) {
      // branch-free (the tile's loads stay in flight together): a row past the end loads the
      // last existing row (nrows >= 1) and is then replaced by zeros
      const int rr = r < nrows ? r : nrows - 1;
      s8v v = *reinterpret_cast<const s8v*>(g + (long)rr * ld + col);
      if (r >= nrows) v = s8v{0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<s8v*>(lds + r * LDH + col) = v;
    } else {
      *reinterpret_cast<s8v*>(lds + r * LDH + col) = *reinterpret_cast<const s8v*>(g + (long)r * ld + col);
    }
  }
}

// Row of a fragment loaded straight from global memory: the tail variant clamps rows >= S to
// the last row (such a lane computes a copy of row S - 1; nothing of it is stored).
template <bool TAIL>
__device__ __forceinline__ int frag_row(int row, int S) {
  if constexpr (TAIL) return row < S ? row : S - 1;
  return row;
}

// C-layout 16 x 16 NT fp32 (NT <= 4 tiles) -> bf16 slab [16][PLD] of this wave
template <int NT>
__device__ __forceinline__ void slab_store(short* slab, const f4v (&v)[NT], int lane) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[((lane >> 4) * 4 + r) * PLD + t * 16 + (lane & 15)] = (short)f2bf(v[t][r]);
}

// A fragment (16 rows x 32 k, k-step kk) from a wave slab
__device__ __forceinline__ bf16x8 slab_frag(const short* slab, int kk, int lane) {
  s8v v = *reinterpret_cast<const s8v*>(slab + (lane & 15) * PLD + kk * 32 + 8 * (lane >> 4));
  return __builtin_bit_cast(bf16x8, v);
}

// A fragment straight from global rows (row-major, k contiguous)
__device__ __forceinline__ bf16x8 gfrag(const bf16_t* rowp, int kk, int lane) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const s8v*>(rowp + kk * 32 + 8 * (lane >> 4)));
}

// MFMA operand fragments of an LDS tile at row pitch LD (the lane mapping of read_frag in
// ca_mfma_core.h, which is tied to pitch 72): k contiguous ...
template <int LD>
__device__ __forceinline__ bf16x8 frag_kc(const short* lds, int r0, int k0, int lane) {
  s8v v = *reinterpret_cast<const s8v*>(lds + (r0 + (lane & 15)) * LD + k0 + 8 * (lane >> 4));
  return __builtin_bit_cast(bf16x8, v);
}
// ... and element (r, k) at lds[k * LD + r] (r contiguous): the transposed read
template <int LD>
__device__ __forceinline__ bf16x8 frag_nc(const short* lds, int r0, int k0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const short* b0 = lds + (k0 + 8 * g + q) * LD + r0 + 4 * p;
  s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(b0));
  s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(b0 + 4 * LD));
  s8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// Output staging of the generic kernels: C-layout 16 x HD fp32 (HD / 16 tiles) -> 16-B row stores,
// through the wave's [16][PLD] slab in column groups of SW = min(HD, 64): one group at HD <= 64,
// two 64-column halves at HD = 128 (wave barriers order a half's row reads before the next half's
// writes).  row_ok(r): row r of the wave's 16 exists.
template <int HD>
struct Stage {
  static constexpr int SW = HD < 64 ? HD : 64;  // columns per group
  static constexpr int NG = HD / SW;            // groups
  static constexpr int NT = SW / 16;            // C tiles per group
  static constexpr int CPR = SW / 8;            // 16-B chunks per row of a group
  static constexpr int CSH = SW == 32 ? 2 : 3;  // log2(CPR)
  static constexpr int NI = 16 * CPR / 64;      // chunks per lane
};
// Group G and the ones after it, as straight-line code (compile-time recursion, not a loop).
// One slab: row r of the wave's 16 is row `rowb + r` of dst (pitch ld), the head at column hoff,
// and exists iff row0 + r < lim.
template <int HD, bool TAIL, int G = 0>
__device__ __forceinline__ void stage_out(short* slab, const f4v (&v)[HD / 16], bf16_t* dst, long rowb, long ld,
                                          int hoff, int row0, int lim, int lane) {
  using St = Stage<HD>;
  if (G) __builtin_amdgcn_wave_barrier();  // the previous half's row reads precede these writes
  slab_store(slab, reinterpret_cast<const f4v(&)[St::NT]>(v[G * St::NT]), lane);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < St::NI; ++i) {
    const int c = lane + i * 64;  // 16 rows x CPR chunks
    const int r = c >> St::CSH, col = (c & (St::CPR - 1)) * 8;
    if (!TAIL || row0 + r < lim)
      *reinterpret_cast<s8v*>(dst + (rowb + r) * ld + hoff + G * St::SW + col) =
          *reinterpret_cast<const s8v*>(slab + r * PLD + col);
  }
  if constexpr (G + 1 < St::NG) stage_out<HD, TAIL, G + 1>(slab, v, dst, rowb, ld, hoff, row0, lim, lane);
}
// Two slabs (dK, dV): drow = row 0 of the wave's 16 in the K half, the V half C columns on
template <int HD, bool TAIL, int G = 0>
__device__ __forceinline__ void stage_out2(short* pslab, short* dslab, const f4v (&dk)[HD / 16],
                                           const f4v (&dv)[HD / 16], bf16_t* drow, long ld, int C, int row0, int lim,
                                           int lane) {
  using St = Stage<HD>;
  if (G) __builtin_amdgcn_wave_barrier();
  slab_store(pslab, reinterpret_cast<const f4v(&)[St::NT]>(dk[G * St::NT]), lane);
  slab_store(dslab, reinterpret_cast<const f4v(&)[St::NT]>(dv[G * St::NT]), lane);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < St::NI; ++i) {
    const int c = lane + i * 64;
    const int r = c >> St::CSH, col = (c & (St::CPR - 1)) * 8;
    if (!TAIL || row0 + r < lim) {
      *reinterpret_cast<s8v*>(drow + (long)r * ld + G * St::SW + col) =
          *reinterpret_cast<const s8v*>(pslab + r * PLD + col);
      *reinterpret_cast<s8v*>(drow + (long)r * ld + C + G * St::SW + col) =
          *reinterpret_cast<const s8v*>(dslab + r * PLD + col);
    }
  }
  if constexpr (G + 1 < St::NG) stage_out2<HD, TAIL, G + 1>(pslab, dslab, dk, dv, drow, ld, C, row0, lim, lane);
}

// The HD / 32 k-steps of a head-dim contraction, ascending, as compile-time recursion (each step's
// offsets are constants, as in hand-unrolled code): the A fragments of a global row ...
template <int NK, int KK = 0>
__device__ __forceinline__ void gfrags(bf16x8* f, const bf16_t* rowp, int lane) {
  f[KK] = gfrag(rowp, KK, lane);
  if constexpr (KK + 1 < NK) gfrags<NK, KK + 1>(f, rowp, lane);
}
// ... and acc += A[kk] x (rows r0 .. r0 + 15 of a k-contiguous LDS tile at pitch LD)
template <int LD, int NK, int KK = 0>
__device__ __forceinline__ void mfma_hd(f4v& acc, const bf16x8* af, const short* lds, int r0, int lane) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[KK], frag_kc<LD>(lds, r0, KK * 32, lane), acc, 0, 0, 0);
  if constexpr (KK + 1 < NK) mfma_hd<LD, NK, KK + 1>(acc, af, lds, r0, lane);
}

__device__ __forceinline__ float grp16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float grp16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The 64-row block of a workgroup of the generic kernels.  Causal work per workgroup grows
// (forward, dQ) or shrinks (dK/dV) with the block index, and the hardware hands consecutive
// workgroup ids to its XCDs and their shader engines round-robin: whenever gridDim.x divides that
// period, the same engine gets the longest block of every (batch, head), and the causal launch
// takes as long as the full one (measured: 1.00 x at S = 256 .. 2048).  So the block index is
// rotated by a multiplicative hash of the (batch, head) index: every engine then gets a random
// mix of lengths, whatever the period and gridDim.x (a plain rotation by the index still leaves
// gridDim.x = 2 and 4 at 1.00 x in a model of 32 round-robin engines; the hash stays within
// 0.03 of (n + 1) / 2n for n = 2 .. 32).  Workgroup-uniform.
template <bool CAUSAL>
__device__ __forceinline__ int block_x() {
  if constexpr (CAUSAL) {
    const uint32_t rot = ((blockIdx.y + gridDim.y * blockIdx.z) * 0x9E3779B1u) >> 16;
    return (int)((blockIdx.x + rot) % gridDim.x);
  }
  return (int)blockIdx.x;
}

// Arguments of the one-workgroup kernels and of the prep kernel (the generic kernels take GenArgs)
struct AttnArgs {
  const bf16_t* qkv;   // [B*S][3*H*D]
  const bf16_t* out;   // ctx [B*S][H*D] (bwd: O)
  const bf16_t* dout;  // dctx (bwd)
  bf16_t* ctx;         // fwd output
  bf16_t* dqkv;        // bwd output [B*S][3*H*D]
  float* lse;          // [B][H][S] (log2 domain)
  float* dvec;         // [B][H][S] rowsum(dO*O)
  const int* key_len;  // [B] or null
  int B, S, H;
  float scale;
  DropCfg drop;
};

// Dv[b,h,q] = sum_d dO[q, h*HD+d] * O[q, h*HD+d]: HD / 8 lanes x 8 elements per (row, head),
// 2048 / HD (row, head) pairs per workgroup
template <int HD>
__global__ void __launch_bounds__(256) attn_bwd_prep_kernel(AttnArgs a) {
  constexpr int D = HD, LPR = HD / 8;
  const long g = (long)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
  const int sub = threadIdx.x & (LPR - 1);
  const int H = a.H, S = a.S, C = H * D;
  const long rows = (long)a.B * S * H;
  if (g >= rows) return;
  const long row = g / H;  // b*S + q
  const int h = (int)(g - row * H);
  const bf16_t* po = a.out + row * C + h * D + sub * 8;
  const bf16_t* pd = a.dout + row * C + h * D + sub * 8;
  us8 uo = *reinterpret_cast<const us8*>(po), ud = *reinterpret_cast<const us8*>(pd);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += bf2f(uo[j]) * bf2f(ud[j]);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if constexpr (LPR > 4) s += __shfl_xor(s, 4, 64);
  if constexpr (LPR > 8) s += __shfl_xor(s, 8, 64);
  if (sub == 0) {
    const long b = row / S, q = row - b * S;
    a.dvec[(b * H + h) * S + q] = s;
  }
}

// ---------------------------------------------------------------------------
// The generic kernels <TAIL, MASK, CAUSAL>: T queries q[B*T][H*D] (row pitch ldq) against S keys /
// values packed as kv[B*S][2*H*D] (K | V, row pitch ldkv), gradients to dq (pitch lddq) and dkv
// (K | V, pitch lddkv).  Cross-attention passes two tensors, T and S independent, and contiguous
// gradients (lddq = C, lddkv = 2C).  Self-attention passes the column ranges of the packed
// projection: q = qkv, kv = qkv + C, dq = dqkv, dkv = dqkv + C, every pitch 3C, T == S.  Both run
// the same instantiation, so they store the same bits on the same rows.  Forward and dQ run on
// ceil(T / 64) query blocks and loop over the key blocks below key_len; dK/dV runs on
// ceil(S / 64) key blocks and loops over the query blocks.  TAIL = T or S is not a multiple of
// 64: every clamp, zero fill, lse / Dv guard and store guard uses the length of the tensor its
// rows come from.  The dropout element index is (b*H + h)*T*S + q*S + key.
//
// MASK: a byte per score, read through strides (0 = broadcast axis, key stride 1): the score of
// (b, h, q, key) takes part iff key < key_len[b] and mask[b*msb + h*msh + q*mst + key] != 0; key
// blocks at or past key_len are still not read.  A query that sees no key is possible then: its
// context is exactly 0, its lse is stored as 0, and it adds exactly 0 to dQ, dK and dV (the
// backward selects p = 0 for a hidden element, it never multiplies by a masked exp2f); a key no
// query sees gets exact-zero dK / dV rows.
//
// CAUSAL (needs T == S; the self-attention entry points are its only callers): see the header.
// Every statement of MASK and of CAUSAL is under its if constexpr, and the two are not combined:
// a masked causal call ANDs the triangle into its mask before it gets here.
struct GenArgs {
  const bf16_t* q;     // [B*T] rows of H*D, pitch ldq
  const bf16_t* kv;    // [B*S] rows of 2*H*D, pitch ldkv
  const bf16_t* dout;  // dctx [B*T][H*D] (bwd)
  bf16_t* ctx;         // fwd output [B*T][H*D]
  bf16_t* dq;          // bwd output [B*T] rows of H*D, pitch lddq
  bf16_t* dkv;         // bwd output [B*S] rows of 2*H*D, pitch lddkv
  float* lse;          // [B][H][T] (log2 domain)
  float* dvec;         // [B][H][T] rowsum(dO*O)
  const int* key_len;  // [B] or null
  long ldq, ldkv, lddq, lddkv;
  int B, T, S, H;
  float scale;
  DropCfg drop;
  const uint8_t* mask;  // MASK: element (b, h, q, key) at b*msb + h*msh + q*mst + key, != 0 = visible
  long msb, msh, mst;   // element strides; 0 = broadcast axis; (T - 1)*mst + S < 2^31
};

// MASK: the visibility bytes of a lane's 16 elements of a 64x64 score block, packed to bit 4t + r
// for the element of C tile t, register r.
//
// Forward and dQ (queries on rows): element (t, r) is row 4 (lane >> 4) + r, key 16 t + (lane & 15),
// so each of the 16 byte loads reads 16 consecutive bytes of 4 mask rows per wave, every byte of
// the tile once per workgroup, at any alignment of the rows (S is arbitrary).  Offsets inside a
// (batch, head) slice are 32-bit.  TAIL clamps the key to S - 1 (such an element is hidden by
// key < key_len already) and the offset to the slice's last byte (rows >= T compute copies that
// are never stored, whatever they see), so no byte past row T or key S is read.
// The loads are issued before the K / V tile loads of the block and packed after them.
struct MaskRaw {
  uint32_t v[16];
};
template <bool TAIL>
__device__ __forceinline__ MaskRaw mask_load_q(const uint8_t* mb, uint32_t mst, int row0, int k0, int T, int S, int lane) {
  MaskRaw m;
  if constexpr (TAIL) {
    const uint32_t last = (uint32_t)(T - 1) * mst + (uint32_t)(S - 1);  // the slice's last byte
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kc = k0 + t * 16 + (lane & 15);
      const uint32_t kt = (uint32_t)row0 * mst + (uint32_t)(kc < S ? kc : S - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t o = kt + (uint32_t)r * mst;  // rows >= T (never stored) read the last byte
        m.v[t * 4 + r] = mb[o < last ? o : last];
      }
    }
  } else {
    const uint32_t vb = (uint32_t)row0 * mst + (uint32_t)(lane & 15);  // the only per-lane, loop-invariant part
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t o = vb + ((uint32_t)k0 + (uint32_t)r * mst);
#pragma unroll
      for (int t = 0; t < 4; ++t) m.v[t * 4 + r] = mb[o + t * 16];
    }
  }
  return m;
}
__device__ __forceinline__ uint32_t mask_pack_q(const MaskRaw& m) {
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) bits |= (m.v[i] != 0 ? 1u : 0u) << i;
  // pin the packed word: without this the compiler tests the 16 bytes where the bits are used and
  // keeps them in registers through the whole block (the dQ kernel then spills)
  asm volatile("" : "+v"(bits));
  return bits;
}

// dK/dV (keys on rows): element (t, r) is key 4 (lane >> 4) + r of the wave's 16, query
// 16 t + (lane & 15).  Reading that directly would put the 16 lanes of a row group on 16 mask rows
// per load.  Instead load i reads the same shape as above -- queries 4 i + (lane >> 4), key
// (lane & 15) of the wave's 16: 16 consecutive bytes of 4 rows -- and the transpose is done on the
// wave's ballots: the 16 ballots are the wave's whole 64 x 16 visibility tile, bit 16 g' + c' of
// ballot i being query 4 i + g', key c'.  Lane (g, c) takes, for tile t, ballot 4 t + (c >> 2) and
// the 4 bits from 16 (c & 3) + 4 g.  No LDS, no alignment condition; TAIL clamps query and key.
template <bool TAIL>
__device__ __forceinline__ MaskRaw mask_load_k(const uint8_t* mb, uint32_t mst, int q0, int kw, int T, int S, int lane) {
  MaskRaw m;
  int key = kw + (lane & 15);
  if constexpr (TAIL) key = key < S ? key : S - 1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if constexpr (TAIL) {
      const int q = q0 + 4 * i + (lane >> 4);
      m.v[i] = mb[(uint32_t)(q < T ? q : T - 1) * mst + (uint32_t)key];
    } else {
      const uint32_t vb = (uint32_t)(lane >> 4) * mst + (uint32_t)key;  // the only per-lane, loop-invariant part
      m.v[i] = mb[vb + (uint32_t)(q0 + 4 * i) * mst];
    }
  }
  return m;
}
__device__ __forceinline__ uint32_t mask_pack_k(const MaskRaw& m, int lane) {
  const int sel = (lane & 15) >> 2, sh = 16 * (lane & 3) + 4 * (lane >> 4);
  uint32_t bits = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint64_t b0 = __ballot(m.v[4 * t] != 0), b1 = __ballot(m.v[4 * t + 1] != 0);
    const uint64_t b2 = __ballot(m.v[4 * t + 2] != 0), b3 = __ballot(m.v[4 * t + 3] != 0);
    const uint64_t w = sel == 0 ? b0 : (sel == 1 ? b1 : (sel == 2 ? b2 : b3));
    bits |= ((uint32_t)(w >> sh) & 0xFu) << (4 * t);
  }
  asm volatile("" : "+v"(bits));  // as in mask_pack_q
  return bits;
}

template <int HD, bool TAIL, bool MASK, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_fwd_kernel(GenArgs a) {
  static_assert(!(MASK && CAUSAL), "a masked causal call carries the triangle in its mask");
  constexpr int D = HD, LDH = HD + 8, NK = HD / 32, NO = HD / 16;  // k-steps of Q K^T, output tiles
  __shared__ __attribute__((aligned(16))) short Ks[KB * LDH];
  __shared__ __attribute__((aligned(16))) short Vs[KB * LDH];
  __shared__ __attribute__((aligned(16))) short Ps[4][16 * PLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int bx = block_x<CAUSAL>();
  const int T = a.T, S = a.S, H = a.H, C = H * D;
  const long ldkv = a.ldkv;
  const int q0 = bx * QB + wave * 16;
  int klen = a.key_len ? a.key_len[b] : S;
  klen = klen < 1 ? 1 : (klen > S ? S : klen);
  const bf16_t* kbase = a.kv + (long)b * S * ldkv + h * D;
  const bf16_t* qrow = a.q + ((long)b * T + frag_row<TAIL>(q0 + (lane & 15), T)) * a.ldq + h * D;
  bf16x8 qf[NK];
  gfrags<NK>(qf, qrow, lane);
  const float c2 = a.scale * LOG2E;
  const long bh = (long)b * H + h;
  const uint64_t bhts = (uint64_t)bh * T * S;  // dropout index of element (q, key): bhts + q*S + key
  const uint8_t* mb = nullptr;
  if constexpr (MASK) mb = a.mask + b * a.msb + h * a.msh;

  f4v o[NO];
  // causal: lr = the row sum of the probabilities as the P V product sees them (rounded to bf16).
  // The context is divided by lr, so its weights sum to one exactly; the log-sum-exp keeps the
  // unrounded sum l, which is what the backward recomputes P from.  A causal row has as few as one
  // or two visible keys, where dS = P (dP - Dv) nearly cancels and Dv = rowsum(dO * ctx) must not
  // carry the weights' rounding as an absolute error: dividing by l left 2.0e-2 on a dK block at
  // S = 2 where dividing by lr leaves 7.6e-3.  The non-causal kernels divide by l.
  float m[4], l[4], lr[4];
#pragma unroll
  for (int t = 0; t < NO; ++t) o[t] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = lr[r] = 0.f;
  }
  short* slab = Ps[wave];
  int nkb = (klen + KB - 1) / KB;  // key blocks entirely past key_len are not read
  // causal: key blocks past the diagonal one (QB == KB) are entirely in the future
  if constexpr (CAUSAL) nkb = nkb < bx + 1 ? nkb : bx + 1;
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * KB;
    MaskRaw mraw;
    if constexpr (MASK) mraw = mask_load_q<TAIL>(mb, (uint32_t)a.mst, q0 + (lane >> 4) * 4, k0, T, S, lane);
    __syncthreads();
    tile_load<TAIL, HD>(Ks, kbase + (long)k0 * ldkv, ldkv, tid, S - k0);
    tile_load<TAIL, HD>(Vs, kbase + (long)k0 * ldkv + C, ldkv, tid, S - k0);
    uint32_t vis = 0;
    if constexpr (MASK) vis = mask_pack_q(mraw);  // here: the mask bytes arrive before the tile's
    __syncthreads();
    const bool diag = CAUSAL && kb == bx;  // the only block that needs key <= q
    f4v s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f4v{0.f, 0.f, 0.f, 0.f};
      mfma_hd<LDH, NK>(s[t], qf, Ks, t * 16, lane);
    }
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -INFINITY;
      int kend = klen;  // first masked key of this row
      if constexpr (CAUSAL) {
        const int q = q0 + (lane >> 4) * 4 + r;
        kend = (diag && q + 1 < klen) ? q + 1 : klen;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int key = k0 + t * 16 + (lane & 15);
        bool seen = key < kend;
        if constexpr (MASK) seen = seen && ((vis >> (4 * t + r)) & 1u);
        const float v = seen ? s[t][r] * c2 : -INFINITY;
        s[t][r] = v;
        mx = fmaxf(mx, v);
      }
      mx = grp16_max(mx);
      const float mn = fmaxf(m[r], mx);
      // MASK: a row that has seen no key yet has m = mn = -inf; subtracting 0 instead keeps
      // alpha = p = exp2(-inf) = 0 where -inf - -inf would be NaN
      float ms = mn;
      if constexpr (MASK) ms = mn == -INFINITY ? 0.f : mn;
      alpha[r] = exp2f(m[r] - ms);
      m[r] = mn;
      float ls = 0.f, lsr = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float p = exp2f(s[t][r] - ms);
        ls += p;
        if constexpr (CAUSAL) lsr += bf2f(f2bf(p));
        s[t][r] = p;
      }
      l[r] = l[r] * alpha[r] + ls;
      if constexpr (CAUSAL) lr[r] = lr[r] * alpha[r] + lsr;
    }
    if (a.drop.on) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t q = q0 + (lane >> 4) * 4 + r;
          const uint32_t key = k0 + t * 16 + (lane & 15);
          s[t][r] *= drop_mul(a.drop, bhts + (q * (uint32_t)S + key));
        }
    }
#pragma unroll
    for (int t = 0; t < NO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[t][r] *= alpha[r];
    slab_store(slab, s, lane);
    __builtin_amdgcn_wave_barrier();
    const bf16x8 p0 = slab_frag(slab, 0, lane), p1 = slab_frag(slab, 1, lane);
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p0, frag_nc<LDH>(Vs, t * 16, 0, lane), o[t], 0, 0, 0);
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p1, frag_nc<LDH>(Vs, t * 16, 32, lane), o[t], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lt = grp16_sum(l[r]);
    inv[r] = 1.f / (CAUSAL ? grp16_sum(lr[r]) : lt);
    float lse = m[r] + log2f(lt);
    if constexpr (MASK) {  // a row with no visible key: context 0, lse 0 (the backward selects p = 0)
      inv[r] = lt > 0.f ? inv[r] : 0.f;
      lse = lt > 0.f ? lse : 0.f;
    }
    if ((lane & 15) == 0 && (!TAIL || q0 + (lane >> 4) * 4 + r < T)) a.lse[bh * T + q0 + (lane >> 4) * 4 + r] = lse;
  }
  // normalise, stage through the wave slab (Stage<HD>: 64-column halves at HD = 128), 16-B row stores
#pragma unroll
  for (int t = 0; t < NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[t][r] *= inv[r];
  if constexpr (HD == 64) {  // the one-group case, written out
    slab_store(slab, o, lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + i * 64;  // 16 rows x 8 chunks
      const int r = c >> 3, col = (c & 7) * 8;
      if (!TAIL || q0 + r < T)
        *reinterpret_cast<s8v*>(a.ctx + ((long)b * T + q0 + r) * C + h * D + col) =
            *reinterpret_cast<const s8v*>(slab + r * PLD + col);
    }
  } else {
    stage_out<HD, TAIL>(slab, o, a.ctx, (long)b * T + q0, C, h * D, q0, T, lane);
  }
}

// grid: ceil(S / 64) key blocks; rows of keys >= key_len[b] are stored as exact zeros
template <int HD, bool TAIL, bool MASK, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_bwd_dkv_kernel(GenArgs a) {
  static_assert(!(MASK && CAUSAL), "a masked causal call carries the triangle in its mask");
  constexpr int D = HD, LDH = HD + 8, NK = HD / 32, NO = HD / 16;  // k-steps of K Q^T / V dO^T, dK / dV tiles
  __shared__ __attribute__((aligned(16))) short Qs[QB * LDH];
  __shared__ __attribute__((aligned(16))) short Gs[QB * LDH];  // dO
  __shared__ __attribute__((aligned(16))) short Ps[4][16 * PLD];
  __shared__ __attribute__((aligned(16))) short Ds[4][16 * PLD];
  __shared__ float lse_s[QB], dv_s[QB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int bx = block_x<CAUSAL>();
  const int T = a.T, S = a.S, H = a.H, C = H * D;
  const long ldq = a.ldq, ldkv = a.ldkv, lddkv = a.lddkv;
  const int k0 = bx * KB + wave * 16;  // this wave's 16 keys
  int klen = a.key_len ? a.key_len[b] : S;
  klen = klen < 1 ? 1 : (klen > S ? S : klen);
  const long bh = (long)b * H + h;
  const uint64_t bhts = (uint64_t)bh * T * S;  // dropout index of element (q, key): bhts + q*S + key
  const bf16_t* qbase = a.q + (long)b * T * ldq + h * D;
  const bf16_t* gbase = a.dout + (long)b * T * C + h * D;
  const bf16_t* krow = a.kv + ((long)b * S + frag_row<TAIL>(k0 + (lane & 15), S)) * ldkv + h * D;
  const bf16_t* vrow = krow + C;
  bf16x8 kf[NK], vf[NK];
  gfrags<NK>(kf, krow, lane);
  gfrags<NK>(vf, vrow, lane);
  const float c2 = a.scale * LOG2E;
  f4v dk[NO], dv[NO];
#pragma unroll
  for (int t = 0; t < NO; ++t) dk[t] = dv[t] = f4v{0.f, 0.f, 0.f, 0.f};
  short* pslab = Ps[wave];
  short* dslab = Ds[wave];
  const bool any_valid = (uint32_t)bx * KB < (uint32_t)klen;
  const int nqb = any_valid ? (T + QB - 1) / QB : 0;
  const uint8_t* mb = nullptr;
  if constexpr (MASK) mb = a.mask + b * a.msb + h * a.msh;
  // causal: query blocks before the diagonal one (QB == KB) see none of this block's keys
  for (int qb = CAUSAL ? bx : 0; qb < nqb; ++qb) {
    const int q0 = qb * QB;
    const bool diag = CAUSAL && qb == bx;  // the only block that needs key <= q
    MaskRaw mraw;
    if constexpr (MASK) mraw = mask_load_k<TAIL>(mb, (uint32_t)a.mst, q0, k0, T, S, lane);
    __syncthreads();
    tile_load<TAIL, HD>(Qs, qbase + (long)q0 * ldq, ldq, tid, T - q0);
    tile_load<TAIL, HD>(Gs, gbase + (long)q0 * C, C, tid, T - q0);
    if (tid < QB) {
      const bool live = !TAIL || q0 + tid < T;  // queries >= T: no lse / Dv entry exists
      lse_s[tid] = live ? a.lse[bh * T + q0 + tid] : 0.f;
      dv_s[tid] = live ? a.dvec[bh * T + q0 + tid] : 0.f;
    }
    __syncthreads();
    uint32_t vis = 0;
    if constexpr (MASK) vis = mask_pack_k(mraw, lane);
    // S^T: rows = keys (this wave), cols = queries
    f4v p[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] = f4v{0.f, 0.f, 0.f, 0.f};
      mfma_hd<LDH, NK>(p[t], kf, Qs, t * 16, lane);
      dp[t] = f4v{0.f, 0.f, 0.f, 0.f};
      mfma_hd<LDH, NK>(dp[t], vf, Gs, t * 16, lane);
    }
    f4v pd[4], ds[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int qi = t * 16 + (lane & 15);
      const float ls = lse_s[qi], dvq = dv_s[qi];
      const bool qlive = !TAIL || q0 + qi < T;  // a query column >= T adds p = dS = 0
      int kend = klen;  // first masked key of this query column
      if constexpr (CAUSAL) kend = (diag && q0 + qi + 1 < klen) ? q0 + qi + 1 : klen;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + (lane >> 4) * 4 + r;
        bool seen = key < kend && qlive;
        if constexpr (MASK) seen = seen && ((vis >> (4 * t + r)) & 1u);
        const float pr = seen ? exp2f(p[t][r] * c2 - ls) : 0.f;
        const float mul =
            a.drop.on ? drop_mul(a.drop, bhts + ((uint32_t)(q0 + qi) * (uint32_t)S + (uint32_t)key)) : 1.f;
        pd[t][r] = pr * mul;
        ds[t][r] = pr * (dp[t][r] * mul - dvq);
      }
    }
    slab_store(pslab, pd, lane);
    slab_store(dslab, ds, lane);
    __builtin_amdgcn_wave_barrier();
    const bf16x8 pa0 = slab_frag(pslab, 0, lane), pa1 = slab_frag(pslab, 1, lane);
    const bf16x8 da0 = slab_frag(dslab, 0, lane), da1 = slab_frag(dslab, 1, lane);
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa0, frag_nc<LDH>(Gs, t * 16, 0, lane), dv[t], 0, 0, 0);
      dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa1, frag_nc<LDH>(Gs, t * 16, 32, lane), dv[t], 0, 0, 0);
      dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da0, frag_nc<LDH>(Qs, t * 16, 0, lane), dk[t], 0, 0, 0);
      dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da1, frag_nc<LDH>(Qs, t * 16, 32, lane), dk[t], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int t = 0; t < NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dk[t][r] *= a.scale;
  // stage through the slabs (Stage<HD>) -> 16-B stores into dkv (K and V halves)
  if constexpr (HD == 64) {  // the one-group case, written out
    slab_store(pslab, dk, lane);
    slab_store(dslab, dv, lane);
    __builtin_amdgcn_wave_barrier();
    bf16_t* drow = a.dkv + ((long)b * S + k0) * lddkv + h * D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + i * 64;
      const int r = c >> 3, col = (c & 7) * 8;
      if (!TAIL || k0 + r < S) {
        *reinterpret_cast<s8v*>(drow + (long)r * lddkv + col) = *reinterpret_cast<const s8v*>(pslab + r * PLD + col);
        *reinterpret_cast<s8v*>(drow + (long)r * lddkv + C + col) =
            *reinterpret_cast<const s8v*>(dslab + r * PLD + col);
      }
    }
  } else {
    bf16_t* drow = a.dkv + ((long)b * S + k0) * lddkv + h * D;
    stage_out2<HD, TAIL>(pslab, dslab, dk, dv, drow, lddkv, C, k0, S, lane);
  }
}

// grid: ceil(T / 64) query blocks.  Three waves per SIMD are asked for: left alone, the tail and the
// causal instantiations come out a few index registers above the 168 of three waves (174 and
// 141 + 32 = 173) and run two; asked, every instantiation fits in 162 or fewer without scratch.
// The plain non-tail one reaches three waves unasked (136 + 32) but is 4 - 5 % faster per forward +
// backward call with the request (156 + 0): docs/performance.md, "One generic attention kernel family".
// That is HD = 64, and HD = 32 takes the same request (it fits in 130 or fewer).  HD = 128 carries 8 dQ
// tiles and 4 + 4 fragment registers: asked for three waves it spills (16 - 72 bytes per lane), asked for
// two it fits in 198 or fewer without scratch (docs/performance.md, "Attention head dimensions").
template <int HD>
constexpr int DQ_WAVES = HD == 128 ? 2 : 3;
template <int HD, bool TAIL, bool MASK, bool CAUSAL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DQ_WAVES<HD>))) attn_bwd_dq_kernel(GenArgs a) {
  static_assert(!(MASK && CAUSAL), "a masked causal call carries the triangle in its mask");
  constexpr int D = HD, LDH = HD + 8, NK = HD / 32, NO = HD / 16;  // k-steps of Q K^T / dO V^T, dQ tiles
  __shared__ __attribute__((aligned(16))) short Ks[KB * LDH];
  __shared__ __attribute__((aligned(16))) short Vs[KB * LDH];
  __shared__ __attribute__((aligned(16))) short Ds[4][16 * PLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int bx = block_x<CAUSAL>();
  const int T = a.T, S = a.S, H = a.H, C = H * D;
  const long ldkv = a.ldkv;
  const int q0 = bx * QB + wave * 16;
  int klen = a.key_len ? a.key_len[b] : S;
  klen = klen < 1 ? 1 : (klen > S ? S : klen);
  const long bh = (long)b * H + h;
  const uint64_t bhts = (uint64_t)bh * T * S;  // dropout index of element (q, key): bhts + q*S + key
  const bf16_t* kbase = a.kv + (long)b * S * ldkv + h * D;
  const long qr = (long)b * T + frag_row<TAIL>(q0 + (lane & 15), T);
  const bf16_t* qrow = a.q + qr * a.ldq + h * D;
  const bf16_t* grow = a.dout + qr * C + h * D;
  bf16x8 qf[NK], gf[NK];
  gfrags<NK>(qf, qrow, lane);
  gfrags<NK>(gf, grow, lane);
  const float c2 = a.scale * LOG2E;
  float ls[4], dvq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = frag_row<TAIL>(q0 + (lane >> 4) * 4 + r, T);
    ls[r] = a.lse[bh * T + q];
    dvq[r] = a.dvec[bh * T + q];
  }
  const uint8_t* mb = nullptr;
  if constexpr (MASK) mb = a.mask + b * a.msb + h * a.msh;
  f4v dq[NO];
#pragma unroll
  for (int t = 0; t < NO; ++t) dq[t] = f4v{0.f, 0.f, 0.f, 0.f};
  short* dslab = Ds[wave];
  int nkb = (klen + KB - 1) / KB;  // key blocks entirely past key_len are not read
  // causal: key blocks past the diagonal one (QB == KB) are entirely in the future
  if constexpr (CAUSAL) nkb = nkb < bx + 1 ? nkb : bx + 1;
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * KB;
    MaskRaw mraw;
    if constexpr (MASK) mraw = mask_load_q<TAIL>(mb, (uint32_t)a.mst, q0 + (lane >> 4) * 4, k0, T, S, lane);
    __syncthreads();
    tile_load<TAIL, HD>(Ks, kbase + (long)k0 * ldkv, ldkv, tid, S - k0);
    tile_load<TAIL, HD>(Vs, kbase + (long)k0 * ldkv + C, ldkv, tid, S - k0);
    uint32_t vis = 0;
    if constexpr (MASK) vis = mask_pack_q(mraw);  // here: the mask bytes arrive before the tile's
    __syncthreads();
    const bool diag = CAUSAL && kb == bx;  // the only block that needs key <= q
    f4v s[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f4v{0.f, 0.f, 0.f, 0.f};
      mfma_hd<LDH, NK>(s[t], qf, Ks, t * 16, lane);
      dp[t] = f4v{0.f, 0.f, 0.f, 0.f};
      mfma_hd<LDH, NK>(dp[t], gf, Vs, t * 16, lane);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0 + t * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t q = q0 + (lane >> 4) * 4 + r;
        bool seen = key < klen;
        if constexpr (CAUSAL) seen = seen && (!diag || key <= (int)q);
        if constexpr (MASK) seen = seen && ((vis >> (4 * t + r)) & 1u);
        const float pr = seen ? exp2f(s[t][r] * c2 - ls[r]) : 0.f;
        const float mul = a.drop.on ? drop_mul(a.drop, bhts + (q * (uint32_t)S + (uint32_t)key)) : 1.f;
        s[t][r] = pr * (dp[t][r] * mul - dvq[r]);
      }
    }
    slab_store(dslab, s, lane);
    __builtin_amdgcn_wave_barrier();
    const bf16x8 d0 = slab_frag(dslab, 0, lane), d1 = slab_frag(dslab, 1, lane);
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      dq[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d0, frag_nc<LDH>(Ks, t * 16, 0, lane), dq[t], 0, 0, 0);
      dq[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d1, frag_nc<LDH>(Ks, t * 16, 32, lane), dq[t], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int t = 0; t < NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dq[t][r] *= a.scale;
  if constexpr (HD == 64) {  // the one-group case, written out
    slab_store(dslab, dq, lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = lane + i * 64;
      const int r = c >> 3, col = (c & 7) * 8;
      if (!TAIL || q0 + r < T)
        *reinterpret_cast<s8v*>(a.dq + ((long)b * T + q0 + r) * a.lddq + h * D + col) =
            *reinterpret_cast<const s8v*>(dslab + r * PLD + col);
    }
  } else {
    stage_out<HD, TAIL>(dslab, dq, a.dq, (long)b * T + q0, a.lddq, h * D, q0, T, lane);
  }
}

// ---------------------------------------------------------------------------
// Fused backward for short sequences (S = 64 or 128, BERT fine-tuning): ONE workgroup per
// (batch, head) holds the whole head in LDS, so the three-kernel path's prep pass, its
// second recomputation of P / dP / the dropout hash (dQ kernel) and its per-block reloads
// of Q / dO / K / V all disappear:
//   load   Q, dO, K -> LDS; this wave's 16 K / V rows -> A fragments; Dv = rowsum(dO * O)
//   A      (wave w = keys 16w..16w+15, all S queries)
//          S^T = K Q^T, dP^T = V dO^T  ->  P, dS = P (dP * mask - Dv)  -> LDS [q][key]
//          dV = P^T dO, dK = dS^T Q    (P^T / dS^T as transposed reads of the [q][key] arrays)
//   B      (wave w = queries 16w..16w+15)  dQ = dS K   (dS rows straight from LDS)
// Every P / dS element is computed (and its dropout bit hashed) once instead of twice.
// LDS: 2 x [S][72] + [S][S + 8] bf16 = 72 KB at S = 128 (two 8-wave blocks per CU; the
// first version kept K, P and dS in separate arrays, 124 KB, one block per CU: 37-38 us).

// C-layout 16 x 64 fp32 (4 column tiles, lane l: row 4 (l >> 4) + r, column 16 t + (l & 15))
// -> bf16 [16][LDT] slab, then 16-B row stores to dst rows (pitch ld)
__device__ __forceinline__ void stage_store(short* slab, const f4v (&v)[4], bf16_t* dst, long ld, int lane) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[((lane >> 4) * 4 + r) * LDT + t * 16 + (lane & 15)] = (short)f2bf(v[t][r]);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + i * 64;
    const int r = c >> 3, col = (c & 7) * 8;
    *reinterpret_cast<s8v*>(dst + (long)r * ld + col) = *reinterpret_cast<const s8v*>(slab + r * LDT + col);
  }
}

template <int SQ, bool CAUSAL>
__global__ void __launch_bounds__(SQ * 4) __attribute__((amdgpu_waves_per_eu(4))) attn_bwd_fused_kernel(AttnArgs a) {
  constexpr int NW = SQ / 16, NT = NW * 64, TQ = SQ / 16, PL = SQ + 8, LCH = SQ * 8 / NT;
  // Qs: Q; Gs: dO (phase A), then K (phase B); Xs [q][key]: each wave's P columns, then
  // its dS columns (P is dead once dV is accumulated).  72 KB at S = 128: two blocks per CU.
  __shared__ __attribute__((aligned(16))) short Qs[SQ * LDT];
  __shared__ __attribute__((aligned(16))) short Gs[SQ * LDT];
  __shared__ __attribute__((aligned(16))) short Xs[SQ * PL];
  __shared__ float lse_s[SQ], dv_s[SQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x;
  const int b = bh / a.H, h = bh - b * a.H;
  const int H = a.H, C = H * D;
  const long ldq = 3L * C;
  int klen = a.key_len ? a.key_len[b] : SQ;
  klen = klen < 1 ? 1 : (klen > SQ ? SQ : klen);
  const uint64_t bhss = (uint64_t)bh * SQ * SQ;
  const bf16_t* base = a.qkv + (long)b * SQ * ldq;
  const bf16_t* gbase = a.dout + (long)b * SQ * C + h * D;
  const bf16_t* obase = a.out + (long)b * SQ * C + h * D;

  // ---- loads: Q / dO tiles, Dv = rowsum(dO * O)
#pragma unroll
  for (int i = 0; i < LCH; ++i) {
    const int c = tid + i * NT;
    const int r = c >> 3, col = (c & 7) * 8;
    const s8v qv = *reinterpret_cast<const s8v*>(base + (long)r * ldq + h * D + col);
    const us8 gv = *reinterpret_cast<const us8*>(gbase + (long)r * C + col);
    const us8 ov = *reinterpret_cast<const us8*>(obase + (long)r * C + col);
    *reinterpret_cast<s8v*>(Qs + r * LDT + col) = qv;
    *reinterpret_cast<us8*>(Gs + r * LDT + col) = gv;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bf2f(gv[j]) * bf2f(ov[j]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if ((c & 7) == 0) dv_s[r] = s;
  }
  if (tid < SQ) lse_s[tid] = a.lse[(long)bh * SQ + tid];
  const int k0 = wave * 16;
  const bf16_t* krow = base + (long)(k0 + (lane & 15)) * ldq + C + h * D;
  const bf16_t* vrow = krow + C;
  const bf16x8 kf0 = gfrag(krow, 0, lane), kf1 = gfrag(krow, 1, lane);
  const bf16x8 vf0 = gfrag(vrow, 0, lane), vf1 = gfrag(vrow, 1, lane);
  const float c2 = a.scale * LOG2E;
  __syncthreads();

  // ---- phase A: this wave's 16 keys against all queries
  s4v dsr[TQ];  // this wave's dS^T values, held until P's columns are consumed
  {
    f4v p[TQ], dp[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
      p[t] = f4v{0.f, 0.f, 0.f, 0.f};
      p[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, frag_kc<LDT>(Qs, t * 16, 0, lane), p[t], 0, 0, 0);
      p[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, frag_kc<LDT>(Qs, t * 16, 32, lane), p[t], 0, 0, 0);
      dp[t] = f4v{0.f, 0.f, 0.f, 0.f};
      dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, frag_kc<LDT>(Gs, t * 16, 0, lane), dp[t], 0, 0, 0);
      dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, frag_kc<LDT>(Gs, t * 16, 32, lane), dp[t], 0, 0, 0);
    }
    // p[t][r] = S^T[key = k0 + 4 (l >> 4) + r][q = 16 t + (l & 15)]
    const int kr = k0 + (lane >> 4) * 4;
    const int cdiag = (lane & 15) + 1 - kr;  // causal: qi + 1 - kr at t = 0
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
      const int qi = t * 16 + (lane & 15);
      const float ls = lse_s[qi], dvq = dv_s[qi];
      s4v pk;
      // causal: keys kr + r, r < nvis, are visible to this query column (kr + r < klen and kr + r <= qi);
      // one count per column, because a second per-element test spilled at S = 128
      int nvis = klen - kr;
      if constexpr (CAUSAL) nvis = nvis < cdiag + t * 16 ? nvis : cdiag + t * 16;
      float dm[4] = {1.f, 1.f, 1.f, 1.f};  // the row's four consecutive keys: two hashes
      if (a.drop.on) drop_mul4(a.drop, bhss + (uint32_t)(qi * SQ + kr), dm);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kr + r;
        const float pr = (CAUSAL ? r < nvis : key < klen) ? exp2f(p[t][r] * c2 - ls) : 0.f;
        const float mul = dm[r];
        pk[r] = (short)f2bf(pr * mul);
        dsr[t][r] = (short)f2bf(pr * (dp[t][r] * mul - dvq));
      }
      *reinterpret_cast<s4v*>(Xs + qi * PL + kr) = pk;
    }
  }
  f4v dk[4], dv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dk[t] = dv[t] = f4v{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int kk = 0; kk < SQ / 32; ++kk) {
    const bf16x8 pa = frag_nc<PL>(Xs, k0, kk * 32, lane);  // P^T: row = key, k = query
#pragma unroll
    for (int t = 0; t < 4; ++t)
      dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, frag_nc<LDT>(Gs, t * 16, kk * 32, lane), dv[t], 0, 0, 0);
  }
  // P's columns of this wave are read: overwrite them with dS
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  {
    const int kr = k0 + (lane >> 4) * 4;
#pragma unroll
    for (int t = 0; t < TQ; ++t) *reinterpret_cast<s4v*>(Xs + (t * 16 + (lane & 15)) * PL + kr) = dsr[t];
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int kk = 0; kk < SQ / 32; ++kk) {
    const bf16x8 da = frag_nc<PL>(Xs, k0, kk * 32, lane);  // dS^T
#pragma unroll
    for (int t = 0; t < 4; ++t)
      dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, frag_nc<LDT>(Qs, t * 16, kk * 32, lane), dk[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dk[t][r] *= a.scale;
  __syncthreads();  // every wave's dS columns written; dO no longer read

  // K into the dO region (its load latency is covered by the CU's other block)
#pragma unroll
  for (int i = 0; i < LCH; ++i) {
    const int c = tid + i * NT;
    const int r = c >> 3, col = (c & 7) * 8;
    *reinterpret_cast<s8v*>(Gs + r * LDT + col) = *reinterpret_cast<const s8v*>(base + (long)r * ldq + C + h * D + col);
  }
  __syncthreads();

  // ---- phase B: dQ for this wave's 16 queries
  const int q0 = wave * 16;
  f4v dq[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dq[t] = f4v{0.f, 0.f, 0.f, 0.f};
  const int nkk = (klen + 31) / 32;
  for (int kk = 0; kk < nkk; ++kk) {
    const bf16x8 da = frag_kc<PL>(Xs, q0, kk * 32, lane);  // dS: row = query, k = key
#pragma unroll
    for (int t = 0; t < 4; ++t)
      dq[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, frag_nc<LDT>(Gs, t * 16, kk * 32, lane), dq[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dq[t][r] *= a.scale;
  __syncthreads();  // dS and K no longer read: every region is staging space now

  bf16_t* drow = a.dqkv + ((long)b * SQ + k0) * ldq + h * D;
  stage_store(Qs + wave * 16 * LDT, dk, drow + C, ldq, lane);
  stage_store(Gs + wave * 16 * LDT, dv, drow + 2 * C, ldq, lane);
  stage_store(Xs + wave * 16 * LDT, dq, a.dqkv + ((long)b * SQ + q0) * ldq + h * D, ldq, lane);
}

// Forward for S = 64 / 128: one workgroup per (batch, head), all S keys' K and V issued
// to LDS up front (one memory round trip instead of one per 64-key block), then each
// wave's 16 query rows take an exact (not online) softmax over the whole key row.
// LDS: 2 x [S][72] = 36 KB at S = 128.  Once every wave holds its scores in registers the
// K image is dead, and each wave stages its P (64 keys at a time, [16][72]) and finally its
// output tile in its own 16 rows of it -- three 8-wave blocks per CU (72 VGPRs), so the
// B x H = 768 blocks of BERT-base b64 run in one round instead of 1.5 (per-wave P slabs
// beside K / V took 72 KB: two blocks per CU).
template <int SQ, bool CAUSAL>
__global__ void __launch_bounds__(SQ * 4) attn_fwd_short_kernel(AttnArgs a) {
  constexpr int NW = SQ / 16, NT = NW * 64, TK = SQ / 16;
  static_assert(NW * 16 == SQ, "one 16-row slab of the K image per wave");
  __shared__ __attribute__((aligned(16))) short Ks[SQ * LDT];
  __shared__ __attribute__((aligned(16))) short Vs[SQ * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x;
  const int b = bh / a.H, h = bh - b * a.H;
  const int C = a.H * D;
  const long ldq = 3L * C;
  int klen = a.key_len ? a.key_len[b] : SQ;
  klen = klen < 1 ? 1 : (klen > SQ ? SQ : klen);
  const uint64_t bhss = (uint64_t)bh * SQ * SQ;
  const bf16_t* base = a.qkv + (long)b * SQ * ldq;
#pragma unroll
  for (int i = 0; i < SQ * 8 / NT; ++i) {
    const int c = tid + i * NT;
    const int r = c >> 3, col = (c & 7) * 8;
    const s8v kv = *reinterpret_cast<const s8v*>(base + (long)r * ldq + C + h * D + col);
    const s8v vv = *reinterpret_cast<const s8v*>(base + (long)r * ldq + 2 * C + h * D + col);
    *reinterpret_cast<s8v*>(Ks + r * LDT + col) = kv;
    *reinterpret_cast<s8v*>(Vs + r * LDT + col) = vv;
  }
  const int q0 = wave * 16;
  const bf16_t* qrow = base + (long)(q0 + (lane & 15)) * ldq + h * D;
  const bf16x8 qf0 = gfrag(qrow, 0, lane), qf1 = gfrag(qrow, 1, lane);
  const float c2 = a.scale * LOG2E;
  __syncthreads();
  // s[t][r] = S[q = q0 + 4 (l >> 4) + r][key = 16 t + (l & 15)]
  f4v s[TK];
#pragma unroll
  for (int t = 0; t < TK; ++t) {
    s[t] = f4v{0.f, 0.f, 0.f, 0.f};
    if (CAUSAL && t > wave) continue;  // keys 16 t .. 16 t + 15 all follow this wave's queries: masked below
    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf0, frag_kc<LDT>(Ks, t * 16, 0, lane), s[t], 0, 0, 0);
    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf1, frag_kc<LDT>(Ks, t * 16, 32, lane), s[t], 0, 0, 0);
  }
  // causal: lr = the row sum of the probabilities as the P V product sees them (rounded to bf16);
  // the context is normalised by it, the log-sum-exp keeps the unrounded sum (see attn_fwd_kernel)
  float m[4], l[4], lr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float mx = -INFINITY;
    int kend = klen;  // first masked key of this row
    if constexpr (CAUSAL) {
      const int q = q0 + (lane >> 4) * 4 + r;
      kend = q + 1 < klen ? q + 1 : klen;
    }
#pragma unroll
    for (int t = 0; t < TK; ++t) {
      const int key = t * 16 + (lane & 15);
      const float v = key < kend ? s[t][r] * c2 : -INFINITY;
      s[t][r] = v;
      mx = fmaxf(mx, v);
    }
    m[r] = grp16_max(mx);
    float ls = 0.f, lsr = 0.f;
#pragma unroll
    for (int t = 0; t < TK; ++t) {
      const float p = exp2f(s[t][r] - m[r]);
      ls += p;
      if constexpr (CAUSAL) lsr += bf2f(f2bf(p));
      s[t][r] = p;
    }
    l[r] = grp16_sum(ls);
    if constexpr (CAUSAL) lr[r] = grp16_sum(lsr);
  }
  // every wave's QK^T reads of Ks are done past this barrier: its rows become P slabs
  __syncthreads();
  short* slab = Ks + wave * 16 * LDT;
  f4v o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int half = 0; half < SQ / 64; ++half) {
    if (CAUSAL && half * 64 > q0 + 15) continue;  // P is zero for these 64 keys
    if (half) __builtin_amdgcn_wave_barrier();  // the previous half's P reads precede these writes
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int t = half * 4 + tt;
      // keys across lanes: a lane pair shares each row's hash (drop_mul_lanepair; SQ is even)
      float dm[4] = {1.f, 1.f, 1.f, 1.f};
      if (a.drop.on) {
        static_assert(SQ % 2 == 0, "lane-pair dropout hashing needs an even row length");
        const int keyev = t * 16 + (lane & 14);
#pragma unroll
        for (int rr = 0; rr < 4; rr += 2) {
          const int qh = q0 + (lane >> 4) * 4 + rr + (lane & 1);
          drop_mul_lanepair(a.drop, (bhss + (uint32_t)(qh * SQ + keyev)) >> 1, lane, dm[rr], dm[rr + 1]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[((lane >> 4) * 4 + r) * LDT + tt * 16 + (lane & 15)] = (short)f2bf(s[t][r] * dm[r]);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const bf16x8 pf = frag_kc<LDT>(slab, 0, k2 * 32, lane);
      const int kk = half * 2 + k2;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, frag_nc<LDT>(Vs, t * 16, kk * 32, lane), o[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.f / (CAUSAL ? lr[r] : l[r]);
    if ((lane & 15) == 0) a.lse[(long)bh * SQ + q0 + (lane >> 4) * 4 + r] = m[r] + log2f(l[r]);
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t][r] *= inv;
  }
  __builtin_amdgcn_wave_barrier();
  stage_store(slab, o, a.ctx + ((long)b * SQ + q0) * C + h * D, C, lane);
}

bool shape_ok(int S, int H) { return S > 0 && H > 0; }

// S = 64 / 128 only
template <bool CAUSAL>
void launch_fwd_short(const AttnArgs& a, hipStream_t s) {
  if (a.S == 128) attn_fwd_short_kernel<128, CAUSAL><<<a.B * a.H, 512, 0, s>>>(a);
  else attn_fwd_short_kernel<64, CAUSAL><<<a.B * a.H, 256, 0, s>>>(a);
}
template <bool CAUSAL>
void launch_bwd_fused(const AttnArgs& a, hipStream_t s) {
  if (a.S == 128) attn_bwd_fused_kernel<128, CAUSAL><<<a.B * a.H, 512, 0, s>>>(a);
  else attn_bwd_fused_kernel<64, CAUSAL><<<a.B * a.H, 256, 0, s>>>(a);
}

bool cross_shape_ok(int B, int T, int S, int H) {
  return B > 0 && T > 0 && S > 0 && H > 0 && (long)T * S <= 0x7fffffffL;  // q*S + key is a 32-bit index
}
// mask strides: non-negative, and a (batch, head) slice addressable with 32-bit offsets
bool cross_mask_ok(const uint8_t* mask, long sb, long sh, long st, int T, int S) {
  return !mask || (sb >= 0 && sh >= 0 && st >= 0 && (long)(T - 1) * st + S <= 0x7fffffffL);
}
void cross_set_mask(GenArgs& a, const uint8_t* mask, long sb, long sh, long st) {
  a.mask = mask; a.msb = sb; a.msh = sh; a.mst = st;
}
// The generic kernels' view of a packed-qkv call: Q and K | V, and their gradients, are column
// ranges of rows at pitch 3C
GenArgs self_args(const AttnArgs& s, int hd) {
  const int C = s.H * hd;
  GenArgs a{};
  a.q = s.qkv; a.kv = s.qkv + C; a.dout = s.dout; a.ctx = s.ctx; a.dq = s.dqkv;
  a.dkv = s.dqkv ? s.dqkv + C : nullptr;  // forward: no gradients
  a.lse = s.lse; a.dvec = s.dvec; a.key_len = s.key_len;
  a.ldq = a.ldkv = a.lddq = a.lddkv = 3L * C;
  a.B = s.B; a.T = a.S = s.S; a.H = s.H; a.scale = s.scale; a.drop = s.drop;
  return a;
}

// The generic launchers; (MASK, CAUSAL) is (false, false), (true, false) or (false, true)
static_assert(QB == KB, "causal: one grid for the key-block and the query-block kernels, diagonal block = own block");
bool gen_tail(const GenArgs& a) { return a.T % QB != 0 || a.S % KB != 0; }
dim3 gen_qgrid(const GenArgs& a) { return dim3((a.T + QB - 1) / QB, a.H, a.B); }
dim3 gen_kgrid(const GenArgs& a) { return dim3((a.S + KB - 1) / KB, a.H, a.B); }
template <int HD, bool MASK, bool CAUSAL>
void launch_fwd_hd(const GenArgs& a, hipStream_t s) {
  if (gen_tail(a)) attn_fwd_kernel<HD, true, MASK, CAUSAL><<<gen_qgrid(a), 256, 0, s>>>(a);
  else attn_fwd_kernel<HD, false, MASK, CAUSAL><<<gen_qgrid(a), 256, 0, s>>>(a);
}
template <int HD, bool MASK, bool CAUSAL>
void launch_bwd_dkv_hd(const GenArgs& a, hipStream_t s) {
  if (gen_tail(a)) attn_bwd_dkv_kernel<HD, true, MASK, CAUSAL><<<gen_kgrid(a), 256, 0, s>>>(a);
  else attn_bwd_dkv_kernel<HD, false, MASK, CAUSAL><<<gen_kgrid(a), 256, 0, s>>>(a);
}
template <int HD, bool MASK, bool CAUSAL>
void launch_bwd_dq_hd(const GenArgs& a, hipStream_t s) {
  if (gen_tail(a)) attn_bwd_dq_kernel<HD, true, MASK, CAUSAL><<<gen_qgrid(a), 256, 0, s>>>(a);
  else attn_bwd_dq_kernel<HD, false, MASK, CAUSAL><<<gen_qgrid(a), 256, 0, s>>>(a);
}
// Head-dim dispatch; hd is one of the supported widths (head_dim_ok, checked by every entry point)
bool head_dim_ok(int hd) { return hd == 32 || hd == 64 || hd == 128; }
template <bool MASK, bool CAUSAL>
void launch_fwd(const GenArgs& a, int hd, hipStream_t s) {
  if (hd == 32) launch_fwd_hd<32, MASK, CAUSAL>(a, s);
  else if (hd == 128) launch_fwd_hd<128, MASK, CAUSAL>(a, s);
  else launch_fwd_hd<64, MASK, CAUSAL>(a, s);
}
template <bool MASK, bool CAUSAL>
void launch_bwd_dkv(const GenArgs& a, int hd, hipStream_t s) {
  if (hd == 32) launch_bwd_dkv_hd<32, MASK, CAUSAL>(a, s);
  else if (hd == 128) launch_bwd_dkv_hd<128, MASK, CAUSAL>(a, s);
  else launch_bwd_dkv_hd<64, MASK, CAUSAL>(a, s);
}
template <bool MASK, bool CAUSAL>
void launch_bwd_dq(const GenArgs& a, int hd, hipStream_t s) {
  if (hd == 32) launch_bwd_dq_hd<32, MASK, CAUSAL>(a, s);
  else if (hd == 128) launch_bwd_dq_hd<128, MASK, CAUSAL>(a, s);
  else launch_bwd_dq_hd<64, MASK, CAUSAL>(a, s);
}
// Dv = rowsum(dO * O) over a.B * a.S query rows of a.H heads
void launch_prep(const AttnArgs& a, int hd, hipStream_t s) {
  const long pairs = (long)a.B * a.S * a.H;
  if (hd == 32) attn_bwd_prep_kernel<32><<<ca_cdiv(pairs, 64), 256, 0, s>>>(a);
  else if (hd == 128) attn_bwd_prep_kernel<128><<<ca_cdiv(pairs, 16), 256, 0, s>>>(a);
  else attn_bwd_prep_kernel<64><<<ca_cdiv(pairs, 32), 256, 0, s>>>(a);
}

// CLOUD_AMD_ATTN_FUSED_BWD=0 keeps the three-kernel backward at S <= 128 (A/B runs)
bool fused_bwd_enabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("CLOUD_AMD_ATTN_FUSED_BWD");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v != 0;
}

}  // namespace

extern "C" {

// ctx = softmax(Q K^T * scale + keymask) (dropout) V ; lse[B][H][S] saved for the backward.
// causal != 0: key j is visible to query i iff j <= i (and j < key_len[b]).
int ca_attn_fwd(const bf16_t* qkv, bf16_t* ctx, float* lse, const int* key_len, int B, int S, int H, int hd,
                float scale, float p_drop, uint64_t seed, int causal, hipStream_t s) {
  if (!shape_ok(S, H) || !head_dim_ok(hd)) return -1;
  AttnArgs a{};
  a.qkv = qkv; a.ctx = ctx; a.lse = lse; a.key_len = key_len;
  a.B = B; a.S = S; a.H = H; a.scale = scale; a.drop = make_drop(p_drop, seed);
  if ((S == 64 || S == 128) && hd == D && fused_bwd_enabled()) {
    if (causal) launch_fwd_short<true>(a, s);
    else launch_fwd_short<false>(a, s);
    CA_LAUNCH_CHECK();
    return 0;
  }
  if (causal) launch_fwd<false, true>(self_args(a, hd), hd, s);
  else launch_fwd<false, false>(self_args(a, hd), hd, s);
  CA_LAUNCH_CHECK();
  return 0;
}

// dqkv (all three thirds written) from dctx; dvec: [B][H][S] fp32 scratch.
int ca_attn_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, float* dvec,
                bf16_t* dqkv, const int* key_len, int B, int S, int H, int hd, float scale, float p_drop,
                uint64_t seed, int causal, hipStream_t s) {
  if (!shape_ok(S, H) || !head_dim_ok(hd)) return -1;
  AttnArgs a{};
  a.qkv = qkv; a.out = out; a.dout = dout; a.lse = const_cast<float*>(lse); a.dvec = dvec; a.dqkv = dqkv;
  a.key_len = key_len; a.B = B; a.S = S; a.H = H; a.scale = scale; a.drop = make_drop(p_drop, seed);
  if ((S == 64 || S == 128) && hd == D && fused_bwd_enabled()) {
    if (causal) launch_bwd_fused<true>(a, s);
    else launch_bwd_fused<false>(a, s);
    CA_LAUNCH_CHECK();
    return 0;
  }
  launch_prep(a, hd, s);
  CA_LAUNCH_CHECK();
  const GenArgs g = self_args(a, hd);
  if (causal) launch_bwd_dkv<false, true>(g, hd, s);
  else launch_bwd_dkv<false, false>(g, hd, s);
  CA_LAUNCH_CHECK();
  if (causal) launch_bwd_dq<false, true>(g, hd, s);
  else launch_bwd_dq<false, false>(g, hd, s);
  CA_LAUNCH_CHECK();
  return 0;
}

// Cross-attention (head dim hd): ctx[B*T][H*hd] = softmax(Q K^T * scale + keymask) (dropout) V for q rows at pitch
// ldq and kv = K | V rows at pitch ldkv (elements; multiples of 8, 16-byte aligned bases);
// lse[B][H][T] saved for the backward.
// mask (null = none): byte (b, h, q, key) at b*msb + h*msh + q*mst + key, element strides, 0 = broadcast;
// a score takes part iff key < key_len[b] and its byte is non-zero.  A query that sees no key gets
// context 0 and lse 0, and contributes 0 to every gradient.
int ca_attn_cross_fwd(const bf16_t* q, const bf16_t* kv, bf16_t* ctx, float* lse, const int* key_len,
                      const uint8_t* mask, long msb, long msh, long mst, int B, int T, int S, int H, int hd, long ldq,
                      long ldkv, float scale, float p_drop, uint64_t seed, hipStream_t s) {
  if (!cross_shape_ok(B, T, S, H) || !head_dim_ok(hd) || !cross_mask_ok(mask, msb, msh, mst, T, S)) return -1;
  GenArgs a{};
  a.q = q; a.kv = kv; a.ctx = ctx; a.lse = lse; a.key_len = key_len; a.ldq = ldq; a.ldkv = ldkv;
  a.B = B; a.T = T; a.S = S; a.H = H; a.scale = scale; a.drop = make_drop(p_drop, seed);
  cross_set_mask(a, mask, msb, msh, mst);
  if (mask) launch_fwd<true, false>(a, hd, s);
  else launch_fwd<false, false>(a, hd, s);
  CA_LAUNCH_CHECK();
  return 0;
}

// dq[B*T][H*hd] and dkv[B*S][2*H*hd] (every row written) from dctx; dvec: [B][H][T] fp32 scratch.
int ca_attn_cross_bwd(const bf16_t* q, const bf16_t* kv, const bf16_t* out, const bf16_t* dout, const float* lse,
                      float* dvec, bf16_t* dq, bf16_t* dkv, const int* key_len, const uint8_t* mask, long msb,
                      long msh, long mst, int B, int T, int S, int H, int hd, long ldq, long ldkv, float scale,
                      float p_drop, uint64_t seed, hipStream_t s) {
  if (!cross_shape_ok(B, T, S, H) || !head_dim_ok(hd) || !cross_mask_ok(mask, msb, msh, mst, T, S)) return -1;
  AttnArgs p{};  // Dv = rowsum(dO * O) over the B*T query rows
  p.out = out; p.dout = dout; p.dvec = dvec; p.B = B; p.S = T; p.H = H;
  launch_prep(p, hd, s);
  CA_LAUNCH_CHECK();
  GenArgs a{};
  a.q = q; a.kv = kv; a.dout = dout; a.lse = const_cast<float*>(lse); a.dvec = dvec; a.dq = dq; a.dkv = dkv;
  a.key_len = key_len; a.ldq = ldq; a.ldkv = ldkv; a.lddq = (long)H * hd; a.lddkv = 2L * H * hd;
  a.B = B; a.T = T; a.S = S; a.H = H; a.scale = scale; a.drop = make_drop(p_drop, seed);
  cross_set_mask(a, mask, msb, msh, mst);
  if (mask) launch_bwd_dkv<true, false>(a, hd, s);
  else launch_bwd_dkv<false, false>(a, hd, s);
  CA_LAUNCH_CHECK();
  if (mask) launch_bwd_dq<true, false>(a, hd, s);
  else launch_bwd_dq<false, false>(a, hd, s);
  CA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
