// Attention for the SD UNet on MFMA (v_mfma_f32_32x32x16_bf16), with the Prompt-to-Prompt edits
// applied inside the kernels so probabilities are never materialised in HBM.
//
// Common structure (a wave works on groups of 32 query rows; workgroup = 4 waves):
//   * "swapped" QK^T: S^T[kv][q] = mfma(A = K tile, B = Q^T) -> a lane owns ONE query column
//     (q = lane & 31) and 16 of the 32 kv rows of the tile; the other 16 live in lane ^ 32.  Row
//     max / row sum are in-register reductions + one cross-half exchange.
//   * P feeds the PV MFMA straight from registers: O^T[d][q] = mfma(A = V^T tile, B = P^T).  The
//     B-operand wants 8 consecutive k per lane while a lane holds kv = (r&3) + 8(r>>2) + 4*half;
//     the contraction order over kv is free, so either the V^T fragment is read with the SAME
//     permutation (cross_attn: two 8-byte LDS reads) or the S^T rows are visited in a permuted
//     order that makes the lane's 8 values consecutive (self_attn: one 16-byte read).
//   * V arrives transposed (V^T[h*d + dd][b*N + token]) from a GEMM with swapped operands.
//   * Q is pre-scaled by softmax_scale * log2(e) (folded into W_q), so exp2 is used directly.
//
// self_attn: flash / online softmax over 64-row KV tiles, DMA-staged and software-pipelined (see
//   the section comment below).  P2P self-attention replacement (ptp_classes.py:194-200:
//   P_tar <- P_src) needs no probabilities at all: the target row just uses the SOURCE row's Q
//   and K (qk_src[b]).
// cross_attn: 77 (padded 96) keys, whole K/V^T in LDS, exact softmax.  For a (src,tar) pair the
//   wave computes P_src, then P_new = P_src . A + bvec * P_tar with the per-step 96x96 mixing
//   matrix on MFMA (Replace / Refine / Reweight and the cross_replace_alpha blend all fold into
//   (A, bvec), see hedit/p2p/ptp_classes.py::_mix_tables), accumulates the post-edit maps into the fp32 store when
//   asked, and finishes with P.V for both rows.
#include "common.h"
#include "kernels.h"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // (not HIP's uint4 struct, which SROA handles badly)

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
#ifndef SA_BURST
#define SA_BURST 0          // measurement builds only (tools/build_variant.sh ... attn "-DSA_BURST=n"): bit 0 phases, bit 1 + priority
#endif

template <int D>
struct HeadCfg {
  static constexpr int DP = (D + 15) / 16 * 16;   // K-dim of QK^T, padded
  static constexpr int DK = DP / 16;
  static constexpr int DT = (D + 31) / 32;        // 32-row tiles of O^T
  static constexpr int KS = DP + 8;               // LDS row stride of K (elements)
  static constexpr int DCH = D / 8;               // 16-byte chunks per K row
};

// ============================================================================ self-attention
// Flash attention over 64-row KV tiles, organised around what limits it on CDNA4: per 32x32 score
// block a lane has ~55 VALU instructions of softmax work (sub, exp2, max, bf16 pack) against
// 3 + 4 MFMAs (d = 40), and a wave issues in order -- an MFMA queued behind a busy matrix pipe
// blocks the VALU work after it.  So:
//   * KV tiles go global -> LDS by DMA (global_load_lds, no staging VGPRs, no ds_write) into a ring
//     of four stages (three for d >= 80, where four would cost the second workgroup per CU): the
//     DMA of tile t+2 is issued when tile t is handed over and retired with a counted vmcnt, so a
//     tile has two tiles of work to land (an LDS-DMA needs ~0.85 us under load); one barrier per tile.  Tiles are dense (no row padding): the
//     source chunk each lane fetches is XOR-swizzled so that the b128 fragment reads are
//     conflict-free for every head dim.
//   * the work is cut into "units" (32 kv rows x 32 queries) and software-pipelined across them:
//     block U issues P.V of unit U-1, QK^T of unit U+2 and the row max of unit U+1 around the
//     exp/pack work of unit U.  All MFMAs in a block are independent of its VALU work, so they
//     interleave instead of serialising.
//   * two accumulator streams per wave alternate between units, which keeps the lazy max rescale
//     of a stream away from the P.V still in flight for it.  QG = 2: the streams are two groups of
//     32 queries (K / V^T fragments are shared by the pair); QG = 1 (large head dims): one query
//     group, the streams are the two 32-row halves of every KV tile, merged at the end.
//   * the S^T rows of a half tile are visited in a permuted order (kv_perm) chosen so that the 8
//     probabilities a lane packs for the P.V B-operand belong to 8 CONSECUTIVE kv rows: the V^T
//     A-fragment is then a single b128 read of the natural layout.
//   * when the head dim leaves pad rows in the last 32-row V^T tile, pad row D holds ones: the P.V
//     MFMA also produces the softmax denominator and the per-element VALU add disappears.
template <int D>
__device__ __forceinline__ int k_swz(int row) {
  if (D == 32 || D == 160) return (row >> 2) & 3;
  if (D == 64) return (row >> 1) & 7;
  if (D == 80) return (row >> 4) & 1;
  return 0;   // 80-byte rows (d = 40) are conflict-free as they are
}
__device__ __forceinline__ int v_swz(int row) { return (row >> 1) & 7; }

template <int D, int QG>
struct SelfCfg {
  using H = HeadCfg<D>;
  static constexpr int DCH = D / 8;                    // 16-byte chunks per K row
  static constexpr int K_BYTES = 64 * DCH * 16;
  static constexpr int V_ROWS = H::DT * 32;
  static constexpr int V_BYTES = V_ROWS * 128;
  static constexpr int STAGE = K_BYTES + V_BYTES;
  static constexpr int KI = DCH, VI = D / 8;           // 1 KiB DMA instructions per tile (K, V^T)
  static constexpr int TI = KI + VI, NI = (TI + 3) / 4;
  // LDS ring: 4 stages (DMA two tiles ahead) when two workgroups of that still fit a CU, else 3
  static constexpr int NSTG = 2 * 4 * STAGE <= 160 * 1024 ? 4 : 3;
  static constexpr int PD = NSTG - 2;                  // prefetch distance in KV tiles
  static constexpr int DUMP = TI % 4 ? 4096 : 0;       // parking area for DMA slots without a chunk
  static constexpr int TOTAL = NSTG * STAGE + DUMP;
  static constexpr int UT = 2 * QG;                    // units per KV tile
};

template <int D, int QG, int NS>
__global__ __launch_bounds__(256, (D <= 80 ? 2 : 1)) void self_attn_kernel(SelfAttnParams p) {
  static_assert(QG == 1 || NS == 2, "two query groups are two streams");
  using H = HeadCfg<D>;
  using C = SelfCfg<D, QG>;
  constexpr bool ONES = H::DT * 32 > D;
  constexpr int DK = H::DK, DT = H::DT;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = lane & 31, hi = lane >> 5;
  // XCD-aware block order.  Workgroup i is observed to run on XCD i % 8 (speed only, never correctness): give every XCD
  // one contiguous chunk of the (row, head, query block) sequence, query blocks innermost, so that the blocks which
  // stream the same K / V^T of one (row, head) share one 4 MB L2 instead of all eight fetching their own copy
  // (measured before: 3.6x the algorithmic HBM traffic).
  const int qblocks = (p.N + 128 * QG - 1) / (128 * QG);
  int v;
  {
    const int nb = (int)gridDim.x, bid = (int)blockIdx.x;
    const int xcd = bid & 7, seq = bid >> 3, q8 = nb >> 3, r8 = nb & 7;
    v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + seq;
  }
  const int qblk = v % qblocks;
  const int h = (v / qblocks) % p.heads, b = v / (qblocks * p.heads);
  const int bqk = p.qk_src ? p.qk_src[b] : b;                       // P2P self-replace: q and k of another row
  const int bk = p.kv_src ? p.kv_src[b] : bqk;                      // mutual self-attention: k and v of another row
  const int bv = p.kv_src ? p.kv_src[b] : b;
  const int q_base = qblk * (128 * QG) + wave * (32 * QG) + ql;

  // zero LDS once (pad rows of V^T must be finite zeros), then the row of ones
  for (int i = tid; i < C::TOTAL / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (ONES) {
    for (int i = tid; i < C::NSTG * 64; i += 256)
      reinterpret_cast<bf16_t*>(smem + (i >> 6) * C::STAGE + C::K_BYTES + D * 128)[i & 63] = ST_ONE_BITS;
  }

  // Q fragments (B operand): lane holds Q[q][ks*16 + hi*8 .. +8]; zero beyond D, so whatever the
  // K fragment read picks up in the pad columns (the next row's data) never contributes
  bf16x8 qf[QG][DK];
#pragma unroll
  for (int g = 0; g < QG; ++g) {
    const int q_row = q_base + g * 32;
    const bool q_ok = q_row < p.N;
    const bf16_t* qp = p.q + ((long)bqk * p.N + (q_ok ? q_row : 0)) * p.ldq + h * D;
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
      const int c = ks * 16 + hi * 8;
      union { u32x4 u; bf16x8 v; } x;
      x.u = (u32x4){0, 0, 0, 0};
      if (q_ok && c < D) x.u = *reinterpret_cast<const u32x4*>(qp + c);
      qf[g][ks] = x.v;
    }
  }

  // ---- DMA plan: instruction i = wave + 4n moves 1 KiB (64 lanes x 16 B) of the tile.  Everything
  // that does not depend on the tile is fixed here -- per-lane source pointer of tile 0, the
  // (wave-uniform) byte stride per tile and LDS target -- so that issuing a tile is three
  // instructions per DMA and free of branches: a wave whose last slot has no chunk to fetch
  // (TI % 4 != 0) re-fetches its previous chunk into a dump area behind the ring instead.
  // Buffer addressing (base descriptor in SGPRs + 32-bit lane offset + scalar tile offset): the
  // DMA needs no per-lane 64-bit pointer arithmetic at all and moves one address dword per lane
  // instead of two.
  unsigned dma_voff[C::NI];
  int dma_step[C::NI], dma_dst[C::NI];
  bool dma_is_k[C::NI];
#if defined(__HIP_DEVICE_COMPILE__)     // (the resource type only exists in the device pass)
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(p.k + (long)bk * p.N * p.ldk + h * D), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(p.vt + (long)h * D * p.ldvt + (long)bv * p.N), (short)0, 0x7fffffff, 0x00020000);
#endif
#pragma unroll
  for (int n = 0; n < C::NI; ++n) {
    const int i = wave + 4 * n;
    const bool real = i < C::TI;
    const int ii = real ? i : i - 4;                  // the chunk a dump slot re-fetches
    dma_is_k[n] = ii < C::KI;
    if (ii < C::KI) {
      const int s = ii * 64 + lane;
      const int row = s / C::DCH, cs = s - row * C::DCH;
      dma_voff[n] = (unsigned)(row * p.ldk + (cs ^ k_swz<D>(row)) * 8) * 2u;
      dma_step[n] = 128 * p.ldk;                      // bytes per 64 rows of K
      dma_dst[n] = ii * 1024;
    } else {
      const int s = (ii - C::KI) * 64 + lane;
      const int row = s >> 3, cs = s & 7;
      dma_voff[n] = (unsigned)(((long)row * p.ldvt + (cs ^ v_swz(row)) * 8) * 2);
      dma_step[n] = 128;                              // bytes per 64 columns of V^T
      dma_dst[n] = C::K_BYTES + (ii - C::KI) * 1024;
    }
    if (!real) dma_dst[n] = -1;
  }
  auto dma_tile = [&](int t, int stage) __attribute__((always_inline)) {
    char* sb = smem + stage * C::STAGE;
#pragma unroll
    for (int n = 0; n < C::NI; ++n) {
      char* dst = dma_dst[n] >= 0 ? sb + dma_dst[n] : smem + C::NSTG * C::STAGE + wave * 1024;
#if defined(__HIP_DEVICE_COMPILE__)
      if (dma_is_k[n])
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (__attribute__((address_space(3))) void*)dst, 16, dma_voff[n], t * dma_step[n], 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, (__attribute__((address_space(3))) void*)dst, 16, dma_voff[n], t * dma_step[n], 0, 0);
#else
      (void)dst;
#endif
    }
  };

  // ---- fragment addressing
  // K-tile row read by lane ql for S^T row ql of a half tile (see header): kv_perm
  // PV16 (d = 40): P.V on v_mfma_f32_16x16x32_bf16 -- O^T as 16-row tiles, 48 rows (40 + the ones row + pad) instead of
  // 64: six MFMAs of 16 cycles instead of four of 32 per unit, three b128 V^T reads instead of four.  Its B operand
  // wants lane l = 32 hi + 16 g + i to hold, for the 16 queries of group g', the 8 consecutive kv of block 2 hi + g.
  // The lane owns query 16 g + i with the blocks r = 0..7 and r = 8..15 of its S^T column; with the K rows permuted so
  // that block c of half hi is kv block 2 hi + c, one v_permlane16_swap per packed dword (block 0 of the g = 1 lanes
  // against block 1 of the g = 0 lanes) leaves "the block for queries 0..15" in the first and "the block for queries
  // 16..31" in the second register set of every lane.
#ifdef SA_NO_PV16   // measurement build: P.V on 32 x 32 x 16 tiles again (4 MFMAs of 32 cycles, no permlane16_swap)
  constexpr bool PV16 = false;
#else
  constexpr bool PV16 = D == 40 && QG == 2 && NS == 2;
#endif
  constexpr int DT16 = (D + 16) / 16;                   // 16-row tiles of O^T, the ones row included
  const int kv_perm = PV16 ? 16 * ((ql >> 2) & 1) + 8 * (ql >> 4) + 4 * ((ql >> 3) & 1) + (ql & 3)
                           : 16 * (ql >> 4) + 8 * ((ql >> 2) & 1) + 4 * ((ql >> 3) & 1) + (ql & 3);
  // byte offset (inside a stage) of the K fragment (sub, ks): the swizzle only touches the low
  // bits of the chunk index, so NPAR per-lane bases + compile-time offsets cover every ks
  constexpr int RS = C::DCH * 16;                       // K row stride
  constexpr int NPAR = D == 64 ? 4 : 2;
  int k_lane[NPAR];
#pragma unroll
  for (int par = 0; par < NPAR; ++par) {
    const int c = par * 2 + hi;
    k_lane[par] = kv_perm * RS + ((c ^ k_swz<D>(kv_perm)) * 16);
  }
  auto k_addr = [&](int sub, int ks) __attribute__((always_inline)) {
    return k_lane[ks % NPAR] + (ks / NPAR) * (NPAR * 32) + sub * 32 * RS;
  };
  // V^T fragment (dt, half) of sub: row dt*32+ql, chunk sub*4 + half*2 + hi
  int v_lane[2][2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int half = 0; half < 2; ++half)
      v_lane[sub][half] = C::K_BYTES + ql * 128 + (((sub * 4 + half * 2 + hi) ^ v_swz(ql)) * 16);
  auto v_addr = [&](int sub, int dt, int half) __attribute__((always_inline)) {
    return v_lane[sub][half] + dt * 4096;      // v_swz(dt*32 + ql) == v_swz(ql)
  };
  // PV16: A fragment of tile dt = row 16 dt + (lane & 15), the 8 kv of block lane >> 4 (one b128)
  int v16_lane[2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
    v16_lane[sub] = C::K_BYTES + (lane & 15) * 128 + (((sub * 4 + (lane >> 4)) ^ v_swz(lane & 15)) * 16);

  f32x16 o[NS][DT];
  f32x4 o16[NS][2][DT16];                               // PV16: [stream][16-query half][tile]
  bf16x8 vf16[DT16];
  float m_run[NS], l_run[NS];
  const int ntiles = p.N / 64;
  const int TU = ntiles * C::UT;
  __syncthreads();          // zero / ones fill done

  // Lazy rescale: the running maximum (log2 domain) of a stream is only raised -- and O, l
  // rescaled -- when some row's block maximum exceeds it by more than RESCALE_THR; until then
  // probabilities are formed against the stale maximum and are bounded by 2^RESCALE_THR (bf16 has
  // fp32's exponent range, fp32 accumulators: no precision is lost).
  constexpr float RESCALE_THR = 10.0f;

  // FOLD (head dims with pad columns in the QK^T contraction, i.e. d = 40): K gets a column of
  // ones and Q the column -m_run, so the MFMA delivers S - m_run directly and the 16 subtractions
  // per unit disappear.  m_run is kept bf16-representable so the shift is exact, and softmax is
  // invariant to WHICH shift a row uses as long as numerator and denominator share it.
  constexpr bool FOLD = H::DP > D;
  constexpr int KS_P = FOLD ? D / 16 : 0, HI_P = (D % 16) / 8;   // fragment / lane half holding column D
  static_assert(D % 8 == 0, "head dim must be a multiple of 8");

  f32x16 S[4];
  bf16x8 kf[DK], vf[DT][2], pfa[2], pfb[2];
  float mx_next;          // row max of the unit whose softmax comes next

  // unit U -> (tile, sub, stream a, query group g)
  auto unit_tile = [&](int U) __attribute__((always_inline)) { return QG == 2 ? (U >> 2) : (U >> 1); };
  auto stage_of = [&](int U) __attribute__((always_inline)) { return smem + (unit_tile(U) % C::NSTG) * C::STAGE; };

  auto read_kf = [&](const char* st, int sub) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(st + k_addr(sub, ks));
  };
  // FOLD: column D of K := 1 (the lanes of half HI_P read the next row's data there).  Applied
  // right before the fragment's first use so the LDS latency of read_kf stays covered.
  auto fix_kf = [&]() __attribute__((always_inline)) {
    union { u32x4 u; bf16x8 v; } x;
    x.v = kf[KS_P];
    const bool padl = hi == HI_P;
    x.u[0] = padl ? (uint32_t)ST_ONE_BITS : x.u[0];
    x.u[1] = padl ? 0u : x.u[1];
    x.u[2] = padl ? 0u : x.u[2];
    x.u[3] = padl ? 0u : x.u[3];
    kf[KS_P] = x.v;
  };
  auto set_q_shift = [&](int g, float m) __attribute__((always_inline)) {   // Q[:, D] := -m (bf16-exact)
    union { u32x4 u; bf16x8 v; } x;
    x.v = qf[g][KS_P];
    const uint32_t bits = st_exact_bits(-m);
    x.u[0] = (hi == HI_P) ? bits : x.u[0];
    qf[g][KS_P] = x.v;
  };
  auto read_vf = [&](const char* st, int sub) __attribute__((always_inline)) {
    if constexpr (PV16) {
#pragma unroll
      for (int dt = 0; dt < DT16; ++dt) vf16[dt] = *reinterpret_cast<const bf16x8*>(st + v16_lane[sub] + dt * 2048);
      return;
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      vf[dt][0] = *reinterpret_cast<const bf16x8*>(st + v_addr(sub, dt, 0));
      vf[dt][1] = *reinterpret_cast<const bf16x8*>(st + v_addr(sub, dt, 1));
    }
  };
  auto do_qk = [&](f32x16& s, int g) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) s = MFMA_32x32x16_ST(kf[ks], qf[g][ks], s, 0, 0, 0);
  };
  // running max over 4 more values of a score block (v_max3 x2; a plain fmaxf chain picks up
  // canonicalising v_max x,x pairs on the MFMA results)
  auto max4 = [&](float& m, const f32x16& sn, int c) __attribute__((always_inline)) {
    m = fmaxf(fmaxf(fmaxf(fmaxf(m, sn[4 * c + 0]), sn[4 * c + 1]), sn[4 * c + 2]), sn[4 * c + 3]);   // 2 x v_max3
    asm volatile("" : "+v"(m));     // pins the two v_max3 between the surrounding MFMAs
  };
  auto max_halves = [&](float mxa, float mxb) __attribute__((always_inline)) {
    float mx;
    mx = fmaxf(mxa, mxb);
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
  };

  // (re)start: accumulators, the ring's first tiles, scores of units 0 and 1, max of unit 0
  auto start = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      m_run[a] = FOLD ? 0.f : -1e30f;                      // FOLD: Q's pad column is 0: S - 0
      l_run[a] = 0.f;
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[a][t][r] = 0.f;
#pragma unroll
      for (int gq = 0; gq < 2; ++gq)
#pragma unroll
        for (int t = 0; t < DT16; ++t) o16[a][gq][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int t = 0; t < DT16; ++t) vf16[t] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (FOLD) {
#pragma unroll
      for (int g = 0; g < QG; ++g) set_q_shift(g, 0.f);
    }
    pfa[0] = pfa[1] = pfb[0] = pfb[1] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vf[dt][0] = vf[dt][1] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t <= C::PD && t < ntiles; ++t) dma_tile(t, t);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    read_kf(smem, 0);
    if (FOLD) fix_kf();
    do_qk(S[0], 0);
    if (QG == 1) { read_kf(smem, 1); if (FOLD) fix_kf(); }
    do_qk(S[1], QG == 2 ? 1 : 0);
    float mxa = -1e30f, mxb = -1e30f;
    max4(mxa, S[0], 0); max4(mxa, S[0], 1); max4(mxb, S[0], 2); max4(mxb, S[0], 3);
    mx_next = max_halves(mxa, mxb);
  };

  // one pipelined block; J = U mod 4 is compile-time
  // PINNED (see "Pinned shift" below): no row maximum, no rescale -- the stream keeps the shift it has
  auto block = [&](auto jc, auto guard, auto pinned, int U) __attribute__((always_inline)) {
    constexpr int J = decltype(jc)::value;
    constexpr bool GUARD = decltype(guard)::value;        // tail iteration: units U+1, U+2 may not exist
    constexpr bool PINNED = decltype(pinned)::value;
    constexpr int JJ = QG == 2 ? J : (J & 1);             // index inside the tile
    constexpr int SUB = QG == 2 ? (JJ >> 1) : JJ;
    constexpr int A = NS == 2 ? (J & 1) : 0;              // stream of unit U
    constexpr int AP = NS == 2 ? (A ^ 1) : 0;             // stream of unit U-1
    constexpr int JN = (J + 2) & 3;                       // unit U+2
    constexpr int SUBN = QG == 2 ? (JN >> 1) : (JN & 1);
    constexpr int GN = QG == 2 ? (JN & 1) : 0;
    bf16x8 (&pf_prev)[2] = (J & 1) ? pfa : pfb;           // P of unit U-1
    bf16x8 (&pf_cur)[2] = (J & 1) ? pfb : pfa;
    const char* st_cur = stage_of(U);

    // (Round 2 issued every MFMA between s_setprio 1 / 0: on a two-wave SIMD a prioritised MFMA kept the matrix pipe fed,
    // 88 -> 70 cycles for [MFMA + 6 VALU] x 2 in tools/ubench/overlap.hip.  With today's loop -- 92 instructions per unit,
    // the SIMD's issue slots the scarce resource, DESIGN.md 5.0 item 7 -- the 14 s_setprio per unit cost more than the
    // priority buys: 2.1 % faster without them at d = 40, 1.5 % at d = 80.)
    auto mfma_hi = [&](const bf16x8& x, const bf16x8& y, f32x16& acc) __attribute__((always_inline)) {
      acc = MFMA_32x32x16_ST(x, y, acc, 0, 0, 0);
    };
    constexpr int NPV = PV16 ? 2 * DT16 : 2 * DT;
    // with a single stream the P.V of unit U-1 (formed against the old maximum) has to be
    // accumulated before the rescale for unit U
    if (NS == 1) {
#pragma unroll
      for (int i = 0; i < NPV; ++i) mfma_hi(vf[i % DT][i / DT], pf_prev[i / DT], o[AP][i % DT]);
    }
    // 1. lazy rescale of stream A for unit U.  mx_next: FOLD ? max(S - m_run) : max(S)
    if (!PINNED) {
      const float over = FOLD ? mx_next : mx_next - m_run[A];
      const bool first = FOLD && U < 2;                   // pins the shift to the first block's max
      if (first || !__all(over <= RESCALE_THR)) {
        float alpha;
        if (FOLD) {
          const float m_new = (float)(st_elem_t)(m_run[A] + fmaxf(over, first ? -1e30f : 0.f));
          const float delta = m_new - m_run[A];
          alpha = fast_exp2(-delta);
          m_run[A] = m_new;
#pragma unroll
          for (int r = 0; r < 16; ++r) S[J][r] -= delta;
          set_q_shift(QG == 2 ? A : 0, m_new);
        } else {
          const float m_new = fmaxf(m_run[A], mx_next);
          alpha = fast_exp2(m_run[A] - m_new);
          m_run[A] = m_new;
        }
        l_run[A] *= alpha;
        if constexpr (PV16) {      // this lane's accumulators belong to queries 16 g' + (lane & 15): their owners' factors
#pragma unroll
          for (int gq = 0; gq < 2; ++gq) {
            const float al = __shfl(alpha, (lane & 32) + 16 * gq + (lane & 15), 64);
#pragma unroll
            for (int dt = 0; dt < DT16; ++dt) o16[A][gq][dt] *= al;
          }
        } else {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[A][dt][r] *= alpha;
        }
      }
    }
    const bool has2 = !GUARD || U + 2 < TU;
    const bool has1 = !GUARD || U + 1 < TU;
    // 2. K fragments of unit U+2 (shared by a pair of units when QG == 2)
    if (has2 && (QG == 1 || (JN & 1) == 0)) read_kf(stage_of(U + 2), SUBN);

    // 3. the block's MFMAs -- P.V of unit U-1 (other stream) and QK^T of unit U+2, merged so
    // that no MFMA directly follows the one it depends on -- with the exp/pack work of unit U and
    // the row max of unit U+1 cut into 8 chunks and spread over the gaps
    union { uint32_t u[4]; bf16x8 v; } pk[2];
    float ls = 0.f, mxa = -1e30f, mxb = -1e30f;
    // piece i of 8: probabilities 2i, 2i+1 of unit U (2 exp + 1 pack) and, for odd i, 4 more
    // values of the row max of unit U+1.  The empty volatile asm after each piece keeps it where
    // it is written (the compiler would otherwise collect this pure work behind the last MFMA of
    // the block).  NOTE: the VALU work itself must stay compiler-visible -- instructions inside
    // inline asm get none of the software-managed MFMA hazard padding (XDL result read / source
    // overwrite), which showed up as run-to-run differences when these pieces were asm.
    auto valu_piece = [&](int i) __attribute__((always_inline)) {
      const float e0 = fast_exp2(FOLD ? S[J][2 * i] : S[J][2 * i] - m_run[A]);
      const float e1 = fast_exp2(FOLD ? S[J][2 * i + 1] : S[J][2 * i + 1] - m_run[A]);
      uint32_t p0 = pack_bf16x2(e0, e1);
      asm volatile("" : "+v"(p0));
      if (!ONES) ls += e0 + e1;
      pk[i >> 2].u[i & 3] = p0;
      if (!PINNED && (i & 1) && has1) max4((i >> 1) < 2 ? mxa : mxb, S[(J + 1) & 3], i >> 1);
    };
    constexpr int NPVS = NS == 2 ? NPV : 0;                // P.V MFMAs still to issue here
    constexpr int NM = NPVS + DK;
    if (has2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) S[JN][r] = 0.f;
    }
#if SA_BURST
    if (SA_BURST & 2) __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
    for (int sl = 0; sl < NM; ++sl) {
      const int qk_before = (sl * DK) / NM, qk_after = ((sl + 1) * DK) / NM;
      if (qk_after > qk_before) {
        if (has2) {
          if (FOLD && qk_before == KS_P && (QG == 1 || (JN & 1) == 0)) fix_kf();
          mfma_hi(kf[qk_before], qf[GN][qk_before], S[JN]);
        }
      } else {
        const int i = sl - qk_before;                      // index among the P.V MFMAs
        if constexpr (PV16)
          o16[AP][i / DT16][i % DT16] = MFMA_16x16x32_ST(vf16[i % DT16], pf_prev[i / DT16], o16[AP][i / DT16][i % DT16], 0, 0, 0);
        else
          mfma_hi(vf[i % DT][i / DT], pf_prev[i / DT], o[AP][i % DT]);
        // V^T fragments of unit U (kept for the pair when QG == 2) once the last P.V is issued
        if (i == NPVS - 1 && (QG == 1 || (JJ & 1) == 0)) read_vf(st_cur, SUB);
      }
#if !SA_BURST
#pragma unroll
      for (int c = (sl * 8) / NM; c < ((sl + 1) * 8) / NM; ++c) valu_piece(c);
#endif
    }
#if SA_BURST
    // measurement build: the block's MFMAs as one burst, then its VALU work as one phase (two waves of a SIMD can then run in
    // anti-phase: one bursting on the matrix pipe, the other on the VALU port)
    if (SA_BURST & 2) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 8; ++c) valu_piece(c);
    __builtin_amdgcn_sched_barrier(0);
#endif
    if (NS == 1 && (QG == 1 || (JJ & 1) == 0)) read_vf(st_cur, SUB);
    if (!ONES) l_run[A] += ls;
    if constexpr (PV16) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const auto sw = __builtin_amdgcn_permlane16_swap(pk[0].u[w], pk[1].u[w], false, false);
        pk[0].u[w] = sw[0];
        pk[1].u[w] = sw[1];
      }
    }
    pf_cur[0] = pk[0].v;
    pf_cur[1] = pk[1].v;
    // keep the exp/pack work HERE: its only consumer is the P.V in the next block, and LLVM
    // would otherwise sink it across the rescale branch right in front of those MFMAs
    asm volatile("" : "+v"(pf_cur[0]), "+v"(pf_cur[1]));
    if (!PINNED && has1) {
      mx_next = max_halves(mxa, mxb);
      asm volatile("" : "+v"(mx_next));
    }
  };

  // tile hand-over before the block that first touches tile tn: everyone's DMA for it has landed,
  // and nobody reads tile tn-2 any more -> its stage takes tile tn+1
  // DMA instructions this wave issues per tile (instruction i = wave + 4n < TI): the vmcnt that lets
  // exactly one younger tile stay in flight
  constexpr int my_dma = C::NI;
  auto hand_over = [&](int tn) __attribute__((always_inline)) {
    if (tn < ntiles) {
      if (C::PD == 2 && tn + 1 < ntiles) {
        // (test twin of the schedule, tests/test_gpu_ring_hazard.py: everything in flight lands before the barrier)
        if (p.test_flags & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // tile tn has landed when at most the DMAs of tile tn+1 are outstanding
        if (my_dma == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (my_dma == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (my_dma == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_barrier" ::: "memory");
      if (tn + C::PD < ntiles) dma_tile(tn + C::PD, (tn + C::PD) % C::NSTG);
    }
  };

  using std::integral_constant;
  using std::false_type;
  using std::true_type;
  // Pinned shift.  Softmax is invariant to the shift a row uses, and bf16 / fp32 carry 2^+-127: once a stream has a shift
  // from its first units (the maximum over their 32 or 64 kv rows), tracking the running maximum only guards against
  // scores that exceed it by ~2^100 -- which the row's denominator reveals afterwards.  So a pass with PIN = true runs the
  // first four units with the full max / rescale logic and every later unit with none (8 v_max3, the cross-half exchange,
  // the compare and the branch: 13 of ~42 VALU instructions per unit, on a kernel whose VALU and matrix pipes are both
  // ~70 % busy), and the caller checks the denominators: a block in which any row's denominator reached 2^60 (or is not
  // finite) repeats its work with PIN = false -- the exact online softmax, whatever the scores.  Which path a block takes
  // depends on its own rows only, so results stay independent of the batch.
  auto pass = [&](auto pin) __attribute__((always_inline)) {
    constexpr bool PIN = decltype(pin)::value;
    start();
    int U = 0;
    if (PIN) {                         // (the caller guarantees TU >= 6)
      if (QG == 1) hand_over((U >> 1) + 1);
      block(integral_constant<int, 0>{}, false_type{}, false_type{}, U);
      block(integral_constant<int, 1>{}, false_type{}, false_type{}, U + 1);
      if (QG == 2) hand_over((U >> 2) + 1); else hand_over((U >> 1) + 2);
      block(integral_constant<int, 2>{}, false_type{}, false_type{}, U + 2);
      block(integral_constant<int, 3>{}, false_type{}, false_type{}, U + 3);
      U = 4;
    }
    for (; U + 6 <= TU; U += 4) {      // every unit up to U+5 exists: no guards inside
      if (QG == 1) hand_over((U >> 1) + 1);
      block(integral_constant<int, 0>{}, false_type{}, pin, U);
      block(integral_constant<int, 1>{}, false_type{}, pin, U + 1);
      if (QG == 2) hand_over((U >> 2) + 1); else hand_over((U >> 1) + 2);
      block(integral_constant<int, 2>{}, false_type{}, pin, U + 2);
      block(integral_constant<int, 3>{}, false_type{}, pin, U + 3);
    }
    {                                  // tail: the last 2 or 4 units
      if (QG == 1) hand_over((U >> 1) + 1);
      block(integral_constant<int, 0>{}, true_type{}, pin, U);
      block(integral_constant<int, 1>{}, true_type{}, pin, U + 1);
      if (U + 2 < TU) {
        if (QG == 2) hand_over((U >> 2) + 1); else hand_over((U >> 1) + 2);
        block(integral_constant<int, 2>{}, true_type{}, pin, U + 2);
        block(integral_constant<int, 3>{}, true_type{}, pin, U + 3);
      }
    }
    // drain: P.V of the last unit (stream 1; TU is even)
    {
      bf16x8 (&pf_last)[2] = pfb;    // the last unit is odd: its block packed into pfb
      constexpr int AL = NS - 1;
      if constexpr (PV16) {
#pragma unroll
        for (int gq = 0; gq < 2; ++gq)
#pragma unroll
          for (int dt = 0; dt < DT16; ++dt)
            o16[AL][gq][dt] = MFMA_16x16x32_ST(vf16[dt], pf_last[gq], o16[AL][gq][dt], 0, 0, 0);
      } else {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[AL][dt] = MFMA_32x32x16_ST(vf[dt][0], pf_last[0], o[AL][dt], 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[AL][dt] = MFMA_32x32x16_ST(vf[dt][1], pf_last[1], o[AL][dt], 0, 0, 0);
      }
    }
  };

  constexpr int dl = D - (DT - 1) * 32;            // pad row D inside the last tile (ONES)
  constexpr int r1 = (dl & 3) + 4 * (dl >> 3);
  constexpr int h1 = (dl >> 2) & 1;
  // PV16: row D of O^T is row D % 16 of tile D / 16 = register D % 4 of the lanes with lane >> 4 == (D % 16) / 4
  auto denom16 = [&](int a, int gq) __attribute__((always_inline)) {
    return __shfl(o16[a][gq][D / 16][D % 4], 16 * ((D % 16) / 4) + (lane & 15), 64);
  };
  auto denom = [&](int a) __attribute__((always_inline)) {
    if (ONES) return __shfl(o[a][DT - 1][ONES ? r1 : 0], ql + 32 * h1, 64);
    return l_run[a] + __shfl_xor(l_run[a], 32, 64);
  };
  auto write_out = [&](const f32x16 (&acc)[DT], float inv, int q_row) __attribute__((always_inline)) {
    if (q_row < p.N) {
      bf16_t* op = p.out + ((long)b * p.N + q_row) * p.ldo + h * D;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const int d0 = dt * 32 + 8 * gg + 4 * hi;
          if (d0 < D) {
            uint2 w;
            w.x = pack_bf16x2(acc[dt][gg * 4 + 0] * inv, acc[dt][gg * 4 + 1] * inv);
            w.y = pack_bf16x2(acc[dt][gg * 4 + 2] * inv, acc[dt][gg * 4 + 3] * inv);
            *reinterpret_cast<uint2*>(op + d0) = w;
          }
        }
    }
  };
  {
    // (d = 64 keeps the exact pass only: with its 244 registers the two passes' live ranges no longer fit 256)
    constexpr bool CAN_PIN = D != 64;
    int redo = 1;
    if (CAN_PIN && TU >= 6 && !(p.test_flags & 2)) {
      pass(true_type{});
      bool bad = false;
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        // (half storage: a probability must stay below 65504, so a denominator of 2^15 already sends the block to the exact pass)
        constexpr float DEN_MAX = HEDIT_F16 ? 0x1p15f : 0x1p60f;
        if constexpr (PV16) bad |= !(denom16(a, 0) < DEN_MAX) || !(denom16(a, 1) < DEN_MAX);
        else bad |= !(denom(a) < DEN_MAX);
      }
      redo = __syncthreads_or(bad ? 1 : 0);        // (also: nobody reads the ring any more)
    }
    if (redo) pass(false_type{});
  }
  if constexpr (PV16) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int gq = 0; gq < 2; ++gq) {
        const float inv = 1.0f / denom16(g, gq);
        const int q_row = qblk * (128 * QG) + wave * (32 * QG) + g * 32 + gq * 16 + (lane & 15);
        if (q_row < p.N) {
          bf16_t* op = p.out + ((long)b * p.N + q_row) * p.ldo + h * D;
#pragma unroll
          for (int dt = 0; dt < DT16; ++dt) {
            const int d0 = dt * 16 + 4 * (lane >> 4);
            if (d0 < D) {
              uint2 w;
              w.x = pack_bf16x2(o16[g][gq][dt][0] * inv, o16[g][gq][dt][1] * inv);
              w.y = pack_bf16x2(o16[g][gq][dt][2] * inv, o16[g][gq][dt][3] * inv);
              *reinterpret_cast<uint2*>(op + d0) = w;
            }
          }
        }
      }
  } else if (QG == 2) {
#pragma unroll
    for (int g = 0; g < 2; ++g) write_out(o[g], 1.0f / denom(g), q_base + g * 32);
  } else {
    if (NS == 2) {   // merge the two KV-half streams
      const float m = fmaxf(m_run[0], m_run[NS - 1]);
      const float f0 = fast_exp2(m_run[0] - m), f1 = fast_exp2(m_run[NS - 1] - m);
      if (!ONES) l_run[0] = l_run[0] * f0 + l_run[NS - 1] * f1;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[0][dt][r] = o[0][dt][r] * f0 + o[NS - 1][dt][r] * f1;
    }
    write_out(o[0], 1.0f / denom(0), q_base);
  }
}

template <int D, int QG, int NS>
int launch_self(const SelfAttnParams& p, hipStream_t st) {
  using C = SelfCfg<D, QG>;
#ifdef SA_OCC1      // measurement build: one workgroup per CU (one wave per SIMD) through an LDS request two cannot share
  constexpr int LDS = C::TOTAL > 84 * 1024 ? C::TOTAL : 84 * 1024;
#else
  constexpr int LDS = C::TOTAL;
#endif
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&self_attn_kernel<D, QG, NS>), LDS)) return rc;
  dim3 grid(cdiv(p.N, 128 * QG) * p.heads * p.B);
  hipLaunchKernelGGL((self_attn_kernel<D, QG, NS>), grid, dim3(256), LDS, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

// ============================================================================ cross-attention
constexpr int CTXP = HEDIT_CTXP;
constexpr int WS = 100;    // LDS row stride (elements) of the 96-wide V^T and mix tiles

template <int D>
struct CrossSmem {
  using H = HeadCfg<D>;
  static constexpr int K_BYTES = 96 * H::KS * 2;
  static constexpr int V_BYTES = H::DT * 32 * WS * 2;
  static constexpr int MIX_BYTES = 96 * WS * 2;
  static constexpr int BV_BYTES = 96 * 4;
  static constexpr int TOTAL = K_BYTES + V_BYTES + MIX_BYTES + BV_BYTES;
};

template <int D>
__global__ __launch_bounds__(256, (D <= 80 ? 2 : 1)) void cross_attn_kernel(CrossAttnParams p) {
  using H = HeadCfg<D>;
  using S = CrossSmem<D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sK = reinterpret_cast<bf16_t*>(smem);
  bf16_t* sV = reinterpret_cast<bf16_t*>(smem + S::K_BYTES);
  bf16_t* sM = reinterpret_cast<bf16_t*>(smem + S::K_BYTES + S::V_BYTES);
  float* sB = reinterpret_cast<float*>(smem + S::K_BYTES + S::V_BYTES + S::MIX_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y;
  const int item = blockIdx.z;
  const bool is_pair = item < p.n_pairs;
  const int b0 = is_pair ? p.pair_src[item] : p.singles[item - p.n_pairs];
  const int b1 = is_pair ? p.pair_tar[item] : -1;
  const int q_row = blockIdx.x * 128 + wave * 32 + ql;
  const bool q_ok = q_row < p.N;

  for (int i = tid; i < (S::K_BYTES + S::V_BYTES) / 8; i += 256) reinterpret_cast<uint2*>(smem)[i] = make_uint2(0, 0);
  if (is_pair) {
    // mixing matrix (already transposed: mixT[n][w]) and bvec of this pair
    const bf16_t* src = p.mixT + (long)item * 96 * 96;
    for (int i = tid; i < 96 * 12; i += 256) {
      const int row = i / 12, c = i - row * 12;
      const uint4 u = *reinterpret_cast<const uint4*>(src + row * 96 + c * 8);
      uint2* dst = reinterpret_cast<uint2*>(sM + row * WS + c * 8);
      dst[0] = make_uint2(u.x, u.y);
      dst[1] = make_uint2(u.z, u.w);
    }
    if (tid < 96) sB[tid] = p.bvec[(long)item * 96 + tid];
  }
  __syncthreads();

  auto stage = [&](int b) {
    const bf16_t* kbase = p.k + (long)b * CTXP * p.ldk + h * D;
    for (int idx = tid; idx < CTXP * H::DCH; idx += 256) {
      const int row = idx / H::DCH, c = idx - row * H::DCH;
      *reinterpret_cast<uint4*>(sK + row * H::KS + c * 8) =
          *reinterpret_cast<const uint4*>(kbase + (long)row * p.ldk + c * 8);
    }
    const bf16_t* vbase = p.vt + (long)h * D * p.ldvt + (long)b * CTXP;
    for (int idx = tid; idx < D * (CTXP / 8); idx += 256) {
      const int row = idx / (CTXP / 8), c = idx - row * (CTXP / 8);
      const uint4 u = *reinterpret_cast<const uint4*>(vbase + (long)row * p.ldvt + c * 8);
      uint2* dst = reinterpret_cast<uint2*>(sV + row * WS + c * 8);
      dst[0] = make_uint2(u.x, u.y);
      dst[1] = make_uint2(u.z, u.w);
    }
  };

  auto load_q = [&](int b, bf16x8* qf) {
    const bf16_t* qp = p.q + ((long)b * p.N + (q_ok ? q_row : 0)) * p.ldq + h * D;
#pragma unroll
    for (int ks = 0; ks < H::DK; ++ks) {
      const int c = ks * 16 + hi * 8;
      union { uint4 u; bf16x8 v; } x;
      x.u = make_uint4(0, 0, 0, 0);
      if (q_ok && c < D) x.u = *reinterpret_cast<const uint4*>(qp + c);
      qf[ks] = x.v;
    }
  };

  // exact softmax over the 77 valid keys; returns normalised probabilities in pr[3][16]
  auto probs = [&](const bf16x8* qf, float (*pr)[16]) {
    float mx = -1e30f;
#pragma unroll
    for (int nt = 0; nt < 3; ++nt) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < H::DK; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (nt * 32 + ql) * H::KS + ks * 16 + hi * 8);
        s = MFMA_32x32x16_ST(kf, qf[ks], s, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float v = n < HEDIT_MAXW ? s[r] : -1e30f;
        pr[nt][r] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float ls = 0.f;
#pragma unroll
    for (int nt = 0; nt < 3; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { pr[nt][r] = fast_exp2(pr[nt][r] - mx); ls += pr[nt][r]; }
    ls += __shfl_xor(ls, 32, 64);
    const float inv = 1.0f / ls;
#pragma unroll
    for (int nt = 0; nt < 3; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) pr[nt][r] *= inv;
  };

  auto accumulate_store = [&](int which, float (*pr)[16]) {
    if (p.store == nullptr || !q_ok) return;
    float* dst = p.store + ((((long)item * 2 + which) * p.heads + h) * p.N + q_row) * HEDIT_MAXW;
#pragma unroll
    for (int nt = 0; nt < 3; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (n < HEDIT_MAXW) dst[n] += pr[nt][r];
      }
  };

  auto pv_and_write = [&](int b, const bf16x8 (*pf)[2]) {
    f32x16 o[H::DT];
#pragma unroll
    for (int dt = 0; dt < H::DT; ++dt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
      for (int nt = 0; nt < 3; ++nt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 vf = read_perm_frag(sV, dt * 32 + ql, WS, nt * 32 + 16 * s2 + 4 * hi);
          o[dt] = MFMA_32x32x16_ST(vf, pf[nt][s2], o[dt], 0, 0, 0);
        }
    }
    if (q_ok) {
      bf16_t* op = p.out + ((long)b * p.N + q_row) * p.ldo + h * D;
#pragma unroll
      for (int dt = 0; dt < H::DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d0 = dt * 32 + 8 * g + 4 * hi;
          if (d0 < D) {
            uint2 w;
            w.x = pack_bf16x2(o[dt][g * 4 + 0], o[dt][g * 4 + 1]);
            w.y = pack_bf16x2(o[dt][g * 4 + 2], o[dt][g * 4 + 3]);
            *reinterpret_cast<uint2*>(op + d0) = w;
          }
        }
    }
  };

  bf16x8 qf[H::DK];
  float pr[3][16];
  bf16x8 pf[3][2];

  // ---- first (or only) row
  stage(b0);
  __syncthreads();
  load_q(b0, qf);
  probs(qf, pr);
  if (is_pair) accumulate_store(0, pr);
#pragma unroll
  for (int nt = 0; nt < 3; ++nt) { pf[nt][0] = pack_p8(pr[nt]); pf[nt][1] = pack_p8(pr[nt] + 8); }
  pv_and_write(b0, pf);
  if (!is_pair) return;

  // ---- mixed source part of the target probabilities: mix[n][q] = sum_w mixT[n][w] P_src[w][q]
  f32x16 mix[3];
#pragma unroll
  for (int nt = 0; nt < 3; ++nt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) mix[nt][r] = 0.f;
#pragma unroll
    for (int wt = 0; wt < 3; ++wt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 mf = read_perm_frag(sM, nt * 32 + ql, WS, wt * 32 + 16 * s2 + 4 * hi);
        mix[nt] = MFMA_32x32x16_ST(mf, pf[wt][s2], mix[nt], 0, 0, 0);
      }
  }
  __syncthreads();          // everyone is done with the source K / V^T
  stage(b1);
  __syncthreads();
  load_q(b1, qf);
  probs(qf, pr);
#pragma unroll
  for (int nt = 0; nt < 3; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(sB + nt * 32 + 8 * g + 4 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) pr[nt][g * 4 + j] = mix[nt][g * 4 + j] + bv[j] * pr[nt][g * 4 + j];
    }
  accumulate_store(1, pr);
#pragma unroll
  for (int nt = 0; nt < 3; ++nt) { pf[nt][0] = pack_p8(pr[nt]); pf[nt][1] = pack_p8(pr[nt] + 8); }
  pv_and_write(b1, pf);
}

template <int D>
int launch_cross(const CrossAttnParams& p, hipStream_t st) {
  using S = CrossSmem<D>;
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&cross_attn_kernel<D>), S::TOTAL)) return rc;
  dim3 grid(cdiv(p.N, 128), p.heads, p.n_pairs + p.n_single);
  hipLaunchKernelGGL((cross_attn_kernel<D>), grid, dim3(256), S::TOTAL, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

// ============================================================================ materialised probabilities
// The slow path behind hedit_unet_set_attn_hook: a controller written in the host language sees (and may rewrite) the
// attention probabilities the way the reference's processor hands them over (ptp_utils.py:98-106: `attention_probs`
// [batch * heads][queries][keys], softmax done, before the product with V).  Two plain kernels, fp32 probabilities in HBM,
// no MFMA: this path exists for protocol coverage, the edits that matter run inside the fused kernels above.
//
// probs: one block = 16 queries of one (batch row, head).  Scores in log2 units (Q is pre-scaled), softmax over the keys
// in three passes over the block's own 16 rows of the output.
// STORE = the fused path's <= 32 x 32 SELF maps (AttentionStore on save_attn passes, ptp_classes.py:135-150): the block's 16
// score rows live in LDS (M <= 1024: 64 KB), the probabilities of the conditional rows -- pair p's source and target row,
// the target reading the source's q and k inside the self-replace window (qk_src) -- are ADDED to the store
// [n_pairs][2][heads][N][M] (the sum over steps the reference's between_steps forms); nothing else is written.
template <bool STORE>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnProbsParams p) {
  __shared__ float qs[16][168];
  extern __shared__ float sc_rows[];             // STORE: [16][M]
  const int bh = blockIdx.y, h = bh % p.heads;
  int b = bh / p.heads;
  if constexpr (STORE) {
    const int pair = b >> 1;
    b = (b & 1) ? p.pair_tar[pair] : p.pair_src[pair];
  }
  const int bq = (STORE && p.qk_src) ? p.qk_src[b] : b;        // whose q and k this row attends with
  const int q0 = blockIdx.x * 16, tid = threadIdx.x;
  for (int i = tid; i < 16 * p.d; i += 256) {
    const int r = i / p.d, c = i % p.d;
    const int q = q0 + r;
    qs[r][c] = q < p.N ? bf16_to_f32(p.q[((long)bq * p.N + q) * p.ldq + h * p.d + c]) : 0.f;
  }
  __syncthreads();
  float* out = STORE ? sc_rows : p.probs + ((long)bh * p.N + q0) * p.M;
  const int rows = min(16, p.N - q0);
  for (int m = tid; m < p.M; m += 256) {
    const bf16_t* kp = p.k + ((long)bq * p.kstride + m) * p.ldk + h * p.d;
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int c = 0; c < p.d; c += 8) {
      const uint4 raw = *reinterpret_cast<const uint4*>(kp + c);
      const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float kv = (j & 1) ? st_hi(w[j >> 1]) : st_lo(w[j >> 1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += qs[r][c + j] * kv;
      }
    }
    for (int r = 0; r < rows; ++r) out[(long)r * p.M + m] = acc[r];
  }
  __syncthreads();
  // softmax of row r by wave r % 4 (base 2: the scores carry log2 e)
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < rows; r += 4) {
    float* row = out + (long)r * p.M;
    float mx = -3.0e38f;
    for (int m = lane; m < p.M; m += 64) mx = fmaxf(mx, row[m]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int m = lane; m < p.M; m += 64) {
      const float e = exp2f(row[m] - mx);
      row[m] = e;
      sum += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.0f / sum;
    if constexpr (STORE) {
      float* acc_row = p.probs + ((long)bh * p.N + q0 + r) * p.M;
      for (int m = lane; m < p.M; m += 64) acc_row[m] += row[m] * inv;
    } else {
      for (int m = lane; m < p.M; m += 64) row[m] *= inv;
    }
  }
}

// apply: out[q][h*d + dd] = sum_m probs[bh][q][m] * V^T[h*d + dd][b*kstride + m]; one block = 16 queries of one (b, h),
// the keys in chunks of 64 through LDS.
__global__ __launch_bounds__(256) void attn_apply_kernel(AttnProbsParams p) {
  constexpr int CH = 64;
  __shared__ float ps[16][CH + 1];
  __shared__ float vs[160][CH + 1];
  const int bh = blockIdx.y, b = bh / p.heads, h = bh % p.heads;
  const int q0 = blockIdx.x * 16, tid = threadIdx.x;
  const int rows = min(16, p.N - q0), d = p.d;
  const int nout = 16 * d;                     // (query, channel) pairs of the block: thread t owns t, t + 256, ...
  float acc[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) acc[i] = 0.f;
  const float* pin = p.probs + ((long)bh * p.N + q0) * p.M;
  for (int m0 = 0; m0 < p.M; m0 += CH) {
    const int mc = min(CH, p.M - m0);
    for (int i = tid; i < 16 * CH; i += 256) {
      const int r = i / CH, c = i % CH;
      ps[r][c] = (r < rows && c < mc) ? pin[(long)r * p.M + m0 + c] : 0.f;
    }
    for (int i = tid; i < d * CH; i += 256) {
      const int r = i / CH, c = i % CH;
      vs[r][c] = c < mc ? bf16_to_f32(p.vt[(long)(h * d + r) * p.ldvt + (long)b * p.kstride + m0 + c]) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int o = tid + i * 256;
      if (o < nout) {
        const int r = o / d, c = o % d;
        float a = acc[i];
        for (int m = 0; m < CH; ++m) a += ps[r][m] * vs[c][m];
        acc[i] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int o = tid + i * 256;
    if (o < nout) {
      const int r = o / d, c = o % d;
      if (r < rows) p.out[((long)b * p.N + q0 + r) * p.ldo + h * d + c] = f32_to_bf16(acc[i]);
    }
  }
}

}  // namespace

int attn_probs_launch(const AttnProbsParams& p, hipStream_t st) {
  ARG_CHECK(p.d % 8 == 0 && p.d <= 160, "attn_probs: head dim must be a multiple of 8, at most 160");
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0, "attn_probs: strides");
  ARG_CHECK(p.M > 0 && p.N > 0 && p.M <= p.kstride, "attn_probs: extents");
  hipLaunchKernelGGL(attn_probs_kernel<false>, dim3(cdiv(p.N, 16), p.B * p.heads), dim3(256), 0, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

// p.probs = the store [n_pairs][2][heads][N][M] (accumulated into), p.B = n_pairs
int attn_self_store_launch(const AttnProbsParams& p, hipStream_t st) {
  ARG_CHECK(p.d % 8 == 0 && p.d <= 160 && p.ldq % 8 == 0 && p.ldk % 8 == 0, "attn_self_store: head dim / strides");
  ARG_CHECK(p.M > 0 && p.N > 0 && p.M <= 1024 && p.M <= p.kstride && p.pair_src && p.pair_tar && p.probs, "attn_self_store: extents");
  const int lds = 16 * p.M * (int)sizeof(float);
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&attn_probs_kernel<true>), lds)) return rc;
  hipLaunchKernelGGL(attn_probs_kernel<true>, dim3(cdiv(p.N, 16), 2 * p.B * p.heads), dim3(256), lds, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

int attn_apply_launch(const AttnProbsParams& p, hipStream_t st) {
  ARG_CHECK(p.d % 8 == 0 && p.d <= 160, "attn_apply: head dim must be a multiple of 8, at most 160");
  ARG_CHECK(p.M > 0 && p.N > 0 && p.M <= p.kstride, "attn_apply: extents");
  hipLaunchKernelGGL(attn_apply_kernel, dim3(cdiv(p.N, 16), p.B * p.heads), dim3(256), 0, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

int self_attn_launch(const SelfAttnParams& p_in, hipStream_t st) {
  SelfAttnParams p = p_in;
  p.test_flags = hedit_test_flags();       // 0 outside tests/test_gpu_ring_hazard.py
  ARG_CHECK(p.N % 64 == 0, "self_attn: N must be a multiple of 64");
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldvt % 8 == 0 && p.ldo % 4 == 0, "self_attn: strides");
  switch (p.d) {
    case 32: return launch_self<32, 2, 2>(p, st);
    case 40: return launch_self<40, 2, 2>(p, st);
    case 64: return launch_self<64, 2, 2>(p, st);
    case 80: return launch_self<80, 1, 1>(p, st);
    case 160: return launch_self<160, 1, 1>(p, st);
    default:
      hedit_set_error("self_attn: unsupported head dim " + std::to_string(p.d) + " (32,40,64,80,160)");
      return HEDIT_ERR_ARG;
  }
}

int cross_attn_launch(const CrossAttnParams& p, hipStream_t st) {
  ARG_CHECK(p.n_pairs + p.n_single > 0, "cross_attn: nothing to do");
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldvt % 8 == 0 && p.ldo % 4 == 0, "cross_attn: strides");
  switch (p.d) {
    case 32: return launch_cross<32>(p, st);
    case 40: return launch_cross<40>(p, st);
    case 64: return launch_cross<64>(p, st);
    case 80: return launch_cross<80>(p, st);
    case 160: return launch_cross<160>(p, st);
    default:
      hedit_set_error("cross_attn: unsupported head dim " + std::to_string(p.d) + " (32,40,64,80,160)");
      return HEDIT_ERR_ARG;
  }
}
