// Multi-head attention backward without a T x T tensor in HBM (flash style): what the input gradient of the SD UNet needs at
// its 64 x 64 level, where the single-head attention_bwd of blocks.h would write six 4096 x 4096 buffers per image and head.
//
// Operands in the forward's layouts (SelfAttnParams): q, k as [B*N][ld] with head h at column h*d, q PRE-SCALED by
// scale*log2(e); v row-major like k; dO and O as [B*N][ld].  In the exp2 domain, with s = q'.k:
//     P = 2^(s - lse),  lse = m + log2(l)        delta_i = sum_d dO_id O_id        dP = dO V^T
//     dS = ln2 P o (dP - delta)                  dq' = dS K      dk = dS^T q'      dv = P^T dO
// dq' is the gradient with respect to the pre-scaled q: multiplying by the (scaled) W_q^T afterwards needs no further factor.
//
// Two kernels, every output element ONE fp32 MFMA chain over the tiles of the other side in a fixed order (no atomics, no
// split: batch rows are the bits of single calls):
//   dq kernel    a wave owns 32 query rows (the query on the MFMA lane, the "swapped" S^T = K Q^T of attn.hip) and walks the
//                key tiles twice: a first sweep takes the row statistics (online max / sum per lane, halves folded at the
//                end) -- the forward kernel keeps none and is not touched --, the second recomputes S^T, forms dS^T and
//                accumulates dq^T = K^T dS^T.  delta is a prologue over the wave's own dO / O rows.  (lse, delta) go to a
//                small fp32 buffer for the second kernel.  A key count M < the key stride with a mask on the last tile is the
//                cross-attention form (77 keys of HEDIT_CTXP rows): rows >= M are never read.
//   dk/dv kernel a wave owns 32 key rows (the key on the lane) and walks the query tiles: S = Q K^T and dP = dO V^T come out
//                with the query in the registers, so P and dS are already the B operands of dv^T = dO^T P and dk^T = Q^T dS.
// An accumulator tile is the next product's operand without lane movement (its registers 8s .. 8s+7 rounded to storage are
// k-step s, k in the order 16s + 8(j>>2) + 4(lane>>5) + (j&3)); the other operand of those products is read in the same k
// order from a TRANSPOSED LDS image of the staged tile (two 8-byte reads), which the staging writes next to the row-major
// image that the S / dP products read (one 16-byte read per k-step).  Drained schedule: one barrier pair per tile.
// Head dims 32, 40, 64, 80, 160; the contraction of d = 40 is padded to 48 with exact zeros on both operands.
//
// dk / dv of the CONTEXT form (the text-context gradient, unetgrad.h) are a third and fourth kernel further down: the same
// products as the dk/dv kernel, split over the queries into fp32 partials that a reduce kernel adds in a fixed order.
#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int TS = 32;        // rows of a staged tile
constexpr int TP = 40;        // LDS row stride (elements) of the transposed image: 32 + 8 (80 B: 8-byte reads stay aligned)
constexpr int BWD_THREADS = 128;
constexpr float LN2F = 0.6931471805599453f;

template <int D>
struct BwdCfg {
  static constexpr int DP = (D + 15) / 16 * 16;   // contraction length of S and dP
  static constexpr int NS = DP / 16;              // k-steps of 16
  static constexpr int DT = (D + 31) / 32;        // 32-row output tiles over d
  static constexpr int RS = DP + 8;               // LDS row stride (elements) of the row-major image
  static constexpr int R_ELEMS = TS * RS;
  static constexpr int T_ELEMS = DT * 32 * TP;
};

__device__ __forceinline__ bf16x8 as_frag(u32x4 u) { return __builtin_bit_cast(bf16x8, u); }

// 8 consecutive elements (16 B)
__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* p) { return as_frag(*reinterpret_cast<const u32x4*>(p)); }

// k-step s of a transposed image row for lane half hh: columns 16s + 4hh .. +3 and 16s + 8 + 4hh .. +3
__device__ __forceinline__ bf16x8 ld_tfrag(const bf16_t* row, int s, int hh) {
  const u32x2 a = *reinterpret_cast<const u32x2*>(row + 16 * s + 4 * hh);
  const u32x2 b = *reinterpret_cast<const u32x2*>(row + 16 * s + 8 + 4 * hh);
  return as_frag((u32x4){a.x, a.y, b.x, b.y});
}

// 8 accumulator registers rounded to storage: one k-step of the next product
__device__ __forceinline__ bf16x8 acc_frag(const float* x) {
  return as_frag((u32x4){pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7])});
}

template <int NT = BWD_THREADS>
__device__ __forceinline__ void zero_lds(bf16_t* p, int n) {
  for (int i = threadIdx.x; i < n; i += NT) p[i] = 0;
}

// rows 0 .. 31 of src (already at the tile's first row and the head's first column), D columns each, into the row-major
// image R and (WITH_T) the transposed image T.  Rows >= nvalid are not read: they become zeros.  Columns >= D of R and
// rows >= D of T keep the zeros of zero_lds.
template <int D, bool WITH_T, int NT = BWD_THREADS>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ src, long ld, int nvalid, bf16_t* R, bf16_t* T) {
  constexpr int CH = D / 8;
  for (int i = threadIdx.x; i < TS * CH; i += NT) {
    const int r = i / CH, c = i - r * CH;
    u32x4 u = {0u, 0u, 0u, 0u};
    if (r < nvalid) u = *reinterpret_cast<const u32x4*>(src + (long)r * ld + c * 8);
    *reinterpret_cast<u32x4*>(R + r * BwdCfg<D>::RS + c * 8) = u;
    if (WITH_T) {
#pragma unroll
      for (int j = 0; j < 8; ++j) T[(c * 8 + j) * TP + r] = (bf16_t)(u[j >> 1] >> (16 * (j & 1)));
    }
  }
}

// acc (+)= rows of R . own fragments, over the NS k-steps
template <int D>
__device__ __forceinline__ f32x16 rows_dot(const bf16_t* R, int r, int hh, const bf16x8* own) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int s = 0; s < BwdCfg<D>::NS; ++s)
    acc = MFMA_32x32x16_ST(ld_frag(R + r * BwdCfg<D>::RS + 16 * s + 8 * hh), own[s], acc, 0, 0, 0);
  return acc;
}

// the wave's own 32 rows as B operands: lane (r, hh) holds columns 16s + 8hh .. +7 of row r; columns >= D are zeros
template <int D>
__device__ __forceinline__ void load_own(const bf16_t* __restrict__ row, int hh, bf16x8* f) {
#pragma unroll
  for (int s = 0; s < BwdCfg<D>::NS; ++s) {
    const int d0 = 16 * s + 8 * hh;
    u32x4 u = {0u, 0u, 0u, 0u};
    if (d0 < D) u = *reinterpret_cast<const u32x4*>(row + d0);
    f[s] = as_frag(u);
  }
}

// acc tiles [d][own row] -> dst row (4 consecutive d per register group: 8-byte stores)
template <int D>
__device__ __forceinline__ void store_own(const f32x16* acc, bf16_t* row, int hh) {
#pragma unroll
  for (int t = 0; t < BwdCfg<D>::DT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 32 * t + 8 * g + 4 * hh;
      if (d0 < D) {
        u32x2 o;
        o.x = pack_bf16x2(acc[t][4 * g + 0], acc[t][4 * g + 1]);
        o.y = pack_bf16x2(acc[t][4 * g + 2], acc[t][4 * g + 3]);
        *reinterpret_cast<u32x2*>(row + d0) = o;
      }
    }
}

template <int D>
__global__ __launch_bounds__(BWD_THREADS) void attn_bwd_dq_kernel(AttnBwdParams p) {
  using Cf = BwdCfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t sK[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sV[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sKt[Cf::T_ELEMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nqb = p.N / 64;
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int h = bh % p.heads, b = bh / p.heads;
  const int qi = qb * 64 + wave * 32 + r;              // query of this lane inside the image
  const long qrow = (long)b * p.N + qi;

  zero_lds(sK, Cf::R_ELEMS);
  zero_lds(sV, Cf::R_ELEMS);
  zero_lds(sKt, Cf::T_ELEMS);

  bf16x8 qf[Cf::NS], dof[Cf::NS];
  load_own<D>(p.q + qrow * p.ldq + h * D, hh, qf);
  load_own<D>(p.dout + qrow * p.lddo + h * D, hh, dof);
  float delta = 0.f;
#pragma unroll
  for (int s = 0; s < Cf::NS; ++s) {
    const int d0 = 16 * s + 8 * hh;
    if (d0 < D) {
      float a[8], c[8];
      unpack8(*reinterpret_cast<const uint4*>(p.dout + qrow * p.lddo + h * D + d0), a);
      unpack8(*reinterpret_cast<const uint4*>(p.o + qrow * p.ldo + h * D + d0), c);
#pragma unroll
      for (int j = 0; j < 8; ++j) delta += a[j] * c[j];
    }
  }
  delta += __shfl_xor(delta, 32, 64);

  const bf16_t* kbase = p.k + (long)b * p.kstride * p.ldk + h * D;
  const bf16_t* vbase = p.v + (long)b * p.kstride * p.ldv + h * D;
  const int ntile = (p.M + TS - 1) / TS;

  // sweep 1: row statistics.  Lane (r, hh) sees 16 of the tile's 32 keys of its query; the halves are folded at the end.
  float m = -1e30f, l = 0.f;
  for (int t = 0; t < ntile; ++t) {
    const int nvalid = p.M - t * TS;
    __syncthreads();
    stage_tile<D, false>(kbase + (long)t * TS * p.ldk, p.ldk, nvalid, sK, nullptr);
    __syncthreads();
    const f32x16 S = rows_dot<D>(sK, r, hh, qf);
    float tm = m;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((i & 3) + 8 * (i >> 2) + 4 * hh < nvalid) tm = fmaxf(tm, S[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((i & 3) + 8 * (i >> 2) + 4 * hh < nvalid) sum += exp2f(S[i] - tm);
    l = l * exp2f(m - tm) + sum;
    m = tm;
  }
  const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
  const float mm = fmaxf(m, mo);
  const float lse = mm + log2f(l * exp2f(m - mm) + lo * exp2f(mo - mm));
  if (p.stats && hh == 0) {
    float* st = p.stats + ((long)bh * p.N + qi) * 2;
    st[0] = lse;
    st[1] = delta;
  }
  if (!p.dq) return;      // statistics only (uniform over the launch): what the context dk / dv entry point asks for

  // sweep 2: dq^T [d][query] += K^T dS^T
  f32x16 dq[Cf::DT];
#pragma unroll
  for (int t = 0; t < Cf::DT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[t][i] = 0.f;
  for (int t = 0; t < ntile; ++t) {
    const int nvalid = p.M - t * TS;
    __syncthreads();
    stage_tile<D, true>(kbase + (long)t * TS * p.ldk, p.ldk, nvalid, sK, sKt);
    stage_tile<D, false>(vbase + (long)t * TS * p.ldv, p.ldv, nvalid, sV, nullptr);
    __syncthreads();
    const f32x16 S = rows_dot<D>(sK, r, hh, qf);
    const f32x16 dP = rows_dot<D>(sV, r, hh, dof);
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool ok = (i & 3) + 8 * (i >> 2) + 4 * hh < nvalid;
      ds[i] = ok ? LN2F * exp2f(S[i] - lse) * (dP[i] - delta) : 0.f;
    }
    const bf16x8 dsf[2] = {acc_frag(ds), acc_frag(ds + 8)};
#pragma unroll
    for (int tt = 0; tt < Cf::DT; ++tt)
#pragma unroll
      for (int s = 0; s < 2; ++s) dq[tt] = MFMA_32x32x16_ST(ld_tfrag(sKt + (32 * tt + r) * TP, s, hh), dsf[s], dq[tt], 0, 0, 0);
  }
  store_own<D>(dq, p.dq + qrow * p.lddq + h * D, hh);
}

template <int D>
__global__ __launch_bounds__(BWD_THREADS) void attn_bwd_dkv_kernel(AttnBwdParams p) {
  using Cf = BwdCfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t sQ[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sDO[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sQt[Cf::T_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sDOt[Cf::T_ELEMS];
  __shared__ float sSt[TS * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nkb = p.N / 64;
  const int kb = blockIdx.x % nkb, bh = blockIdx.x / nkb;
  const int h = bh % p.heads, b = bh / p.heads;
  const long krow = (long)b * p.N + kb * 64 + wave * 32 + r;

  zero_lds(sQ, Cf::R_ELEMS);
  zero_lds(sDO, Cf::R_ELEMS);
  zero_lds(sQt, Cf::T_ELEMS);
  zero_lds(sDOt, Cf::T_ELEMS);

  bf16x8 kf[Cf::NS], vf[Cf::NS];
  load_own<D>(p.k + krow * p.ldk + h * D, hh, kf);
  load_own<D>(p.v + krow * p.ldv + h * D, hh, vf);

  f32x16 dk[Cf::DT], dv[Cf::DT];
#pragma unroll
  for (int t = 0; t < Cf::DT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[t][i] = dv[t][i] = 0.f;

  const int ntile = p.N / TS;
  for (int t = 0; t < ntile; ++t) {
    const long q0 = (long)b * p.N + (long)t * TS;
    __syncthreads();
    stage_tile<D, true>(p.q + q0 * p.ldq + h * D, p.ldq, TS, sQ, sQt);
    stage_tile<D, true>(p.dout + q0 * p.lddo + h * D, p.lddo, TS, sDO, sDOt);
    if (threadIdx.x < TS * 2) sSt[threadIdx.x] = p.stats[((long)bh * p.N + (long)t * TS) * 2 + threadIdx.x];
    __syncthreads();
    const f32x16 S = rows_dot<D>(sQ, r, hh, kf);        // [query][key]: the query in the registers
    const f32x16 dP = rows_dot<D>(sDO, r, hh, vf);
    float pr[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = (i & 3) + 8 * (i >> 2) + 4 * hh;
      pr[i] = exp2f(S[i] - sSt[2 * qi]);
      ds[i] = LN2F * pr[i] * (dP[i] - sSt[2 * qi + 1]);
    }
    const bf16x8 pf[2] = {acc_frag(pr), acc_frag(pr + 8)};
    const bf16x8 dsf[2] = {acc_frag(ds), acc_frag(ds + 8)};
#pragma unroll
    for (int tt = 0; tt < Cf::DT; ++tt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dv[tt] = MFMA_32x32x16_ST(ld_tfrag(sDOt + (32 * tt + r) * TP, s, hh), pf[s], dv[tt], 0, 0, 0);
        dk[tt] = MFMA_32x32x16_ST(ld_tfrag(sQt + (32 * tt + r) * TP, s, hh), dsf[s], dk[tt], 0, 0, 0);
      }
  }
  store_own<D>(dk, p.dk + krow * p.lddkv + h * D, hh);
  store_own<D>(dv, p.dv + krow * p.lddkv + h * D, hh);
}

// ---- dk / dv of the context form: p.M (77) keys in p.kstride (80) rows per image, 64 .. 4096 queries.  The self form's grid
// would be three key tiles per (image, head), each walking every query tile; here the QUERIES are split: a block is (image,
// head, query chunk) with one wave per 32-key tile, all of which read the one staged Q / dO tile, and writes the chunk's fp32
// partial [key][d]; a second kernel sums the chunks in ascending order and rounds once.  The chunk length depends on nothing
// but the build, so a batch row has the bits of its single call.
constexpr int CTX_WAVES = 3;                     // keys 0 .. 31, 32 .. 63, 64 .. 76
constexpr int CTX_THREADS = CTX_WAVES * 64;
constexpr int CTX_CHUNK = 128;                   // queries of a block (the last chunk of an image may be shorter)

template <int D>
__global__ __launch_bounds__(CTX_THREADS) void attn_bwd_ctx_part_kernel(AttnBwdParams p, float* __restrict__ part_k,
                                                                        float* __restrict__ part_v, int nchunk) {
  using Cf = BwdCfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t sQ[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sDO[Cf::R_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sQt[Cf::T_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t sDOt[Cf::T_ELEMS];
  __shared__ float sSt[TS * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int c = blockIdx.x % nchunk, bh = blockIdx.x / nchunk;
  const int h = bh % p.heads, b = bh / p.heads;
  const int key = wave * 32 + r;                 // key of this lane inside the image
  const bool kvalid = key < p.M;                 // rows >= M are never read; their P and dS are zero

  zero_lds<CTX_THREADS>(sQ, Cf::R_ELEMS);
  zero_lds<CTX_THREADS>(sDO, Cf::R_ELEMS);
  zero_lds<CTX_THREADS>(sQt, Cf::T_ELEMS);
  zero_lds<CTX_THREADS>(sDOt, Cf::T_ELEMS);

  bf16x8 kf[Cf::NS], vf[Cf::NS];
#pragma unroll
  for (int s = 0; s < Cf::NS; ++s) kf[s] = vf[s] = as_frag((u32x4){0u, 0u, 0u, 0u});
  if (kvalid) {
    const long krow = (long)b * p.kstride + key;
    load_own<D>(p.k + krow * p.ldk + h * D, hh, kf);
    load_own<D>(p.v + krow * p.ldv + h * D, hh, vf);
  }

  f32x16 dk[Cf::DT], dv[Cf::DT];
#pragma unroll
  for (int t = 0; t < Cf::DT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[t][i] = dv[t][i] = 0.f;

  const int t0 = c * (CTX_CHUNK / TS);
  const int t1 = min(t0 + CTX_CHUNK / TS, p.N / TS);
  for (int t = t0; t < t1; ++t) {
    const long q0 = (long)b * p.N + (long)t * TS;
    __syncthreads();
    stage_tile<D, true, CTX_THREADS>(p.q + q0 * p.ldq + h * D, p.ldq, TS, sQ, sQt);
    stage_tile<D, true, CTX_THREADS>(p.dout + q0 * p.lddo + h * D, p.lddo, TS, sDO, sDOt);
    if (threadIdx.x < TS * 2) sSt[threadIdx.x] = p.stats[((long)bh * p.N + (long)t * TS) * 2 + threadIdx.x];
    __syncthreads();
    const f32x16 S = rows_dot<D>(sQ, r, hh, kf);        // [query][key]: the query in the registers
    const f32x16 dP = rows_dot<D>(sDO, r, hh, vf);
    float pr[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = (i & 3) + 8 * (i >> 2) + 4 * hh;
      pr[i] = kvalid ? exp2f(S[i] - sSt[2 * qi]) : 0.f;
      ds[i] = kvalid ? LN2F * pr[i] * (dP[i] - sSt[2 * qi + 1]) : 0.f;
    }
    const bf16x8 pf[2] = {acc_frag(pr), acc_frag(pr + 8)};
    const bf16x8 dsf[2] = {acc_frag(ds), acc_frag(ds + 8)};
#pragma unroll
    for (int tt = 0; tt < Cf::DT; ++tt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dv[tt] = MFMA_32x32x16_ST(ld_tfrag(sDOt + (32 * tt + r) * TP, s, hh), pf[s], dv[tt], 0, 0, 0);
        dk[tt] = MFMA_32x32x16_ST(ld_tfrag(sQt + (32 * tt + r) * TP, s, hh), dsf[s], dk[tt], 0, 0, 0);
      }
  }
  if (key < p.kstride) {      // partial [image][head][chunk][key][d]; rows M .. kstride - 1 hold the zeros accumulated above
    const long row = ((long)bh * nchunk + c) * p.kstride + key;
#pragma unroll
    for (int t = 0; t < Cf::DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * t + 8 * g + 4 * hh;
        if (d0 < D) {
          *reinterpret_cast<f32x4*>(part_k + row * D + d0) = (f32x4){dk[t][4 * g], dk[t][4 * g + 1], dk[t][4 * g + 2], dk[t][4 * g + 3]};
          *reinterpret_cast<f32x4*>(part_v + row * D + d0) = (f32x4){dv[t][4 * g], dv[t][4 * g + 1], dv[t][4 * g + 2], dv[t][4 * g + 3]};
        }
      }
  }
}

// dk, dv [B*kstride][lddkv] at head column h*D = the chunks' partials summed in ascending order (fp32), rounded once; rows >= M
// are written as exact zeros.  One thread per (image, head, key row, 4 columns) of both outputs.
__global__ __launch_bounds__(256) void attn_bwd_ctx_reduce_kernel(AttnBwdParams p, const float* __restrict__ part_k,
                                                                  const float* __restrict__ part_v, int nchunk, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int dq4 = p.d / 4;
  const int g = (int)(idx % dq4);
  const long rowi = idx / dq4;                   // (image * heads + head) * kstride + key
  const int key = (int)(rowi % p.kstride);
  const long bh = rowi / p.kstride;
  const int h = (int)(bh % p.heads);
  const long b = bh / p.heads;
  f32x4 sk = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
  if (key < p.M) {
    const long first = (bh * nchunk * p.kstride + key) * p.d + 4 * g;
    const long step = (long)p.kstride * p.d;
    for (int c = 0; c < nchunk; ++c) {
      sk += *reinterpret_cast<const f32x4*>(part_k + first + c * step);
      sv += *reinterpret_cast<const f32x4*>(part_v + first + c * step);
    }
  }
  const long o = (b * p.kstride + key) * p.lddkv + h * p.d + 4 * g;
  *reinterpret_cast<u32x2*>(p.dk + o) = (u32x2){pack_bf16x2(sk[0], sk[1]), pack_bf16x2(sk[2], sk[3])};
  *reinterpret_cast<u32x2*>(p.dv + o) = (u32x2){pack_bf16x2(sv[0], sv[1]), pack_bf16x2(sv[2], sv[3])};
}

template <int D>
int launch_ctx_kv(const AttnBwdParams& p, float* part, hipStream_t st) {
  const int nchunk = (p.N + CTX_CHUNK - 1) / CTX_CHUNK;
  const long nblk = (long)p.B * p.heads * nchunk;
  float* part_v = part + nblk * p.kstride * D;
  hipLaunchKernelGGL(attn_bwd_ctx_part_kernel<D>, dim3((unsigned)nblk), dim3(CTX_THREADS), 0, st, p, part, part_v, nchunk);
  LAUNCH_CHECK();
  const long total = (long)p.B * p.heads * p.kstride * (D / 4);
  hipLaunchKernelGGL(attn_bwd_ctx_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p, part, part_v, nchunk, total);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

template <int D>
int launch_bwd(const AttnBwdParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((long)p.B * p.heads * (p.N / 64));
  hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, dim3(grid), dim3(BWD_THREADS), 0, st, p);
  LAUNCH_CHECK();
  if (p.dk) {
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<D>, dim3(grid), dim3(BWD_THREADS), 0, st, p);
    LAUNCH_CHECK();
  }
  return HEDIT_OK;
}

}  // namespace

size_t attn_bwd_ws_bytes(int B, int N, int heads) { return (size_t)B * heads * N * 2 * sizeof(float); }

int attn_bwd_launch(const AttnBwdParams& p, hipStream_t st) {
  ARG_CHECK(p.B >= 1 && p.heads >= 1 && p.N >= 64 && p.N % 64 == 0, "attn_bwd: N must be a multiple of 64");
  ARG_CHECK((long)p.B * p.heads * (p.N / 64) < (1L << 31) && (long)p.B * p.N < (1L << 31), "attn_bwd: tensor too large");
  ARG_CHECK(p.M >= TS && p.M <= p.kstride, "attn_bwd: 32 <= keys <= key stride");
  const int C = p.heads * p.d;
  ARG_CHECK(p.dq || (p.stats && !p.dk && !p.dv), "attn_bwd: without dq the launch takes the statistics only");
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.ldo % 8 == 0 && p.lddo % 8 == 0 && (!p.dq || p.lddq % 8 == 0),
            "attn_bwd: row strides must be multiples of 8");
  ARG_CHECK(p.ldq >= C && p.ldk >= C && p.ldv >= C && p.ldo >= C && p.lddo >= C && (!p.dq || p.lddq >= C),
            "attn_bwd: row strides must cover heads * d");
  if (p.dk || p.dv) {
    ARG_CHECK(p.dk && p.dv && p.stats, "attn_bwd: dk, dv and the statistics buffer come together");
    ARG_CHECK(p.M == p.N && p.kstride == p.N, "attn_bwd: dk / dv are the self-attention form");
    ARG_CHECK(p.lddkv % 8 == 0 && p.lddkv >= C, "attn_bwd: dk / dv row stride");
  }
  switch (p.d) {
    case 32: return launch_bwd<32>(p, st);
    case 40: return launch_bwd<40>(p, st);
    case 64: return launch_bwd<64>(p, st);
    case 80: return launch_bwd<80>(p, st);
    case 160: return launch_bwd<160>(p, st);
  }
  hedit_set_error("bad argument: attn_bwd: head dim must be 32, 40, 64, 80 or 160");
  return HEDIT_ERR_ARG;
}

int attn_bwd_ctx_chunk(int N) { (void)N; return CTX_CHUNK; }

size_t attn_bwd_ctx_kv_ws_bytes(int B, int N, int heads, int d) {
  const size_t nchunk = (size_t)(N + CTX_CHUNK - 1) / CTX_CHUNK;
  return 2 * (size_t)B * heads * nchunk * HEDIT_CTXP * d * sizeof(float);
}

// dk / dv of the context form from the (lse, delta) that attn_bwd_launch left in p.stats; `part`: attn_bwd_ctx_kv_ws_bytes
int attn_bwd_ctx_kv_launch(const AttnBwdParams& p, float* part, hipStream_t st) {
  ARG_CHECK(p.B >= 1 && p.heads >= 1 && p.N >= 64 && p.N % 64 == 0, "attn_bwd_ctx_kv: N must be a multiple of 64");
  ARG_CHECK((long)p.B * p.heads * ((p.N + CTX_CHUNK - 1) / CTX_CHUNK) < (1L << 31) && (long)p.B * p.N < (1L << 31),
            "attn_bwd_ctx_kv: tensor too large");
  ARG_CHECK(p.M >= 1 && p.M <= p.kstride && p.kstride <= CTX_WAVES * 32 && p.kstride == HEDIT_CTXP,
            "attn_bwd_ctx_kv: the keys are the context rows");
  ARG_CHECK(p.dk && p.dv && p.stats && part, "attn_bwd_ctx_kv: dk, dv, the statistics and the partial buffer come together");
  ARG_CHECK(reinterpret_cast<uintptr_t>(part) % 16 == 0, "attn_bwd_ctx_kv: the partial buffer must be 16-byte aligned");
  const int C = p.heads * p.d;
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.lddo % 8 == 0 && p.lddkv % 8 == 0,
            "attn_bwd_ctx_kv: row strides must be multiples of 8");
  ARG_CHECK(p.ldq >= C && p.ldk >= C && p.ldv >= C && p.lddo >= C && p.lddkv >= C, "attn_bwd_ctx_kv: row strides must cover heads * d");
  switch (p.d) {
    case 32: return launch_ctx_kv<32>(p, part, st);
    case 40: return launch_ctx_kv<40>(p, part, st);
    case 64: return launch_ctx_kv<64>(p, part, st);
    case 80: return launch_ctx_kv<80>(p, part, st);
    case 160: return launch_ctx_kv<160>(p, part, st);
  }
  hedit_set_error("bad argument: attn_bwd_ctx_kv: head dim must be 32, 40, 64, 80 or 160");
  return HEDIT_ERR_ARG;
}
