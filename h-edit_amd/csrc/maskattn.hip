// Mask-guided mutual self-attention (text-guided/masactrl/masactrl.py:71-148) on MFMA.
//
// The reference runs, per target row, two full softmaxes over the source row's keys -- one with the background keys filled
// with finfo.min, one with the foreground keys filled -- and blends the two outputs with the target's binary mask.  With
// binary masks that is ONE softmax per query over the keys of the query's own class (the +1 the reference adds to the
// foreground logits is a common shift of everything a query admits and drops out).  A query whose class has no key at all
// sees sim + finfo.min on every key, which in fp32 absorbs sim: a uniform softmax, the mean of V.  Here such a query admits
// every key with one and the same score (`uniform` below).
//
// Structure: cross_attn's fragment layouts (attn.hip) on a flash loop.  A workgroup = 4 waves = 128 queries of one (listed row,
// head); a wave owns 32 queries, a lane one query column and 16 of the 32 kv rows of a score block (the other 16 in lane ^ 32).
//   * prologue: the key counts per class of the kv row (one pass over its N class bytes), the queries' classes, and which
//     classes the block's queries want at all;
//   * per 64-key tile: the wave ballots the tile's class bytes.  A tile none of whose classes is wanted is not loaded;
//     otherwise K / V^T go global -> registers -> LDS between two barriers (no DMA ring, no counted waits), S^T = K Q^T, the
//     class test in registers BEFORE the row maximum, online softmax in fp32, O^T += V^T P^T;
//   * the running maximum starts at a large finite negative and a rejected logit contributes an explicit zero, so a tile in
//     which a query admits nothing multiplies its state by exactly 1 and adds exactly 0.
// A block reads its own row's operands only: the result of a row has the same bits in any batch, `rows` order or n_rows.
#include "common.h"
#include "kernels.h"

namespace {

template <int D>
struct MCfg {
  static constexpr int DP = (D + 15) / 16 * 16;   // K-dim of QK^T, padded
  static constexpr int DK = DP / 16;
  static constexpr int DT = (D + 31) / 32;        // 32-row tiles of O^T
  static constexpr int KS = DP + 8;               // LDS row stride of K (elements)
  static constexpr int VS = 68;                   // LDS row stride of V^T (elements)
  static constexpr int DCH = D / 8;               // 16-byte chunks per K row
  static constexpr int K_BYTES = 64 * KS * 2;
  static constexpr int V_BYTES = DT * 32 * VS * 2;
  static constexpr int TOTAL = K_BYTES + V_BYTES;
};

constexpr float NEG = -1e30f;

template <int D>
__global__ __launch_bounds__(256) void masked_self_attn_kernel(MaskedSelfAttnParams p) {
  using C = MCfg<D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_red[4];
  __shared__ unsigned s_want[4];
  bf16_t* sK = reinterpret_cast<bf16_t*>(smem);
  bf16_t* sV = reinterpret_cast<bf16_t*>(smem + C::K_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y;
  const int b = p.rows[blockIdx.z];
  if (b < 0 || b >= p.B) return;                       // (uniform: a bad list entry computes nothing)
  const int kb = p.kv_src[b];
  if (kb < 0 || kb >= p.B) return;
  const int N = p.N;
  const int q_row = blockIdx.x * 128 + wave * 32 + ql;
  const bool q_ok = q_row < N;
  const uint8_t* ck = p.cls_k + (long)kb * N;

  // pad columns of K and pad rows of V^T must be finite zeros: staging never writes them
  for (int i = tid; i < C::TOTAL / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  // ---- keys per class of the kv row
  int c1 = 0;
  for (int i = tid; i < N / 4; i += 256) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(ck)[i];
    c1 += ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c1 += __shfl_xor(c1, o, 64);
  if (lane == 0) s_red[wave] = c1;
  __syncthreads();
  const int cnt1 = s_red[0] + s_red[1] + s_red[2] + s_red[3], cnt0 = N - cnt1;

  // ---- the query's class; `uniform`: its class has no key -> every key admitted, with equal weight
  const bool cq = q_ok ? p.cls_q[(long)b * N + q_row] != 0 : false;
  const bool uniform = !q_ok || (cq ? cnt1 : cnt0) == 0;
  {
    const bool w0 = q_ok && (uniform || !cq), w1 = q_ok && (uniform || cq);
    const unsigned bits = (__ballot(w0) != 0 ? 1u : 0u) | (__ballot(w1) != 0 ? 2u : 0u);
    if (lane == 0) s_want[wave] = bits;
  }
  __syncthreads();
  const unsigned want = s_want[0] | s_want[1] | s_want[2] | s_want[3];

  // Q fragments (B operand): lane holds Q[q][ks*16 + hi*8 .. +8], zero beyond D
  bf16x8 qf[C::DK];
  {
    const bf16_t* qp = p.q + ((long)b * N + (q_ok ? q_row : 0)) * p.ldq + h * D;
#pragma unroll
    for (int ks = 0; ks < C::DK; ++ks) {
      const int c = ks * 16 + hi * 8;
      union { uint4 u; bf16x8 v; } x;
      x.u = make_uint4(0, 0, 0, 0);
      if (q_ok && c < D) x.u = *reinterpret_cast<const uint4*>(qp + c);
      qf[ks] = x.v;
    }
  }

  f32x16 o[C::DT];
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_run = NEG, l_run = 0.f;

  const bf16_t* kbase = p.k + (long)kb * N * p.ldk + h * D;
  const bf16_t* vbase = p.vt + (long)h * D * p.ldvt + (long)kb * N;
  const int ntiles = N / 64;
  for (int t = 0; t < ntiles; ++t) {
    // the tile's classes: bit j of m1 = class of key t*64 + j (the same in every wave)
    const unsigned long long m1 = __ballot(ck[t * 64 + lane] != 0);
    const bool has1 = m1 != 0ull, has0 = m1 != ~0ull;
    if (!((has0 && (want & 1u)) || (has1 && (want & 2u)))) continue;      // nobody here admits any of its keys: not loaded

    __syncthreads();                                  // the previous tile's fragments have been read
    for (int idx = tid; idx < 64 * C::DCH; idx += 256) {
      const int row = idx / C::DCH, c = idx - row * C::DCH;
      *reinterpret_cast<uint4*>(sK + row * C::KS + c * 8) =
          *reinterpret_cast<const uint4*>(kbase + ((long)t * 64 + row) * p.ldk + c * 8);
    }
    for (int idx = tid; idx < D * 8; idx += 256) {
      const int row = idx >> 3, c = idx & 7;
      const uint4 u = *reinterpret_cast<const uint4*>(vbase + (long)row * p.ldvt + t * 64 + c * 8);
      uint2* dst = reinterpret_cast<uint2*>(sV + row * C::VS + c * 8);
      dst[0] = make_uint2(u.x, u.y);
      dst[1] = make_uint2(u.z, u.w);
    }
    __syncthreads();

    // scores, class test, block maximum
    float s[2][16];
    float mx = NEG;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < C::DK; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (nt * 32 + ql) * C::KS + ks * 16 + hi * 8);
        acc = MFMA_32x32x16_ST(kf, qf[ks], acc, 0, 0, 0);
      }
      // register r of the lane is key nt*32 + (r & 3) + 8 (r >> 2) + 4 hi
      const uint32_t kc = (uint32_t)(m1 >> (nt * 32 + 4 * hi));
      const uint32_t adm = uniform ? 0xffffffffu : (cq ? kc : ~kc);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool a = (adm >> ((r & 3) + 8 * (r >> 2))) & 1u;
        // a query without keys of its class: every logit is the same (the reference's sim + finfo.min == finfo.min)
        const float v = a ? (uniform ? 0.f : acc[r]) : NEG;
        s[nt][r] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);             // nothing admitted: mx = NEG <= m_run, the state stays as it is
    const float alpha = m_new == m_run ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float ls = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = s[nt][r] > 0.5f * NEG ? __builtin_amdgcn_exp2f(s[nt][r] - m_new) : 0.f;
        s[nt][r] = e;
        ls += e;
      }
    l_run = l_run * alpha + ls;
    bf16x8 pf[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) { pf[nt][0] = pack_p8(s[nt]); pf[nt][1] = pack_p8(s[nt] + 8); }
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 vf = read_perm_frag(sV, dt * 32 + ql, C::VS, nt * 32 + 16 * s2 + 4 * hi);
          o[dt] = MFMA_32x32x16_ST(vf, pf[nt][s2], o[dt], 0, 0, 0);
        }
    }
  }

  const float l = l_run + __shfl_xor(l_run, 32, 64);
  if (q_ok) {
    const float inv = 1.0f / l;
    bf16_t* op = p.out + ((long)b * N + q_row) * p.ldo + h * D;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = dt * 32 + 8 * g + 4 * hi;
        if (d0 < D) {
          uint2 w;
          w.x = pack_bf16x2(o[dt][g * 4 + 0] * inv, o[dt][g * 4 + 1] * inv);
          w.y = pack_bf16x2(o[dt][g * 4 + 2] * inv, o[dt][g * 4 + 3] * inv);
          *reinterpret_cast<uint2*>(op + d0) = w;
        }
      }
  }
}

template <int D>
int launch_masked(const MaskedSelfAttnParams& p, hipStream_t st) {
  using C = MCfg<D>;
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&masked_self_attn_kernel<D>), C::TOTAL)) return rc;
  dim3 grid(cdiv(p.N, 128), p.heads, p.n_rows);
  hipLaunchKernelGGL((masked_self_attn_kernel<D>), grid, dim3(256), C::TOTAL, st, p);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

// ---- the auto variant's masks (masactrl.py:212-232, :252-275).  The reference keeps the head-mean probabilities of every
// 256-token cross-attention layer of the pass, averages them over the layers, sums the chosen token columns, normalises
// per image and thresholds.  Everything up to the normalisation is linear, so the accumulator holds, per conditional row and
// pixel, the SUM over layers of (head mean of the token-column sum); the layer count divides it when a mask is formed.
//
// accumulate: one block per conditional row r (r < rows / 2: a source row, the `ref` tokens; else a target row, `cur`), one
// thread per pixel; tokens ascending inside a head, heads ascending, in fp32.
__global__ __launch_bounds__(256) void masa_accumulate_kernel(const float* probs, int heads, int rows, const int* ref, int n_ref,
                                                              const int* cur, int n_cur, float* acc) {
  const int r = blockIdx.x, pix = threadIdx.x;
  const int* tok = r < rows / 2 ? ref : cur;
  const int nt = r < rows / 2 ? n_ref : n_cur;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) {
    const float* row = probs + (((long)r * heads + h) * 256 + pix) * HEDIT_MAXW;
    float sh = 0.f;
    for (int i = 0; i < nt; ++i) {
      const int t = tok[i];
      if (t >= 0 && t < HEDIT_MAXW) sh += row[t];
    }
    s += sh;
  }
  acc[r * 256 + pix] += s / (float)heads;
}

// auto_mask: block (image i, which): which = 0 the key mask from the source row's map acc[i], 1 the query mask from the
// target row's map acc[n + i].  map = acc / count; (map - min) / (max - min) >= thres on the 16 x 16 grid (a constant map:
// class 0 everywhere, where the reference divides 0 by 0), then nearest to res x res: source index floor(dst * 16 / res).
// cls [4 n][res * res]: key masks go to the source rows i and 2 n + i, query masks to the target rows n + i and 3 n + i.
__global__ __launch_bounds__(256) void masa_auto_mask_kernel(const float* acc, int count, int n, int res, float thres, uint8_t* cls) {
  __shared__ float s_min[4], s_max[4];
  __shared__ uint8_t s_cls[256];
  const int i = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
  const float v = acc[(which * n + i) * 256 + tid] / (float)count;
  float mn = v, mx = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((tid & 63) == 0) { s_min[tid >> 6] = mn; s_max[tid >> 6] = mx; }
  __syncthreads();
  mn = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
  mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  s_cls[tid] = (mx > mn && (v - mn) / (mx - mn) >= thres) ? 1 : 0;
  __syncthreads();
  const int N = res * res;
  uint8_t* r0 = cls + (long)(which * n + i) * N;
  uint8_t* r1 = cls + (long)((2 + which) * n + i) * N;
  for (int dst = tid; dst < N; dst += 256) {
    const int y = dst / res, x = dst - y * res;
    const uint8_t c = s_cls[(y * 16 / res) * 16 + (x * 16 / res)];
    r0[dst] = c;
    r1[dst] = c;
  }
}

}  // namespace

int masa_accumulate_launch(const float* probs, int heads, int rows, const int* ref, int n_ref, const int* cur, int n_cur, float* acc,
                           hipStream_t st) {
  ARG_CHECK(probs && acc && ref && cur, "masa_accumulate: operands");
  ARG_CHECK(heads > 0 && rows > 0 && rows % 2 == 0 && n_ref > 0 && n_cur > 0, "masa_accumulate: extents");
  hipLaunchKernelGGL(masa_accumulate_kernel, dim3(rows), dim3(256), 0, st, probs, heads, rows, ref, n_ref, cur, n_cur, acc);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

int masa_auto_mask_launch(const float* acc, int count, int n, int res, float thres, uint8_t* cls, hipStream_t st) {
  ARG_CHECK(acc && cls, "masa_auto_mask: operands");
  ARG_CHECK(count > 0 && n > 0 && n <= 65535, "masa_auto_mask: no map collected / images");
  ARG_CHECK(res >= 1 && res <= 64, "masa_auto_mask: layer resolution must be in [1, 64]");
  hipLaunchKernelGGL(masa_auto_mask_kernel, dim3(n, 2), dim3(256), 0, st, acc, count, n, res, thres, cls);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

int masked_self_attn_launch(const MaskedSelfAttnParams& p, hipStream_t st) {
  ARG_CHECK(p.q && p.k && p.vt && p.out, "masked_self_attn: operands");
  ARG_CHECK(p.rows && p.n_rows > 0 && p.n_rows <= 65535, "masked_self_attn: no rows listed");
  ARG_CHECK(p.kv_src, "masked_self_attn: classes need kv_src");
  ARG_CHECK(p.cls_q && p.cls_k, "masked_self_attn: class arrays");
  ARG_CHECK(reinterpret_cast<uintptr_t>(p.cls_k) % 4 == 0, "masked_self_attn: cls_k must be 4-byte aligned");
  ARG_CHECK(p.B > 0 && p.heads > 0 && p.heads <= 65535, "masked_self_attn: extents");
  ARG_CHECK(p.N % 64 == 0 && p.N >= 64 && p.N <= 4096, "masked_self_attn: N must be a multiple of 64 in [64, 4096]");
  ARG_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldvt % 8 == 0 && p.ldo % 4 == 0, "masked_self_attn: strides");
  switch (p.d) {
    case 32: return launch_masked<32>(p, st);
    case 40: return launch_masked<40>(p, st);
    case 64: return launch_masked<64>(p, st);
    case 80: return launch_masked<80>(p, st);
    case 160: return launch_masked<160>(p, st);
    default:
      hedit_set_error("masked_self_attn: unsupported head dim " + std::to_string(p.d) + " (32,40,64,80,160)");
      return HEDIT_ERR_ARG;
  }
}
