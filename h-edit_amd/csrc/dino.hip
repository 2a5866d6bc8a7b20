// The DINO ViT key extractor and the key self-similarity distance as a native forward-only executor: the Structure Distance
// column of the PIE-Bench evaluator (the reference's text-guided/evaluation/matrics_calculator.py:12-171 VitExtractor,
// :174-246 LossG.calculate_global_ssim_loss, :390-410).  Both images, as 0..255 floats times their masks, are resized to
// R x R (bilinear, align_corners = False, no antialias), normalised with the ImageNet constants ON THE 0..255 VALUES (the
// reference's quirk, kept), run through the public DINO ViT (facebookresearch/dino vision_transformer.py: conv patch
// embedding with bias, cls_token + pos_embed, no pre-LayerNorm, pre-LN blocks with LayerNorm eps 1e-6, fused qkv with bias,
// exact erf GELU) up to the KEYS of block `key_layer`, [L][W] per image with the bias included; then
//   S = K K^T / max(|k_i| |k_j|, 1e-8),   dist = mean((S_a - S_b)^2).
//
// Key-only depth: blocks 0 .. key_layer - 1 run whole; block key_layer runs norm1 and the key third of qkv (rows [W, 2W) of
// the weight, N = W).  Its projection, its MLP, the later blocks and the final norm have no parameter slot at all.
//
// Arithmetic as in clipimg.hip: fp32 token stream, LayerNorm / softmax / GELU in fp32, every linear layer a three-term
// split-bf16 product with fp32 accumulation (pnet.hip), canonical chunk order with the batch in M: a batch gives the bytes
// of single calls.  The output is fp32 and nothing here reads the storage type, so both builds give the same bits.  The
// kernels every encoder runs (patches, tokens with the conv bias, LayerNorm with eps 1e-6, out = res + raw + bias, and the
// same without a residual for the keys) are those of encoder.hip and the block forward is encoder.h's.
//
// This file's own: the preprocess kernel, attention for any token count on the exact-fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), and the self-similarity head, which forms both Gram tiles on
// the same instruction and never writes an L x L matrix.
#include "encoder.h"

namespace {

constexpr float LN_EPS = 1e-6f;
constexpr int HD = 64;
constexpr int LMAX = 1025;          // tokens: (256 / 8)^2 + 1; the attention's LDS does not depend on L, this caps the workspace
constexpr int MAX_SIDE = 4096;  // largest input side

// ---- preprocess: x [B][3][S][S] (0..255, masked) -> y [B][3][R][R] = (bilinear(x) - mean_c) / std_c.  torch's
// upsample_bilinear2d with align_corners = False: src = (dst + 0.5) * (S / R) - 0.5, clamped at 0; the upper neighbour
// clamped to S - 1; value = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).  S == R: the copy (both weights 1 and 0).
__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int S, int R) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  const float sc = (float)S / (float)R;
  const long total = (long)B * 3 * R * R;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % R), oy = (int)((i / R) % R);
    const long pl = i / ((long)R * R);
    const int c = (int)(pl % 3);
    const float* src = x + pl * S * S;
    float v;
    if (S == R) {
      v = src[(long)oy * S + ox];
    } else {
      float fy = ((float)oy + 0.5f) * sc - 0.5f, fx = ((float)ox + 0.5f) * sc - 0.5f;
      fy = fy < 0.f ? 0.f : fy;
      fx = fx < 0.f ? 0.f : fx;
      int y0 = (int)fy, x0 = (int)fx;
      y0 = y0 > S - 1 ? S - 1 : y0;
      x0 = x0 > S - 1 ? S - 1 : x0;
      const int y1 = y0 < S - 1 ? y0 + 1 : y0, x1 = x0 < S - 1 ? x0 + 1 : x0;
      const float ly = fy - (float)y0, lx = fx - (float)x0;
      const float hy = 1.f - ly, hx = 1.f - lx;
      const float v00 = src[(long)y0 * S + x0], v01 = src[(long)y0 * S + x1];
      const float v10 = src[(long)y1 * S + x0], v11 = src[(long)y1 * S + x1];
      v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
    const float m = c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]), s = c == 0 ? sd[0] : (c == 1 ? sd[1] : sd[2]);
    y[i] = (v - m) / s;
  }
}

// ---- bidirectional attention over the L tokens of one image, head dimension 64, fp32, any L, on v_mfma_f32_32x32x2_f32.
// qkv: [B*L][3W] raw (bias added on load), head h uses columns [h*64, h*64+64) of the q / k / v thirds.
//
// A wave owns 32 query rows (a "row block") through all keys.  With r = lane & 31, g = lane >> 5:
//   S^T = K Q^T   A operand = K[key r][d], B operand = Q[query r][d], d = 8 c + 4 g + e for MFMA (c, e), c = 0..7 rising,
//                 e = 0..3 rising: a lane reads ONE 16-byte vector of K per c.  The 32 x 32 result puts the scores of query r
//                 against the keys kk(i, g) = 8 (i >> 2) + 4 g + (i & 3) into register i of lanes r and r + 32: the row
//                 maximum and the row sum are a reduction over 16 registers (i rising) and one exchange with lane ^ 32.
//   O^T = V^T P^T A operand = V[key kk(i, g)][d = 32 t + r], B operand = register i of P, for i = 0..15 rising and the two
//                 halves t of the head dimension: the k-order of the value sum follows register ownership.
//
// The tile rule.  Key tile u holds the keys [32 u, min(32 u + 32, L)); the tiles are visited in rising order and the running
// (m, s, o) of a row is rescaled once per tile (a tile with maximum m' scales s and o by exp(m - max(m, m'))).  The keys
// past L of the last tile are staged as zeros and their scores set to -3e38 before the maximum, so their probability is
// exactly 0 and they add 0 * 0.  All of this -- tile bounds, key order inside a tile, rescale sequence -- is a function of L
// alone: not of the batch, not of the number of slices, not of which wave or workgroup has the row.  Tiles are staged TK =
// 64 keys (two tiles) per barrier pair; staging groups tiles, it does not reorder them.
//
// LDS: K rows padded to 68 floats, V rows to 72 (the two half-waves of a V read are 4 rows apart: 4 x 72 = 32 banks):
// 64 x (68 + 72) x 4 B = 35840 B whatever L is.  The row blocks of an (image, head) are dealt in passes of 4 (one per
// wave) to the gridDim.z workgroups round-robin; `slices` only sizes the grid.
constexpr int KP = 68, VP = 72, TK = 64, QB = 32, PASS_ROWS = 4 * QB;
constexpr size_t ATTN_LDS = (size_t)TK * (KP + VP) * 4;

inline int attn_slices(int L, int slices) {
  const int passes = (L + PASS_ROWS - 1) / PASS_ROWS;
  return slices > 0 && slices < passes ? slices : passes;
}

__global__ __launch_bounds__(256) void mfma_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias, float* __restrict__ A, int L,
                                                        int W, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ks = sm;                    // [TK][KP]
  float* Vs = sm + TK * KP;          // [TK][VP]
  const int h = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, g = lane >> 5;
  const float* base = qkv + (long)b * L * 3 * W;
  const int passes = (L + PASS_ROWS - 1) / PASS_ROWS;
  for (int pass = blockIdx.z; pass < passes; pass += gridDim.z) {       // uniform over the workgroup: every wave meets every barrier
    const int q0 = pass * PASS_ROWS + wv * QB;
    const bool active = q0 < L;                                         // uniform over the wave
    const int qi = q0 + r < L ? q0 + r : L - 1;                         // a clamped duplicate when the rows run out: computed, not stored
    f32x4 q[8];
    {
      const float* qp = base + (long)qi * 3 * W + h * HD + 4 * g;
      const float* qb = bias + h * HD + 4 * g;
#pragma unroll
      for (int c = 0; c < 8; ++c) q[c] = (*reinterpret_cast<const f32x4*>(qp + 8 * c) + *reinterpret_cast<const f32x4*>(qb + 8 * c)) * scale;
    }
    float m = -3.0e38f, s = 0.f;
    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    for (int t0 = 0; t0 < L; t0 += TK) {
      const int n = L - t0 < TK ? L - t0 : TK;
      __syncthreads();                 // the previous stage is no longer read
      for (int i = threadIdx.x; i < TK * (HD / 4); i += 256) {
        const int row = i >> 4, c = (i & 15) * 4;
        f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if (row < n) {
          const float* src = base + (long)(t0 + row) * 3 * W + h * HD + c;
          kv = *reinterpret_cast<const f32x4*>(src + W) + *reinterpret_cast<const f32x4*>(bias + W + h * HD + c);
          vv = *reinterpret_cast<const f32x4*>(src + 2 * W) + *reinterpret_cast<const f32x4*>(bias + 2 * W + h * HD + c);
        }
        *reinterpret_cast<f32x4*>(Ks + row * KP + c) = kv;
        *reinterpret_cast<f32x4*>(Vs + row * VP + c) = vv;
      }
      __syncthreads();
      if (!active) continue;           // no barrier is skipped: both are above
      for (int u0 = 0; u0 < n; u0 += QB) {
        f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
        const float* kr = Ks + (u0 + r) * KP + 4 * g;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + 8 * c);
#pragma unroll
          for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[e], q[c][e], st, 0, 0, 0);
        }
        const int left = n - u0;       // keys of this tile in range (>= 1)
        float mx = -3.0e38f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int kk = 8 * (i >> 2) + 4 * g + (i & 3);
          st[i] = kk < left ? st[i] : -3.0e38f;
          mx = fmaxf(mx, st[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float nm = fmaxf(m, mx);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { st[i] = __expf(st[i] - nm); sum += st[i]; }
        sum += __shfl_xor(sum, 32, 64);
        const float f = __expf(m - nm);                                 // the first tile scales zeros by exp(-3e38 - nm) = 0
        s = s * f + sum;
        m = nm;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o0[i] *= f; o1[i] *= f; }
        const float* vr = Vs + (u0 + 4 * g) * VP + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float* vp = vr + (8 * (i >> 2) + (i & 3)) * VP;
          o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], st[i], o0, 0, 0, 0);
          o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32], st[i], o1, 0, 0, 0);
        }
      }
    }
    if (active && q0 + r < L) {
      // register i of o_t: d = 32 t + 8 (i >> 2) + 4 g + (i & 3) of query r: four consecutive floats per (t, i >> 2)
      float* out = A + ((long)b * L + q0 + r) * W + h * HD + 4 * g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = o0[4 * j + e] / s; c[e] = o1[4 * j + e] / s; }
        *reinterpret_cast<f32x4*>(out + 8 * j) = a;
        *reinterpret_cast<f32x4*>(out + 32 + 8 * j) = c;
      }
    }
  }
}

// ---- the self-similarity head.  keys [2N][L][W]: pair n = images n (a) and N + n (b).
// norms: nrm[img][l] = sqrt(sum_w k^2), one wave per row, lane-strided then the xor tree
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ k, float* __restrict__ nrm, long rows, int W) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* kr = k + row * W;
  float s = 0.f;
  for (int i = lane; i < W; i += 64) s += kr[i] * kr[i];
  s = wave_sum(s);
  if (lane == 0) nrm[row] = sqrtf(s);
}
// One wave per 32 x 32 tile (ti, tj) of the two L x L matrices: both Gram tiles K_a K_a^T and K_b K_b^T on
// v_mfma_f32_32x32x2_f32 with the k-order (c rising over chunks of 8, e = 0..3, half-wave g: w = 8 c + 4 g + e), each entry
// divided by max(n_i n_j, 1e-8), the difference squared, and summed: a lane adds its 16 registers in rising order (entries
// outside L x L add 0), the wave folds with the xor tree, part[n][ti * T + tj] gets the tile's sum.  Rows past L read row
// L - 1 (finite, masked out of the sum).  Nothing here depends on N.  grid (T, T, N), W % 8 == 0.
__global__ __launch_bounds__(64) void selfsim_tile_kernel(const float* __restrict__ keys, const float* __restrict__ nrm, int N, int L, int W,
                                                          float* __restrict__ part) {
  const int lane = threadIdx.x, r = lane & 31, g = lane >> 5;
  const int tj = blockIdx.x, ti = blockIdx.y, n = blockIdx.z;
  const int i0 = ti * 32, j0 = tj * 32;
  const int ia = i0 + r < L ? i0 + r : L - 1, jb = j0 + r < L ? j0 + r : L - 1;
  const float* Ka = keys + (size_t)n * L * W;
  const float* Kb = keys + (size_t)(N + n) * L * W;
  const float* ai = Ka + (size_t)ia * W + 4 * g;
  const float* aj = Ka + (size_t)jb * W + 4 * g;
  const float* bi = Kb + (size_t)ia * W + 4 * g;
  const float* bj = Kb + (size_t)jb * W + 4 * g;
  f32x16 ga, gb;
#pragma unroll
  for (int i = 0; i < 16; ++i) { ga[i] = 0.f; gb[i] = 0.f; }
  for (int c = 0; c < W; c += 8) {
    const f32x4 xa = *reinterpret_cast<const f32x4*>(ai + c), ya = *reinterpret_cast<const f32x4*>(aj + c);
    const f32x4 xb = *reinterpret_cast<const f32x4*>(bi + c), yb = *reinterpret_cast<const f32x4*>(bj + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ga = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], ya[e], ga, 0, 0, 0);
      gb = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[e], yb[e], gb, 0, 0, 0);
    }
  }
  // register i: row i0 + 8 (i >> 2) + 4 g + (i & 3), column j0 + r
  const float* na = nrm + (size_t)n * L;
  const float* nb = nrm + (size_t)(N + n) * L;
  const bool jok = j0 + r < L;
  const float naj = na[jb], nbj = nb[jb];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = i0 + 8 * (i >> 2) + 4 * g + (i & 3);
    const int rc = row < L ? row : L - 1;
    const float sa = ga[i] / fmaxf(na[rc] * naj, 1e-8f), sb = gb[i] / fmaxf(nb[rc] * nbj, 1e-8f);
    const float d = sa - sb;
    sum += jok && row < L ? d * d : 0.f;
  }
  sum = wave_sum(sum);
  if (lane == 0) part[((size_t)n * gridDim.y + ti) * gridDim.x + tj] = sum;
}
// dist[n] = (sum of the tile sums of pair n) / L^2: thread t adds the slots t, t + 256, ... in rising order, then a fixed
// binary tree over the 256 threads.  grid (N)
__global__ __launch_bounds__(256) void selfsim_sum_kernel(const float* __restrict__ part, int tiles, int L, float* __restrict__ dist) {
  __shared__ float s[256];
  const int n = blockIdx.x;
  float v = 0.f;
  for (int i = threadIdx.x; i < tiles; i += 256) v += part[(size_t)n * tiles + i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dist[n] = s[0] / ((float)L * (float)L);
}

// facebookresearch/dino vision_transformer.py: blocks.<i>
constexpr EncNames DINO_BLOCK_NAMES = {{".norm1.weight", ".norm1.bias", ".attn.qkv.weight", ".attn.qkv.bias", ".attn.proj.weight", ".attn.proj.bias",
                                        ".norm2.weight", ".norm2.bias", ".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.fc2.weight", ".mlp.fc2.bias"}};

}  // namespace

struct HEDIT_HANDLE hedit_dino : ParamStore {
  hedit_dino_cfg cfg;
  int L = 0, P = 0;
  int slices = 0;                 // > 0: the attention grid's slice count (hedit_dino_set_slices), else one per pass
  float *conv_w = nullptr, *conv_b = nullptr, *cls = nullptr, *pos = nullptr;
  PConv conv;
  std::vector<EncBlock> blocks;   // key_layer whole blocks
  float *kln_g = nullptr, *kln_b = nullptr, *kw = nullptr, *kb = nullptr;      // block key_layer: norm1 and the fused qkv (its key third is used)
  PConv key;
};

namespace {

// image [B][3][S][S] (0..255, masked) -> keys [B][L][W] (workspace or caller memory; written by the last kernel)
int run_keys(hedit_dino* h, PF& f, const float* image, int B, int S, float* keys) {
  const bool dry = f.dry();
  hipStream_t st = f.st;
  const int W = h->cfg.width, L = h->L, R = h->cfg.input_resolution, p = h->cfg.patch_size, heads = h->cfg.heads;
  const int K0 = 3 * p * p;
  const long Mp = (long)B * (L - 1), M = (long)B * L;
  const float ascale = 0.125f;     // 64^-0.5
  float *img, *X0, *Em, *T;
  TRY(aalloc(f, &img, (size_t)B * 3 * R * R));
  if (!dry) { hipLaunchKernelGGL(prep_kernel, egrid((long)B * 3 * R * R), dim3(256), 0, st, image, img, B, S, R); LAUNCH_CHECK(); }
  TRY(aalloc(f, &X0, (size_t)Mp * K0));
  if (!dry) TRY(enc_patchify_launch(img, X0, B, R, p, 0, st));
  TRY(lin(f, X0, K0, P_COPY, nullptr, nullptr, h->conv, false, Mp, &Em));
  TRY(aalloc(f, &T, (size_t)M * W));
  if (!dry) TRY(enc_tokens_launch(Em, h->conv_b, h->cls, h->pos, T, B, L, W, st));
  f.ar.free(Em);
  f.ar.free(X0);
  f.ar.free(img);
  auto attn = [&](const float* qkv, const float* bias, float* A) -> int {
    hipLaunchKernelGGL(mfma_attn_kernel, dim3(heads, B, attn_slices(L, h->slices)), dim3(256), ATTN_LDS, st, qkv, bias, A, L, W, ascale);
    LAUNCH_CHECK();
    return HEDIT_OK;
  };
  for (const EncBlock& k : h->blocks) TRY(enc_block_forward(f, k, T, M, W, P_GELU, LN_EPS, attn));      // exact (erf) GELU
  // block key_layer: norm1 and the key third of qkv
  float *a, *raw;
  TRY(aalloc(f, &a, (size_t)M * W));
  TRY(ln(f, T, h->kln_g, h->kln_b, M, W, LN_EPS, a));
  TRY(lin(f, a, W, P_COPY, nullptr, nullptr, h->key, false, M, &raw));
  if (!dry) TRY(enc_add_bias_res_launch(raw, h->kb + W, nullptr, keys, M * W, W, st));      // out = raw + bias: the keys
  f.ar.free(raw);
  f.ar.free(a);
  f.ar.free(T);
  return HEDIT_OK;
}

int run_keys_entry(hedit_dino* h, const float* image, int B, int S, float* keys, void* ws, size_t ws_bytes, hipStream_t st, bool dry, size_t* peak) {
  PF f = make_pf(B, ws, ws_bytes, st, dry);
  TRY(run_keys(h, f, image, B, S, keys));
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

// a, b [N][3][S][S] -> dist [N].  Both images of all N pairs go through the network as ONE batch of 2 N.
int run_dist(hedit_dino* h, const float* a, const float* b, int N, int S, float* dist, void* ws, size_t ws_bytes, hipStream_t st, bool dry,
             size_t* peak) {
  PF f = make_pf(2 * N, ws, ws_bytes, st, dry);
  const int W = h->cfg.width, L = h->L;
  const size_t one = (size_t)N * 3 * S * S;
  const int T = cdiv(L, 32);
  float *both, *keys, *nrm, *part;
  TRY(aalloc(f, &keys, (size_t)2 * N * L * W));
  TRY(aalloc(f, &nrm, (size_t)2 * N * L));
  TRY(aalloc(f, &part, (size_t)N * T * T));
  TRY(aalloc(f, &both, 2 * one));
  if (!dry) {
    HIP_TRY(hipMemcpyAsync(both, a, one * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(both + one, b, one * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  TRY(run_keys(h, f, both, 2 * N, S, keys));
  f.ar.free(both);
  if (!dry) {
    const long rows = (long)2 * N * L;
    hipLaunchKernelGGL(row_norm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, keys, nrm, rows, W);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(selfsim_tile_kernel, dim3(T, T, N), dim3(64), 0, st, keys, nrm, N, L, W, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(selfsim_sum_kernel, dim3(N), dim3(256), 0, st, part, T * T, L, dist);
    LAUNCH_CHECK();
  }
  f.ar.free(part);
  f.ar.free(nrm);
  f.ar.free(keys);
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

}  // namespace

HEDIT_LIFECYCLE(dino, hedit_dino, "DINO ViT", no_pre_destroy)

extern "C" {

int hedit_dino_create(const hedit_dino_cfg* cfg, hedit_dino** out) try {
  ARG_CHECK(cfg && out, "null");
  ARG_CHECK(cfg->width > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->patch_size > 0 && cfg->input_resolution > 0, "dino: sizes must be positive");
  ARG_CHECK(cfg->width % 64 == 0 && cfg->width % cfg->heads == 0 && cfg->width / cfg->heads == 64, "dino: head dimension must be 64");
  ARG_CHECK(cfg->input_resolution % cfg->patch_size == 0, "dino: input_resolution must be a multiple of patch_size");
  ARG_CHECK(cfg->key_layer >= 0 && cfg->key_layer < cfg->layers, "dino: key_layer must be in [0, layers)");
  const long P = cfg->input_resolution / cfg->patch_size;
  ARG_CHECK(P * P + 1 <= LMAX, "dino: at most 1025 tokens");
  const int L = (int)(P * P + 1);
  TRY(gemm_prepare());
  hedit_dino* h = new hedit_dino();
  h->cfg = *cfg;
  h->P = (int)P; h->L = L;
  const int W = cfg->width, p = cfg->patch_size;
  {
    h->cls = dalloc<float>(h, W);
    add_slot(h, "cls_token", Pack::F32, h->cls, W, 0, 0, 3, 1, 1, W, 1);
    h->pos = dalloc<float>(h, (size_t)L * W);
    add_slot(h, "pos_embed", Pack::F32, h->pos, (size_t)L * W, 0, 0, 3, 1, L, W, 1);
  }
  h->conv_w = f32conv(h, "patch_embed.proj.weight", W, 3, p);
  h->conv_b = vec(h, "patch_embed.proj.bias", W);
  for (int i = 0; i < cfg->key_layer; ++i) h->blocks.push_back(enc_add_block(h, "blocks." + std::to_string(i), DINO_BLOCK_NAMES, W));
  {
    const std::string pre = "blocks." + std::to_string(cfg->key_layer);
    const EncNames& n = DINO_BLOCK_NAMES;
    h->kln_g = vec(h, pre + n.s[0], W); h->kln_b = vec(h, pre + n.s[1], W);
    h->kw = mat(h, pre + n.s[2], 3 * W, W); h->kb = vec(h, pre + n.s[3], 3 * W);
  }
  return handle_created(h, out);
} catch (...) { return hedit_abi_catch(); }

int hedit_dino_finalize(hedit_dino* h, void* stream) try {
  ARG_CHECK(h, "null");
  TRY(handle_loaded(h));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int W = h->cfg.width, p = h->cfg.patch_size;
  TRY(pack_fwd(h, h->conv, h->conv_w, W, 3 * p * p, false, st));
  for (EncBlock& k : h->blocks) TRY(enc_pack_block(h, k, W, true, st));
  TRY(pack_fwd(h, h->key, h->kw + (size_t)W * W, W, W, false, st));    // rows [W, 2W) of qkv: the keys
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&mfma_attn_kernel), (int)ATTN_LDS)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (h->alloc_failed) { hedit_set_error("hipMalloc failed while packing the DINO ViT's weights"); return HEDIT_ERR_HIP; }
  h->finalized = true;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* A test knob (the grid-independence test resizes the attention grid with it).  slices > 0: the number of workgroups the
 * query rows of one (image, head) are dealt to, clamped to the number of 128-row passes; 0: one per pass (the default).  The
 * output bits do not depend on it. */
int hedit_dino_set_slices(hedit_dino* h, int slices) try {
  ARG_CHECK(h && slices >= 0, "dino_set_slices: slices >= 0");
  h->slices = slices;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* bytes hedit_dino_structure_distance needs for N pairs of S x S images; hedit_dino_keys with B <= 2 N images needs no more */
size_t hedit_dino_workspace_bytes(hedit_dino* h, int N, int S) try {
  if (!h || N < 1 || N > HEDIT_DINO_MAX_PAIRS || S < h->cfg.patch_size || S > MAX_SIDE) return 0;
  size_t peak = 0;
  const int rc = run_dist(h, nullptr, nullptr, N, S, nullptr, nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* image fp32 [B][3][S][S], 0..255 scale, already multiplied by its mask -> keys fp32 [B][L][W] of block key_layer (bias
 * included).  Every argument is checked before the first launch. */
int hedit_dino_keys(hedit_dino* h, const float* image, int B, int S, float* keys, void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && image && keys, "dino_keys: null");
  TRY(handle_finalized(h));
  ARG_CHECK(B >= 1 && B <= 2 * HEDIT_DINO_MAX_PAIRS, "dino_keys: 1 <= B <= 128");
  ARG_CHECK(S >= h->cfg.patch_size && S <= MAX_SIDE, "dino_keys: S must be in [patch_size, 4096]");
  ARG_CHECK(workspace, "dino_keys: null workspace");
  size_t need = 0;
  TRY(run_keys_entry(h, nullptr, B, S, nullptr, nullptr, 0, nullptr, true, &need));
  TRY(ws_check("dino_keys", need, workspace_bytes));
  return run_keys_entry(h, image, B, S, keys, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

/* a, b fp32 [N][3][S][S] as above -> dist fp32 [N], dist[n] = mean((S(a_n) - S(b_n))^2).  Every argument is checked before
 * the first launch. */
int hedit_dino_structure_distance(hedit_dino* h, const float* a, const float* b, int N, int S, float* dist, void* workspace, size_t workspace_bytes,
                                  void* stream) try {
  ARG_CHECK(h && a && b && dist, "dino_structure_distance: null");
  TRY(handle_finalized(h));
  ARG_CHECK(N >= 1 && N <= HEDIT_DINO_MAX_PAIRS, "dino_structure_distance: 1 <= N <= 64");
  ARG_CHECK(S >= h->cfg.patch_size && S <= MAX_SIDE, "dino_structure_distance: S must be in [patch_size, 4096]");
  ARG_CHECK(workspace, "dino_structure_distance: null workspace");
  size_t need = 0;
  TRY(run_dist(h, nullptr, nullptr, N, S, nullptr, nullptr, 0, nullptr, true, &need));
  TRY(ws_check("dino_structure_distance", need, workspace_bytes));
  return run_dist(h, a, b, N, S, dist, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
