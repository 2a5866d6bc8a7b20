// The CLIP image tower as a native executor: `CLIP.encode_image` of the reference's text-guided-n-style/clip_guidance/clip/
// model.py:202-236 (VisionTransformer) = transformers' CLIPVisionModelWithProjection, the model the PIE-Bench evaluator
// scores edits with (text-guided/evaluation/matrics_calculator.py:274, CLIP ViT-L/14).  Patch embedding, class token +
// positional embedding, ln_pre, ALL `layers` pre-LN ResidualAttentionBlocks (fused q/k/v projection, bidirectional
// multi-head attention, QuickGELU MLP), ln_post on the class row, times `visual.proj`.  Forward only.
//
// Arithmetic as in vit.hip / text.hip: fp32 token stream, LayerNorm / softmax / QuickGELU in fp32, every contraction a
// three-term split-bf16 product with fp32 accumulation (pnet.hip), canonical chunk order with the batch in M: a batch gives
// the bytes of single calls.  The output is fp32 and nothing here reads the storage type, so both builds give the same bits.
// Parameters by the OpenAI CLIP state_dict names (`visual.conv1.weight` ... `visual.ln_post.weight`, `visual.proj`).
//
// The kernels every encoder runs (patches, tokens, LayerNorm forward, out = res + raw + bias, the row gather) are those of
// encoder.hip and the block forward is encoder.h's.  What is this file's own is the attention kernel: vit.hip keeps all keys
// and values of an (image, head) in LDS, which ends at 200 tokens; this one walks them in tiles.
#include "encoder.h"

namespace {

constexpr float LN_EPS = 1e-5f;

// ---- bidirectional attention over the L tokens of one image, head dimension 64, fp32, any L: the keys and values of an
// (image, head) pass through LDS in tiles of TK = 128 rows and the softmax is carried across the tiles (running maximum m,
// running sum s, running output o; a tile with maximum m' first scales s and o by exp(m - max(m, m'))).  qkv: [B*L][3W]
// raw (bias added on load), head h uses columns [h*64, h*64+64) of the q / k / v thirds.
//
// LDS: K and V tiles as fp32 rows padded to 68 floats (16-byte aligned; the four 16-lane groups of a ds_read_b128 with
// lane = row hit all 64 banks) = 2 x 128 x 68 x 4 B = 69632 B, plus the probabilities of the 8 rows in flight, 8 x 128 x 4 B
// = 4096 B: 73728 B = 72 KiB whatever L is, so two workgroups share the 160 KiB of a CU (vit.hip's whole-head layout would
// need 140 KB at 257 tokens and does not fit at 577).
//
// The tile rule.  Tile t holds the keys [128 t, min(128 t + 128, L)); the tiles are visited in rising order; both are
// functions of L alone.  The query rows are cut into passes of RP = 32: pass P gives wave w (of 4) the row pairs
// (32 P + 8 u + w, 32 P + 8 u + w + 4), u = 0..3, and a wave carries (m, s, o) of its 8 rows in registers through all tiles
// of the pass -- so K and V are staged L / 32 times per (image, head), not L / 8 times.  The passes are dealt to the
// gridDim.z workgroups of the (image, head) round-robin (one pass each by default).  What a row computes -- the tile bounds, the order of the keys
// inside a tile (score j by lane j mod 64; the value sum in two chains of quads, folded at the end), the rescale
// sequence -- depends on L only: not on the batch, not on the number of slices, not on which wave or workgroup has the
// row.  No log-sum-exp is written: there is no backward pass.
constexpr int HD = 64, HP = 68, TK = 128, RP = 32, NPAIR = 4, LMAX = 577;
constexpr size_t ATTN_LDS = (size_t)(2 * TK * HP + 8 * TK) * 4;
typedef __attribute__((ext_vector_type(4))) float fl4;

// slices per (image, head): one workgroup per pass (9 at 257 tokens: the 512 workgroup slots of the MI355X's 256 CUs pick
// them up as they free, where 4 slices of 3 / 2 / 2 / 2 passes would wait for the longest).  It only sizes the grid, the
// result does not depend on it (`slices` > 0 overrides it: the tests do).
inline int attn_slices(int L, int slices) {
  const int passes = (L + RP - 1) / RP;
  return slices > 0 && slices < passes ? slices : passes;
}

__global__ __launch_bounds__(256, 2) void tiled_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias, float* __restrict__ A,
                                                            int L, int W, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ks = sm;
  float* Vs = sm + TK * HP;
  float* ps = Vs + TK * HP;            // [8][TK]
  const int h = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* pa = ps + (2 * wv) * TK;
  float* pb = pa + TK;
  const float* base = qkv + (long)b * L * 3 * W;
  const float* qbias = bias + h * HD;
  const int passes = (L + RP - 1) / RP;
  for (int pass = blockIdx.z; pass < passes; pass += gridDim.z) {       // uniform over the workgroup: every wave meets every barrier
    float m[NPAIR][2], s[NPAIR][2], o[NPAIR][2];
#pragma unroll
    for (int u = 0; u < NPAIR; ++u)
#pragma unroll
      for (int e = 0; e < 2; ++e) { m[u][e] = -3.0e38f; s[u][e] = 0.f; o[u][e] = 0.f; }
    for (int t0 = 0; t0 < L; t0 += TK) {
      const int n = L - t0 < TK ? L - t0 : TK;
      __syncthreads();                 // the previous tile is no longer read
      for (int i = threadIdx.x; i < n * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float* src = base + (long)(t0 + r) * 3 * W + h * HD + c;
        *reinterpret_cast<fl4*>(Ks + r * HP + c) = *reinterpret_cast<const fl4*>(src + W) + *reinterpret_cast<const fl4*>(bias + W + h * HD + c);
        *reinterpret_cast<fl4*>(Vs + r * HP + c) = *reinterpret_cast<const fl4*>(src + 2 * W) + *reinterpret_cast<const fl4*>(bias + 2 * W + h * HD + c);
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NPAIR; ++u) {
        const int i0 = pass * RP + u * 8 + wv;
        if (i0 >= L) continue;         // uniform over the wave; no barrier below
        const bool two = i0 + 4 < L;
        const int i1 = two ? i0 + 4 : i0;      // a clamped duplicate when the rows run out: computed, not stored
        fl4 qa[16], qb[16];
        const float* q0 = base + (long)i0 * 3 * W + h * HD;
        const float* q1 = base + (long)i1 * 3 * W + h * HD;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const fl4 bq = *reinterpret_cast<const fl4*>(qbias + 4 * c);
          qa[c] = (*reinterpret_cast<const fl4*>(q0 + 4 * c) + bq) * scale;
          qb[c] = (*reinterpret_cast<const fl4*>(q1 + 4 * c) + bq) * scale;
        }
        float ma = -3.0e38f, mb = -3.0e38f;
        for (int j = lane; j < n; j += 64) {
          const float* row = Ks + j * HP;
          float sa = 0.f, sb = 0.f;
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const fl4 k = *reinterpret_cast<const fl4*>(row + 4 * c);
            sa += qa[c][0] * k[0] + qa[c][1] * k[1] + qa[c][2] * k[2] + qa[c][3] * k[3];
            sb += qb[c][0] * k[0] + qb[c][1] * k[1] + qb[c][2] * k[2] + qb[c][3] * k[3];
          }
          pa[j] = sa; pb[j] = sb;
          ma = fmaxf(ma, sa); mb = fmaxf(mb, sb);
        }
        // p[] is written per lane and read across lanes below without a barrier: LDS operations of one wave complete in
        // order (as in vit.hip's attn_fwd_kernel)
        const float na = fmaxf(m[u][0], wave_max(ma)), nb = fmaxf(m[u][1], wave_max(mb));
        float suma = 0.f, sumb = 0.f;
        for (int j = lane; j < n; j += 64) {
          const float ea = __expf(pa[j] - na), eb = __expf(pb[j] - nb);
          pa[j] = ea; pb[j] = eb;
          suma += ea; sumb += eb;
        }
        suma = wave_sum(suma); sumb = wave_sum(sumb);
        // o[lane] += sum_j p[j] V[j][lane]: two partial chains per row (even / odd quads), folded at the end, then a serial tail
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        int j = 0;
        for (; j + 8 <= n; j += 8) {
          const fl4 p0 = *reinterpret_cast<const fl4*>(pa + j), p1 = *reinterpret_cast<const fl4*>(pb + j);
          const fl4 r0 = *reinterpret_cast<const fl4*>(pa + j + 4), r1 = *reinterpret_cast<const fl4*>(pb + j + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = Vs[(j + e) * HP + lane], v2 = Vs[(j + 4 + e) * HP + lane];
            a0 += p0[e] * v; a1 += p1[e] * v;
            b0 += r0[e] * v2; b1 += r1[e] * v2;
          }
        }
        for (; j < n; ++j) { const float v = Vs[j * HP + lane]; a0 += pa[j] * v; a1 += pb[j] * v; }
        // the first tile scales zeros by exp(-3e38 - na) = 0
        const float fa = __expf(m[u][0] - na), fb = __expf(m[u][1] - nb);
        s[u][0] = s[u][0] * fa + suma; s[u][1] = s[u][1] * fb + sumb;
        o[u][0] = o[u][0] * fa + (a0 + b0); o[u][1] = o[u][1] * fb + (a1 + b1);
        m[u][0] = na; m[u][1] = nb;
      }
    }
#pragma unroll
    for (int u = 0; u < NPAIR; ++u) {
      const int i0 = pass * RP + u * 8 + wv;
      if (i0 >= L) continue;
      A[((long)b * L + i0) * W + h * HD + lane] = o[u][0] / s[u][0];
      if (i0 + 4 < L) A[((long)b * L + i0 + 4) * W + h * HD + lane] = o[u][1] / s[u][1];
    }
  }
}

}  // namespace

struct HEDIT_HANDLE hedit_clipimg : ParamStore {
  hedit_clipimg_cfg cfg;
  int L = 0, P = 0;
  int slices = 0;                 // > 0: the attention grid's slice count (hedit_clipimg_set_slices), else one per pass
  float *conv_w = nullptr, *cls = nullptr, *pos = nullptr, *lnpg = nullptr, *lnpb = nullptr, *lnog = nullptr, *lnob = nullptr,
        *proj_w = nullptr;
  PConv conv, proj;
  std::vector<EncBlock> blocks;
};

namespace {

// img [B][3][R][R] (CLIP-normalised) -> out [B][embed_dim]
int run(hedit_clipimg* h, const float* img, int B, float* out, void* ws, size_t ws_bytes, hipStream_t st, bool dry, size_t* peak) {
  PF f = make_pf(B, ws, ws_bytes, st, dry);
  const int W = h->cfg.width, L = h->L, R = h->cfg.input_resolution, p = h->cfg.patch_size, heads = h->cfg.heads, E = h->cfg.embed_dim;
  const int K0 = 3 * p * p;
  const long Mp = (long)B * (L - 1), M = (long)B * L;
  const float ascale = 1.0f / sqrtf((float)HD);
  float *X0, *Em, *T0, *T;
  TRY(aalloc(f, &X0, (size_t)Mp * K0));
  if (!dry) TRY(enc_patchify_launch(img, X0, B, R, p, 0, st));
  TRY(lin(f, X0, K0, P_COPY, nullptr, nullptr, h->conv, false, Mp, &Em));
  f.ar.free(X0);
  TRY(aalloc(f, &T0, (size_t)M * W));
  if (!dry) TRY(enc_tokens_launch(Em, nullptr, h->cls, h->pos, T0, B, L, W, st));
  f.ar.free(Em);
  TRY(aalloc(f, &T, (size_t)M * W));
  TRY(ln(f, T0, h->lnpg, h->lnpb, M, W, LN_EPS, T));
  f.ar.free(T0);
  auto attn = [&](const float* qkv, const float* bias, float* A) -> int {
    hipLaunchKernelGGL(tiled_attn_kernel, dim3(heads, B, attn_slices(L, h->slices)), dim3(256), ATTN_LDS, st, qkv, bias, A, L, W, ascale);
    LAUNCH_CHECK();
    return HEDIT_OK;
  };
  for (const EncBlock& k : h->blocks) TRY(enc_block_forward(f, k, T, M, W, P_QGELU, LN_EPS, attn));
  // ln_post on the class row, times visual.proj: text.hip's pooled path with row 0
  float *Rw, *N, *o;
  TRY(aalloc(f, &Rw, (size_t)B * W));
  if (!dry) TRY(enc_gather_rows_launch(T, nullptr, Rw, B, L, W, st));
  TRY(aalloc(f, &N, (size_t)B * W));
  TRY(ln(f, Rw, h->lnog, h->lnob, B, W, LN_EPS, N));
  TRY(lin(f, N, W, P_COPY, nullptr, nullptr, h->proj, true, B, &o));            // one M = B GEMM: x @ visual.proj
  if (!dry) HIP_TRY(hipMemcpyAsync(out, o, (size_t)B * E * sizeof(float), hipMemcpyDeviceToDevice, st));
  f.ar.free(o);
  f.ar.free(N);
  f.ar.free(Rw);
  f.ar.free(T);
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

}  // namespace

HEDIT_LIFECYCLE(clipimg, hedit_clipimg, "CLIP image tower", no_pre_destroy)

extern "C" {

int hedit_clipimg_create(const hedit_clipimg_cfg* cfg, hedit_clipimg** out) try {
  ARG_CHECK(cfg && out, "null");
  ARG_CHECK(cfg->width > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->patch_size > 0 && cfg->input_resolution > 0 && cfg->embed_dim > 0,
            "clipimg: sizes must be positive");
  ARG_CHECK(cfg->width % 64 == 0 && cfg->width % cfg->heads == 0 && cfg->width / cfg->heads == 64, "clipimg: head dimension must be 64");
  ARG_CHECK(cfg->input_resolution % cfg->patch_size == 0, "clipimg: input_resolution must be a multiple of patch_size");
  ARG_CHECK(cfg->embed_dim % 4 == 0, "clipimg: embed_dim must be a multiple of 4");
  const int P = cfg->input_resolution / cfg->patch_size;
  ARG_CHECK(P <= 24 && P * P + 1 <= LMAX, "clipimg: at most 577 tokens");
  const int L = P * P + 1;
  TRY(gemm_prepare());
  hedit_clipimg* h = new hedit_clipimg();
  h->cfg = *cfg;
  h->P = P; h->L = L;
  const int W = cfg->width, p = cfg->patch_size, E = cfg->embed_dim;
  h->conv_w = f32conv(h, "visual.conv1.weight", W, 3, p);
  h->cls = vec(h, "visual.class_embedding", W);
  h->pos = mat(h, "visual.positional_embedding", L, W);
  h->lnpg = vec(h, "visual.ln_pre.weight", W);
  h->lnpb = vec(h, "visual.ln_pre.bias", W);
  for (int i = 0; i < cfg->layers; ++i)
    h->blocks.push_back(enc_add_block(h, "visual.transformer.resblocks." + std::to_string(i), CLIP_BLOCK_NAMES, W));
  h->lnog = vec(h, "visual.ln_post.weight", W);
  h->lnob = vec(h, "visual.ln_post.bias", W);
  h->proj_w = mat(h, "visual.proj", W, E);
  return handle_created(h, out);
} catch (...) { return hedit_abi_catch(); }

int hedit_clipimg_finalize(hedit_clipimg* h, void* stream) try {
  ARG_CHECK(h, "null");
  TRY(handle_loaded(h));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int W = h->cfg.width, p = h->cfg.patch_size;
  // conv1 weight [W][3][p][p] flattened = a linear map over (c, ky, kx)
  TRY(pack_fwd(h, h->conv, h->conv_w, W, 3 * p * p, false, st));
  for (EncBlock& k : h->blocks) TRY(enc_pack_block(h, k, W, true, st));
  TRY(pack_fwd(h, h->proj, h->proj_w, W, h->cfg.embed_dim, true, st));
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&tiled_attn_kernel), (int)ATTN_LDS)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (h->alloc_failed) { hedit_set_error("hipMalloc failed while packing the CLIP image tower's weights"); return HEDIT_ERR_HIP; }
  h->finalized = true;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* A test knob (the slice-independence test resizes the grid with it).  slices > 0: the number of workgroups the query rows of one (image, head) are dealt to, clamped to the number of 32-row
 * passes; 0: one per pass (the default).  The output bits do not depend on it. */
int hedit_clipimg_set_slices(hedit_clipimg* h, int slices) try {
  ARG_CHECK(h && slices >= 0, "clipimg_set_slices: slices >= 0");
  h->slices = slices;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

size_t hedit_clipimg_workspace_bytes(hedit_clipimg* h, int B) try {
  if (!h || B < 1 || B > HEDIT_CLIPIMG_MAX_BATCH) return 0;
  size_t peak = 0;
  const int rc = run(h, nullptr, B, reinterpret_cast<float*>(4096), nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* image fp32 [B][3][R][R], CLIP-normalised and resized -> out fp32 [B][embed_dim] (not normalised).  Every argument is
 * checked before the first launch. */
int hedit_clipimg_encode(hedit_clipimg* h, const float* image, int B, float* out, void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && image && out, "clipimg_encode: null");
  ARG_CHECK(B >= 1 && B <= HEDIT_CLIPIMG_MAX_BATCH, "clipimg_encode: 1 <= B <= 256");
  ARG_CHECK(workspace, "clipimg_encode: null workspace");
  TRY(handle_finalized(h));
  size_t need = 0;
  TRY(run(h, nullptr, B, out, nullptr, 0, nullptr, true, &need));
  TRY(ws_check("clipimg_encode", need, workspace_bytes));
  return run(h, image, B, out, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
