// The prompt encoder as a native executor: `CLIP.encode_text` of the reference's text-guided-n-style/clip_guidance/clip/
// model.py:367-380 = transformers' CLIPTextModel of SD-1.x.  Token embedding gather +
// positional embedding, `layers` pre-LN ResidualAttentionBlocks with a causal mask (fused q/k/v projection, multi-head
// attention, QuickGELU MLP, model.py:153-190), ln_final; optionally the pooled output: the ln_final row at a given position
// per prompt, times `text_projection` when the model has one.  Forward only.
//
// Arithmetic as in vit.hip: fp32 token stream, LayerNorm / softmax / QuickGELU in fp32, every contraction a three-term
// split-bf16 product with fp32 accumulation (pnet.hip), canonical chunk order with the batch in M: a batch gives the bytes
// of single calls.  The output is fp32 and nothing here reads the storage type, so both builds give the same bits.
// Parameters by the OpenAI CLIP state_dict names (`token_embedding.weight`, `transformer.resblocks.0.attn.in_proj_weight` ...).
//
// The kernels every encoder runs (LayerNorm, out = res + raw + bias, the row gather) are those of encoder.hip and the block
// forward is encoder.h's; what is this file's own is the embedding gather and the causal attention kernel.
#include "encoder.h"

namespace {

constexpr float LN_EPS = 1e-5f;

// T[b][l] = tok[clamp(ids[b][l])] + pos[l].  An id outside [0, vocab) never reads outside the table; rejecting it is the
// caller's job (hedit.text.NativeClipText does).
__global__ __launch_bounds__(256) void embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                    float* __restrict__ T, long rows, int L, int W, int vocab) {
  const long total = rows * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int w = (int)(i % W);
    const long row = i / W;
    const int l = (int)(row % L);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    T[i] = tok[(long)id * W + w] + pos[(long)l * W + w];
  }
}

// ---- causal attention over the L tokens of one prompt, head dimension 64, fp32.  qkv: [B*L][3W] raw (bias added on load),
// head h uses columns [h*64, h*64+64) of the q / k / v thirds.  K and V of one (prompt, head) are resident in LDS, rows
// padded to 68 floats (16-byte aligned; the four 16-lane groups of a ds_read_b128 with lane = row hit all 64 banks): at
// L = 77 that is 2 x 77 x 68 x 4 B = 42 KB + 1.3 KB of probabilities, so three workgroups share a CU.
//
// Row i reads keys and values j <= i and nothing else: the score, max, sum and value loops all run over n = i + 1 entries,
// so the bits of row i are a function of the tokens 0..i alone (the prefix property), and the triangle costs half the square.
// One wave produces one row at a time, in an order fixed by n.  The work of a row grows with i, so the rows are dealt to
// the G = 4 * gridDim.z waves of a (prompt, head) in boustrophedon order -- round r gives wave g row r G + g when r is even
// and r G + (G - 1 - g) when r is odd -- which evens out the triangle to within one row per pair of rounds.  Which wave
// computes a row changes nothing about its arithmetic, so the result does not depend on the slice count.
constexpr int HD = 64, HP = 68, LMAX = 200;
typedef __attribute__((ext_vector_type(4))) float fl4;

inline int attn_lp(int L) { return (L + 3) / 4 * 4; }
inline size_t attn_lds(int L) { return (size_t)(2 * L * HP + 4 * attn_lp(L)) * 4; }
// slices per (prompt, head): 768 = three workgroups (44 KB of LDS each at L = 77) on each of the MI355X's 256 CUs in one
// round, at most 4 (16 waves for 77 rows).  A constant, not a device query: it only sizes the grid, the result does not depend on it.
inline int attn_slices(int heads, int B) {
  const int z = 768 / (heads * B);
  return z < 1 ? 1 : (z > 4 ? 4 : z);
}

__global__ __launch_bounds__(256) void causal_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bias, float* __restrict__ A,
                                                          int L, int W, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ks = sm;
  float* Vs = sm + L * HP;
  float* ps = Vs + L * HP;             // [4][Lp]
  const int h = blockIdx.x, b = blockIdx.y;
  const float* base = qkv + (long)b * L * 3 * W;
  for (int i = threadIdx.x; i < L * (HD / 4); i += 256) {
    const int r = i >> 4, c = (i & 15) * 4;
    const float* src = base + (long)r * 3 * W + h * HD + c;
    *reinterpret_cast<fl4*>(Ks + r * HP + c) = *reinterpret_cast<const fl4*>(src + W) + *reinterpret_cast<const fl4*>(bias + W + h * HD + c);
    *reinterpret_cast<fl4*>(Vs + r * HP + c) = *reinterpret_cast<const fl4*>(src + 2 * W) + *reinterpret_cast<const fl4*>(bias + 2 * W + h * HD + c);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* p = ps + wv * ((L + 3) / 4 * 4);      // attn_lp(L)
  const int G = 4 * gridDim.z, g = blockIdx.z * 4 + wv;
  for (int r = 0; r * G < L; ++r) {
    const int i = r * G + ((r & 1) ? G - 1 - g : g);
    if (i >= L) continue;
    const int n = i + 1;
    fl4 q[16];
    const float* qs = base + (long)i * 3 * W + h * HD;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      q[c] = (*reinterpret_cast<const fl4*>(qs + 4 * c) + *reinterpret_cast<const fl4*>(bias + h * HD + 4 * c)) * scale;
    float m = -3.0e38f;
    for (int j = lane; j < n; j += 64) {
      const float* row = Ks + j * HP;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const fl4 k = *reinterpret_cast<const fl4*>(row + 4 * c);
        s += q[c][0] * k[0] + q[c][1] * k[1] + q[c][2] * k[2] + q[c][3] * k[3];
      }
      p[j] = s;
      m = fmaxf(m, s);
    }
    m = wave_max(m);
    // p[] is written per lane and read across lanes below without a barrier: LDS operations of one wave complete in order
    // (as in vit.hip's attn_fwd_kernel)
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float e = __expf(p[j] - m);
      p[j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    // o[lane] = sum_{j < n} p[j] V[j][lane]: two partial chains (even / odd quads), folded at the end, then a serial tail
    float a0 = 0.f, a1 = 0.f;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
      const fl4 p0 = *reinterpret_cast<const fl4*>(p + j), p1 = *reinterpret_cast<const fl4*>(p + j + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a0 += p0[e] * Vs[(j + e) * HP + lane];
        a1 += p1[e] * Vs[(j + 4 + e) * HP + lane];
      }
    }
    for (; j < n; ++j) a0 += p[j] * Vs[j * HP + lane];
    A[((long)b * L + i) * W + h * HD + lane] = (a0 + a1) / sum;
  }
}

}  // namespace

struct HEDIT_HANDLE hedit_text : ParamStore {
  hedit_text_cfg cfg;
  float *tok = nullptr, *pos = nullptr, *lnfg = nullptr, *lnfb = nullptr, *proj_w = nullptr;
  PConv proj;
  std::vector<EncBlock> blocks;
};

namespace {

int run(hedit_text* h, const int32_t* ids, int B, int L, float* hidden, const int32_t* pool_index, float* pooled, void* ws, size_t ws_bytes,
        hipStream_t st, bool dry, size_t* peak) {
  PF f = make_pf(B, ws, ws_bytes, st, dry);
  const int W = h->cfg.width, heads = h->cfg.heads, P = h->cfg.proj_dim;
  const long M = (long)B * L;
  const float ascale = 1.0f / sqrtf((float)HD);
  float* T;
  TRY(aalloc(f, &T, (size_t)M * W));
  if (!dry) { hipLaunchKernelGGL(embed_kernel, egrid(M * W), dim3(256), 0, st, ids, h->tok, h->pos, T, M, L, W, h->cfg.vocab_size); LAUNCH_CHECK(); }
  auto attn = [&](const float* qkv, const float* bias, float* A) -> int {
    hipLaunchKernelGGL(causal_attn_kernel, dim3(heads, B, attn_slices(heads, B)), dim3(256), attn_lds(L), st, qkv, bias, A, L, W, ascale);
    LAUNCH_CHECK();
    return HEDIT_OK;
  };
  for (const EncBlock& k : h->blocks) TRY(enc_block_forward(f, k, T, M, W, P_QGELU, LN_EPS, attn));
  if (hidden) TRY(ln(f, T, h->lnfg, h->lnfb, M, W, LN_EPS, hidden));
  if (pooled) {
    // the ln_final row at pool_index[b]: gathered before the LayerNorm (a per-row operation, so the bits are those of `hidden`)
    float *R, *N = nullptr, *out;
    TRY(aalloc(f, &R, (size_t)B * W));
    if (!dry) TRY(enc_gather_rows_launch(T, pool_index, R, B, L, W, st));
    if (P > 0) TRY(aalloc(f, &N, (size_t)B * W));
    TRY(ln(f, R, h->lnfg, h->lnfb, B, W, LN_EPS, P > 0 ? N : pooled));
    if (P > 0) {
      TRY(lin(f, N, W, P_COPY, nullptr, nullptr, h->proj, true, B, &out));      // one M = B GEMM: x @ text_projection
      if (!dry) HIP_TRY(hipMemcpyAsync(pooled, out, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, st));
      f.ar.free(out);
      f.ar.free(N);
    }
    f.ar.free(R);
  }
  f.ar.free(T);
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

}  // namespace

HEDIT_LIFECYCLE(text, hedit_text, "text encoder", no_pre_destroy)

extern "C" {

int hedit_text_create(const hedit_text_cfg* cfg, hedit_text** out) try {
  ARG_CHECK(cfg && out, "null");
  ARG_CHECK(cfg->width > 0 && cfg->layers > 0 && cfg->heads > 0 && cfg->vocab_size > 0 && cfg->context_length > 0 && cfg->proj_dim >= 0,
            "text: sizes must be positive (proj_dim may be 0)");
  ARG_CHECK(cfg->width % 64 == 0 && cfg->width / cfg->heads == 64 && cfg->width % cfg->heads == 0, "text: head dimension must be 64");
  ARG_CHECK(cfg->context_length <= LMAX, "text: context_length at most 200");
  ARG_CHECK(cfg->proj_dim % 4 == 0, "text: proj_dim must be a multiple of 4");
  TRY(gemm_prepare());
  hedit_text* h = new hedit_text();
  h->cfg = *cfg;
  const int W = cfg->width;
  h->tok = mat(h, "token_embedding.weight", cfg->vocab_size, W);       // stays fp32: it is only gathered
  h->pos = mat(h, "positional_embedding", cfg->context_length, W);
  for (int i = 0; i < cfg->layers; ++i)
    h->blocks.push_back(enc_add_block(h, "transformer.resblocks." + std::to_string(i), CLIP_BLOCK_NAMES, W));
  h->lnfg = vec(h, "ln_final.weight", W);
  h->lnfb = vec(h, "ln_final.bias", W);
  if (cfg->proj_dim > 0) h->proj_w = mat(h, "text_projection", W, cfg->proj_dim);
  return handle_created(h, out);
} catch (...) { return hedit_abi_catch(); }

int hedit_text_finalize(hedit_text* h, void* stream) try {
  ARG_CHECK(h, "null");
  TRY(handle_loaded(h));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int W = h->cfg.width;
  for (EncBlock& k : h->blocks) TRY(enc_pack_block(h, k, W, true, st));
  if (h->cfg.proj_dim > 0) TRY(pack_fwd(h, h->proj, h->proj_w, W, h->cfg.proj_dim, true, st));
  // the limit is remembered per (kernel, device), so it is set for the longest context any handle may have
  if (int rc = hedit_dyn_lds(reinterpret_cast<const void*>(&causal_attn_kernel), (int)attn_lds(LMAX))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (h->alloc_failed) { hedit_set_error("hipMalloc failed while packing the text encoder's weights"); return HEDIT_ERR_HIP; }
  h->finalized = true;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

size_t hedit_text_workspace_bytes(hedit_text* h, int B, int L) try {
  if (!h || B < 1 || L < 1 || L > h->cfg.context_length) return 0;
  size_t peak = 0;
  const int rc = run(h, nullptr, B, L, reinterpret_cast<float*>(4096), nullptr, reinterpret_cast<float*>(4096), nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* ids int32 [B][L] (device) -> hidden fp32 [B][L][width] after ln_final (or NULL); pooled fp32 [B][proj_dim ? proj_dim : width]
 * = the ln_final row at pool_index[b] (int32 [B], device), times text_projection when the model has one (or NULL).
 * Every argument is checked before the first launch. */
int hedit_text_encode(hedit_text* h, const int32_t* ids, int B, int L, float* hidden, const int32_t* pool_index, float* pooled,
                      void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && ids, "text_encode: null");
  ARG_CHECK(B >= 1, "text_encode: B >= 1");
  ARG_CHECK(L >= 1 && L <= h->cfg.context_length, "text_encode: 1 <= L <= context_length");
  ARG_CHECK(hidden || pooled, "text_encode: nothing to write (hidden and pooled are both null)");
  ARG_CHECK(!pooled || pool_index, "text_encode: pooled needs pool_index");
  ARG_CHECK(workspace, "text_encode: null workspace");
  TRY(handle_finalized(h));
  size_t need = 0;
  TRY(run(h, nullptr, B, L, hidden, pool_index, pooled, nullptr, 0, nullptr, true, &need));
  TRY(ws_check("text_encode", need, workspace_bytes));
  return run(h, ids, B, L, hidden, pool_index, pooled, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
