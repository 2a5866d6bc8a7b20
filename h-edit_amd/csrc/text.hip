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
// The small kernels vit.hip also has (LayerNorm forward, out = res + raw + bias, the LDS row helpers) are restated here
// without the backward pass's by-products (statistics, log-sum-exp) rather than shared: vit.hip is not touched.
#include "pnet.h"

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
// R[b] = T[b][clamp(idx[b])]
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ T, const int32_t* __restrict__ idx, float* __restrict__ R,
                                                          int B, int L, int W) {
  const long total = (long)B * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int w = (int)(i % W), b = (int)(i / W);
    int l = idx[b];
    l = l < 0 ? 0 : (l >= L ? L - 1 : l);
    R[i] = T[((long)b * L + l) * W + w];
  }
}
// LayerNorm over W, one wave per row (the arithmetic of vit.hip's ln_fwd_kernel; no statistics are kept)
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                 float* __restrict__ y, long rows, int W) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * W;
  float s = 0.f;
  for (int i = lane; i < W; i += 64) s += xr[i];
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
  for (int i = lane; i < W; i += 64) { const float d = xr[i] - mean; q += d * d; }
  const float rstd = rsqrtf(wave_sum(q) / (float)W + LN_EPS);
  for (int i = lane; i < W; i += 64) y[row * W + i] = (xr[i] - mean) * rstd * g[i] + b[i];
}
// out = res + raw + bias
__global__ __launch_bounds__(256) void add_bias_res_kernel(const float* __restrict__ raw, const float* __restrict__ bias, const float* __restrict__ res,
                                                           float* __restrict__ out, long total, int W) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) out[i] = res[i] + raw[i] + bias[i % W];
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

struct TBlock {
  float *ln1g, *ln1b, *ln2g, *ln2b, *win, *bin, *wo, *bo, *wfc, *bfc, *wp, *bp;
  PConv in, out, fc, proj;
};

inline dim3 egrid(long total) { return dim3(ew_grid(total)); }

// forward-only packed weight of out = x . w^T, w [O][I] (make_pconv of pnet.h also builds the input-gradient twin, which
// nothing here would read: 0.5 GB at SD size).  transposed: w is [O][I] and the product is x [M][O] . w -> [M][I].
int pack_fwd(ParamStore* h, PConv& c, const float* w, int O, int I, bool transposed, hipStream_t st) {
  c.O = O; c.I = I; c.k = 1;
  c.rows_f = (O + 3) / 4 * 4;
  c.rows_b = (I + 3) / 4 * 4;
  bf16_t*& dst = transposed ? c.wb : c.wf;
  const int rows = transposed ? c.rows_b : c.rows_f, Cin = transposed ? O : I;
  if (!dst) dst = dalloc<bf16_t>(h, (size_t)rows * split_kp(Cin));
  if (!dst) { hedit_set_error("hipMalloc failed for a packed weight"); return HEDIT_ERR_HIP; }
  return pack_split3_w_launch(w, nullptr, dst, O, I, 1, transposed ? 1 : 0, split_cs(Cin), split_kp(Cin), rows, 0, 0, st);
}

}  // namespace

struct hedit_text : ParamStore {
  hedit_text_cfg cfg;
  float *tok = nullptr, *pos = nullptr, *lnfg = nullptr, *lnfb = nullptr, *proj_w = nullptr;
  PConv proj;
  std::vector<TBlock> blocks;
  bool finalized = false;
};

namespace {

int ln(PF& f, const float* x, const float* g, const float* b, long rows, int W, float* y) {
  if (!f.dry()) {
    hipLaunchKernelGGL(ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, f.st, x, g, b, y, rows, W);
    LAUNCH_CHECK();
  }
  return HEDIT_OK;
}

// the M rows of a [M][C] fp32 tensor as a split operand and through one linear layer: out raw [M][N]
int lin(PF& f, const float* x, int C, int op, const float* q, const PConv& c, bool transposed, long M, float** out) {
  bf16_t* A;
  TRY(op_split(f, x, C, op, nullptr, q, 0, nullptr, 0, 1, 1, M, &A));
  TRY(pgemm(f, A, c, transposed, 0, 1, 1, M, out));
  f.ar.free(A);
  return HEDIT_OK;
}

int run(hedit_text* h, const int32_t* ids, int B, int L, float* hidden, const int32_t* pool_index, float* pooled, void* ws, size_t ws_bytes,
        hipStream_t st, bool dry, size_t* peak) {
  PF f{B, st, Arena{}};
  f.ar.dry = dry;
  f.ar.base = reinterpret_cast<char*>(ws);
  f.ar.cap = ws_bytes;
  const int W = h->cfg.width, heads = h->cfg.heads, P = h->cfg.proj_dim;
  const long M = (long)B * L;
  const float ascale = 1.0f / sqrtf((float)HD);
  float* T;
  TRY(palloc(f, &T, (size_t)M * W));
  if (!dry) { hipLaunchKernelGGL(embed_kernel, egrid(M * W), dim3(256), 0, st, ids, h->tok, h->pos, T, M, L, W, h->cfg.vocab_size); LAUNCH_CHECK(); }
  for (const TBlock& k : h->blocks) {
    float *a, *qkv, *A, *raw, *Tmid, *m, *H, *Tn;
    TRY(palloc(f, &a, (size_t)M * W));
    TRY(ln(f, T, k.ln1g, k.ln1b, M, W, a));
    TRY(lin(f, a, W, P_COPY, nullptr, k.in, false, M, &qkv));
    f.ar.free(a);
    TRY(palloc(f, &A, (size_t)M * W));
    if (!dry) {
      hipLaunchKernelGGL(causal_attn_kernel, dim3(heads, B, attn_slices(heads, B)), dim3(256), attn_lds(L), st, qkv, k.bin, A, L, W, ascale);
      LAUNCH_CHECK();
    }
    f.ar.free(qkv);
    TRY(lin(f, A, W, P_COPY, nullptr, k.out, false, M, &raw));
    f.ar.free(A);
    TRY(palloc(f, &Tmid, (size_t)M * W));
    if (!dry) { hipLaunchKernelGGL(add_bias_res_kernel, egrid(M * W), dim3(256), 0, st, raw, k.bo, T, Tmid, M * W, W); LAUNCH_CHECK(); }
    f.ar.free(raw);
    f.ar.free(T);
    TRY(palloc(f, &m, (size_t)M * W));
    TRY(ln(f, Tmid, k.ln2g, k.ln2b, M, W, m));
    TRY(lin(f, m, W, P_COPY, nullptr, k.fc, false, M, &H));
    f.ar.free(m);
    TRY(lin(f, H, 4 * W, P_QGELU, k.bfc, k.proj, false, M, &raw));      // QuickGELU(H + bias) as the operand op
    f.ar.free(H);
    TRY(palloc(f, &Tn, (size_t)M * W));
    if (!dry) { hipLaunchKernelGGL(add_bias_res_kernel, egrid(M * W), dim3(256), 0, st, raw, k.bp, Tmid, Tn, M * W, W); LAUNCH_CHECK(); }
    f.ar.free(raw);
    f.ar.free(Tmid);
    T = Tn;
  }
  if (hidden) TRY(ln(f, T, h->lnfg, h->lnfb, M, W, hidden));
  if (pooled) {
    // the ln_final row at pool_index[b]: gathered before the LayerNorm (a per-row operation, so the bits are those of `hidden`)
    float *R, *N = nullptr, *out;
    TRY(palloc(f, &R, (size_t)B * W));
    if (!dry) { hipLaunchKernelGGL(gather_rows_kernel, egrid((long)B * W), dim3(256), 0, st, T, pool_index, R, B, L, W); LAUNCH_CHECK(); }
    if (P > 0) TRY(palloc(f, &N, (size_t)B * W));
    TRY(ln(f, R, h->lnfg, h->lnfb, B, W, P > 0 ? N : pooled));
    if (P > 0) {
      TRY(lin(f, N, W, P_COPY, nullptr, h->proj, true, B, &out));      // one M = B GEMM: x @ text_projection
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
  auto mat = [&](const std::string& name, int O, int I) {
    float* d = dalloc<float>(h, (size_t)O * I);
    add_slot(h, name, 0, d, (size_t)O * I, O, I, 2, O, I, 1, 1);
    return d;
  };
  h->tok = mat("token_embedding.weight", cfg->vocab_size, W);       // stays fp32: it is only gathered
  h->pos = mat("positional_embedding", cfg->context_length, W);
  for (int i = 0; i < cfg->layers; ++i) {
    const std::string pre = "transformer.resblocks." + std::to_string(i);
    TBlock k{};
    k.ln1g = vec(h, pre + ".ln_1.weight", W); k.ln1b = vec(h, pre + ".ln_1.bias", W);
    k.win = mat(pre + ".attn.in_proj_weight", 3 * W, W); k.bin = vec(h, pre + ".attn.in_proj_bias", 3 * W);
    k.wo = mat(pre + ".attn.out_proj.weight", W, W); k.bo = vec(h, pre + ".attn.out_proj.bias", W);
    k.ln2g = vec(h, pre + ".ln_2.weight", W); k.ln2b = vec(h, pre + ".ln_2.bias", W);
    k.wfc = mat(pre + ".mlp.c_fc.weight", 4 * W, W); k.bfc = vec(h, pre + ".mlp.c_fc.bias", 4 * W);
    k.wp = mat(pre + ".mlp.c_proj.weight", W, 4 * W); k.bp = vec(h, pre + ".mlp.c_proj.bias", W);
    h->blocks.push_back(k);
  }
  h->lnfg = vec(h, "ln_final.weight", W);
  h->lnfb = vec(h, "ln_final.bias", W);
  if (cfg->proj_dim > 0) h->proj_w = mat("text_projection", W, cfg->proj_dim);
  if (h->alloc_failed) {
    hedit_set_error("hipMalloc failed while creating the text encoder");
    store_free(h);
    delete h;
    return HEDIT_ERR_HIP;
  }
  *out = h;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

void hedit_text_destroy(hedit_text* h) try {
  if (!h) return;
  store_free(h);
  delete h;
} catch (...) { (void)hedit_abi_catch(); }

int hedit_text_num_params(const hedit_text* h) { return h ? (int)h->slots.size() : 0; }
const char* hedit_text_param_name(const hedit_text* h, int i) try {
  if (!h || i < 0 || i >= (int)h->slots.size()) return nullptr;
  return h->slots[i].name.c_str();
} catch (...) { (void)hedit_abi_catch(); return nullptr; }
int hedit_text_param_shape(const hedit_text* h, int i, int* ndim, int* dims4) try {
  ARG_CHECK(h && ndim && dims4 && i >= 0 && i < (int)h->slots.size(), "param index");
  *ndim = h->slots[i].ndim;
  for (int k = 0; k < 4; ++k) dims4[k] = h->slots[i].dims[k];
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }
int hedit_text_load(hedit_text* h, const char* name, const float* w, size_t numel, void* stream) try {
  ARG_CHECK(h && name && w, "null");
  h->finalized = false;
  return store_load(h, "text encoder", name, w, numel, reinterpret_cast<hipStream_t>(stream));
} catch (...) { return hedit_abi_catch(); }
int hedit_text_missing(const hedit_text* h) { return h ? store_missing(h) : -1; }

int hedit_text_finalize(hedit_text* h, void* stream) try {
  ARG_CHECK(h, "null");
  if (store_missing(h) != 0) {
    hedit_set_error("text encoder has " + std::to_string(store_missing(h)) + " unloaded parameters");
    return HEDIT_ERR_STATE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int W = h->cfg.width;
  for (TBlock& k : h->blocks) {
    TRY(pack_fwd(h, k.in, k.win, 3 * W, W, false, st));
    TRY(pack_fwd(h, k.out, k.wo, W, W, false, st));
    TRY(pack_fwd(h, k.fc, k.wfc, 4 * W, W, false, st));
    TRY(pack_fwd(h, k.proj, k.wp, W, 4 * W, false, st));
  }
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
  if (run(h, nullptr, B, L, reinterpret_cast<float*>(4096), nullptr, reinterpret_cast<float*>(4096), nullptr, 0, nullptr, true, &peak) != HEDIT_OK)
    return 0;
  return peak + 4096;
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
  if (!h->finalized) { hedit_set_error("call hedit_text_finalize after loading the parameters"); return HEDIT_ERR_STATE; }
  size_t need = 0;
  TRY(run(h, nullptr, B, L, hidden, pool_index, pooled, nullptr, 0, nullptr, true, &need));
  if (workspace_bytes < need) {
    hedit_set_error("bad argument: text_encode: workspace too small (need " + std::to_string(need) + " bytes, got " +
                    std::to_string(workspace_bytes) + ")");
    return HEDIT_ERR_ARG;
  }
  return run(h, ids, B, L, hidden, pool_index, pooled, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
