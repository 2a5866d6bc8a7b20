// The SD-1.x eps-network as a native executor: owns the packed bf16 weights, plans activation
// memory inside a caller-provided workspace (first-fit arena, stream-ordered reuse) and walks the
// network issuing the HIP kernels of gemm.hip / norm.hip / attn.hip on one stream.  One C call
// per UNet evaluation replaces the ~700 eager launches of the reference stack.
//
// Architecture = diffusers' UNet2DConditionModel as used by SD-1.4/1.5;
// parameter names are the diffusers state_dict keys so real checkpoints load unchanged.
#include <array>
#include <map>
#include <string>
#include <vector>

#include "exec.h"
#include "kernels.h"
#include "store.h"

namespace {

struct Res {
  int cin, cout, temb_off;
  float *n1g, *n1b, *n2g, *n2b, *conv2_b, *sc_b;
  bf16_t *conv1, *conv2, *sc_w;
  bf16_t *conv1_t = nullptr, *conv2_t = nullptr, *sc_t = nullptr;   // input-gradient weights (hedit_unet_create_grad)
};

struct Attn {
  int C;
  float *gn_g, *gn_b, *pin_b, *ln1g, *ln1b, *ln2g, *ln2b, *ln3g, *ln3b, *o1_b, *o2_b, *ff1_b, *ff2_b, *pout_b;
  bf16_t *pin, *w_qk, *w_v1, *w_o1, *w_q2, *w_k2, *w_v2, *w_o2, *ff1, *ff2, *pout;
  // C == ffn_fused_channels(): the token-local layers run as three chain kernels (linchain.hip x 2, ffn.hip) on these weight streams
  // (+ the packed FF1 bias); pin / w_qk / w_v1 / w_o1 / w_q2 / w_o2 / ff1 / ff2 / ff1_b / pout are then not materialised
  bf16_t *frs = nullptr, *k1s = nullptr, *ffs = nullptr;
  float* ff1_bp = nullptr;
  int ctx_off = 0;      // first row of this block's attn2.to_k / to_v in the UNet-wide matrices (hedit_unet::wk2_all / wv2_all)
  // hedit_unet_create_grad: transposed weights ([I][O]; the two queries with their scale), FF1 in the checkpoint's row order
  // (value rows, then gate rows) with its bias -- the taped forward keeps the FF1 pre-activation --, and at the chain width
  // the unfused forward weights above as well
  bf16_t *pin_t = nullptr, *wq1_t = nullptr, *wk1_t = nullptr, *wv1_t = nullptr, *wo1_t = nullptr, *wq2_t = nullptr, *wo2_t = nullptr,
         *ff1_t = nullptr, *ff2_t = nullptr, *pout_t = nullptr, *ff1n = nullptr;
  float* ff1_bn = nullptr;
};

struct Block {
  std::vector<Res> res;
  std::vector<Attn> attn;
  bool has_attn = false, has_sampler = false;
  bf16_t* samp_w = nullptr;
  bf16_t* samp_t = nullptr;     // input-gradient weight of the sampler: down [I][9][O] taps in place, up taps flipped
  float* samp_b = nullptr;
  int ch = 0;
};

}  // namespace

struct HEDIT_HANDLE hedit_unet : ParamStore {
  hedit_unet_cfg cfg;
  int temb_dim = 0, temb_total = 0;
  // stem / head
  float *conv_in_w = nullptr, *conv_in_b = nullptr, *te1_b = nullptr, *te2_b = nullptr;
  bf16_t *te1_w = nullptr, *te2_w = nullptr, *temb_w_all = nullptr, *conv_out_w = nullptr;
  float *temb_b_all = nullptr, *conv1_b_all = nullptr, *gn_out_g = nullptr, *gn_out_b = nullptr, *conv_out_b = nullptr;
  std::vector<Block> down, up;
  Res mid_res[2];
  Attn mid_attn;
  int32_t* iota = nullptr;
  int iota_cap = 0;
  // sampled launch timing (bench.py roofline): HIP event pairs on the launch stream
  bool prof_on = false;
  std::vector<hipEvent_t> prof_pool;
  struct ProfRec { int kind; double flops, bytes; int e0, e1; int m = 0, n = 0, k = 0, tag = 0; };
  std::vector<ProfRec> prof_recs;
  size_t prof_next = 0;
  // host-language attention controller (hedit_unet_set_attn_hook): when set, every attention layer materialises its
  // probabilities, hands them to the hook and multiplies whatever comes back with V (attn.hip, slow path)
  hedit_attn_hook_fn hook = nullptr;
  void* hook_user = nullptr;
  // attn2.to_k / attn2.to_v of EVERY transformer block, stacked along the output channels: the context projections depend
  // on the prompt only, so one forward computes them for all blocks in two launches ([B*80][ctx_n] and its transpose form)
  // instead of two small launches per block (32 per call on SD-1.x)
  bf16_t *wk2_all = nullptr, *wv2_all = nullptr;
  int ctx_n = 0, ctx_next = 0;
  // hedit_unet_workspace_bytes by (B, height, width, hook set): the answer covers every row map, i.e. one dry run per
  // number of distinct latents, so it is worked out once per shape
  std::map<std::array<int, 4>, size_t> ws_cache;
  // hedit_unet_create_grad only: input-gradient twins of the head / tail convolutions, a zero bias vector, and the
  // outstanding tape of hedit_unet_forward_keep (a GradTape, unetgrad.h)
  bool grad = false;
  bf16_t* conv_in_t = nullptr;
  float *conv_out_t = nullptr, *zero_bias = nullptr;
  void* tape = nullptr;
  void (*tape_free)(void*) = nullptr;
  // hedit_unet_create_grad_ctx only: [wk2_all | wv2_all]^T as [cross_attention_dim][2 * ctx_n] -- block b's to_k^T at columns
  // ctx_off .., its to_v^T at ctx_n + ctx_off .. -- the weight of the one GEMM that turns every dK / dV into d_ctx
  bf16_t* wkv2_t = nullptr;
};

namespace {

// grad handle: the linear slot just added also fills its transposed twin *t and, where the forward-only handle keeps the
// weight in a chain stream only (fwd != nullptr), the unfused forward copy *fwd (allocated here unless it is set)
void grad_lin(hedit_unet* h, int O, int I, float scale, bf16_t** t, bf16_t** fwd = nullptr) {
  if (!h->grad) return;
  *t = twin<bf16_t>(h, Pack::LinearT, (size_t)O * I, nullptr, scale);
  if (fwd) *fwd = twin<bf16_t>(h, Pack::Linear, (size_t)O * I, *fwd, scale);
}

Res make_res(hedit_unet* h, const std::string& pre, int cin, int cout, int& temb_off) {
  Res r{};
  r.cin = cin; r.cout = cout; r.temb_off = temb_off;
  r.n1g = vec(h, pre + ".norm1.weight", cin);
  r.n1b = vec(h, pre + ".norm1.bias", cin);
  r.conv1 = conv3(h, pre + ".conv1.weight", cout, cin);
  if (h->grad) r.conv1_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)cout * cin * 9);
  vec(h, pre + ".conv1.bias", cout, h->conv1_b_all + temb_off);
  lin(h, pre + ".time_emb_proj.weight", cout, h->temb_dim, false, h->temb_w_all + (size_t)temb_off * h->temb_dim);
  vec(h, pre + ".time_emb_proj.bias", cout, h->temb_b_all + temb_off);
  r.n2g = vec(h, pre + ".norm2.weight", cout);
  r.n2b = vec(h, pre + ".norm2.bias", cout);
  r.conv2 = conv3(h, pre + ".conv2.weight", cout, cout);
  if (h->grad) r.conv2_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)cout * cout * 9);
  r.conv2_b = vec(h, pre + ".conv2.bias", cout);
  if (cin != cout) {
    r.sc_w = lin(h, pre + ".conv_shortcut.weight", cout, cin, true);
    grad_lin(h, cout, cin, 1.f, &r.sc_t);
    r.sc_b = vec(h, pre + ".conv_shortcut.bias", cout);
  }
  temb_off += cout;
  return r;
}

Attn make_attn(hedit_unet* h, const std::string& pre, int C) {
  Attn a{};
  a.C = C;
  const int ctx = h->cfg.cross_attention_dim;
  const int d = C / h->cfg.heads;
  const float qscale = 1.0f / sqrtf((float)d) * 1.4426950408889634f;   // softmax scale * log2(e)
  a.gn_g = vec(h, pre + ".norm.weight", C);
  a.gn_b = vec(h, pre + ".norm.bias", C);
  // At the level ffn.hip / linchain.hip exist for, the token-local layers of the block run as three kernels -- GroupNorm apply +
  // proj_in + norm1 + q | k | v^T;  attn1.to_out + residual + norm2 + attn2.to_q;  attn2.to_out + residual + norm3 +
  // feed-forward + proj_out + residual -- and their weights go into those kernels' streams (Pack::ChainLayer / FfnLayer), the FF1
  // bias into its packed form (Pack::FfnBias); none of them is kept as a GEMM operand.
  const bool chain = C == ffn_fused_channels();
  auto stream_slot = [&](const std::string& name, bf16_t* stream, int lay, int which, int O, int I, float scale, int ndim) {
    PackDst& d = add_slot(h, name, lay ? Pack::ChainLayer : Pack::FfnLayer, stream, (size_t)O * I, O, I, ndim, O, I, 1, 1).to;
    d.scale = scale; d.which = which; d.lay = lay;
  };
  const std::string tb = pre + ".transformer_blocks.0";
  if (chain) {
    a.frs = dalloc<bf16_t>(h, lin_chain_stream_bytes(4) / sizeof(bf16_t));
    a.k1s = dalloc<bf16_t>(h, lin_chain_stream_bytes(2) / sizeof(bf16_t));
    a.ffs = dalloc<bf16_t>(h, ffn_stream_bytes(1, 1) / sizeof(bf16_t));
    a.ff1_bp = dalloc<float>(h, ffn_bias_bytes() / sizeof(float));
    stream_slot(pre + ".proj_in.weight", a.frs, 4, 0, C, C, 1.f, 4);
  } else {
    a.pin = lin(h, pre + ".proj_in.weight", C, C, true);
  }
  grad_lin(h, C, C, 1.f, &a.pin_t, chain ? &a.pin : nullptr);
  a.pin_b = vec(h, pre + ".proj_in.bias", C);
  a.ln1g = vec(h, tb + ".norm1.weight", C);
  a.ln1b = vec(h, tb + ".norm1.bias", C);
  if (chain) {
    bf16_t *wq = nullptr, *wk = nullptr;
    if (h->grad) {
      a.w_qk = dalloc<bf16_t>(h, (size_t)2 * C * C);
      wq = a.w_qk;
      wk = a.w_qk ? a.w_qk + (size_t)C * C : nullptr;
    }
    stream_slot(tb + ".attn1.to_q.weight", a.frs, 4, 1, C, C, qscale, 2);
    grad_lin(h, C, C, qscale, &a.wq1_t, &wq);
    stream_slot(tb + ".attn1.to_k.weight", a.frs, 4, 2, C, C, 1.f, 2);
    grad_lin(h, C, C, 1.f, &a.wk1_t, &wk);
    stream_slot(tb + ".attn1.to_v.weight", a.frs, 4, 3, C, C, 1.f, 2);
    grad_lin(h, C, C, 1.f, &a.wv1_t, &a.w_v1);
    stream_slot(tb + ".attn1.to_out.0.weight", a.k1s, 2, 0, C, C, 1.f, 2);
    grad_lin(h, C, C, 1.f, &a.wo1_t, &a.w_o1);
  } else {
    a.w_qk = dalloc<bf16_t>(h, (size_t)2 * C * C);
    lin(h, tb + ".attn1.to_q.weight", C, C, false, a.w_qk, qscale);
    grad_lin(h, C, C, qscale, &a.wq1_t);
    lin(h, tb + ".attn1.to_k.weight", C, C, false, a.w_qk + (size_t)C * C);
    grad_lin(h, C, C, 1.f, &a.wk1_t);
    a.w_v1 = lin(h, tb + ".attn1.to_v.weight", C, C);
    grad_lin(h, C, C, 1.f, &a.wv1_t);
    a.w_o1 = lin(h, tb + ".attn1.to_out.0.weight", C, C);
    grad_lin(h, C, C, 1.f, &a.wo1_t);
  }
  a.o1_b = vec(h, tb + ".attn1.to_out.0.bias", C);
  a.ln2g = vec(h, tb + ".norm2.weight", C);
  a.ln2b = vec(h, tb + ".norm2.bias", C);
  if (chain) stream_slot(tb + ".attn2.to_q.weight", a.k1s, 2, 1, C, C, qscale, 2);
  else a.w_q2 = lin(h, tb + ".attn2.to_q.weight", C, C, false, nullptr, qscale);
  grad_lin(h, C, C, qscale, &a.wq2_t, chain ? &a.w_q2 : nullptr);
  a.ctx_off = h->ctx_next;
  h->ctx_next += C;
  a.w_k2 = lin(h, tb + ".attn2.to_k.weight", C, ctx, false, h->wk2_all + (size_t)a.ctx_off * ctx);
  if (h->wkv2_t) twin<bf16_t>(h, Pack::LinearT, (size_t)C * ctx, h->wkv2_t + a.ctx_off, 1.f, 2L * h->ctx_n);
  a.w_v2 = lin(h, tb + ".attn2.to_v.weight", C, ctx, false, h->wv2_all + (size_t)a.ctx_off * ctx);
  if (h->wkv2_t) twin<bf16_t>(h, Pack::LinearT, (size_t)C * ctx, h->wkv2_t + h->ctx_n + a.ctx_off, 1.f, 2L * h->ctx_n);
  if (chain) {
    stream_slot(tb + ".attn2.to_out.0.weight", a.ffs, 0, 0, C, C, 1.f, 2);
  } else {
    a.w_o2 = lin(h, tb + ".attn2.to_out.0.weight", C, C);
  }
  grad_lin(h, C, C, 1.f, &a.wo2_t, chain ? &a.w_o2 : nullptr);
  a.o2_b = vec(h, tb + ".attn2.to_out.0.bias", C);
  a.ln3g = vec(h, tb + ".norm3.weight", C);
  a.ln3b = vec(h, tb + ".norm3.bias", C);
  if (chain) {
    stream_slot(tb + ".ff.net.0.proj.weight", a.ffs, 0, 1, 8 * C, C, 1.f, 2);
    grad_lin(h, 8 * C, C, 1.f, &a.ff1_t, &a.ff1n);
    add_slot(h, tb + ".ff.net.0.proj.bias", Pack::FfnBias, a.ff1_bp, (size_t)8 * C, 0, 0, 1, 8 * C, 1, 1, 1);
    if (h->grad) a.ff1_bn = twin<float>(h, Pack::F32, (size_t)8 * C);
    stream_slot(tb + ".ff.net.2.weight", a.ffs, 0, 2, C, 4 * C, 1.f, 2);
    grad_lin(h, C, 4 * C, 1.f, &a.ff2_t, &a.ff2);
  } else {
    a.ff1 = lin(h, tb + ".ff.net.0.proj.weight", 8 * C, C);
    h->slots.back().to.kind = Pack::GegluRows;
    grad_lin(h, 8 * C, C, 1.f, &a.ff1_t, &a.ff1n);
    a.ff1_b = vec(h, tb + ".ff.net.0.proj.bias", 8 * C);
    h->slots.back().to.kind = Pack::GegluBias;
    if (h->grad) a.ff1_bn = twin<float>(h, Pack::F32, (size_t)8 * C);
    a.ff2 = lin(h, tb + ".ff.net.2.weight", C, 4 * C);
    grad_lin(h, C, 4 * C, 1.f, &a.ff2_t);
  }
  a.ff2_b = vec(h, tb + ".ff.net.2.bias", C);
  if (chain) {
    stream_slot(pre + ".proj_out.weight", a.ffs, 0, 3, C, C, 1.f, 4);
  } else {
    a.pout = lin(h, pre + ".proj_out.weight", C, C, true);
  }
  grad_lin(h, C, C, 1.f, &a.pout_t, chain ? &a.pout : nullptr);
  a.pout_b = vec(h, pre + ".proj_out.bias", C);
  return a;
}

// ------------------------------------------------------------------------------ forward
struct Fwd {
  hedit_unet* h;
  int B;
  hipStream_t st;
  Arena ar;
  const hedit_p2p_plan* plan;
  const float* temb_all;     // fused (time_emb_proj(silu(temb)) + conv1.bias) of every ResBlock
  const bf16_t* ctxb;        // [B*80][ctx_dim]
  const bf16_t* k2_all = nullptr;    // [B*80][ctx_n]: attn2 keys of every block (columns ctx_off .. ctx_off + C)
  const bf16_t* vt2_all = nullptr;   // [ctx_n][B*80]: attn2 values, transposed
  int store_idx = 0;
  int store_self_idx = 0;
  int tblock = 0;            // transformer blocks visited so far in this call (MasaCtrl / PnP layer gates)
  int rblock = 0;            // ResNet blocks visited so far (PnP feature injection)
  int place = 0;             // 0 down, 1 mid, 2 up: where the transformer block being executed sits (the hook's argument)
  int hook_layer = 0;        // attention layers handed to the hook so far in this call
  int masa_count = 0;        // plan.masa_auto: 256-token cross-attention layers folded into the accumulator so far in this call
  int masa_layer = 0;        // plan.masa_auto: self-attention layers under kv_src so far (index into h_masa_dump)
  const RowMap* map = nullptr;   // hedit_unet_forward_shared: batch row -> distinct latent (null in a dry run)
  bool dry() const { return ar.dry; }
};

// The rows of one latent stay identical until the first cross-attention, so that part runs once per DISTINCT latent: the
// helpers take the batch from f.B, which this guard sets for a scope -- on the one Fwd, whose arena goes on.
struct BatchScope {
  Fwd& f;
  int saved;
  BatchScope(Fwd& f_, int rows) : f(f_), saved(f_.B) { f.B = rows; }
  ~BatchScope() { f.B = saved; }
  BatchScope(const BatchScope&) = delete;
  BatchScope& operator=(const BatchScope&) = delete;
};

// kernel classes of the sampled profiler
enum { PK_CONV = 0, PK_LINEAR = 1, PK_SELF_ATTN = 2, PK_CROSS_ATTN = 3, PK_NORM = 4, PK_OTHER = 5, PK_COUNT = 6 };

struct ProfScope {
  hedit_unet* h;
  hipStream_t st;
  int rec = -1;
  ProfScope(Fwd& f, int kind, double flops, double bytes = 0.0);
  ~ProfScope() {
    if (rec >= 0) (void)hipEventRecord(h->prof_pool[h->prof_recs[rec].e1], st);
  }
};

// bytes = ALGORITHMIC HBM bytes of the launch(es) in the scope: every operand read once, every result written once
ProfScope::ProfScope(Fwd& f, int kind, double flops, double bytes) : h(f.h), st(f.st) {
  if (f.dry() || !h->prof_on || h->prof_next + 2 > h->prof_pool.size()) return;
  hedit_unet::ProfRec r;
  r.kind = kind; r.flops = flops; r.bytes = bytes; r.e0 = (int)h->prof_next; r.e1 = (int)h->prof_next + 1;
  h->prof_next += 2;
  h->prof_recs.push_back(r);
  rec = (int)h->prof_recs.size() - 1;
  (void)hipEventRecord(h->prof_pool[r.e0], st);
}

// batch_in: which extent of the GEMM carries the batch (1 = M, 2 = N, 0 = neither).  The K-chunking is taken from
// the per-image extent times a fixed nominal batch, so the summation order of a layer is a property of the
// layer, not of the launch (see gemm_canonical_chunk).
// unique operand bytes + result bytes of one GEMM launch (bf16 operands; conv: the input image once, not nine times)
double gemm_alg_bytes(const Fwd& f, const GemmParams& p) {
  const double a = p.mode == 0 ? (double)p.M * p.K : (double)f.B * p.Hin * p.Win * p.Cin;
  const double c = p.raw_f32 ? 4.0 * p.M * p.N : 2.0 * p.M * (p.geglu ? p.N / 2 : p.N);
  return 2.0 * a + 2.0 * (double)p.N * p.K + c + (p.residual ? 2.0 * p.M * p.N : 0.0);
}

int run_gemm(Fwd& f, GemmParams p, int batch_in = 1) {
  if (!p.raw_f32 && !p.geglu) {
    const int mn = batch_in == 1 ? p.M / f.B * GEMM_NOMINAL_BATCH : p.M;
    const int nn = batch_in == 2 ? p.N / f.B * GEMM_NOMINAL_BATCH : p.N;
    p.chunk_kt = gemm_canonical_chunk(mn, nn, p.K);
  }
  const int splits = gemm_plan_splits(p.M, p.N, p.K, p.chunk_kt);
  float* part = nullptr;
  if (splits > 1) TRY(aalloc(f, &part, (size_t)splits * p.M * p.N));
  {
    ProfScope ps(f, p.mode == 0 ? PK_LINEAR : PK_CONV, 2.0 * p.M * p.N * p.K, gemm_alg_bytes(f, p));
    if (ps.rec >= 0) {
      auto& r = f.h->prof_recs[ps.rec];
      r.m = p.M; r.n = p.N; r.k = p.K;
      r.tag = p.mode | (p.geglu ? 8 : 0) | (p.residual ? 16 : 0) | (splits > 1 ? 32 : 0) | (p.chunk_kt ? 64 : 0);
    }
    RUN(f, gemm_launch(p, splits, part, f.st));
  }
  if (part) f.ar.free(part);
  return HEDIT_OK;
}

int linear(Fwd& f, const bf16_t* A, int M, int K, const bf16_t* W, int N, const float* bias,
           const bf16_t* residual, bf16_t* C, int ldc, int batch_in = 1) {
  GemmParams p{};
  p.A = A; p.W = W; p.M = M; p.N = N; p.K = K; p.lda = K; p.mode = 0;
  p.bias = bias; p.residual = residual; p.ldr = N; p.C = C; p.ldc = ldc;
  return run_gemm(f, p, batch_in);
}

// C = A W^T + bias (+ residual), then y = LayerNorm(C).  Behind a split-K launch (small batches) the reduce pass
// normalises too; otherwise the LayerNorm is its own launch, as before -- the same bits either way (kernels.h).
int linear_ln(Fwd& f, const bf16_t* A, int M, int K, const bf16_t* W, int N, const float* bias, const bf16_t* residual, bf16_t* C,
              const float* g, const float* b, float eps, bf16_t* y) {
  GemmParams p{};
  p.A = A; p.W = W; p.M = M; p.N = N; p.K = K; p.lda = K; p.mode = 0;
  p.bias = bias; p.residual = residual; p.ldr = N; p.C = C; p.ldc = N;
  int done = 0;
  p.ln_gamma = g; p.ln_beta = b; p.ln_out = y; p.ln_eps = eps; p.ln_done = &done;
  TRY(run_gemm(f, p));
  if (!done) {
    ProfScope ps(f, PK_NORM, 0.0, 4.0 * M * N);
    RUN(f, layernorm_launch(C, y, g, b, (long)M, N, eps, f.st));
  }
  return HEDIT_OK;
}

int conv3x3(Fwd& f, const bf16_t* X, int Hin, int Win, int Cin, const bf16_t* W, int Cout, const float* bias,
            const bf16_t* residual, bf16_t* Y, int mode, int ldy = 0) {
  GemmParams p{};
  p.mode = mode;
  p.Hin = Hin; p.Win = Win; p.Cin = Cin;
  p.Hout = mode == 2 ? Hin / 2 : (mode == 3 ? Hin * 2 : Hin);
  p.Wout = mode == 2 ? Win / 2 : (mode == 3 ? Win * 2 : Win);
  p.A = X; p.W = W; p.M = f.B * p.Hout * p.Wout; p.N = Cout; p.K = 9 * Cin; p.lda = Cin;
  p.bias = bias; p.residual = residual; p.ldr = Cout; p.C = Y; p.ldc = ldy ? ldy : Cout;
  return run_gemm(f, p);
}

int groupnorm(Fwd& f, const bf16_t* x, bf16_t* y, const float* g, const float* b, int HW, int C, float eps, int silu) {
  float* ws;
  TRY(aalloc(f, &ws, groupnorm_ws_bytes(f.B, HW, C) / sizeof(float)));
  {
    ProfScope ps(f, PK_NORM, 0.0, 6.0 * f.B * (double)HW * C);
    RUN(f, groupnorm_launch(x, y, g, b, f.B, HW, C, f.h->cfg.norm_num_groups, eps, silu, ws, f.st));
  }
  f.ar.free(ws);
  return HEDIT_OK;
}

// x [M][cin] -> *out [M][cout] (allocated here; x is NOT freed)
// dst / ldd: write the result into an existing buffer with row stride ldd (the left columns of the next
// skip concatenation) instead of allocating a contiguous [M][cout] one
int resblock(Fwd& f, const Res& r, const bf16_t* x, int H, int W, bf16_t** out, bf16_t* dst = nullptr, int ldd = 0) {
  const size_t M = (size_t)f.B * H * W;
  bf16_t *a1, *h1, *a2, *sc = nullptr, *y;
  TRY(aalloc(f, &a1, M * r.cin));
  TRY(groupnorm(f, x, a1, r.n1g, r.n1b, H * W, r.cin, 1e-5f, 1));
  TRY(aalloc(f, &h1, M * r.cout));
  TRY(conv3x3(f, a1, H, W, r.cin, r.conv1, r.cout, f.temb_all + r.temb_off, nullptr, h1, 1));
  f.ar.free(a1);
  TRY(aalloc(f, &a2, M * r.cout));
  TRY(groupnorm(f, h1, a2, r.n2g, r.n2b, H * W, r.cout, 1e-5f, 1));
  f.ar.free(h1);
  const bf16_t* res = x;
  if (r.sc_w) {
    TRY(aalloc(f, &sc, M * r.cout));
    TRY(linear(f, x, (int)M, r.cin, r.sc_w, r.cout, r.sc_b, nullptr, sc, r.cout));
    res = sc;
  }
  {   // Plug-and-Play feature injection: the target rows' conv2 input becomes the source rows'
    const hedit_p2p_plan* pl = (f.plan && f.plan->mode > 0) ? f.plan : nullptr;
    if (pl && pl->feat_src && f.rblock == pl->feat_resblock) RUN(f, copy_rows_launch(a2, pl->feat_src, f.B, (long)H * W * r.cout, f.st));
    ++f.rblock;
  }
  if (dst) {
    y = dst;
  } else {
    TRY(aalloc(f, &y, M * r.cout));
  }
  TRY(conv3x3(f, a2, H, W, r.cout, r.conv2, r.cout, r.conv2_b, res, y, 1, dst ? ldd : 0));
  f.ar.free(a2);
  if (sc) f.ar.free(sc);
  *out = y;
  return HEDIT_OK;
}

// One attention layer through the host-language controller: probabilities to HBM, the hook (which may rewrite them in
// place, on the launch stream), then probabilities . V.  Reference: ptp_utils.py:98-106.
int hooked_attention(Fwd& f, const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* vt, long ldvt, bf16_t* out, int ldo,
                     int N, int Mk, int kstride, int heads, int d, int is_cross) {
  AttnProbsParams ap{};
  ap.q = q; ap.ldq = ldq; ap.k = k; ap.ldk = ldk; ap.vt = vt; ap.ldvt = ldvt; ap.out = out; ap.ldo = ldo;
  ap.B = f.B; ap.N = N; ap.M = Mk; ap.kstride = kstride; ap.heads = heads; ap.d = d;
  TRY(aalloc(f, &ap.probs, (size_t)f.B * heads * N * Mk));
  const int layer = f.hook_layer++;
  if (!f.dry()) {
    TRY(attn_probs_launch(ap, f.st));
    const int rc = f.h->hook(f.h->hook_user, ap.probs, f.B * heads, N, Mk, is_cross, f.place, layer, f.st);
    if (rc != 0) {
      hedit_set_error("unet: the attention hook failed at layer " + std::to_string(layer) + " (code " + std::to_string(rc) + ")");
      return HEDIT_ERR_ARG;
    }
    TRY(attn_apply_launch(ap, f.st));
  }
  f.ar.free(ap.probs);
  return HEDIT_OK;
}

void chain_prof(Fwd& f, ProfScope& ps, size_t M, int C, int layers, int tag) {
  if (ps.rec >= 0) {
    auto& r = f.h->prof_recs[ps.rec];
    r.m = (int)M; r.n = C; r.k = layers * C; r.tag = tag;
  }
}

// A transformer block in two halves.  transformer_stem: everything in front of the cross-attention -- GroupNorm, proj_in,
// norm1, the self-attention, attn1.to_out + residual, norm2, attn2.to_q.  None of it sees the text context, so rows that
// carry the same latent give the same *t1 (the residual stream) and *q2 (the cross-attention's query), both [M][C] and
// allocated here; x is NOT freed.
int transformer_stem(Fwd& f, const Attn& a, const bf16_t* x, int H, int W, bf16_t** t1_out, bf16_t** q2_out) {
  const int C = a.C, N = H * W, B = f.B, heads = f.h->cfg.heads, d = C / heads;
  const size_t M = (size_t)B * N;
  const hedit_p2p_plan* pl = (f.plan && f.plan->mode > 0) ? f.plan : nullptr;
  bf16_t *xn, *t0, *tn, *qk, *vt, *ao, *t1, *q2;

  const bool chain = a.ffs != nullptr;
  TRY(aalloc(f, &t0, M * C));
  TRY(aalloc(f, &qk, M * 2 * C));
  TRY(aalloc(f, &vt, M * C));
  if (chain) {
    // GroupNorm statistics, then normalisation + proj_in -> norm1 -> q | k | v^T in ONE kernel (linchain.hip): x is read once,
    // t0 (the residual stream), q, k and v^T are written, nothing else touches HBM
    float* ws;
    const float* ss = nullptr;
    TRY(aalloc(f, &ws, groupnorm_ws_bytes(B, N, C) / sizeof(float)));
    { ProfScope ps(f, PK_NORM, 0.0, 2.0 * M * C); RUN(f, groupnorm_affine_launch(x, a.gn_g, a.gn_b, B, N, C, f.h->cfg.norm_num_groups, 1e-6f, ws, f.st, &ss)); }
    LinChainParams lc{};
    lc.a = x; lc.lda = C; lc.gn_ss = ss; lc.rows_per_image = N; lc.bias_pre = a.pin_b;
    lc.gamma = a.ln1g; lc.beta = a.ln1b; lc.eps = 1e-5f; lc.stream = a.frs;
    lc.out_mid = t0; lc.ldmid = C; lc.out_q = qk; lc.ldq = 2 * C; lc.out_k = qk + C; lc.ldk = 2 * C; lc.out = vt; lc.ldo = (long)M;
    lc.M = (int)M; lc.C = C;
    {
      ProfScope ps(f, PK_LINEAR, 2.0 * M * 4.0 * C * C, 10.0 * M * C + 8.0 * C * C);      // x read; t0, q, k, v^T written; weights once
      chain_prof(f, ps, M, C, 4, 129);                                                   // tag 129: GroupNorm .. q | k | v^T
      RUN(f, lin_chain_launch(lc, f.st));
    }
    f.ar.free(ws);
  } else {
    TRY(aalloc(f, &xn, M * C));
    TRY(groupnorm(f, x, xn, a.gn_g, a.gn_b, N, C, 1e-6f, 0));
    // ---- proj_in, norm1 and the self-attention projections
    TRY(aalloc(f, &tn, M * C));
    TRY(linear_ln(f, xn, (int)M, C, a.pin, C, a.pin_b, nullptr, t0, a.ln1g, a.ln1b, 1e-5f, tn));
    f.ar.free(xn);
    TRY(linear(f, tn, (int)M, C, a.w_qk, 2 * C, nullptr, nullptr, qk, 2 * C));
    TRY(linear(f, a.w_v1, C, C, tn, (int)M, nullptr, nullptr, vt, (int)M, 2));   // V^T = W_v . X^T
    f.ar.free(tn);
  }
  TRY(aalloc(f, &ao, M * C));
  {
    SelfAttnParams sp{};
    sp.q = qk; sp.ldq = 2 * C; sp.k = qk + C; sp.ldk = 2 * C; sp.vt = vt; sp.ldvt = (long)M;
    sp.out = ao; sp.ldo = C; sp.B = B; sp.N = N; sp.heads = heads; sp.d = d;
    sp.qk_src = (pl && pl->qk_src && N <= (pl->qk_max_tokens > 0 ? pl->qk_max_tokens : 1024) && f.tblock >= pl->qk_first_block)
                    ? pl->qk_src : nullptr;
    sp.kv_src = (pl && pl->kv_src && f.tblock >= pl->kv_first_block) ? pl->kv_src : nullptr;
    ++f.tblock;
    // mask-guided MasaCtrl: class arrays of this token count, where the mutual attention applies (forward_checks has refused
    // the combinations that cannot run: a hook, no kv_src, qk_src, a non-square latent)
    const uint8_t *cls_q = nullptr, *cls_k = nullptr;
    if (pl && pl->n_masa_rows > 0 && sp.kv_src && !pl->masa_auto) {
      for (int r = 0; r < pl->n_masa_res && !cls_q; ++r)
        if (pl->h_masa_tokens[r] == N) { cls_q = pl->h_masa_cls_q[r]; cls_k = pl->h_masa_cls_k[r]; }
    } else if (pl && pl->n_masa_rows > 0 && sp.kv_src) {
      // auto: the class array of this resolution from the maps collected so far in this pass; none yet: unmasked
      const int layer = f.masa_layer++;
      if (f.masa_count > 0 && N % 64 == 0 && N <= 4096) {
        uint8_t* cls = (pl->h_masa_dump && layer < pl->n_masa_dump && pl->h_masa_dump[layer])
                           ? pl->h_masa_dump[layer]
                           : reinterpret_cast<uint8_t*>(pl->masa_ws) + (size_t)pl->masa_images * 2 * 256 * sizeof(float);
        ProfScope ps(f, PK_SELF_ATTN, 0.0, 2048.0 * pl->masa_images + (double)B * N);
        RUN(f, masa_auto_mask_launch(reinterpret_cast<const float*>(pl->masa_ws), f.masa_count, pl->masa_images, W, pl->masa_thres,
                                     cls, f.st));
        cls_q = cls_k = cls;
      }
    }
    if (f.h->hook) {
      TRY(hooked_attention(f, sp.q, sp.ldq, sp.k, sp.ldk, sp.vt, sp.ldvt, ao, C, N, N, N, heads, d, 0));
    } else if (cls_q) {
      ProfScope ps(f, PK_SELF_ATTN, 4.0 * B * (double)N * N * C, 8.0 * M * C);
      // the rows that are not listed (the source rows) on the plain kernel, one launch per contiguous run with offset base
      // pointers: it is batch-invariant, so they keep the bits of a pass without masks (and of the inversion's calls)
      for (int r0 = 0; r0 < B;) {
        auto listed = [&](int r) {
          for (int i = 0; i < pl->n_masa_rows; ++i)
            if (pl->h_masa_rows[i] == r) return true;
          return false;
        };
        if (listed(r0)) { ++r0; continue; }
        int r1 = r0 + 1;
        while (r1 < B && !listed(r1)) ++r1;
        SelfAttnParams run = sp;
        run.q = sp.q + (size_t)r0 * N * sp.ldq; run.k = sp.k + (size_t)r0 * N * sp.ldk; run.vt = sp.vt + (size_t)r0 * N;
        run.out = sp.out + (size_t)r0 * N * sp.ldo; run.B = r1 - r0; run.kv_src = nullptr;
        RUN(f, self_attn_launch(run, f.st));
        r0 = r1;
      }
      MaskedSelfAttnParams mp{};
      mp.q = sp.q; mp.ldq = sp.ldq; mp.k = sp.k; mp.ldk = sp.ldk; mp.vt = sp.vt; mp.ldvt = sp.ldvt; mp.out = sp.out; mp.ldo = sp.ldo;
      mp.B = B; mp.N = N; mp.heads = heads; mp.d = d;
      mp.rows = pl->masa_rows; mp.n_rows = pl->n_masa_rows; mp.kv_src = sp.kv_src;
      mp.cls_q = cls_q; mp.cls_k = cls_k;
      RUN(f, masked_self_attn_launch(mp, f.st));
    } else {
      ProfScope ps(f, PK_SELF_ATTN, 4.0 * B * (double)N * N * C, 8.0 * M * C);      // q, k, v^T read, out written
      RUN(f, self_attn_launch(sp, f.st));
    }
    // the reference's store also keeps the <= 32 x 32 self maps; on request (plan.h_store_self) they are materialised for the
    // conditional rows beside the fused kernel, which never forms them
    if (N <= 1024) {
      if (pl && pl->mode == 2 && pl->h_store_self && f.store_self_idx < pl->n_store_self && !f.h->hook) {
        AttnProbsParams ap{};
        ap.q = sp.q; ap.ldq = sp.ldq; ap.k = sp.k; ap.ldk = sp.ldk; ap.probs = pl->h_store_self[f.store_self_idx];
        ap.B = pl->n_pairs; ap.N = N; ap.M = N; ap.kstride = N; ap.heads = heads; ap.d = d;
        ap.pair_src = pl->pair_src; ap.pair_tar = pl->pair_tar; ap.qk_src = sp.qk_src;
        RUN(f, attn_self_store_launch(ap, f.st));
      }
      f.store_self_idx++;
    }
  }
  f.ar.free(qk);
  f.ar.free(vt);
  TRY(aalloc(f, &t1, M * C));
  TRY(aalloc(f, &q2, M * C));
  if (chain) {
    // attn1.to_out + residual -> norm2 -> attn2.to_q in ONE kernel: t1 (the residual stream) and the query are written
    LinChainParams lc{};
    lc.a = ao; lc.lda = C; lc.r1 = t0; lc.ldr1 = C; lc.bias_pre = a.o1_b;
    lc.gamma = a.ln2g; lc.beta = a.ln2b; lc.eps = 1e-5f; lc.stream = a.k1s;
    lc.out_mid = t1; lc.ldmid = C; lc.out = q2; lc.ldo = C; lc.M = (int)M; lc.C = C;
    ProfScope ps(f, PK_LINEAR, 2.0 * M * 2.0 * C * C, 8.0 * M * C + 4.0 * C * C);          // ao, t0 read; t1, q written
    chain_prof(f, ps, M, C, 2, 130);                                                     // tag 130: attn1.to_out .. attn2.to_q
    RUN(f, lin_chain_launch(lc, f.st));
  } else {
    // ---- attn1.to_out + residual, norm2; cross-attention (P2P edits + store happen inside the kernel)
    TRY(aalloc(f, &tn, M * C));
    TRY(linear_ln(f, ao, (int)M, C, a.w_o1, C, a.o1_b, t0, t1, a.ln2g, a.ln2b, 1e-5f, tn));
    TRY(linear(f, tn, (int)M, C, a.w_q2, C, nullptr, nullptr, q2, C));
    f.ar.free(tn);
  }
  f.ar.free(ao);
  f.ar.free(t0);
  *t1_out = t1;
  *q2_out = q2;
  return HEDIT_OK;
}

// transformer_rest: the cross-attention and the block tail on x (the block's input and last residual), t1 and q2, which
// it frees; x [M][C] -> *out [M][C] (allocated here; x is NOT freed)
int transformer_rest(Fwd& f, const Attn& a, const bf16_t* x, bf16_t* t1, bf16_t* q2, int H, int W, bf16_t** out,
                     bf16_t* dst = nullptr, int ldd = 0) {
  const int C = a.C, N = H * W, B = f.B, heads = f.h->cfg.heads, d = C / heads;
  const size_t M = (size_t)B * N;
  const hedit_p2p_plan* pl = (f.plan && f.plan->mode > 0) ? f.plan : nullptr;
  bf16_t *tn, *ao, *k2, *vt2, *t2, *gf, *t3, *y;
  const bool chain = a.ffs != nullptr;
  const int MC = B * HEDIT_CTXP;
  k2 = const_cast<bf16_t*>(f.k2_all) + a.ctx_off;                      // row stride ctx_n
  vt2 = const_cast<bf16_t*>(f.vt2_all) + (size_t)a.ctx_off * MC;
  const int ldk2 = f.h->ctx_n;
  TRY(aalloc(f, &ao, M * C));
  {
    CrossAttnParams cp{};
    cp.q = q2; cp.ldq = C; cp.k = k2; cp.ldk = ldk2; cp.vt = vt2; cp.ldvt = MC; cp.out = ao; cp.ldo = C;
    cp.B = B; cp.N = N; cp.heads = heads; cp.d = d;
    const bool stored_layer = N <= 1024;
    if (pl) {
      cp.n_pairs = pl->n_pairs; cp.pair_src = pl->pair_src; cp.pair_tar = pl->pair_tar;
      cp.mixT = reinterpret_cast<const bf16_t*>(pl->mixT); cp.bvec = pl->bvec;
      cp.singles = pl->singles; cp.n_single = pl->n_single;
      cp.store = (pl->mode == 2 && stored_layer && pl->h_store && f.store_idx < pl->n_store) ? pl->h_store[f.store_idx] : nullptr;
    } else {
      cp.n_pairs = 0; cp.singles = f.h->iota; cp.n_single = B;
    }
    if (stored_layer) f.store_idx++;
    if (f.h->hook) {
      TRY(hooked_attention(f, cp.q, cp.ldq, cp.k, cp.ldk, cp.vt, cp.ldvt, ao, C, N, HEDIT_MAXW, HEDIT_CTXP, heads, d, 1));
    } else {
      ProfScope ps(f, PK_CROSS_ATTN, 4.0 * B * (double)N * HEDIT_MAXW * C, 4.0 * M * C + 4.0 * MC * C);
      RUN(f, cross_attn_launch(cp, f.st));
    }
    if (pl && pl->masa_auto && pl->n_masa_rows > 0 && N == 256 && !f.h->hook) {
      // mask-guided MasaCtrl, auto variant: beside the fused kernel (which never forms them) the probabilities of the 2 n
      // conditional rows -- the contiguous block from row 2 n -- are materialised and folded into the map accumulator
      const int n = pl->masa_images;
      float* acc = reinterpret_cast<float*>(pl->masa_ws);
      float* probs = reinterpret_cast<float*>(reinterpret_cast<char*>(pl->masa_ws) + (size_t)n * 2 * 256 * sizeof(float) + (size_t)B * 4096);
      AttnProbsParams ap{};
      ap.q = q2 + (size_t)2 * n * N * C; ap.ldq = C; ap.k = k2 + (size_t)2 * n * HEDIT_CTXP * ldk2; ap.ldk = ldk2;
      ap.probs = probs; ap.B = 2 * n; ap.N = N; ap.M = HEDIT_MAXW; ap.kstride = HEDIT_CTXP; ap.heads = heads; ap.d = d;
      ProfScope ps(f, PK_CROSS_ATTN, 4.0 * n * (double)N * HEDIT_MAXW * C, 8.0 * n * heads * N * HEDIT_MAXW);
      RUN(f, attn_probs_launch(ap, f.st));
      RUN(f, masa_accumulate_launch(probs, heads, 2 * n, pl->masa_ref_tokens, pl->n_masa_ref, pl->masa_cur_tokens, pl->n_masa_cur,
                                    acc, f.st));
      ++f.masa_count;
    }
  }
  f.ar.free(q2);
  if (chain) {
    // attn2.to_out + residual -> LayerNorm -> FF1 -> GEGLU -> FF2 + residual -> proj_out + residual in ONE kernel: rows in
    // registers, weights streamed (ffn.hip).  The result goes where proj_out's would (dst / ldd: the next concatenation).
    if (dst) {
      y = dst;
    } else {
      TRY(aalloc(f, &y, M * C));
    }
    FfnParams fp{};
    fp.a = ao; fp.lda = C; fp.x = t1; fp.ldx = C; fp.r2 = x; fp.ldr2 = C;
    fp.bias_pre = a.o2_b; fp.bias_post = a.pout_b;
    fp.gamma = a.ln3g; fp.beta = a.ln3b; fp.eps = 1e-5f;
    fp.stream = a.ffs; fp.bias1p = a.ff1_bp; fp.bias2 = a.ff2_b; fp.out = y; fp.ldo = dst ? ldd : C; fp.M = (int)M; fp.C = C;
    {
      ProfScope ps(f, PK_LINEAR, 2.0 * M * 14.0 * C * C, 8.0 * M * C + 28.0 * C * C);      // a, t1, x read, out written; weights once
      chain_prof(f, ps, M, C, 14, 128);                                                  // tag 128: the fused block tail
      RUN(f, ffn_fused_launch(fp, f.st));
    }
    f.ar.free(ao);
    f.ar.free(t1);
    *out = y;
    return HEDIT_OK;
  }
  TRY(aalloc(f, &t2, M * C));
  // ---- attn2.to_out + residual, norm3, GEGLU feed-forward
  TRY(aalloc(f, &tn, M * C));
  TRY(linear_ln(f, ao, (int)M, C, a.w_o2, C, a.o2_b, t1, t2, a.ln3g, a.ln3b, 1e-5f, tn));
  f.ar.free(ao);
  f.ar.free(t1);
  TRY(aalloc(f, &gf, M * 4 * C));
  {
    GemmParams gp{};
    gp.A = tn; gp.W = a.ff1; gp.M = (int)M; gp.N = 8 * C; gp.K = C; gp.lda = C; gp.mode = 0;
    gp.bias = a.ff1_b; gp.residual = nullptr; gp.ldr = 0; gp.C = gf; gp.ldc = 4 * C; gp.geglu = 1;
    ProfScope ps(f, PK_LINEAR, 2.0 * gp.M * gp.N * gp.K, gemm_alg_bytes(f, gp));
    RUN(f, gemm_launch(gp, 1, nullptr, f.st));
  }
  f.ar.free(tn);
  TRY(aalloc(f, &t3, M * C));
  TRY(linear(f, gf, (int)M, 4 * C, a.ff2, C, a.ff2_b, t2, t3, C));
  f.ar.free(gf);
  f.ar.free(t2);

  if (dst) {
    y = dst;
  } else {
    TRY(aalloc(f, &y, M * C));
  }
  TRY(linear(f, t3, (int)M, C, a.pout, C, a.pout_b, x, y, dst ? ldd : C));
  f.ar.free(t3);
  *out = y;
  return HEDIT_OK;
}

// x [M][C] -> *out [M][C] (allocated here; x is NOT freed)
int transformer(Fwd& f, const Attn& a, const bf16_t* x, int H, int W, bf16_t** out, bf16_t* dst = nullptr, int ldd = 0) {
  bf16_t *t1, *q2;
  TRY(transformer_stem(f, a, x, H, W, &t1, &q2));
  return transformer_rest(f, a, x, t1, q2, H, W, out, dst, ldd);
}

struct Skip { bf16_t* p; int C; bool per_latent = false; };   // per_latent: one image per distinct latent, read through the row map

// May the part in front of the first cross-attention run once per distinct latent?  Only while nothing in it looks at
// another row or hands a row's self-attention to the caller.  N0 = tokens of the first transformer block.
bool stem_shareable(const hedit_unet* h, const hedit_p2p_plan* plan, int D, int B, int N0) {
  if (D >= B || h->hook || h->down.empty() || !h->down[0].has_attn) return false;
  const hedit_p2p_plan* pl = (plan && plan->mode > 0) ? plan : nullptr;
  if (!pl) return true;
  if (pl->feat_src && pl->feat_resblock <= 0) return false;
  if (pl->kv_src && pl->kv_first_block <= 0) return false;
  if (pl->qk_src && N0 <= (pl->qk_max_tokens > 0 ? pl->qk_max_tokens : 1024) && pl->qk_first_block <= 0) return false;
  if (pl->mode == 2 && pl->h_store_self && pl->n_store_self > 0 && N0 <= 1024) return false;
  return true;
}

// The block's input, t1 and q2 of the first transformer, computed per distinct latent, become per batch row: one launch
int broadcast_stem(Fwd& f, size_t row_elems, bf16_t** x, bf16_t** t1, bf16_t** q2, int D) {
  bf16_t** narrow[3] = {x, t1, q2};
  bf16_t* wide[3];
  const void* src[3];
  void* dst[3];
  for (int i = 0; i < 3; ++i) {
    TRY(aalloc(f, &wide[i], (size_t)f.B * row_elems));
    src[i] = *narrow[i];
    dst[i] = wide[i];
  }
  {
    ProfScope ps(f, PK_OTHER, 0.0, 3.0 * (D + f.B) * (double)row_elems * sizeof(bf16_t));
    RUN(f, gather_rows_launch(src, dst, 3, f.B, (long)(row_elems * sizeof(bf16_t)), *f.map, f.st));
  }
  for (int i = 0; i < 3; ++i) {
    f.ar.free(*narrow[i]);
    *narrow[i] = wide[i];
  }
  return HEDIT_OK;
}

// The text context of a call: fp32 [B][77][ctx_dim] -> bf16 padded to 80 rows per item, then the attn2 keys / values of ALL
// transformer blocks in two launches.  They stay live for the whole pass (the blocks read their column / row slice):
// 2 * B * 80 * ctx_n * 2 bytes = 4 MB per batch row for SD-1.5 (ctx_n = 12480), 0.48 GB at the bench's 120 rows -- arena
// allocations like every other (hedit_unet_workspace_bytes counts them), or the memory of a hedit_unet_context, which runs this
// very routine once (hedit_unet_context_create) for the calls that are handed the object instead of the fp32 rows.
int project_context(Fwd& f, const float* ctx) {
  hedit_unet* h = f.h;
  const hedit_unet_cfg& c = h->cfg;
  const int MC = f.B * HEDIT_CTXP;
  bf16_t *ctxb, *k2a, *vt2a;
  TRY(aalloc(f, &ctxb, (size_t)MC * c.cross_attention_dim));
  RUN(f, ctx_pad_launch(ctx, ctxb, f.B, c.cross_attention_dim, f.st));
  f.ctxb = ctxb;
  TRY(aalloc(f, &k2a, (size_t)MC * h->ctx_n));
  TRY(aalloc(f, &vt2a, (size_t)MC * h->ctx_n));
  TRY(linear(f, ctxb, MC, c.cross_attention_dim, h->wk2_all, h->ctx_n, nullptr, nullptr, k2a, h->ctx_n));
  TRY(linear(f, h->wv2_all, h->ctx_n, c.cross_attention_dim, ctxb, MC, nullptr, nullptr, vt2a, MC, 2));
  f.k2_all = k2a;
  f.vt2_all = vt2a;
  return HEDIT_OK;
}

}  // namespace

// include/hedit.h: a snapshot of project_context's three results for `B` rows, in memory of its own
struct HEDIT_HANDLE hedit_unet_context {
  const hedit_unet* owner = nullptr;     // compared, never dereferenced: the object may outlive its network
  int B = 0;
  void* buf = nullptr;
  const bf16_t *ctxb = nullptr, *k2_all = nullptr, *vt2_all = nullptr;
};

namespace {

// D == 0: x holds one latent per batch row.  D > 0 (hedit_unet_forward_shared): x holds D distinct latents and row r
// evaluates latent map->src[r]; a dry run takes the row COUNT only (map == nullptr).  cx: the projected context of these B rows
// (then ctx is not read and the three launches of project_context are skipped).
int forward_impl(hedit_unet* h, const float* x, float t, const float* ctx, int B, int H0, int W0,
                 const hedit_p2p_plan* plan, float* eps_out, void* ws, size_t ws_bytes, hipStream_t st,
                 bool dry, size_t* peak, int D = 0, const RowMap* map = nullptr, const hedit_unet_context* cx = nullptr) {
  const hedit_unet_cfg& c = h->cfg;
  Fwd f;
  f.h = h; f.B = B; f.st = st; f.plan = plan; f.map = map;
  f.ar.base = reinterpret_cast<char*>(ws); f.ar.cap = ws_bytes; f.ar.dry = dry;
  const int ch0 = c.block_out_channels[0];

  if (!dry && h->iota_cap < B) {
    hedit_set_error("batch larger than " + std::to_string(h->iota_cap) + " rows");
    return HEDIT_ERR_ARG;
  }

  // mask-guided MasaCtrl, auto variant: the map accumulator starts every pass at zero
  if (!dry && plan && plan->mode > 0 && plan->masa_auto && plan->n_masa_rows > 0)
    HIP_TRY(hipMemsetAsync(plan->masa_ws, 0, (size_t)plan->masa_images * 2 * 256 * sizeof(float), st));

  // ---- text context
  if (cx) {
    f.ctxb = cx->ctxb; f.k2_all = cx->k2_all; f.vt2_all = cx->vt2_all;
  } else {
    TRY(project_context(f, ctx));
  }

  // ---- time embedding chain (the timestep is shared by the batch, so this is one GEMV chain)
  float *te0, *te1, *te2, *temb_all;
  TRY(aalloc(f, &te0, (size_t)ch0));
  TRY(aalloc(f, &te1, (size_t)h->temb_dim));
  TRY(aalloc(f, &te2, (size_t)h->temb_dim));
  TRY(aalloc(f, &temb_all, (size_t)h->temb_total));
  RUN(f, timestep_embed_launch(t, te0, ch0, st));
  RUN(f, gemv_launch(h->te1_w, te0, h->te1_b, nullptr, te1, h->temb_dim, ch0, 0, st));
  RUN(f, gemv_launch(h->te2_w, te1, h->te2_b, nullptr, te2, h->temb_dim, h->temb_dim, 1, st));
  RUN(f, gemv_launch(h->temb_w_all, te2, h->temb_b_all, h->conv1_b_all, temb_all, h->temb_total, h->temb_dim, 1, st));
  f.temb_all = temb_all;

  // ---- stem.  With a row map: once per distinct latent where that is the same arithmetic (stem_shareable), else the
  // latents are spread to one per row first and everything below is the plain path
  int H = H0, W = W0;
  const bool share = D > 0 && stem_shareable(h, plan, D, B, H0 * W0);
  float* xrows = nullptr;
  if (D > 0 && !share) {
    const size_t img = (size_t)c.in_channels * H * W;
    TRY(aalloc(f, &xrows, (size_t)B * img));
    const void* src[1] = {x};
    void* dst[1] = {xrows};
    ProfScope ps(f, PK_OTHER, 0.0, (double)(D + B) * img * sizeof(float));
    RUN(f, gather_rows_launch(src, dst, 1, B, (long)(img * sizeof(float)), *map, st));
    x = xrows;
  }
  bf16_t* cur;
  {
    BatchScope rows(f, share ? D : B);
    TRY(aalloc(f, &cur, (size_t)f.B * H * W * ch0));
    RUN(f, conv_in_launch(x, h->conv_in_w, h->conv_in_b, cur, f.B, c.in_channels, H, W, ch0, st));
  }
  if (xrows) f.ar.free(xrows);
  std::vector<Skip> skips;
  skips.push_back({cur, ch0, share});      // the first skip stays per latent: its concatenation copies it anyway

  // ---- down path
  for (int i = 0; i < c.n_levels; ++i) {
    Block& blk = h->down[i];
    for (size_t j = 0; j < blk.res.size(); ++j) {
      const bool stem = share && i == 0 && j == 0;      // still per latent: up to the first cross-attention
      bf16_t *y, *t1 = nullptr, *q2 = nullptr;
      {
        BatchScope rows(f, stem ? D : B);
        TRY(resblock(f, blk.res[j], cur, H, W, &y));
        if (blk.has_attn) {
          f.place = 0;
          TRY(transformer_stem(f, blk.attn[j], y, H, W, &t1, &q2));
        }
      }
      // cur stays alive as a skip
      cur = y;
      if (stem) TRY(broadcast_stem(f, (size_t)H * W * blk.ch, &cur, &t1, &q2, D));
      if (blk.has_attn) {
        bf16_t* z;
        TRY(transformer_rest(f, blk.attn[j], cur, t1, q2, H, W, &z));
        f.ar.free(cur);
        cur = z;
      }
      skips.push_back({cur, blk.ch});
    }
    if (blk.has_sampler) {
      bf16_t* y;
      TRY(aalloc(f, &y, (size_t)B * (H / 2) * (W / 2) * blk.ch));
      TRY(conv3x3(f, cur, H, W, blk.ch, blk.samp_w, blk.ch, blk.samp_b, nullptr, y, 2));
      H /= 2; W /= 2;
      cur = y;
      skips.push_back({cur, blk.ch});
    }
  }

  // ---- mid (cur is the last skip: do not free it here)
  {
    bf16_t *y, *z, *w;
    TRY(resblock(f, h->mid_res[0], cur, H, W, &y));
    f.place = 1;
    TRY(transformer(f, h->mid_attn, y, H, W, &z));
    f.ar.free(y);
    TRY(resblock(f, h->mid_res[1], z, H, W, &w));
    f.ar.free(z);
    cur = w;
  }
  int cur_c = c.block_out_channels[c.n_levels - 1];

  // ---- up path.  Every concatenation [cur | skip] is laid out before its left half is produced: the block that
  // computes `cur` (ResNet conv2, transformer proj_out or the upsampling conv) writes it straight into the left
  // columns of the next concatenation buffer (row stride = its full width), so only the skip half is copied.
  bool in_cat = false;         // cur already sits in `cat_next`
  bf16_t* cat_next = nullptr;
  for (int i = 0; i < c.n_levels; ++i) {
    Block& blk = h->up[i];
    for (size_t j = 0; j < blk.res.size(); ++j) {
      Skip s = skips.back();
      skips.pop_back();
      bf16_t* cat;
      const size_t M = (size_t)B * H * W;
      if (in_cat) {
        cat = cat_next;
        { ProfScope ps(f, PK_OTHER, 0.0); RUN(f, concat_launch(nullptr, cur_c, s.p, s.C, cat, (long)M, st, s.per_latent ? f.map : nullptr, H * W)); }
      } else {
        TRY(aalloc(f, &cat, M * (cur_c + s.C)));
        { ProfScope ps(f, PK_OTHER, 0.0); RUN(f, concat_launch(cur, cur_c, s.p, s.C, cat, (long)M, st, s.per_latent ? f.map : nullptr, H * W)); }
        f.ar.free(cur);
      }
      f.ar.free(s.p);
      // where does this block's output go next?
      const bool last_res = j + 1 == blk.res.size();
      const bool to_cat = !last_res;                      // next consumer is the next ResNet block of this level
      bf16_t* dst = nullptr;
      int ldd = 0;
      if (to_cat) {
        ldd = blk.ch + skips.back().C;
        TRY(aalloc(f, &dst, M * ldd));
      }
      bf16_t* y;
      if (blk.has_attn) {
        TRY(resblock(f, blk.res[j], cat, H, W, &y));
        f.ar.free(cat);
        bf16_t* z;
        f.place = 2;
        TRY(transformer(f, blk.attn[j], y, H, W, &z, dst, ldd));
        f.ar.free(y);
        cur = z;
      } else {
        TRY(resblock(f, blk.res[j], cat, H, W, &y, dst, ldd));
        f.ar.free(cat);
        cur = y;
      }
      cur_c = blk.ch;
      in_cat = to_cat;
      cat_next = dst;
    }
    if (blk.has_sampler) {
      // the upsampled tensor is the left half of the next level's first concatenation
      const size_t M4 = (size_t)B * H * W * 4;
      const int ldd = blk.ch + skips.back().C;
      bf16_t* dst;
      TRY(aalloc(f, &dst, M4 * ldd));
      TRY(conv3x3(f, cur, H, W, blk.ch, blk.samp_w, blk.ch, blk.samp_b, nullptr, dst, 3, ldd));
      f.ar.free(cur);
      H *= 2; W *= 2;
      cur = dst;
      in_cat = true;
      cat_next = dst;
    }
  }

  // ---- head
  {
    bf16_t* a;
    TRY(aalloc(f, &a, (size_t)B * H * W * ch0));
    TRY(groupnorm(f, cur, a, h->gn_out_g, h->gn_out_b, H * W, ch0, 1e-5f, 1));
    if (c.out_channels != 4 || ch0 % 64 != 0) {
      RUN(f, conv_out_launch(a, h->conv_out_w, h->conv_out_b, eps_out, B, H, W, ch0, c.out_channels, st));
    } else {
      // conv_out as an N = 4 MFMA GEMM (fp32 products) + bias / NCHW pass: the one-wave-per-pixel kernel re-reads the
      // activation nine times (0.99 ms at 120 rows)
      float* prod;
      const size_t M = (size_t)B * H * W;
      TRY(aalloc(f, &prod, M * 4));
      GemmParams p{};
      p.mode = 1; p.Hin = H; p.Win = W; p.Cin = ch0; p.Hout = H; p.Wout = W;
      p.A = a; p.W = h->conv_out_w; p.M = (int)M; p.N = 4; p.K = 9 * ch0; p.lda = ch0; p.raw_f32 = prod; p.ldc = 4;
      TRY(run_gemm(f, p));
      RUN(f, rows_to_nchw_launch(prod, h->conv_out_b, eps_out, B, (long)H * W, 4, 4, st));
      f.ar.free(prod);
    }
    f.ar.free(a);
    f.ar.free(cur);
  }
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

}  // namespace

#include "unetgrad.h"

static void unet_pre_destroy(hedit_unet* h) {
  drop_tape(h);
  for (hipEvent_t e : h->prof_pool) (void)hipEventDestroy(e);
}
HEDIT_LIFECYCLE(unet, hedit_unet, "", unet_pre_destroy)

// =============================================================================== C ABI
// grad: attach the input-gradient twins (hedit_unet_create_grad); without it, exactly the forward-only handle
// ctx: also the transposed context projections (hedit_unet_create_grad_ctx)
static int create_impl(const hedit_unet_cfg* cfg, hedit_unet** out, bool grad, bool ctx = false) {
  ARG_CHECK(cfg && out, "null");
  ARG_CHECK(cfg->n_levels >= 2 && cfg->n_levels <= HEDIT_MAX_LEVELS, "n_levels");
  ARG_CHECK(cfg->in_channels <= 8 && cfg->out_channels <= 4, "in/out channels");
  ARG_CHECK(cfg->cross_attention_dim % 64 == 0, "cross_attention_dim % 64");
  for (int i = 0; i < cfg->n_levels; ++i) {
    ARG_CHECK(cfg->block_out_channels[i] % 64 == 0, "block_out_channels % 64");
    ARG_CHECK(cfg->block_out_channels[i] % cfg->norm_num_groups == 0, "channels % groups");
    const int d = cfg->block_out_channels[i] / cfg->heads;
    ARG_CHECK(d == 32 || d == 40 || d == 64 || d == 80 || d == 160, "head dim must be one of 32,40,64,80,160");
  }
  TRY(gemm_prepare());
  if (grad) ARG_CHECK(cfg->in_channels <= 4, "the input-gradient pass needs in_channels <= 4");
  hedit_unet* h = new hedit_unet();
  h->cfg = *cfg;
  h->grad = grad;
  const int* ch = cfg->block_out_channels;
  const int L = cfg->layers_per_block, n = cfg->n_levels;
  h->temb_dim = ch[0] * 4;

  // channel plan of every ResBlock (needed up-front to size the fused time-embedding projection)
  int total = 0;
  {
    int outc = ch[0];
    for (int i = 0; i < n; ++i) { outc = ch[i]; total += L * outc; }
    total += 2 * ch[n - 1];
    for (int i = 0; i < n; ++i) total += (L + 1) * ch[n - 1 - i];
  }
  h->temb_total = total;
  h->temb_w_all = dalloc<bf16_t>(h, (size_t)total * h->temb_dim);
  h->temb_b_all = dalloc<float>(h, total);
  h->conv1_b_all = dalloc<float>(h, total);

  h->conv_in_w = f32conv(h, "conv_in.weight", ch[0], cfg->in_channels, 3);
  if (grad) {   // [4][9][ch0], rows beyond in_channels zero: the N = 4 route of the head convolution
    h->conv_in_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)4 * 9 * ch[0]);
    if (h->conv_in_t && hipMemset(h->conv_in_t, 0, (size_t)4 * 9 * ch[0] * sizeof(bf16_t)) != hipSuccess) h->alloc_failed = true;
  }
  h->conv_in_b = vec(h, "conv_in.bias", ch[0]);
  h->te1_w = lin(h, "time_embedding.linear_1.weight", h->temb_dim, ch[0]);
  h->te1_b = vec(h, "time_embedding.linear_1.bias", h->temb_dim);
  h->te2_w = lin(h, "time_embedding.linear_2.weight", h->temb_dim, h->temb_dim);
  h->te2_b = vec(h, "time_embedding.linear_2.bias", h->temb_dim);

  for (int i = 0; i < n; ++i) {
    if (cfg->down_has_attn[i]) h->ctx_n += L * ch[i];
    if (cfg->up_has_attn[i]) h->ctx_n += (L + 1) * ch[n - 1 - i];
  }
  h->ctx_n += ch[n - 1];
  h->wk2_all = dalloc<bf16_t>(h, (size_t)h->ctx_n * cfg->cross_attention_dim);
  h->wv2_all = dalloc<bf16_t>(h, (size_t)h->ctx_n * cfg->cross_attention_dim);
  if (ctx) h->wkv2_t = dalloc<bf16_t>(h, (size_t)2 * h->ctx_n * cfg->cross_attention_dim);

  int toff = 0;
  int outc = ch[0];
  for (int i = 0; i < n; ++i) {
    const int inc = outc;
    outc = ch[i];
    Block b;
    b.ch = outc;
    b.has_attn = cfg->down_has_attn[i] != 0;
    const std::string pre = "down_blocks." + std::to_string(i);
    for (int j = 0; j < L; ++j) {
      b.res.push_back(make_res(h, pre + ".resnets." + std::to_string(j), j == 0 ? inc : outc, outc, toff));
      if (b.has_attn) b.attn.push_back(make_attn(h, pre + ".attentions." + std::to_string(j), outc));
    }
    if (i != n - 1) {
      b.has_sampler = true;
      b.samp_w = conv3(h, pre + ".downsamplers.0.conv.weight", outc, outc);
      if (grad) b.samp_t = twin<bf16_t>(h, Pack::Conv3S2Dgrad, (size_t)outc * outc * 9);
      b.samp_b = vec(h, pre + ".downsamplers.0.conv.bias", outc);
    }
    h->down.push_back(b);
  }
  h->mid_attn = make_attn(h, "mid_block.attentions.0", ch[n - 1]);
  h->mid_res[0] = make_res(h, "mid_block.resnets.0", ch[n - 1], ch[n - 1], toff);
  h->mid_res[1] = make_res(h, "mid_block.resnets.1", ch[n - 1], ch[n - 1], toff);
  outc = ch[n - 1];
  for (int i = 0; i < n; ++i) {
    const int prev = outc;
    outc = ch[n - 1 - i];
    const int inp = ch[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
    Block b;
    b.ch = outc;
    b.has_attn = cfg->up_has_attn[i] != 0;
    const std::string pre = "up_blocks." + std::to_string(i);
    for (int j = 0; j < L + 1; ++j) {
      const int skip = j == L ? inp : outc;
      const int rin = j == 0 ? prev : outc;
      b.res.push_back(make_res(h, pre + ".resnets." + std::to_string(j), rin + skip, outc, toff));
      if (b.has_attn) b.attn.push_back(make_attn(h, pre + ".attentions." + std::to_string(j), outc));
    }
    if (i != n - 1) {
      b.has_sampler = true;
      b.samp_w = conv3(h, pre + ".upsamplers.0.conv.weight", outc, outc);
      if (grad) b.samp_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)outc * outc * 9);
      b.samp_b = vec(h, pre + ".upsamplers.0.conv.bias", outc);
    }
    h->up.push_back(b);
  }
  h->gn_out_g = vec(h, "conv_norm_out.weight", ch[0]);
  h->gn_out_b = vec(h, "conv_norm_out.bias", ch[0]);
  h->conv_out_w = conv3(h, "conv_out.weight", cfg->out_channels, ch[0]);
  if (grad) {
    h->conv_out_t = twin<float>(h, Pack::FlipOIHW, (size_t)cfg->out_channels * ch[0] * 9);
    h->zero_bias = dalloc<float>(h, ch[0]);
    if (h->zero_bias && hipMemset(h->zero_bias, 0, ch[0] * sizeof(float)) != hipSuccess) h->alloc_failed = true;
  }
  h->conv_out_b = vec(h, "conv_out.bias", cfg->out_channels);

  {
    // identity row list for "all rows are singles" (controller off), sized once: nothing is allocated or copied
    // synchronously inside hedit_unet_forward
    constexpr int IOTA = 16384;
    std::vector<int32_t> v(IOTA);
    for (int i = 0; i < IOTA; ++i) v[i] = i;
    h->iota = dalloc<int32_t>(h, IOTA);
    if (h->iota && hipMemcpy(h->iota, v.data(), IOTA * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) h->alloc_failed = true;
    h->iota_cap = IOTA;
  }
  // every block must have taken exactly its slice of the stacked attn2.to_k / to_v matrices and of the time-embedding projection
  if (h->ctx_next != h->ctx_n || toff != total) {
    hedit_set_error(h->ctx_next != h->ctx_n ? "internal: stacked context-projection plan mismatch" : "internal: time-embedding plan mismatch");
    hedit_unet_destroy(h);
    return HEDIT_ERR_STATE;
  }
  return handle_created(h, out);
}

extern "C" {

int hedit_unet_create(const hedit_unet_cfg* cfg, hedit_unet** out) try {
  return create_impl(cfg, out, false);
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_create_grad(const hedit_unet_cfg* cfg, hedit_unet** out) try {
  return create_impl(cfg, out, true);
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_create_grad_ctx(const hedit_unet_cfg* cfg, hedit_unet** out) try {
  return create_impl(cfg, out, true, true);
} catch (...) { return hedit_abi_catch(); }

/* 1: the executor keeps this parameter as an unscaled bf16 copy (matrices, convolutions), so handing it over rounded to
   bf16 loses nothing -- what the start-up weight broadcast uses to halve its blob; 0: kept in fp32 or scaled while packed */
int hedit_unet_param_bf16_exact(const hedit_unet* h, int i) try {
  return store_param_bf16_exact(h, i);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* enough for hedit_unet_forward and for hedit_unet_forward_shared under ANY row map: the arena's layout depends on how many
   rows the shared part runs at, so every count of distinct latents gets its dry run (D == B: the latents are spread to one
   per row first, what a call that may not share does) */
size_t hedit_unet_workspace_bytes(hedit_unet* h, int B, int height, int width) try {
  if (!h) return 0;
  const std::array<int, 4> key{B, height, width, h->hook ? 1 : 0};
  auto it = h->ws_cache.find(key);
  if (it != h->ws_cache.end()) return it->second;
  size_t need = 0;
  for (int D = 0; D <= (B <= HEDIT_ROWMAP_MAX ? B : 0); ++D) {
    size_t peak = 0;
    if (forward_impl(h, nullptr, 0.f, nullptr, B, height, width, nullptr, nullptr, nullptr, 0, nullptr, true, &peak, D) != HEDIT_OK) return 0;
    if (peak > need) need = peak;
  }
  need += 4096;
  h->ws_cache[key] = need;
  return need;
} catch (...) { (void)hedit_abi_catch(); return 0; }

static int forward_checks(hedit_unet* h, const float* x, const void* ctx, int B, int height, int width, const hedit_p2p_plan* plan,
                          float* eps_out, void* workspace) {
  ARG_CHECK(h && x && ctx && eps_out && workspace, "null");
  ARG_CHECK(B >= 1, "B");
  const int div = 1 << (h->cfg.n_levels - 1);
  ARG_CHECK(height % div == 0 && width % div == 0, "latent size must be divisible by 2^(levels-1)");
  const int lowest = (height / div) * (width / div);
  ARG_CHECK(lowest % 64 == 0, "lowest-resolution level must have a multiple of 64 tokens");
  TRY(store_require_loaded(h, "UNet"));
  if (plan && plan->mode > 0 && plan->n_masa_rows > 0) {     // mask-guided MasaCtrl: refused by name before anything is launched
    ARG_CHECK(!h->hook, "masa classes: the host-language attention hook cannot run class-matched attention");
    ARG_CHECK(plan->kv_src, "masa classes need kv_src (whose keys, values and key classes a row reads)");
    ARG_CHECK(!plan->qk_src, "masa classes exclude qk_src");
    ARG_CHECK(height == width, "masa classes: non-square layer (the masks are interpolated to square layers)");
    ARG_CHECK(plan->masa_rows && plan->h_masa_rows && plan->n_masa_rows <= B, "masa classes: the listed rows (device and host copy)");
    for (int i = 0; i < plan->n_masa_rows; ++i)
      ARG_CHECK(plan->h_masa_rows[i] >= 0 && plan->h_masa_rows[i] < B, "masa classes: listed rows must lie in [0, B)");
    if (plan->masa_auto) {
      const int n = plan->masa_images;
      ARG_CHECK(n > 0 && B == 4 * n && plan->n_masa_rows == 2 * n, "masa auto: the batch must be 4 * masa_images rows, 2 * masa_images listed");
      ARG_CHECK(plan->masa_ref_tokens && plan->n_masa_ref > 0 && plan->masa_cur_tokens && plan->n_masa_cur > 0, "masa auto: token lists");
      ARG_CHECK(plan->masa_ws && reinterpret_cast<uintptr_t>(plan->masa_ws) % 16 == 0, "masa auto: masa_ws (16-byte aligned)");
      const size_t need = (size_t)n * 2 * 256 * sizeof(float) + (size_t)B * 4096 + (size_t)n * 2 * h->cfg.heads * 256 * HEDIT_MAXW * sizeof(float);
      ARG_CHECK(plan->masa_ws_bytes >= need, "masa auto: masa_ws is too small");
    } else {
      ARG_CHECK(plan->n_masa_res > 0 && plan->h_masa_cls_q && plan->h_masa_cls_k && plan->h_masa_tokens, "masa classes: class arrays");
      for (int r = 0; r < plan->n_masa_res; ++r)
        ARG_CHECK(plan->h_masa_cls_q[r] && plan->h_masa_cls_k[r] && plan->h_masa_tokens[r] > 0, "masa classes: a class array is missing");
    }
  }
  ARG_CHECK(!(h->hook && plan && plan->mode > 0), "an attention hook excludes the in-kernel edits of a plan (pass plan = NULL)");
  if (plan && plan->mode > 0) {
    ARG_CHECK(plan->n_pairs >= 0 && plan->n_pairs + plan->n_single > 0, "plan rows");
    ARG_CHECK(plan->n_pairs == 0 || (plan->pair_src && plan->pair_tar && plan->mixT && plan->bvec), "plan tables");
  }
  return HEDIT_OK;
}

int hedit_unet_forward(hedit_unet* h, const float* x, float t, const float* ctx, int B, int height, int width,
                       const hedit_p2p_plan* plan, float* eps_out, void* workspace, size_t workspace_bytes,
                       void* stream) try {
  TRY(forward_checks(h, x, ctx, B, height, width, plan, eps_out, workspace));
  return forward_impl(h, x, t, ctx, B, height, width, plan, eps_out, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

static int row_map_checks(const float* x, int D, const int* row_latent, int B, RowMap* map) {
  ARG_CHECK(row_latent && D >= 1 && D <= 65535, "row map");
  if (B > HEDIT_ROWMAP_MAX) {
    hedit_set_error("batch larger than " + std::to_string(HEDIT_ROWMAP_MAX) + " rows (the row map of shared latents)");
    return HEDIT_ERR_ARG;
  }
  ARG_CHECK(reinterpret_cast<uintptr_t>(x) % 16 == 0, "x must be 16-byte aligned");
  for (int r = 0; r < B; ++r) {
    ARG_CHECK(row_latent[r] >= 0 && row_latent[r] < D, "row_latent entries must lie in [0, D)");
    map->src[r] = (uint16_t)row_latent[r];
  }
  return HEDIT_OK;
}

int hedit_unet_forward_shared(hedit_unet* h, const float* x, int D, const int* row_latent, float t, const float* ctx, int B,
                              int height, int width, const hedit_p2p_plan* plan, float* eps_out, void* workspace,
                              size_t workspace_bytes, void* stream) try {
  TRY(forward_checks(h, x, ctx, B, height, width, plan, eps_out, workspace));
  RowMap map{};      // handed to the kernels by value: nothing to upload, nothing to keep alive
  TRY(row_map_checks(x, D, row_latent, B, &map));
  return forward_impl(h, x, t, ctx, B, height, width, plan, eps_out, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream), false, nullptr, D, &map);
} catch (...) { return hedit_abi_catch(); }

// ---- a bound text context
int hedit_unet_context_create(hedit_unet* h, const float* ctx, int B, void* stream, hedit_unet_context** out) try {
  ARG_CHECK(h && ctx && out, "null");
  ARG_CHECK(B >= 1, "B");
  TRY(store_require_loaded(h, "UNet"));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone) {
    hedit_set_error("hedit_unet_context_create allocates: not while the stream is capturing");
    return HEDIT_ERR_STATE;
  }
  Fwd f;
  f.h = h; f.B = B; f.st = st; f.plan = nullptr;
  f.ar.dry = true;
  TRY(project_context(f, nullptr));
  const size_t bytes = f.ar.peak;
  void* buf = nullptr;
  if (hipMalloc(&buf, bytes) != hipSuccess) {
    (void)hipGetLastError();
    hedit_set_error("hedit_unet_context_create: out of device memory (" + std::to_string(bytes) + " bytes)");
    return HEDIT_ERR_HIP;
  }
  Fwd g;
  g.h = h; g.B = B; g.st = st; g.plan = nullptr;
  g.ar.base = reinterpret_cast<char*>(buf); g.ar.cap = bytes;
  const int rc = project_context(g, ctx);
  if (rc != HEDIT_OK) {
    (void)hipFree(buf);
    return rc;
  }
  hedit_unet_context* cx = new hedit_unet_context();
  cx->owner = h; cx->B = B; cx->buf = buf;
  cx->ctxb = g.ctxb; cx->k2_all = g.k2_all; cx->vt2_all = g.vt2_all;
  *out = cx;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

void hedit_unet_context_destroy(hedit_unet_context* cx) try {
  if (!cx) return;
  (void)hipFree(cx->buf);      // (waits for the device: no launch that reads it is left)
  delete cx;
} catch (...) { (void)hedit_abi_catch(); }

static int context_checks(const hedit_unet* h, const hedit_unet_context* cx, int B) {
  ARG_CHECK(cx, "null context");
  ARG_CHECK(cx->owner == h, "the context was created on another UNet handle");
  ARG_CHECK(cx->B == B, "the context was created for another number of rows");
  ARG_CHECK(!h->hook, "an attention hook takes the fp32 context rows (hedit_unet_forward)");
  return HEDIT_OK;
}

int hedit_unet_forward_bound(hedit_unet* h, const float* x, float t, const hedit_unet_context* cx, int B, int height, int width,
                             const hedit_p2p_plan* plan, float* eps_out, void* workspace, size_t workspace_bytes,
                             void* stream) try {
  TRY(forward_checks(h, x, cx, B, height, width, plan, eps_out, workspace));
  TRY(context_checks(h, cx, B));
  return forward_impl(h, x, t, nullptr, B, height, width, plan, eps_out, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream), false, nullptr, 0, nullptr, cx);
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_forward_shared_bound(hedit_unet* h, const float* x, int D, const int* row_latent, float t,
                                    const hedit_unet_context* cx, int B, int height, int width, const hedit_p2p_plan* plan,
                                    float* eps_out, void* workspace, size_t workspace_bytes, void* stream) try {
  TRY(forward_checks(h, x, cx, B, height, width, plan, eps_out, workspace));
  TRY(context_checks(h, cx, B));
  RowMap map{};
  TRY(row_map_checks(x, D, row_latent, B, &map));
  return forward_impl(h, x, t, nullptr, B, height, width, plan, eps_out, workspace, workspace_bytes,
                      reinterpret_cast<hipStream_t>(stream), false, nullptr, D, &map, cx);
} catch (...) { return hedit_abi_catch(); }

// ---- input gradient (unetgrad.h)
size_t hedit_unet_grad_workspace_bytes(hedit_unet* h, int B, int height, int width) try {
  if (!h || !h->grad || check_grad_shape(h, B, height, width) != HEDIT_OK) return 0;
  GradTape T;
  tape_init(T, h, B, height, width, nullptr, 0, nullptr, true);
  float dummy = 0.f;   // never dereferenced in the dry run
  int rc = forward_keep_impl(h, T, nullptr, 0.f, nullptr, nullptr);
  if (rc == HEDIT_OK) rc = backward_impl(h, T, &dummy, &dummy);
  if (h->wkv2_t) {      // the arena's peak is the largest of the three walks a context handle can be asked for
    if (rc == HEDIT_OK) rc = backward_impl(h, T, &dummy, &dummy, &dummy);
    if (rc == HEDIT_OK) rc = backward_impl(h, T, &dummy, nullptr, &dummy);
  }
  return dry_run_bytes(rc, T.f.ar.peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

int hedit_unet_forward_keep(hedit_unet* h, const float* x, float t, const float* ctx, int B, int height, int width, float* eps,
                            void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && x && ctx && eps && workspace, "null");
  TRY(check_grad_shape(h, B, height, width));
  TRY(check_grad_handle(h, "hedit_unet_forward_keep"));
  drop_tape(h);
  GradTape* T = new GradTape();
  tape_init(*T, h, B, height, width, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false);
  const int rc = forward_keep_impl(h, *T, x, t, ctx, eps);
  if (rc != HEDIT_OK) {
    delete T;
    return rc;
  }
  h->tape = T;
  h->tape_free = [](void* p) { delete reinterpret_cast<GradTape*>(p); };
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_backward(hedit_unet* h, const float* d_eps, float* d_x, void* workspace, void* stream) try {
  ARG_CHECK(h && d_eps && d_x && workspace, "null");
  TRY(check_grad_handle(h, "hedit_unet_backward"));
  if (!h->tape) {
    hedit_set_error("hedit_unet_backward: no forward is being kept (call hedit_unet_forward_keep first)");
    return HEDIT_ERR_STATE;
  }
  GradTape* T = reinterpret_cast<GradTape*>(h->tape);
  if (T->ws != workspace) {
    hedit_set_error("hedit_unet_backward: not the workspace the kept forward ran in");
    return HEDIT_ERR_ARG;
  }
  T->f.st = reinterpret_cast<hipStream_t>(stream);
  const int rc = backward_impl(h, *T, d_eps, d_x);
  if (rc != HEDIT_OK) drop_tape(h);   // a pass that stopped half way leaves temporaries in the arena
  return rc;
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_backward_ctx(hedit_unet* h, const float* d_eps, float* d_x, float* d_ctx, void* workspace, void* stream) try {
  ARG_CHECK(h && d_eps && d_ctx && workspace, "null");
  TRY(check_grad_handle(h, "hedit_unet_backward_ctx"));
  if (!h->wkv2_t) {
    hedit_set_error("hedit_unet_backward_ctx: this handle has no context-gradient weights (create it with hedit_unet_create_grad_ctx)");
    return HEDIT_ERR_STATE;
  }
  if (!h->tape) {
    hedit_set_error("hedit_unet_backward_ctx: no forward is being kept (call hedit_unet_forward_keep first)");
    return HEDIT_ERR_STATE;
  }
  GradTape* T = reinterpret_cast<GradTape*>(h->tape);
  if (T->ws != workspace) {
    hedit_set_error("hedit_unet_backward_ctx: not the workspace the kept forward ran in");
    return HEDIT_ERR_ARG;
  }
  T->f.st = reinterpret_cast<hipStream_t>(stream);
  const int rc = backward_impl(h, *T, d_eps, d_x, d_ctx);
  if (rc != HEDIT_OK) drop_tape(h);   // a pass that stopped half way leaves temporaries in the arena
  return rc;
} catch (...) { return hedit_abi_catch(); }

void hedit_unet_release(hedit_unet* h) try {
  if (h) drop_tape(h);
} catch (...) { (void)hedit_abi_catch(); }

int hedit_unet_vjp(hedit_unet* h, const float* x, float t, const float* ctx, const float* d_eps, int B, int height, int width,
                   float* d_x, float* eps, void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && x && ctx && d_eps && d_x && eps && workspace, "null");
  TRY(check_grad_shape(h, B, height, width));
  TRY(check_grad_handle(h, "hedit_unet_vjp"));
  drop_tape(h);
  GradTape T;
  tape_init(T, h, B, height, width, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false);
  TRY(forward_keep_impl(h, T, x, t, ctx, eps));
  return backward_impl(h, T, d_eps, d_x);
} catch (...) { return hedit_abi_catch(); }

int hedit_prof_enable(hedit_unet* h, int on, int max_records) try {
  ARG_CHECK(h, "null");
  if (on && (int)h->prof_pool.size() < 2 * max_records) {
    const size_t want = (size_t)2 * max_records;
    while (h->prof_pool.size() < want) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      h->prof_pool.push_back(e);
    }
  }
  h->prof_on = on != 0;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_prof_reset(hedit_unet* h) try {
  ARG_CHECK(h, "null");
  h->prof_recs.clear();
  h->prof_next = 0;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* call after the stream has been synchronised */
int hedit_prof_collect(hedit_unet* h, int kind, double* total_ms, double* total_flops, int64_t* count) try {
  ARG_CHECK(h && total_ms && total_flops && count && kind >= 0 && kind < PK_COUNT, "prof args");
  double ms = 0, fl = 0;
  int64_t n = 0;
  for (auto& r : h->prof_recs) {
    if (r.kind != kind) continue;
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->prof_pool[r.e0], h->prof_pool[r.e1]));
    ms += t;
    fl += r.flops;
    ++n;
  }
  *total_ms = ms; *total_flops = fl; *count = n;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* one row per sampled launch, in launch order: kind, ms, flops, bytes, M, N, K, tag (GEMM launches: mode | 8 geglu |
   16 residual | 32 split-K | 64 chunked); call after the stream has been synchronised */
int hedit_prof_records(hedit_unet* h, double* rows, int max_rows, int* n_rows) try {
  ARG_CHECK(h && rows && n_rows && max_rows >= 0, "prof args");
  int n = 0;
  for (auto& r : h->prof_recs) {
    if (n >= max_rows) break;
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->prof_pool[r.e0], h->prof_pool[r.e1]));
    double* o = rows + (size_t)n * 8;
    o[0] = r.kind; o[1] = t; o[2] = r.flops; o[3] = r.bytes; o[4] = r.m; o[5] = r.n; o[6] = r.k; o[7] = r.tag;
    ++n;
  }
  *n_rows = n;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

/* algorithmic HBM bytes (operands read once, results written once) of the sampled launches of a class */
int hedit_prof_collect_bytes(hedit_unet* h, int kind, double* total_bytes) try {
  ARG_CHECK(h && total_bytes && kind >= 0 && kind < PK_COUNT, "prof args");
  double b = 0;
  for (auto& r : h->prof_recs)
    if (r.kind == kind) b += r.bytes;
  *total_bytes = b;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

static void store_layers(const hedit_unet* h, int height, int width, std::vector<std::pair<int, int>>& v) {
  const hedit_unet_cfg& c = h->cfg;
  int H = height, W = width;
  for (int i = 0; i < c.n_levels; ++i) {
    if (c.down_has_attn[i])
      for (int j = 0; j < c.layers_per_block; ++j)
        if (H * W <= 1024) v.push_back({H * W, 0});
    if (i != c.n_levels - 1) { H /= 2; W /= 2; }
  }
  if (H * W <= 1024) v.push_back({H * W, 1});
  for (int i = 0; i < c.n_levels; ++i) {
    if (c.up_has_attn[i])
      for (int j = 0; j < c.layers_per_block + 1; ++j)
        if (H * W <= 1024) v.push_back({H * W, 2});
    if (i != c.n_levels - 1) { H *= 2; W *= 2; }
  }
}

int hedit_unet_set_attn_hook(hedit_unet* h, hedit_attn_hook_fn fn, void* user) try {
  ARG_CHECK(h, "unet handle");
  h->hook = fn;
  h->hook_user = fn ? user : nullptr;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_num_store_layers(const hedit_unet* h, int height, int width) try {
  if (!h) return 0;
  std::vector<std::pair<int, int>> v;
  store_layers(h, height, width, v);
  return (int)v.size();
} catch (...) { return hedit_abi_catch(); }

int hedit_unet_store_layer_info(const hedit_unet* h, int height, int width, int i, int* tokens, int* place) try {
  ARG_CHECK(h && tokens && place, "null");
  std::vector<std::pair<int, int>> v;
  store_layers(h, height, width, v);
  ARG_CHECK(i >= 0 && i < (int)v.size(), "layer index");
  *tokens = v[i].first;
  *place = v[i].second;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
