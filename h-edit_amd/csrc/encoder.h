// Host side shared by the pre-LN transformer encoders (vit.hip, text.hip, clipimg.hip, dino.hip) on the kernels of
// encoder.hip and the precise GEMM of pnet.h: the block struct, its parameter registration and weight packing, the linear
// layer, LayerNorm, and the forward of one block for the forward-only encoders.  Header-only, like pnet.h; free functions
// and one struct.  What an encoder keeps to itself is its attention kernel, its embedding and its head.
#pragma once
#include "pnet.h"

namespace {

// one pre-LN block: x + out(attn(in(ln1 x))); x + proj(act(fc(ln2 x)))
struct EncBlock {
  float *ln1g, *ln1b, *ln2g, *ln2b, *win, *bin, *wo, *bo, *wfc, *bfc, *wp, *bp;
  PConv in, out, fc, proj;
};

// the state-dict names of a block's twelve parameters after its prefix, in slot order (hedit_*_param_name shows the order):
// ln1 weight, bias; fused qkv weight, bias; attention projection weight, bias; ln2 weight, bias; fc weight, bias; proj weight, bias
struct EncNames { const char* s[12]; };
constexpr EncNames CLIP_BLOCK_NAMES = {{".ln_1.weight", ".ln_1.bias", ".attn.in_proj_weight", ".attn.in_proj_bias", ".attn.out_proj.weight",
                                        ".attn.out_proj.bias", ".ln_2.weight", ".ln_2.bias", ".mlp.c_fc.weight", ".mlp.c_fc.bias",
                                        ".mlp.c_proj.weight", ".mlp.c_proj.bias"}};      // OpenAI CLIP: <prefix>transformer.resblocks.<i>

EncBlock enc_add_block(ParamStore* h, const std::string& pre, const EncNames& n, int W) {
  EncBlock k{};
  k.ln1g = vec(h, pre + n.s[0], W); k.ln1b = vec(h, pre + n.s[1], W);
  k.win = mat(h, pre + n.s[2], 3 * W, W); k.bin = vec(h, pre + n.s[3], 3 * W);
  k.wo = mat(h, pre + n.s[4], W, W); k.bo = vec(h, pre + n.s[5], W);
  k.ln2g = vec(h, pre + n.s[6], W); k.ln2b = vec(h, pre + n.s[7], W);
  k.wfc = mat(h, pre + n.s[8], 4 * W, W); k.bfc = vec(h, pre + n.s[9], 4 * W);
  k.wp = mat(h, pre + n.s[10], W, 4 * W); k.bp = vec(h, pre + n.s[11], W);
  return k;
}

// forward-only packed weight of out = x . w^T, w [O][I] (make_pconv of pnet.h also builds the input-gradient twin, which a
// forward-only encoder would never read: 0.6 GB at ViT-L/14).  transposed: w is [O][I] and the product is x [M][O] . w -> [M][I].
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

// the four packed weights of a block; fwd_only = false also builds the input-gradient operands (vit.hip's backward pass)
int enc_pack_block(ParamStore* h, EncBlock& k, int W, bool fwd_only, hipStream_t st) {
  if (fwd_only) {
    TRY(pack_fwd(h, k.in, k.win, 3 * W, W, false, st));
    TRY(pack_fwd(h, k.out, k.wo, W, W, false, st));
    TRY(pack_fwd(h, k.fc, k.wfc, 4 * W, W, false, st));
    TRY(pack_fwd(h, k.proj, k.wp, W, 4 * W, false, st));
  } else {
    TRY(make_pconv(h, k.in, k.win, nullptr, 3 * W, W, 1, 0, 0, st));
    TRY(make_pconv(h, k.out, k.wo, nullptr, W, W, 1, 0, 0, st));
    TRY(make_pconv(h, k.fc, k.wfc, nullptr, 4 * W, W, 1, 0, 0, st));
    TRY(make_pconv(h, k.proj, k.wp, nullptr, W, 4 * W, 1, 0, 0, st));
  }
  return HEDIT_OK;
}

PF make_pf(int B, void* ws, size_t ws_bytes, hipStream_t st, bool dry) {
  PF f{B, st, Arena{}};
  f.ar.dry = dry;
  f.ar.base = reinterpret_cast<char*>(ws);
  f.ar.cap = ws_bytes;
  return f;
}

// the "need" of an entry's dry run against the caller's workspace
int ws_check(const char* what, size_t need, size_t got) {
  if (got < need) {
    hedit_set_error(std::string("bad argument: ") + what + ": workspace too small (need " + std::to_string(need) + " bytes, got " +
                    std::to_string(got) + ")");
    return HEDIT_ERR_ARG;
  }
  return HEDIT_OK;
}

int ln(PF& f, const float* x, const float* g, const float* b, long rows, int W, float eps, float* y, float* stats = nullptr) {
  if (!f.dry()) TRY(enc_ln_launch(x, g, b, y, stats, rows, W, eps, f.st));
  return HEDIT_OK;
}

// the M rows of a [M][C] fp32 tensor as a split operand (op on x + q, mask from z for the *_GRAD ops) and through one linear
// layer: out raw [M][N].  dgrad: the product with the transposed weight (the input gradient; a [M][O] . w [O][I] projection)
int lin(PF& f, const float* x, int C, int op, const float* q, const float* z, const PConv& c, bool dgrad, long M, float** out) {
  bf16_t* A;
  TRY(op_split(f, x, C, op, nullptr, q, 0, z, 0, 1, 1, M, &A));
  TRY(pgemm(f, A, c, dgrad, 0, 1, 1, M, out));
  f.ar.free(A);
  return HEDIT_OK;
}

// The forward of one block for the forward-only encoders: T [M][W] (arena memory) is replaced by the block's output (T is
// freed).  act_op: the MLP's activation as the operand op of its second GEMM (P_QGELU / P_GELU, of H + bias).
// attn(qkv, bias, A) -> rc launches the caller's attention kernel on the raw qkv [M][3W] (it adds the bias on load).
// The arena is first-fit: the order of the allocs and frees below fixes every *_workspace_bytes.
template <class Attn>
int enc_block_forward(PF& f, const EncBlock& k, float*& T, long M, int W, int act_op, float eps, Attn attn) {
  float *a, *qkv, *A, *raw, *Tmid, *m, *H, *Tn;
  TRY(aalloc(f, &a, (size_t)M * W));
  TRY(ln(f, T, k.ln1g, k.ln1b, M, W, eps, a));
  TRY(lin(f, a, W, P_COPY, nullptr, nullptr, k.in, false, M, &qkv));
  f.ar.free(a);
  TRY(aalloc(f, &A, (size_t)M * W));
  if (!f.dry()) TRY(attn(qkv, k.bin, A));
  f.ar.free(qkv);
  TRY(lin(f, A, W, P_COPY, nullptr, nullptr, k.out, false, M, &raw));
  f.ar.free(A);
  TRY(aalloc(f, &Tmid, (size_t)M * W));
  if (!f.dry()) TRY(enc_add_bias_res_launch(raw, k.bo, T, Tmid, M * W, W, f.st));
  f.ar.free(raw);
  f.ar.free(T);
  TRY(aalloc(f, &m, (size_t)M * W));
  TRY(ln(f, Tmid, k.ln2g, k.ln2b, M, W, eps, m));
  TRY(lin(f, m, W, P_COPY, nullptr, nullptr, k.fc, false, M, &H));
  f.ar.free(m);
  TRY(lin(f, H, 4 * W, act_op, k.bfc, nullptr, k.proj, false, M, &raw));      // act(H + bias) as the operand op
  f.ar.free(H);
  TRY(aalloc(f, &Tn, (size_t)M * W));
  if (!f.dry()) TRY(enc_add_bias_res_launch(raw, k.bp, Tmid, Tn, M * W, W, f.st));
  f.ar.free(raw);
  f.ar.free(Tmid);
  T = Tn;
  return HEDIT_OK;
}

}  // namespace
