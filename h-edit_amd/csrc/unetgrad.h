// Input gradient of the SD UNet: d_x = (d eps / d x)^T d_eps for a plain pass (no plan, no hook), what Noise Map Guidance
// differentiates (text-guided/inversion/p2p_baselines.py:195-293).  Included by unet.hip behind forward_impl; the pixel
// UNet's ddpm.hip::forward_keep_impl / backward_impl is the precedent.
//
// hedit_unet_forward_keep runs the network through the UNFUSED kernels at every width (the chain kernels of the C = 320 level
// keep nothing a backward could use) and records every block: a taped block takes its own GroupNorm statistics, a transformer
// block keeps the inputs of its three LayerNorms, q | k, a row-major V, both attention outputs, the cross-attention query and
// the FF1 pre-activation.  hedit_unet_backward walks the records in reverse; its temporaries go above / between the kept
// buffers and are freed again, so any number of backward passes can follow one forward.  hedit_unet_backward gives the
// gradient with respect to x only.  hedit_unet_backward_ctx (a hedit_unet_create_grad_ctx handle) also forms dK / dV of every
// cross-attention (attnbwd.hip, the context form) into the block's column slice of one [B*80][2 ctx_n] buffer [dK_all | dV_all],
// and after the walk d_ctx = [dK_all | dV_all] [wk2_all | wv2_all] as one fp32 GEMM chain per element.  The forward is the same
// for both; nothing for the timestep or the weights.
#pragma once

namespace {

struct ResTape {
  const Res* r;
  const bf16_t* x;
  bf16_t* h1;
  float *st1, *st2;
  int H, W;
};
struct AttnTape {
  const Attn* a;
  const bf16_t* x;          // the block's input (GroupNorm input and last residual)
  float* st;                // its GroupNorm statistics
  bf16_t *t0, *qk, *v, *ao1, *t1, *q2, *ao2, *t2, *pre;
  int H, W;
};
struct BlkRec {
  ResTape r{};
  AttnTape a{};
  bool has_attn = false;
  int left = 0, right = 0;     // up path: columns of the concatenation [previous block | skip]
};
struct SkipRec { bf16_t* p; int ch, H, W; };
struct GradTape {
  Fwd f;
  std::vector<SkipRec> hs;               // every tensor the down path pushed, in order
  std::vector<BlkRec> down, up;          // in execution order
  ResTape m1{}, m2{};
  AttnTape ma{};
  bf16_t* x_out = nullptr;               // input of conv_norm_out
  float* st_out = nullptr;
  const bf16_t* v2_all = nullptr;        // [B*80][ctx_n]: attn2 values of every block, row-major (the backward's form)
  int B = 0, H = 0, W = 0, H0 = 0, W0 = 0;
  void* ws = nullptr;
};

void tape_init(GradTape& T, hedit_unet* h, int B, int H0, int W0, void* ws, size_t ws_bytes, hipStream_t st, bool dry) {
  T.f = Fwd{};
  T.f.h = h; T.f.B = B; T.f.st = st; T.f.plan = nullptr; T.f.temb_all = nullptr; T.f.ctxb = nullptr;
  T.f.ar.dry = dry;
  T.f.ar.base = reinterpret_cast<char*>(ws);
  T.f.ar.cap = ws_bytes;
  T.B = B; T.H0 = H0; T.W0 = W0; T.ws = ws;
}

// GroupNorm that keeps (mean, rstd) [B][G][2] for its backward
int groupnorm_keep(Fwd& f, const bf16_t* x, bf16_t* y, const float* g, const float* b, int HW, int C, float eps, int silu, float** stats) {
  float *sb, *ws;
  TRY(aalloc(f, &sb, (size_t)f.B * 64 * 2));
  TRY(aalloc(f, &ws, groupnorm_ws_bytes(f.B, HW, C) / sizeof(float)));
  RUN(f, groupnorm_launch(x, y, g, b, f.B, HW, C, f.h->cfg.norm_num_groups, eps, silu, ws, f.st, sb));
  f.ar.free(ws);
  *stats = sb;
  return HEDIT_OK;
}

int groupnorm_bwd(Fwd& f, const bf16_t* x, const bf16_t* dy, const bf16_t* add, bf16_t* dx, const float* g, const float* b,
                  const float* stats, int HW, int C, int silu) {
  float* ws;
  TRY(aalloc(f, &ws, groupnorm_bwd_ws_bytes(f.B, HW, C) / sizeof(float)));
  RUN(f, groupnorm_bwd_launch(x, dy, add, dx, g, b, stats, f.B, HW, C, f.h->cfg.norm_num_groups, silu, ws, f.st, true));
  f.ar.free(ws);
  return HEDIT_OK;
}

// x [M][cin] -> *out [M][cout] (allocated here; x is NOT freed)
int resblock_keep(Fwd& f, const Res& r, const bf16_t* x, int H, int W, bf16_t** out, ResTape* rec) {
  const size_t M = (size_t)f.B * H * W;
  bf16_t *a1, *h1, *a2, *sc = nullptr, *y;
  TRY(aalloc(f, &h1, M * r.cout));
  *rec = ResTape{&r, x, h1, nullptr, nullptr, H, W};
  TRY(aalloc(f, &a1, M * r.cin));
  TRY(groupnorm_keep(f, x, a1, r.n1g, r.n1b, H * W, r.cin, 1e-5f, 1, &rec->st1));
  TRY(conv3x3(f, a1, H, W, r.cin, r.conv1, r.cout, f.temb_all + r.temb_off, nullptr, h1, 1));
  f.ar.free(a1);
  TRY(aalloc(f, &a2, M * r.cout));
  TRY(groupnorm_keep(f, h1, a2, r.n2g, r.n2b, H * W, r.cout, 1e-5f, 1, &rec->st2));
  const bf16_t* res = x;
  if (r.sc_w) {
    TRY(aalloc(f, &sc, M * r.cout));
    TRY(linear(f, x, (int)M, r.cin, r.sc_w, r.cout, r.sc_b, nullptr, sc, r.cout));
    res = sc;
  }
  TRY(aalloc(f, &y, M * r.cout));
  TRY(conv3x3(f, a2, H, W, r.cout, r.conv2, r.cout, r.conv2_b, res, y, 1));
  f.ar.free(a2);
  if (sc) f.ar.free(sc);
  *out = y;
  return HEDIT_OK;
}

// dy [M][cout] -> *dx [M][cin] (allocated here; dy is NOT freed)
int resblock_bwd(Fwd& f, const ResTape& rec, const bf16_t* dy, bf16_t** dx_out) {
  const Res& r = *rec.r;
  const int H = rec.H, W = rec.W;
  const size_t M = (size_t)f.B * H * W;
  bf16_t *da2, *dh1, *da1, *dsc = nullptr, *dx;
  TRY(aalloc(f, &da2, M * r.cout));
  TRY(conv3x3(f, dy, H, W, r.cout, r.conv2_t, r.cout, nullptr, nullptr, da2, 1));
  TRY(aalloc(f, &dh1, M * r.cout));
  TRY(groupnorm_bwd(f, rec.h1, da2, nullptr, dh1, r.n2g, r.n2b, rec.st2, H * W, r.cout, 1));
  f.ar.free(da2);
  TRY(aalloc(f, &da1, M * r.cin));
  TRY(conv3x3(f, dh1, H, W, r.cout, r.conv1_t, r.cin, nullptr, nullptr, da1, 1));
  f.ar.free(dh1);
  const bf16_t* add = dy;
  if (r.sc_w) {
    TRY(aalloc(f, &dsc, M * r.cin));
    TRY(linear(f, dy, (int)M, r.cout, r.sc_t, r.cin, nullptr, nullptr, dsc, r.cin));
    add = dsc;
  }
  TRY(aalloc(f, &dx, M * r.cin));
  TRY(groupnorm_bwd(f, rec.x, da1, add, dx, r.n1g, r.n1b, rec.st1, H * W, r.cin, 1));
  f.ar.free(da1);
  if (dsc) f.ar.free(dsc);
  *dx_out = dx;
  return HEDIT_OK;
}

// The transformer block of transformer_stem / transformer_rest through the unfused kernels, every residual kept.
// x [M][C] -> *out [M][C] (allocated here; x is NOT freed)
int transformer_keep(Fwd& f, const Attn& a, const bf16_t* x, int H, int W, bf16_t** out, AttnTape* rec) {
  const int C = a.C, N = H * W, B = f.B, heads = f.h->cfg.heads, d = C / heads;
  const size_t M = (size_t)B * N;
  const int MC = B * HEDIT_CTXP;
  AttnTape t{};
  t.a = &a; t.x = x; t.H = H; t.W = W;
  bf16_t *xn, *tn, *vt, *gf, *t3, *y;
  // kept buffers first, so the temporaries freed below do not fragment around them
  TRY(aalloc(f, &t.t0, M * C));
  TRY(aalloc(f, &t.qk, M * 2 * C));
  TRY(aalloc(f, &t.v, M * C));
  TRY(aalloc(f, &t.ao1, M * C));
  TRY(aalloc(f, &t.t1, M * C));
  TRY(aalloc(f, &t.q2, M * C));
  TRY(aalloc(f, &t.ao2, M * C));
  TRY(aalloc(f, &t.t2, M * C));
  TRY(aalloc(f, &t.pre, M * 8 * C));
  // GroupNorm, proj_in, norm1, q | k, v
  TRY(aalloc(f, &xn, M * C));
  TRY(groupnorm_keep(f, x, xn, a.gn_g, a.gn_b, N, C, 1e-6f, 0, &t.st));
  TRY(linear(f, xn, (int)M, C, a.pin, C, a.pin_b, nullptr, t.t0, C));
  f.ar.free(xn);
  TRY(aalloc(f, &tn, M * C));
  RUN(f, layernorm_launch(t.t0, tn, a.ln1g, a.ln1b, (long)M, C, 1e-5f, f.st));
  TRY(linear(f, tn, (int)M, C, a.w_qk, 2 * C, nullptr, nullptr, t.qk, 2 * C));
  TRY(linear(f, tn, (int)M, C, a.w_v1, C, nullptr, nullptr, t.v, C));
  // the forward kernel reads V^T [C][M]
  TRY(aalloc(f, &vt, M * C));
  RUN(f, transpose_bf16_launch(t.v, vt, (int)M, C, f.st));
  {
    SelfAttnParams sp{};
    sp.q = t.qk; sp.ldq = 2 * C; sp.k = t.qk + C; sp.ldk = 2 * C; sp.vt = vt; sp.ldvt = (long)M;
    sp.out = t.ao1; sp.ldo = C; sp.B = B; sp.N = N; sp.heads = heads; sp.d = d;
    RUN(f, self_attn_launch(sp, f.st));
  }
  f.ar.free(vt);
  // attn1.to_out + residual, norm2, attn2.to_q, the cross-attention
  TRY(linear(f, t.ao1, (int)M, C, a.w_o1, C, a.o1_b, t.t0, t.t1, C));
  RUN(f, layernorm_launch(t.t1, tn, a.ln2g, a.ln2b, (long)M, C, 1e-5f, f.st));
  TRY(linear(f, tn, (int)M, C, a.w_q2, C, nullptr, nullptr, t.q2, C));
  {
    CrossAttnParams cp{};
    cp.q = t.q2; cp.ldq = C; cp.k = f.k2_all + a.ctx_off; cp.ldk = f.h->ctx_n;
    cp.vt = f.vt2_all + (size_t)a.ctx_off * MC; cp.ldvt = MC; cp.out = t.ao2; cp.ldo = C;
    cp.B = B; cp.N = N; cp.heads = heads; cp.d = d;
    cp.n_pairs = 0; cp.singles = f.h->iota; cp.n_single = B;
    RUN(f, cross_attn_launch(cp, f.st));
  }
  // attn2.to_out + residual, norm3, FF1 (pre-activation kept), GEGLU, FF2 + residual, proj_out + residual
  TRY(linear(f, t.ao2, (int)M, C, a.w_o2, C, a.o2_b, t.t1, t.t2, C));
  RUN(f, layernorm_launch(t.t2, tn, a.ln3g, a.ln3b, (long)M, C, 1e-5f, f.st));
  TRY(linear(f, tn, (int)M, C, a.ff1n, 8 * C, a.ff1_bn, nullptr, t.pre, 8 * C));
  f.ar.free(tn);
  TRY(aalloc(f, &gf, M * 4 * C));
  RUN(f, geglu_launch(t.pre, gf, (long)M, 4 * C, f.st));
  TRY(aalloc(f, &t3, M * C));
  TRY(linear(f, gf, (int)M, 4 * C, a.ff2, C, a.ff2_b, t.t2, t3, C));
  f.ar.free(gf);
  TRY(aalloc(f, &y, M * C));
  TRY(linear(f, t3, (int)M, C, a.pout, C, a.pout_b, x, y, C));
  f.ar.free(t3);
  *rec = t;
  *out = y;
  return HEDIT_OK;
}

// dy [M][C] -> *dx [M][C] (allocated here; dy is NOT freed).  v2: the tape's row-major attn2 values.
// dkv: null, or [B*80][2 ctx_n] = [dK_all | dV_all], whose column slices of this block are written.
int transformer_bwd(Fwd& f, const AttnTape& t, const bf16_t* v2_all, const bf16_t* dy, bf16_t** dx_out, bf16_t* dkv = nullptr) {
  const Attn& a = *t.a;
  const int C = a.C, N = t.H * t.W, B = f.B, heads = f.h->cfg.heads, d = C / heads;
  const size_t M = (size_t)B * N;
  const int Mi = (int)M;
  bf16_t *dt3, *dgf, *dpre, *dtn, *dt2, *dao, *dq2, *dt1, *dq, *dk, *dv, *dt0, *dxn, *dx;
  // proj_out, FF2, GEGLU, FF1, norm3 (+ the residual branch)
  TRY(aalloc(f, &dt3, M * C));
  TRY(linear(f, dy, Mi, C, a.pout_t, C, nullptr, nullptr, dt3, C));
  TRY(aalloc(f, &dgf, M * 4 * C));
  TRY(linear(f, dt3, Mi, C, a.ff2_t, 4 * C, nullptr, nullptr, dgf, 4 * C));
  TRY(aalloc(f, &dpre, M * 8 * C));
  RUN(f, geglu_bwd_launch(t.pre, dgf, dpre, (long)M, 4 * C, f.st));
  f.ar.free(dgf);
  TRY(aalloc(f, &dtn, M * C));
  TRY(linear(f, dpre, Mi, 8 * C, a.ff1_t, C, nullptr, nullptr, dtn, C));
  f.ar.free(dpre);
  TRY(aalloc(f, &dt2, M * C));
  RUN(f, layernorm_bwd_launch(t.t2, dtn, dt3, dt2, a.ln3g, (long)M, C, 1e-5f, f.st));
  f.ar.free(dt3);
  // attn2.to_out, the cross-attention's query, attn2.to_q, norm2
  TRY(aalloc(f, &dao, M * C));
  TRY(linear(f, dt2, Mi, C, a.wo2_t, C, nullptr, nullptr, dao, C));
  TRY(aalloc(f, &dq2, M * C));
  {
    AttnBwdParams p{};
    p.q = t.q2; p.ldq = C; p.k = f.k2_all + a.ctx_off; p.ldk = f.h->ctx_n; p.v = v2_all + a.ctx_off; p.ldv = f.h->ctx_n;
    p.o = t.ao2; p.ldo = C; p.dout = dao; p.lddo = C; p.dq = dq2; p.lddq = C;
    p.B = B; p.N = N; p.M = HEDIT_MAXW; p.kstride = HEDIT_CTXP; p.heads = heads; p.d = d;
    if (dkv) {
      float *st, *part;
      TRY(aalloc(f, &st, attn_bwd_ws_bytes(B, N, heads) / sizeof(float)));
      TRY(aalloc(f, &part, attn_bwd_ctx_kv_ws_bytes(B, N, heads, d) / sizeof(float)));
      p.stats = st;
      RUN(f, attn_bwd_launch(p, f.st));
      p.dk = dkv + a.ctx_off; p.dv = dkv + f.h->ctx_n + a.ctx_off; p.lddkv = 2 * f.h->ctx_n;
      RUN(f, attn_bwd_ctx_kv_launch(p, part, f.st));
      f.ar.free(part); f.ar.free(st);
    } else {
      RUN(f, attn_bwd_launch(p, f.st));
    }
  }
  TRY(linear(f, dq2, Mi, C, a.wq2_t, C, nullptr, nullptr, dtn, C));
  f.ar.free(dq2);
  TRY(aalloc(f, &dt1, M * C));
  RUN(f, layernorm_bwd_launch(t.t1, dtn, dt2, dt1, a.ln2g, (long)M, C, 1e-5f, f.st));
  f.ar.free(dt2);
  // attn1.to_out, the self-attention, q / k / v projections, norm1
  TRY(linear(f, dt1, Mi, C, a.wo1_t, C, nullptr, nullptr, dao, C));
  TRY(aalloc(f, &dq, M * C));
  TRY(aalloc(f, &dk, M * C));
  TRY(aalloc(f, &dv, M * C));
  {
    float* st;
    TRY(aalloc(f, &st, attn_bwd_ws_bytes(B, N, heads) / sizeof(float)));
    AttnBwdParams p{};
    p.q = t.qk; p.ldq = 2 * C; p.k = t.qk + C; p.ldk = 2 * C; p.v = t.v; p.ldv = C;
    p.o = t.ao1; p.ldo = C; p.dout = dao; p.lddo = C; p.dq = dq; p.lddq = C; p.dk = dk; p.dv = dv; p.lddkv = C; p.stats = st;
    p.B = B; p.N = N; p.M = N; p.kstride = N; p.heads = heads; p.d = d;
    RUN(f, attn_bwd_launch(p, f.st));
    f.ar.free(st);
  }
  // d(norm1 output) = dq Wq' + dk Wk + dv Wv, accumulated through the GEMM's residual input
  TRY(linear(f, dq, Mi, C, a.wq1_t, C, nullptr, nullptr, dao, C));
  TRY(linear(f, dk, Mi, C, a.wk1_t, C, nullptr, dao, dq, C));     // dq's buffer is free again
  TRY(linear(f, dv, Mi, C, a.wv1_t, C, nullptr, dq, dtn, C));
  f.ar.free(dv); f.ar.free(dk); f.ar.free(dq); f.ar.free(dao);
  TRY(aalloc(f, &dt0, M * C));
  RUN(f, layernorm_bwd_launch(t.t0, dtn, dt1, dt0, a.ln1g, (long)M, C, 1e-5f, f.st));
  f.ar.free(dt1); f.ar.free(dtn);
  // proj_in, GroupNorm (+ the block's residual)
  TRY(aalloc(f, &dxn, M * C));
  TRY(linear(f, dt0, Mi, C, a.pin_t, C, nullptr, nullptr, dxn, C));
  f.ar.free(dt0);
  TRY(aalloc(f, &dx, M * C));
  TRY(groupnorm_bwd(f, t.x, dxn, dy, dx, a.gn_g, a.gn_b, t.st, N, C, 0));
  f.ar.free(dxn);
  *dx_out = dx;
  return HEDIT_OK;
}

// forward_impl's network with every block recorded; block outputs are contiguous and the concatenations are copies
int forward_keep_impl(hedit_unet* h, GradTape& T, const float* x, float t, const float* ctx, float* eps_out) {
  Fwd& f = T.f;
  const int B = f.B;
  hipStream_t st = f.st;
  const hedit_unet_cfg& c = h->cfg;
  const int ch0 = c.block_out_channels[0];
  if (!f.dry() && h->iota_cap < B) {
    hedit_set_error("batch larger than " + std::to_string(h->iota_cap) + " rows");
    return HEDIT_ERR_ARG;
  }
  // text context and the attn2 keys / values of every block: K and the row-major V stay for the backward
  const int MC = B * HEDIT_CTXP;
  bf16_t *ctxb, *k2a, *v2a, *vt2a;
  TRY(aalloc(f, &k2a, (size_t)MC * h->ctx_n));
  TRY(aalloc(f, &v2a, (size_t)MC * h->ctx_n));
  TRY(aalloc(f, &vt2a, (size_t)MC * h->ctx_n));
  TRY(aalloc(f, &ctxb, (size_t)MC * c.cross_attention_dim));
  RUN(f, ctx_pad_launch(ctx, ctxb, B, c.cross_attention_dim, st));
  TRY(linear(f, ctxb, MC, c.cross_attention_dim, h->wk2_all, h->ctx_n, nullptr, nullptr, k2a, h->ctx_n));
  TRY(linear(f, ctxb, MC, c.cross_attention_dim, h->wv2_all, h->ctx_n, nullptr, nullptr, v2a, h->ctx_n));
  TRY(linear(f, h->wv2_all, h->ctx_n, c.cross_attention_dim, ctxb, MC, nullptr, nullptr, vt2a, MC, 2));
  f.ctxb = ctxb; f.k2_all = k2a; f.vt2_all = vt2a;
  T.v2_all = v2a;

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

  int H = T.H0, W = T.W0;
  bf16_t* x0;
  TRY(aalloc(f, &x0, (size_t)B * H * W * ch0));
  RUN(f, conv_in_launch(x, h->conv_in_w, h->conv_in_b, x0, B, c.in_channels, H, W, ch0, st));
  T.hs.push_back({x0, ch0, H, W});
  for (int i = 0; i < c.n_levels; ++i) {
    const Block& blk = h->down[i];
    for (size_t j = 0; j < blk.res.size(); ++j) {
      T.down.emplace_back();
      BlkRec& br = T.down.back();
      bf16_t* y;
      TRY(resblock_keep(f, blk.res[j], T.hs.back().p, H, W, &y, &br.r));
      if (blk.has_attn) {
        bf16_t* z;
        br.has_attn = true;
        TRY(transformer_keep(f, blk.attn[j], y, H, W, &z, &br.a));      // y stays: the transformer's input
        y = z;
      }
      T.hs.push_back({y, blk.ch, H, W});
    }
    if (blk.has_sampler) {
      bf16_t* y;
      TRY(aalloc(f, &y, (size_t)B * (H / 2) * (W / 2) * blk.ch));
      TRY(conv3x3(f, T.hs.back().p, H, W, blk.ch, blk.samp_w, blk.ch, blk.samp_b, nullptr, y, 2));
      H /= 2; W /= 2;
      T.hs.push_back({y, blk.ch, H, W});
    }
  }
  bf16_t *m1, *m2, *cur;
  int cur_c = T.hs.back().ch;
  TRY(resblock_keep(f, h->mid_res[0], T.hs.back().p, H, W, &m1, &T.m1));
  TRY(transformer_keep(f, h->mid_attn, m1, H, W, &m2, &T.ma));
  TRY(resblock_keep(f, h->mid_res[1], m2, H, W, &cur, &T.m2));
  size_t k = T.hs.size();
  for (int i = 0; i < c.n_levels; ++i) {
    const Block& blk = h->up[i];
    for (size_t j = 0; j < blk.res.size(); ++j) {
      const SkipRec& s = T.hs[--k];
      T.up.emplace_back();
      BlkRec& br = T.up.back();
      br.left = cur_c; br.right = s.ch;
      const size_t M = (size_t)B * H * W;
      bf16_t *cat, *y;
      TRY(aalloc(f, &cat, M * (cur_c + s.ch)));                // stays: the block's input
      RUN(f, concat_launch(cur, cur_c, s.p, s.ch, cat, (long)M, st));
      f.ar.free(cur);                                          // a block's output is nobody's record
      TRY(resblock_keep(f, blk.res[j], cat, H, W, &y, &br.r));
      if (blk.has_attn) {
        bf16_t* z;
        br.has_attn = true;
        TRY(transformer_keep(f, blk.attn[j], y, H, W, &z, &br.a));
        y = z;
      }
      cur = y;
      cur_c = blk.ch;
    }
    if (blk.has_sampler) {
      bf16_t* y;
      TRY(aalloc(f, &y, (size_t)B * H * W * 4 * cur_c));
      TRY(conv3x3(f, cur, H, W, cur_c, blk.samp_w, cur_c, blk.samp_b, nullptr, y, 3));
      f.ar.free(cur);     // linear in its input: nothing to keep
      cur = y;
      H *= 2; W *= 2;
    }
  }
  {
    bf16_t* a;
    TRY(aalloc(f, &a, (size_t)B * H * W * ch0));
    TRY(groupnorm_keep(f, cur, a, h->gn_out_g, h->gn_out_b, H * W, ch0, 1e-5f, 1, &T.st_out));
    if (c.out_channels != 4 || ch0 % 64 != 0) {
      RUN(f, conv_out_launch(a, h->conv_out_w, h->conv_out_b, eps_out, B, H, W, ch0, c.out_channels, st));
    } else {
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
  }
  // only the forward read these
  f.ar.free(temb_all); f.ar.free(te2); f.ar.free(te1); f.ar.free(te0);
  f.ar.free(ctxb); f.ar.free(vt2a);
  f.temb_all = nullptr; f.ctxb = nullptr; f.vt2_all = nullptr;
  T.x_out = cur;
  T.H = H; T.W = W;
  return HEDIT_OK;
}

// d [M][ch] += pending gradient of the same skip tensor (fp32 add, one rounding), which is then released
int add_pending(Fwd& f, bf16_t* d, bf16_t*& pend, const SkipRec& s) {
  if (!pend) return HEDIT_OK;
  RUN(f, slice_add_launch(pend, s.ch, 0, s.ch, d, (long)f.B * s.H * s.W, 1, f.st));
  f.ar.free(pend);
  pend = nullptr;
  return HEDIT_OK;
}

int block_bwd(Fwd& f, const GradTape& T, const BlkRec& br, bf16_t** d, bf16_t* dkv = nullptr, bool attn_only = false) {
  bf16_t* dx;
  if (br.has_attn) {
    TRY(transformer_bwd(f, br.a, T.v2_all, *d, &dx, dkv));
    f.ar.free(*d);
    *d = dx;
  }
  if (attn_only) return HEDIT_OK;
  TRY(resblock_bwd(f, br.r, *d, &dx));
  f.ar.free(*d);
  *d = dx;
  return HEDIT_OK;
}

// d_x = (d eps / d x)^T d_eps from a tape made by forward_keep_impl; the tape is left as it was.  d_ctx (or null): also
// (d eps / d ctx)^T d_eps, fp32 [B][77][cross_attention_dim]; d_x may then be null, and the walk ends above the first
// transformer block of the down path (its ResBlock and conv_in feed d_x alone).
int backward_impl(hedit_unet* h, GradTape& T, const float* d_eps, float* d_x, float* d_ctx = nullptr) {
  Fwd& f = T.f;
  bf16_t* dkv = nullptr;
  const int MC = f.B * HEDIT_CTXP;
  if (d_ctx) TRY(aalloc(f, &dkv, (size_t)MC * 2 * h->ctx_n));
  const int B = f.B;
  hipStream_t st = f.st;
  const hedit_unet_cfg& c = h->cfg;
  const int n = c.n_levels, ch0 = c.block_out_channels[0];
  int H = T.H, W = T.W;
  bf16_t *d, *t;
  // conv_out, conv_norm_out (+ SiLU)
  TRY(aalloc(f, &t, (size_t)B * H * W * ch0));
  RUN(f, conv_in_launch(d_eps, h->conv_out_t, h->zero_bias, t, B, c.out_channels, H, W, ch0, st));
  TRY(aalloc(f, &d, (size_t)B * H * W * ch0));
  TRY(groupnorm_bwd(f, T.x_out, t, nullptr, d, h->gn_out_g, h->gn_out_b, T.st_out, H * W, ch0, 1));
  f.ar.free(t);
  // up path, last executed level first.  Each block's input gradient splits into the part that continues down the up path
  // (left columns) and the pending gradient of its skip tensor (right columns).
  std::vector<bf16_t*> pend(T.hs.size(), nullptr);      // pend[k]: of T.hs[k] (the last executed block took hs[0])
  size_t ui = T.up.size(), k = 0;
  for (int i = n - 1; i >= 0; --i) {
    const Block& blk = h->up[i];
    if (blk.has_sampler) {
      // d(2x upsample + conv) = dgrad conv at the high resolution, then 2x2 block sums
      bf16_t *du, *dx;
      TRY(aalloc(f, &du, (size_t)B * H * W * blk.ch));
      TRY(conv3x3(f, d, H, W, blk.ch, blk.samp_t, blk.ch, nullptr, nullptr, du, 1));
      f.ar.free(d);
      H /= 2; W /= 2;
      TRY(aalloc(f, &dx, (size_t)B * H * W * blk.ch));
      RUN(f, sum2x2_launch(du, dx, B, H, W, blk.ch, st));
      f.ar.free(du);
      d = dx;
    }
    for (size_t j = blk.res.size(); j-- > 0;) {
      const BlkRec& br = T.up[--ui];
      TRY(block_bwd(f, T, br, &d, dkv));            // d: [M][left + right]
      const long M = (long)B * H * W;
      const int ld = br.left + br.right;
      bf16_t* dl;
      TRY(aalloc(f, &dl, (size_t)M * br.left));
      TRY(aalloc(f, &pend[k], (size_t)M * br.right));
      RUN(f, slice_add_launch(d, ld, 0, br.left, dl, M, 0, st));
      RUN(f, slice_add_launch(d, ld, br.left, br.right, pend[k], M, 0, st));
      f.ar.free(d);
      d = dl;
      ++k;
    }
  }
  // middle: its input is the last skip tensor, whose other gradient is pending from the first up block
  {
    bf16_t* dx;
    TRY(resblock_bwd(f, T.m2, d, &dx));
    f.ar.free(d);
    TRY(transformer_bwd(f, T.ma, T.v2_all, dx, &d, dkv));
    f.ar.free(dx);
    TRY(resblock_bwd(f, T.m1, d, &dx));
    f.ar.free(d);
    d = dx;
  }
  k = T.hs.size() - 1;
  TRY(add_pending(f, d, pend[k], T.hs[k]));
  // down path: the consumer on the down path first, then the pending gradient of the up path
  size_t di = T.down.size();
  long stop = -1;                 // without d_x: the first executed block with a transformer is the last one visited
  if (!d_x) {
    stop = (long)T.down.size();
    for (size_t j = 0; j < T.down.size(); ++j)
      if (T.down[j].has_attn) { stop = (long)j; break; }
  }
  bool done = !d_x && stop == (long)T.down.size();      // no transformer on the down path at all
  for (int i = n - 1; i >= 0 && !done; --i) {
    const Block& blk = h->down[i];
    if (blk.has_sampler) {
      --k;
      const SkipRec& s = T.hs[k];
      bf16_t* dx;
      TRY(aalloc(f, &dx, (size_t)B * s.H * s.W * blk.ch));
      RUN(f, conv3x3_s2_dgrad_pad1_launch(d, blk.samp_t, dx, B, s.H, s.W, blk.ch, blk.ch, st));
      f.ar.free(d);
      d = dx;
      TRY(add_pending(f, d, pend[k], s));
    }
    for (size_t j = blk.res.size(); j-- > 0 && !done;) {
      --di;
      done = (long)di == stop;
      TRY(block_bwd(f, T, T.down[di], &d, dkv, done));
      if (done) break;
      --k;
      TRY(add_pending(f, d, pend[k], T.hs[k]));
    }
  }
  if (done)
    for (bf16_t*& q : pend)
      if (q) { f.ar.free(q); q = nullptr; }
  // conv_in: the N = 4 route of the head convolution with the flipped, transposed weight
  if (d_x) {
    float* prod;
    const size_t M = (size_t)B * T.H0 * T.W0;
    TRY(aalloc(f, &prod, M * 4));
    GemmParams p{};
    p.mode = 1; p.Hin = T.H0; p.Win = T.W0; p.Cin = ch0; p.Hout = T.H0; p.Wout = T.W0;
    p.A = d; p.W = h->conv_in_t; p.M = (int)M; p.N = 4; p.K = 9 * ch0; p.lda = ch0; p.raw_f32 = prod; p.ldc = 4;
    TRY(run_gemm(f, p));
    RUN(f, rows_to_nchw_launch(prod, nullptr, d_x, B, (long)T.H0 * T.W0, 4, c.in_channels, st));
    f.ar.free(prod);
  }
  f.ar.free(d);
  if (d_ctx) {
    // d_ctx = dK_all wk2_all + dV_all wv2_all: K = 2 ctx_n in one fp32 chain (raw products: no split, no 16-bit rounding)
    const int dim = h->cfg.cross_attention_dim;
    float* prod;
    TRY(aalloc(f, &prod, (size_t)MC * dim));
    GemmParams p{};
    p.mode = 0; p.A = dkv; p.W = h->wkv2_t; p.M = MC; p.N = dim; p.K = 2 * h->ctx_n; p.lda = 2 * h->ctx_n; p.raw_f32 = prod; p.ldc = dim;
    TRY(run_gemm(f, p));
    if (!f.dry())
      HIP_TRY(hipMemcpy2DAsync(d_ctx, (size_t)HEDIT_MAXW * dim * sizeof(float), prod, (size_t)HEDIT_CTXP * dim * sizeof(float),
                               (size_t)HEDIT_MAXW * dim * sizeof(float), (size_t)f.B, hipMemcpyDeviceToDevice, st));
    f.ar.free(prod);
    f.ar.free(dkv);
  }
  return HEDIT_OK;
}

int check_grad_handle(hedit_unet* h, const char* who) {
  if (!h->grad) {
    hedit_set_error(std::string(who) + ": this handle has no input-gradient weights (create it with hedit_unet_create_grad)");
    return HEDIT_ERR_STATE;
  }
  TRY(store_require_loaded(h, "UNet"));
  if (h->hook) {
    hedit_set_error(std::string(who) + ": the gradient is that of the plain network; clear the attention hook first");
    return HEDIT_ERR_STATE;
  }
  return HEDIT_OK;
}

int check_grad_shape(const hedit_unet* h, int B, int height, int width) {
  ARG_CHECK(B >= 1, "B");
  const int div = 1 << (h->cfg.n_levels - 1);
  ARG_CHECK(height >= div && width >= div && height % div == 0 && width % div == 0, "latent size must be divisible by 2^(levels-1)");
  ARG_CHECK(((height / div) * (width / div)) % 64 == 0, "lowest-resolution level must have a multiple of 64 tokens");
  return HEDIT_OK;
}

void drop_tape(hedit_unet* h) {
  if (h->tape && h->tape_free) h->tape_free(h->tape);
  h->tape = nullptr;
}

}  // namespace
