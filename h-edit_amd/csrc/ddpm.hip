// The pixel-space DDPM UNet of the face-swapping task as a native executor: the eps-network that
// `h_Edit_R` (reference face-swapping/inversion/h_edit_R.py:71,96,118) and the SDE inversion
// (inversion/sde_inversion.py:121) evaluate, i.e. `Model.forward(x, t)` of
// face-swapping/diffusion/diffusion.py:192-341 (blocks :27-189) -- SURVEY.md section 8 rows a21 / a22.
// Built from the blocks of blocks.h on the kernels of gemm.hip / norm.hip, like vae.hip: parameters
// by their state_dict names (`down.{i}.block.{j}.conv1.weight`, `mid.attn_1.q.weight`, ...), NHWC
// bf16 activations in a caller-provided workspace, one C call per evaluation.
//
// Architecture: sinusoidal timestep embedding ([sin|cos], diffusion.py:6-24) -> two dense layers;
// conv_in; per level `num_res_blocks` ResNet blocks (GroupNorm(32, eps 1e-6) + swish, the timestep
// projection added after conv1) each followed by a single-head spatial attention at the listed
// resolutions, stride-2 conv with (0,1,0,1) padding between levels; mid block; the mirrored up path
// with skip concatenation and 2x nearest upsample + conv; GroupNorm + swish + conv_out.
// One timestep per call (the reference always passes `ones(n) * t`).
#include "blocks.h"

namespace {

struct DLevel {
  std::vector<VRes> block;
  std::vector<VAttn> attn;      // empty, or one per block
  bf16_t* samp_w = nullptr;     // down: stride-2 conv, up: conv after the 2x upsample
  bf16_t* samp_t = nullptr;     // its input-gradient weight (hedit_ddpm_create_grad): down [I][9][O] taps in place, up taps flipped
  float* samp_b = nullptr;
  int ch = 0;
};

}  // namespace

struct HEDIT_HANDLE hedit_ddpm : ParamStore {
  hedit_ddpm_cfg cfg;
  int temb_ch = 0;
  bf16_t *t0_w = nullptr, *t1_w = nullptr;
  float *t0_b = nullptr, *t1_b = nullptr;
  float *in_w = nullptr, *in_b = nullptr;
  std::vector<DLevel> down, up;     // up[i] = the reference's up[i] (level i; executed from the last to level 0)
  VRes mid1, mid2;
  VAttn mida;
  float *no_g = nullptr, *no_b = nullptr, *out_b = nullptr;
  bf16_t* out_w = nullptr;
  // hedit_ddpm_create_grad only: input-gradient twins of the head / tail convolutions, a zero bias vector, and the
  // outstanding tape of hedit_ddpm_forward_keep (a GradTape)
  bool grad = false;
  bf16_t* in_t = nullptr;      // conv_in: bf16 [4 rows, zero beyond in_channels][9][ch] for conv_out()'s N = 4 route
  float *out_t = nullptr, *zero_bias = nullptr;
  void* tape = nullptr;
  void (*tape_free)(void*) = nullptr;
};

namespace {

// GroupNorm statistics from the producing convolutions (gnstat.h) -- default of this build, and hedit_test_set_flags bit 2
// flips it so that tests/test_gpu_gn_stats.py can compare both paths on one library
constexpr bool DDPM_GN_FUSE_DEFAULT = true;
bool ddpm_gn_fuse() { return DDPM_GN_FUSE_DEFAULT != ((hedit_test_flags() & 4) != 0); }

int forward_impl(hedit_ddpm* h, const float* x, float t, int B, float* out, void* ws, size_t ws_bytes, hipStream_t st,
                 bool dry, size_t* peak) {
  VF f{32, B, st, Arena{}};
  f.gn_fuse = ddpm_gn_fuse();
  f.ar.dry = dry;
  f.ar.base = reinterpret_cast<char*>(ws);
  f.ar.cap = ws_bytes;
  const hedit_ddpm_cfg& c = h->cfg;
  const int L = c.n_levels, nrb = c.num_res_blocks, ch = c.ch, tc = h->temb_ch;
  // timestep embedding -> dense0 -> swish -> dense1 (diffusion.py:296-300)
  float *emb, *t0, *temb;
  TRY(aalloc(f, &emb, (size_t)ch));
  TRY(aalloc(f, &t0, (size_t)tc));
  TRY(aalloc(f, &temb, (size_t)tc));
  RUN(f, timestep_embed_ddpm_launch(t, emb, ch, st));
  RUN(f, gemv_launch(h->t0_w, emb, h->t0_b, nullptr, t0, tc, ch, 0, st));
  RUN(f, gemv_launch(h->t1_w, t0, h->t1_b, nullptr, temb, tc, tc, 1, st));

  int H = c.image_size, W = c.image_size;
  // st: the tensor's GroupNorm pair statistics, taken by the convolution that produced it (gnstat.h), or nullptr: every
  // GroupNorm whose input carries them skips its own statistics pass over the tensor
  struct Skip { bf16_t* p; int ch; float* st; };
  std::vector<Skip> hs;
  auto stat_of = [](const Skip& s) { return GnStat{s.st, s.ch, nullptr, 0}; };
  bf16_t* x0;
  TRY(aalloc(f, &x0, (size_t)B * H * W * ch));
  RUN(f, conv_in_launch(x, h->in_w, h->in_b, x0, B, c.in_channels, H, W, ch, st));
  hs.push_back({x0, ch, nullptr});
  for (int i = 0; i < L; ++i) {
    const DLevel& lv = h->down[i];
    for (int j = 0; j < nrb; ++j) {
      bf16_t* y;
      float* yst = nullptr;
      const GnStat xs = stat_of(hs.back());
      TRY(resblock(f, lv.block[j], hs.back().p, H, W, &y, nullptr, temb, nullptr, 0, &xs, &yst));
      if (!lv.attn.empty()) {
        bf16_t* a;
        TRY(attention(f, lv.attn[j], y, H, W, &a));
        f.ar.free(y);
        if (yst) f.ar.free(yst);
        yst = nullptr;
        y = a;
      }
      hs.push_back({y, lv.ch, yst});
    }
    if (lv.samp_w) {
      bf16_t* y;
      float* yst = nullptr;
      TRY(aalloc(f, &y, (size_t)B * (H / 2) * (W / 2) * lv.ch));
      if (gn_stats_shape(f, (H / 2) * (W / 2), lv.ch)) TRY(aalloc(f, &yst, (size_t)B * (H / 2) * (W / 2) / 128 * lv.ch));
      TRY(conv3x3(f, hs.back().p, H, W, lv.ch, lv.samp_w, lv.ch, lv.samp_b, nullptr, y, 2, 0, yst));
      H /= 2; W /= 2;
      hs.push_back({y, lv.ch, yst});
    }
  }
  // middle (the last skip stays on the stack: it is popped by the first up block)
  bf16_t *m1, *m2, *cur;
  float* cur_st = nullptr;
  int cur_ch = hs.back().ch;
  {
    const GnStat xs = stat_of(hs.back());
    TRY(resblock(f, h->mid1, hs.back().p, H, W, &m1, nullptr, temb, nullptr, 0, &xs));
  }
  TRY(attention(f, h->mida, m1, H, W, &m2));
  f.ar.free(m1);
  TRY(resblock(f, h->mid2, m2, H, W, &cur, nullptr, temb, nullptr, 0, nullptr, &cur_st));
  f.ar.free(m2);
  // up path.  As in unet.hip, the block that produces `cur` writes it straight into the left columns of the next
  // concatenation buffer; only the skip half is copied.
  bool in_cat = false;
  for (int i = L - 1; i >= 0; --i) {
    const DLevel& lv = h->up[i];
    for (int j = 0; j < nrb + 1; ++j) {
      const Skip s = hs.back();
      hs.pop_back();
      bf16_t *cat, *y;
      const size_t M = (size_t)B * H * W;
      if (in_cat) {
        cat = cur;
        RUN(f, concat_launch(nullptr, cur_ch, s.p, s.ch, cat, (long)M, st));
      } else {
        TRY(aalloc(f, &cat, M * (cur_ch + s.ch)));
        RUN(f, concat_launch(cur, cur_ch, s.p, s.ch, cat, (long)M, st));
        f.ar.free(cur);
      }
      f.ar.free(s.p);
      const bool to_cat = j < nrb;          // the next consumer is the next block of this level
      bf16_t* dst = nullptr;
      int ldd = 0;
      if (to_cat) {
        ldd = lv.ch + hs.back().ch;
        TRY(aalloc(f, &dst, M * ldd));
      }
      // statistics of the concatenation = the pairs of its two producers (both or nothing)
      const GnStat xs = (cur_st && s.st) ? GnStat{cur_st, cur_ch, s.st, s.ch} : GnStat{};
      // the output's statistics, unless its consumer is the upsampling convolution
      const bool want_st = !(j == nrb && lv.samp_w);
      float* yst = nullptr;
      if (!lv.attn.empty()) {
        TRY(resblock(f, lv.block[j], cat, H, W, &y, nullptr, temb, nullptr, 0, &xs));
        f.ar.free(cat);
        bf16_t* a;
        TRY(attention(f, lv.attn[j], y, H, W, &a, nullptr, dst, ldd));
        f.ar.free(y);
        y = a;
      } else {
        TRY(resblock(f, lv.block[j], cat, H, W, &y, nullptr, temb, dst, ldd, &xs, want_st ? &yst : nullptr));
        f.ar.free(cat);
      }
      if (cur_st) f.ar.free(cur_st);
      if (s.st) f.ar.free(s.st);
      cur = y;
      cur_st = yst;
      cur_ch = lv.ch;
      in_cat = to_cat;
    }
    if (lv.samp_w) {
      const int ldd = cur_ch + hs.back().ch;     // left half of the next level's first concatenation
      bf16_t* y;
      float* yst = nullptr;
      TRY(aalloc(f, &y, (size_t)B * H * W * 4 * ldd));
      if (gn_stats_shape(f, 4 * H * W, cur_ch)) TRY(aalloc(f, &yst, (size_t)B * H * W * 4 / 128 * cur_ch));
      TRY(conv3x3(f, cur, H, W, cur_ch, lv.samp_w, cur_ch, lv.samp_b, nullptr, y, 3, ldd, yst));
      f.ar.free(cur);
      if (cur_st) f.ar.free(cur_st);
      cur = y;
      cur_st = yst;
      H *= 2; W *= 2;
      in_cat = true;
    }
  }
  bf16_t* xn;
  TRY(aalloc(f, &xn, (size_t)B * H * W * cur_ch));
  {
    const GnStat xs{cur_st, cur_ch, nullptr, 0};
    TRY(groupnorm(f, cur, xn, h->no_g, h->no_b, H * W, cur_ch, 1, nullptr, cur_st ? &xs : nullptr));
  }
  if (cur_st) f.ar.free(cur_st);
  f.ar.free(cur);
  TRY(conv_out(f, xn, H, W, cur_ch, h->out_w, h->out_b, c.out_ch, out));
  f.ar.free(xn);
  f.ar.free(temb); f.ar.free(t0); f.ar.free(emb);
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}


// ------------------------------------------------------------------ forward with tape + input gradient
// Everything a backward pass needs from its forward: the arena (with the kept buffers still allocated in it) and the
// per-block records.  A backward allocates its temporaries above / between the kept buffers and frees them again; it
// never frees or writes a kept buffer, so any number of backward passes can follow one forward.
struct BlkRec {
  ResRec r{};
  AttnRec a{};
  bool has_attn = false;
  int left = 0, right = 0;     // up path: columns of the concatenation [previous block | skip]
};
struct SkipRec { bf16_t* p; int ch, H, W; };
struct GradTape {
  VF f;
  std::vector<SkipRec> hs;               // every tensor the down path pushed, in order
  std::vector<BlkRec> down, up;          // in execution order
  ResRec m1{}, m2{};
  AttnRec ma{};
  bf16_t* x_out = nullptr;               // input of norm_out
  float* st_out = nullptr;               // its GroupNorm statistics
  int B = 0, H = 0, W = 0, ch_out = 0;
  void* ws = nullptr;
};

void tape_init(GradTape& T, int B, void* ws, size_t ws_bytes, hipStream_t st, bool dry) {
  T.f.groups = 32; T.f.B = B; T.f.st = st;
  T.f.gn_fuse = false;    // a taped block takes its own statistics (the backward needs mean / rstd)
  T.f.ar.dry = dry;
  T.f.ar.base = reinterpret_cast<char*>(ws);
  T.f.ar.cap = ws_bytes;
  T.B = B; T.ws = ws;
}

// forward_impl's network with every block recorded; block outputs are contiguous and the concatenations are copies
int forward_keep_impl(hedit_ddpm* h, GradTape& T, const float* x, float t, float* out) {
  VF& f = T.f;
  const int B = f.B;
  hipStream_t st = f.st;
  const hedit_ddpm_cfg& c = h->cfg;
  const int L = c.n_levels, nrb = c.num_res_blocks, ch = c.ch, tc = h->temb_ch;
  float *emb, *t0, *temb;
  TRY(aalloc(f, &emb, (size_t)ch));
  TRY(aalloc(f, &t0, (size_t)tc));
  TRY(aalloc(f, &temb, (size_t)tc));
  RUN(f, timestep_embed_ddpm_launch(t, emb, ch, st));
  RUN(f, gemv_launch(h->t0_w, emb, h->t0_b, nullptr, t0, tc, ch, 0, st));
  RUN(f, gemv_launch(h->t1_w, t0, h->t1_b, nullptr, temb, tc, tc, 1, st));

  int H = c.image_size, W = c.image_size;
  bf16_t* x0;
  TRY(aalloc(f, &x0, (size_t)B * H * W * ch));
  RUN(f, conv_in_launch(x, h->in_w, h->in_b, x0, B, c.in_channels, H, W, ch, st));
  T.hs.push_back({x0, ch, H, W});
  for (int i = 0; i < L; ++i) {
    const DLevel& lv = h->down[i];
    for (int j = 0; j < nrb; ++j) {
      T.down.emplace_back();
      BlkRec& br = T.down.back();
      bf16_t* y;
      TRY(resblock(f, lv.block[j], T.hs.back().p, H, W, &y, &br.r, temb));
      if (!lv.attn.empty()) {
        bf16_t* a;
        br.has_attn = true;
        TRY(attention(f, lv.attn[j], y, H, W, &a, &br.a));     // y stays: the attention's input
        y = a;
      }
      T.hs.push_back({y, lv.ch, H, W});
    }
    if (lv.samp_w) {
      bf16_t* y;
      TRY(aalloc(f, &y, (size_t)B * (H / 2) * (W / 2) * lv.ch));
      TRY(conv3x3(f, T.hs.back().p, H, W, lv.ch, lv.samp_w, lv.ch, lv.samp_b, nullptr, y, 2));
      H /= 2; W /= 2;
      T.hs.push_back({y, lv.ch, H, W});
    }
  }
  bf16_t *m1, *m2, *cur;
  int cur_ch = T.hs.back().ch;
  TRY(resblock(f, h->mid1, T.hs.back().p, H, W, &m1, &T.m1, temb));
  TRY(attention(f, h->mida, m1, H, W, &m2, &T.ma));
  TRY(resblock(f, h->mid2, m2, H, W, &cur, &T.m2, temb));
  size_t k = T.hs.size();
  for (int i = L - 1; i >= 0; --i) {
    const DLevel& lv = h->up[i];
    for (int j = 0; j < nrb + 1; ++j) {
      const SkipRec& s = T.hs[--k];
      T.up.emplace_back();
      BlkRec& br = T.up.back();
      br.left = cur_ch; br.right = s.ch;
      const size_t M = (size_t)B * H * W;
      bf16_t *cat, *y;
      TRY(aalloc(f, &cat, M * (cur_ch + s.ch)));               // stays: the block's input
      RUN(f, concat_launch(cur, cur_ch, s.p, s.ch, cat, (long)M, st));
      f.ar.free(cur);                                          // a block's output is nobody's record
      TRY(resblock(f, lv.block[j], cat, H, W, &y, &br.r, temb));
      if (!lv.attn.empty()) {
        bf16_t* a;
        br.has_attn = true;
        TRY(attention(f, lv.attn[j], y, H, W, &a, &br.a));
        y = a;
      }
      cur = y;
      cur_ch = lv.ch;
    }
    if (lv.samp_w) {
      bf16_t* y;
      TRY(aalloc(f, &y, (size_t)B * H * W * 4 * cur_ch));
      TRY(conv3x3(f, cur, H, W, cur_ch, lv.samp_w, cur_ch, lv.samp_b, nullptr, y, 3));
      f.ar.free(cur);     // linear in its input: nothing to keep
      cur = y;
      H *= 2; W *= 2;
    }
  }
  bf16_t* xn;
  TRY(aalloc(f, &xn, (size_t)B * H * W * cur_ch));
  TRY(groupnorm(f, cur, xn, h->no_g, h->no_b, H * W, cur_ch, 1, &T.st_out));
  TRY(conv_out(f, xn, H, W, cur_ch, h->out_w, h->out_b, c.out_ch, out));
  f.ar.free(xn);
  f.ar.free(temb); f.ar.free(t0); f.ar.free(emb);
  T.x_out = cur;
  T.H = H; T.W = W; T.ch_out = cur_ch;
  return HEDIT_OK;
}

// d [M][ch] += pending gradient of the same skip tensor (fp32 add, one rounding), which is then released
int add_pending(VF& f, bf16_t* d, bf16_t*& pend, const SkipRec& s) {
  if (!pend) return HEDIT_OK;
  RUN(f, slice_add_launch(pend, s.ch, 0, s.ch, d, (long)f.B * s.H * s.W, 1, f.st));
  f.ar.free(pend);
  pend = nullptr;
  return HEDIT_OK;
}

int block_bwd(VF& f, const BlkRec& br, bf16_t** d) {
  bf16_t* dx;
  if (br.has_attn) {
    TRY(attention_bwd(f, br.a, *d, &dx));
    f.ar.free(*d);
    *d = dx;
  }
  TRY(resblock_bwd(f, br.r, *d, &dx));
  f.ar.free(*d);
  *d = dx;
  return HEDIT_OK;
}

// d_x = (d eps / d x)^T d_eps from a tape made by forward_keep_impl; the tape is left as it was
int backward_impl(hedit_ddpm* h, GradTape& T, const float* d_eps, float* d_x) {
  VF& f = T.f;
  const int B = f.B;
  hipStream_t st = f.st;
  const hedit_ddpm_cfg& c = h->cfg;
  const int L = c.n_levels, nrb = c.num_res_blocks;
  int H = T.H, W = T.W;
  bf16_t *d, *t;
  // conv_out, norm_out (+ swish)
  TRY(aalloc(f, &t, (size_t)B * H * W * T.ch_out));
  RUN(f, conv_in_launch(d_eps, h->out_t, h->zero_bias, t, B, c.out_ch, H, W, T.ch_out, st));
  TRY(aalloc(f, &d, (size_t)B * H * W * T.ch_out));
  TRY(groupnorm_bwd(f, T.x_out, t, nullptr, d, h->no_g, h->no_b, T.st_out, H * W, T.ch_out, 1));
  f.ar.free(t);
  // up path, last executed level first.  Each block's input gradient splits into the part that continues down the up path
  // (left columns) and the pending gradient of its skip tensor (right columns).
  std::vector<bf16_t*> pend(T.hs.size(), nullptr);
  size_t ui = T.up.size(), k = 0;
  for (int i = 0; i < L; ++i) {
    const DLevel& lv = h->up[i];
    if (lv.samp_w) {
      // d(2x upsample + conv) = dgrad conv at the high resolution, then 2x2 block sums
      bf16_t *du, *dx;
      TRY(aalloc(f, &du, (size_t)B * H * W * lv.ch));
      TRY(conv3x3(f, d, H, W, lv.ch, lv.samp_t, lv.ch, nullptr, nullptr, du, 1));
      f.ar.free(d);
      H /= 2; W /= 2;
      TRY(aalloc(f, &dx, (size_t)B * H * W * lv.ch));
      RUN(f, sum2x2_launch(du, dx, B, H, W, lv.ch, st));
      f.ar.free(du);
      d = dx;
    }
    for (int j = nrb; j >= 0; --j) {
      const BlkRec& br = T.up[--ui];
      TRY(block_bwd(f, br, &d));                 // d: [M][left + right]
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
    TRY(attention_bwd(f, T.ma, dx, &d));
    f.ar.free(dx);
    TRY(resblock_bwd(f, T.m1, d, &dx));
    f.ar.free(d);
    d = dx;
  }
  k = T.hs.size() - 1;
  TRY(add_pending(f, d, pend[k], T.hs[k]));
  // down path: the consumer on the down path first, then the pending gradient of the up path
  size_t di = T.down.size();
  for (int i = L - 1; i >= 0; --i) {
    const DLevel& lv = h->down[i];
    if (lv.samp_w) {
      --k;
      const SkipRec& s = T.hs[k];
      bf16_t* dx;
      TRY(aalloc(f, &dx, (size_t)B * s.H * s.W * lv.ch));
      RUN(f, conv3x3_s2_dgrad_launch(d, lv.samp_t, dx, B, s.H, s.W, lv.ch, lv.ch, st));
      f.ar.free(d);
      d = dx;
      TRY(add_pending(f, d, pend[k], s));
    }
    for (int j = nrb - 1; j >= 0; --j) {
      TRY(block_bwd(f, T.down[--di], &d));
      --k;
      TRY(add_pending(f, d, pend[k], T.hs[k]));
    }
  }
  // conv_in: the N = 4 route of conv_out() with the flipped, transposed weight
  TRY(conv_out(f, d, c.image_size, c.image_size, c.ch, h->in_t, nullptr, c.in_channels, d_x));
  f.ar.free(d);
  return HEDIT_OK;
}

int check_grad_handle(const hedit_ddpm* h, const char* who) {
  if (!h->grad) {
    hedit_set_error(std::string(who) + ": this handle has no input-gradient weights (create it with hedit_ddpm_create_grad)");
    return HEDIT_ERR_STATE;
  }
  return store_require_loaded(h, "DDPM UNet");
}

void drop_tape(hedit_ddpm* h) {
  if (h->tape && h->tape_free) h->tape_free(h->tape);
  h->tape = nullptr;
}

}  // namespace

HEDIT_LIFECYCLE(ddpm, hedit_ddpm, "DDPM UNet", drop_tape)

// grad: attach the input-gradient twins (hedit_ddpm_create_grad); without it, exactly the forward-only handle
static int create_impl(const hedit_ddpm_cfg* cfg, hedit_ddpm** out, bool grad) {
  ARG_CHECK(cfg && out, "null");
  ARG_CHECK(cfg->n_levels >= 1 && cfg->n_levels <= 8, "n_levels in 1..8");
  ARG_CHECK(cfg->in_channels >= 1 && cfg->in_channels <= 8 && cfg->out_ch >= 1 && cfg->out_ch <= 4, "in_channels <= 8, out_ch <= 4");
  ARG_CHECK(cfg->ch % 64 == 0, "ch must be a multiple of 64");
  ARG_CHECK(cfg->num_res_blocks >= 1 && cfg->num_res_blocks <= 4, "num_res_blocks in 1..4");
  const int L = cfg->n_levels;
  ARG_CHECK(cfg->image_size % (1 << (L - 1)) == 0, "image_size must be divisible by 2^(n_levels-1)");
  int res = cfg->image_size;
  for (int i = 0; i < L; ++i) {
    ARG_CHECK(cfg->ch_mult[i] >= 1, "ch_mult >= 1");
    if (cfg->attn_level[i]) ARG_CHECK((res * res) % 64 == 0, "attention levels need h*w % 64 == 0");
    if (i < L - 1) res /= 2;
  }
  ARG_CHECK((res * res) % 64 == 0, "the mid block's h*w must be a multiple of 64");
  TRY(gemm_prepare());
  if (grad) ARG_CHECK(cfg->in_channels <= 4, "the input-gradient pass needs in_channels <= 4");
  hedit_ddpm* h = new hedit_ddpm();
  h->cfg = *cfg;
  h->grad = grad;
  const int ch = cfg->ch, tc = 4 * ch, nrb = cfg->num_res_blocks;
  h->temb_ch = tc;
  const BlockNames& nm = NAMES_DDPM;
  h->t0_w = lin(h, "temb.dense.0.weight", tc, ch);
  h->t0_b = vec(h, "temb.dense.0.bias", tc);
  h->t1_w = lin(h, "temb.dense.1.weight", tc, tc);
  h->t1_b = vec(h, "temb.dense.1.bias", tc);
  h->in_w = f32conv(h, "conv_in.weight", ch, cfg->in_channels, 3);
  if (grad) {
    h->in_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)4 * 9 * ch);
    if (h->in_t && hipMemset(h->in_t, 0, (size_t)4 * 9 * ch * sizeof(bf16_t)) != hipSuccess) h->alloc_failed = true;
  }
  h->in_b = vec(h, "conv_in.bias", ch);
  auto mult_in = [&](int i) { return i == 0 ? 1 : cfg->ch_mult[i - 1]; };   // in_ch_mult = (1,) + ch_mult
  int block_in = ch;
  for (int i = 0; i < L; ++i) {
    DLevel lv;
    const std::string pre = "down." + std::to_string(i);
    block_in = ch * mult_in(i);
    const int block_out = ch * cfg->ch_mult[i];
    for (int j = 0; j < nrb; ++j) {
      lv.block.push_back(make_res(h, pre + ".block." + std::to_string(j), block_in, block_out, grad, nm, tc));
      block_in = block_out;
      if (cfg->attn_level[i]) lv.attn.push_back(make_attn(h, pre + ".attn." + std::to_string(j), block_in, grad, nm));
    }
    lv.ch = block_in;
    if (i != L - 1) {
      lv.samp_w = conv3(h, pre + ".downsample.conv.weight", block_in, block_in);
      if (grad) lv.samp_t = twin<bf16_t>(h, Pack::Conv3S2Dgrad, (size_t)block_in * block_in * 9);
      lv.samp_b = vec(h, pre + ".downsample.conv.bias", block_in);
    }
    h->down.push_back(lv);
  }
  h->mid1 = make_res(h, "mid.block_1", block_in, block_in, grad, nm, tc);
  h->mida = make_attn(h, "mid.attn_1", block_in, grad, nm);
  h->mid2 = make_res(h, "mid.block_2", block_in, block_in, grad, nm, tc);
  h->up.resize(L);
  for (int i = L - 1; i >= 0; --i) {
    DLevel lv;
    const std::string pre = "up." + std::to_string(i);
    const int block_out = ch * cfg->ch_mult[i];
    int skip_in = ch * cfg->ch_mult[i];
    for (int j = 0; j < nrb + 1; ++j) {
      if (j == nrb) skip_in = ch * mult_in(i);
      lv.block.push_back(make_res(h, pre + ".block." + std::to_string(j), block_in + skip_in, block_out, grad, nm, tc));
      block_in = block_out;
      if (cfg->attn_level[i]) lv.attn.push_back(make_attn(h, pre + ".attn." + std::to_string(j), block_in, grad, nm));
    }
    lv.ch = block_in;
    if (i != 0) {
      lv.samp_w = conv3(h, pre + ".upsample.conv.weight", block_in, block_in);
      if (grad) lv.samp_t = twin<bf16_t>(h, Pack::Conv3Dgrad, (size_t)block_in * block_in * 9);
      lv.samp_b = vec(h, pre + ".upsample.conv.bias", block_in);
    }
    h->up[i] = lv;
  }
  h->no_g = vec(h, "norm_out.weight", block_in);
  h->no_b = vec(h, "norm_out.bias", block_in);
  h->out_w = conv3(h, "conv_out.weight", cfg->out_ch, block_in);
  if (grad) {
    h->out_t = twin<float>(h, Pack::FlipOIHW, (size_t)cfg->out_ch * block_in * 9);
    h->zero_bias = dalloc<float>(h, block_in);
    if (h->zero_bias && hipMemset(h->zero_bias, 0, block_in * sizeof(float)) != hipSuccess) h->alloc_failed = true;
  }
  h->out_b = vec(h, "conv_out.bias", cfg->out_ch);
  return handle_created(h, out);
}

extern "C" {

int hedit_ddpm_create(const hedit_ddpm_cfg* cfg, hedit_ddpm** out) try {
  return create_impl(cfg, out, false);
} catch (...) { return hedit_abi_catch(); }

int hedit_ddpm_create_grad(const hedit_ddpm_cfg* cfg, hedit_ddpm** out) try {
  return create_impl(cfg, out, true);
} catch (...) { return hedit_abi_catch(); }

size_t hedit_ddpm_workspace_bytes(hedit_ddpm* h, int B) try {
  if (!h || B < 1) return 0;
  size_t peak = 0;
  const int rc = forward_impl(h, nullptr, 0.f, B, nullptr, nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

int hedit_ddpm_forward(hedit_ddpm* h, const float* x, float t, int B, float* eps, void* workspace, size_t workspace_bytes,
                       void* stream) try {
  ARG_CHECK(h && x && eps && workspace, "null");
  ARG_CHECK(B >= 1, "B");
  TRY(handle_loaded(h));
  return forward_impl(h, x, t, B, eps, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

size_t hedit_ddpm_grad_workspace_bytes(hedit_ddpm* h, int B) try {
  if (!h || B < 1 || !h->grad) return 0;
  GradTape T;
  tape_init(T, B, nullptr, 0, nullptr, true);
  float dummy = 0.f;   // never dereferenced in the dry run
  int rc = forward_keep_impl(h, T, nullptr, 0.f, nullptr);
  if (rc == HEDIT_OK) rc = backward_impl(h, T, &dummy, &dummy);
  return dry_run_bytes(rc, T.f.ar.peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

int hedit_ddpm_forward_keep(hedit_ddpm* h, const float* x, float t, int B, float* eps, void* workspace, size_t workspace_bytes,
                            void* stream) try {
  ARG_CHECK(h && x && eps && workspace, "null");
  ARG_CHECK(B >= 1, "B");
  TRY(check_grad_handle(h, "hedit_ddpm_forward_keep"));
  drop_tape(h);
  GradTape* T = new GradTape();
  tape_init(*T, B, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false);
  const int rc = forward_keep_impl(h, *T, x, t, eps);
  if (rc != HEDIT_OK) {
    delete T;
    return rc;
  }
  h->tape = T;
  h->tape_free = [](void* p) { delete reinterpret_cast<GradTape*>(p); };
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_ddpm_backward(hedit_ddpm* h, const float* d_eps, float* d_x, void* workspace, void* stream) try {
  ARG_CHECK(h && d_eps && d_x && workspace, "null");
  TRY(check_grad_handle(h, "hedit_ddpm_backward"));
  if (!h->tape) {
    hedit_set_error("hedit_ddpm_backward: no forward is being kept (call hedit_ddpm_forward_keep first)");
    return HEDIT_ERR_STATE;
  }
  GradTape* T = reinterpret_cast<GradTape*>(h->tape);
  if (T->ws != workspace) {
    hedit_set_error("hedit_ddpm_backward: not the workspace the kept forward ran in");
    return HEDIT_ERR_ARG;
  }
  T->f.st = reinterpret_cast<hipStream_t>(stream);
  const int rc = backward_impl(h, *T, d_eps, d_x);
  if (rc != HEDIT_OK) drop_tape(h);   // a pass that stopped half way leaves temporaries in the arena
  return rc;
} catch (...) { return hedit_abi_catch(); }

void hedit_ddpm_release(hedit_ddpm* h) try {
  if (h) drop_tape(h);
} catch (...) { (void)hedit_abi_catch(); }

int hedit_ddpm_vjp(hedit_ddpm* h, const float* x, float t, const float* d_eps, int B, float* d_x, float* eps, void* workspace,
                   size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && x && d_eps && d_x && eps && workspace, "null");
  ARG_CHECK(B >= 1, "B");
  TRY(check_grad_handle(h, "hedit_ddpm_vjp"));
  drop_tape(h);
  GradTape T;
  tape_init(T, B, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false);
  TRY(forward_keep_impl(h, T, x, t, eps));
  return backward_impl(h, T, d_eps, d_x);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
