/* libhedit_hip.so -- C ABI of the MI355X-native h-Edit hot path.
 *
 * The reference (nktoan/h-edit) is pure Python on third-party CUDA libraries and has NO FFI of
 * its own; the boundary below is therefore build-defined and sits exactly
 * where the reference's Python hands work to "the device":
 *
 *   hedit_unet_forward      replaces  model.unet(x, t, encoder_hidden_states=..,
 *                                     cross_attention_kwargs=..).sample
 *                           call sites text-guided/inversion/p2p_h_edit.py:98,123,245,281,315,458,
 *                                     484,492,613,644,652 and ddpm_inversion.py:130,132
 *                           including the P2P processor/controller body that the reference runs
 *                           inside every attention layer (text-guided/p2p/ptp_utils.py:65-122,
 *                           text-guided/p2p/ptp_classes.py:91-108,135-150,202-227)
 *   hedit_step_base         replaces  CFG mix + reverse_step  (p2p_h_edit.py:614-622 /
 *                                     inversion/inversion_utils.py:84-119)
 *   hedit_step_invert       replaces  one step of the edit-friendly DDPM inversion: z_t = (x_{t-1} - mu_t) / sigma_t and
 *                                     the in-place rewrite x_{t-1} <- mu_t + sigma_t z_t
 *                                     (text-guided/inversion/ddpm_inversion.py:146-162), with hedit_step_base's
 *                                     mu so that the sampler's reconstruction branch retraces it bit for bit
 *   hedit_step_update       replaces  the three CFG mixes, correction, L1 reconstruction pull with
 *                                     its two .item() syncs, and the x_{t-1} update
 *                                     (p2p_h_edit.py:654-692; twins :317-353, :494-514, :125-147)
 *   hedit_unet_set_attn_hook  opens   the reference's hook point for a controller written in the host language: the call
 *                                     `self.controller(attention_probs, is_cross, self.place_in_unet, save_attn)` of
 *                                     text-guided/p2p/ptp_utils.py:98-106 on materialised probabilities (slow path)
 *   hedit_local_blend       replaces  LocalBlend.__call__/get_mask (p2p/ptp_classes.py:44-72)
 *   hedit_local_blend_sub   the same  with substruct_words (p2p/ptp_classes.py:28-38,64-68)
 *   hedit_attn_aggregate    replaces  aggregate_attention (p2p/ptp_classes.py:298-309): the mean over layers and heads of the
 *                                     averaged maps the attention viewers display
 *   hedit_p2p_plan          carries   the per-call edit rule of the registered controller / editor: Prompt-to-Prompt
 *                                     (ptp_classes.py:194-227), MasaCtrl (masactrl/masactrl.py:53-69: kv_src; :71-148: the
 *                                     mask-guided editor with given masks, masa_rows + class arrays) and
 *                                     Plug-and-Play (plug_n_play/pnp_utils.py:29-154: qk_first_block, feat_src)
 *   hedit_vae_encode/decode replaces  model.vae.encode(x).latent_dist.mode() / model.vae.decode(z).sample
 *                                     (main_p2p.py:159,263)
 *   hedit_vae_decode_vjp,   replace   the decoder part of torch.autograd.grad(loss, latents) in the style closure
 *   _keep + _backward                 (text-guided-n-style/inversion/h_edit.py:146-185)
 *   hedit_step_tweedie,     replace   reverse_step_pred_x0 and the rho-normalised style update
 *   hedit_step_style                  (inversion_utils.py:128-140, h_edit.py:167-183)
 *   hedit_step_ef_seed,     replace   the latent-side arithmetic of Edit Friendly's style step, which differentiates the loss
 *   hedit_step_ef_style               through the eps-network: the cotangent handed to hedit_unet_backward, then the sum of the
 *                                     gradient's parts and the rho-normalised update with its two .item() syncs
 *                                     (text-guided-n-style/inversion/ef.py:103-124)
 *   hedit_ddpm_forward      replaces  Model.forward(x, t) of face-swapping/diffusion/diffusion.py:294-341
 *                                     (call sites face-swapping/inversion/h_edit_R.py:71,96,118, sde_inversion.py:121)
 *   hedit_k_*               single-kernel entry points used by the parity tests
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Every pointer is a DEVICE pointer unless the
 *     parameter name starts with h_ .  The caller (PyTorch-ROCm host code) owns every buffer
 *     including the workspace; the library owns only the opaque handle and its packed weights.
 *   - stream-ordered: nothing here synchronises the device; `stream` is a hipStream_t.
 *   - returns 0 on success, a negative code otherwise; hedit_last_error() gives the message of
 *     the last failure on the calling thread.  Never throws, never exits.
 *   - activations inside the UNet are NHWC bf16; latents/eps at the boundary are fp32 NCHW,
 *     exactly the tensors the reference loop holds.
 */
#ifndef HEDIT_H
#define HEDIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEDIT_MAX_LEVELS 8

typedef struct hedit_unet hedit_unet;

/* Architecture of a UNet2DConditionModel (diffusers naming). */
typedef struct {
  int in_channels, out_channels, sample_size;
  int n_levels;
  int block_out_channels[HEDIT_MAX_LEVELS];
  int down_has_attn[HEDIT_MAX_LEVELS]; /* CrossAttnDownBlock2D (1) / DownBlock2D (0)            */
  int up_has_attn[HEDIT_MAX_LEVELS];   /* CrossAttnUpBlock2D (1) / UpBlock2D (0), up-block order */
  int layers_per_block;
  int cross_attention_dim;
  int heads;                           /* "attention_head_dim" of SD-1.x = number of heads      */
  int norm_num_groups;
} hedit_unet_cfg;

/* Per-call Prompt-to-Prompt plan = the state the reference's controller holds, compiled by the
 * host for ONE UNet call (hedit/p2p/plan.py).  All arrays are device memory. */
typedef struct {
  int mode;                 /* 0: controller off; 1: apply edits; 2: apply edits + accumulate store */
  int n_pairs;              /* (source-conditional row, target-conditional row) pairs in the batch  */
  const int32_t* pair_src;  /* [n_pairs] */
  const int32_t* pair_tar;  /* [n_pairs] */
  const int32_t* singles;   /* [n_single] batch rows not in any pair                                */
  int n_single;
  const int32_t* qk_src;    /* [B] self-attention replacement map for layers with <= 32*32 tokens
                               (row b uses q,k of row qk_src[b]); NULL outside the self window      */
  const void* mixT;         /* bf16 [n_pairs][96][96], mixT[n][w] = A[w][n]                         */
  const float* bvec;        /* [n_pairs][96]:  P_new = P_src . A + bvec * P_tar                     */
  float* const* h_store;    /* HOST array of n_store device pointers, one per cross-attention layer
                               with <= 32*32 tokens in call order; each [n_pairs][2][heads][N][77]  */
  int n_store;
  /* MasaCtrl mutual self-attention (text-guided/masactrl/masactrl.py:53-69): in the transformer blocks with
   * index >= kv_first_block (call order, 16 in SD-1.x) row b of every self-attention uses the keys and values
   * of row kv_src[b] (its own queries).  NULL = off. */
  const int32_t* kv_src;    /* [B] */
  int kv_first_block;
  /* Plug-and-Play injection (text-guided/plug_n_play/pnp_utils.py:29-154): the qk_src map above, restricted to the
   * transformer blocks with index >= qk_first_block and to layers with <= qk_max_tokens tokens (0 = the P2P
   * default, 32*32); and feat_src: before conv2 of ResNet block number feat_resblock (call order) row b takes the
   * activations of row feat_src[b], i.e. its conv2 output becomes the source row's (pnp_utils.py:131-140).  NULL = off. */
  int qk_first_block, qk_max_tokens;
  const int32_t* feat_src;  /* [B] */
  int feat_resblock;
  /* The reference's AttentionStore also keeps the SELF maps of the layers with <= 32*32 tokens (ptp_classes.py:135-150).
   * Nothing on the h-Edit path reads them, so the fused path stores them only on request: HOST array of n_store_self
   * device pointers, one per such self-attention layer in call order, each [n_pairs][2][heads][N][N] fp32, accumulated
   * on mode-2 passes (post-edit: inside the self window the target row's map is the source's).  NULL = off. */
  float* const* h_store_self;
  int n_store_self;
  /* Mask-guided MasaCtrl (text-guided/masactrl/masactrl.py:71-148): where kv_src applies, the rows listed in masa_rows (the
   * target rows) attend only to the keys of row kv_src[b] whose class equals the query's class; a query whose class has no key
   * attends to all of them with equal weight (the reference's fp32 result: the mean of V).  masa_rows MUST list exactly the rows with
   * kv_src[b] != b: the rows not listed (the source rows) run plain attention on their OWN keys and values on the unmasked
   * kernel, launched on their contiguous runs, so they keep the bits of a pass without these fields -- a row with
   * kv_src[b] != b that is left out would silently lose its mutual attention (kv_src is device memory: the executor cannot
   * check it).  h_masa_rows is a HOST copy of masa_rows (the executor cuts the runs from it).
   * Classes are bytes 0 / 1 per token, given per layer resolution: HOST arrays of n_masa_res device pointers,
   * h_masa_cls_q[r] / h_masa_cls_k[r] = [B][h_masa_tokens[r]] (query classes read at row b, key classes at row kv_src[b]);
   * h_masa_tokens is a HOST array of the token counts (multiples of 64 up to 4096).  A self-attention layer whose token count
   * is not listed, or that lies outside the kv_first_block gate, runs as without these fields.  Needs kv_src and a square
   * latent; excludes qk_src and an attention hook: each refused by name before anything is launched.  (The taped forward of
   * hedit_unet_forward_keep / _vjp takes no plan at all.)  n_masa_rows = 0 = off. */
  const int32_t* masa_rows;   /* [n_masa_rows] */
  const int32_t* h_masa_rows; /* HOST [n_masa_rows] */
  int n_masa_rows;
  const uint8_t* const* h_masa_cls_q;
  const uint8_t* const* h_masa_cls_k;
  const int32_t* h_masa_tokens;
  int n_masa_res;
  /* The auto variant (masactrl.py:151-286): masa_auto = 1 derives the classes from the pass's own cross-attention maps
   * instead of taking them from h_masa_cls_* (then NULL, n_masa_res = 0).  The batch is [x_orig|null]*n, [x_k|null]*n,
   * [x_orig|src]*n, [x_k|tar]*n with n = masa_images, B = 4 n, masa_rows the 2 n target rows.  Every cross-attention layer
   * with exactly 256 tokens adds the head mean of its probabilities -- the columns masa_ref_tokens summed on the n conditional
   * source rows, masa_cur_tokens on the n conditional target rows (device arrays of token indices < 77) -- to an accumulator.
   * Before a self-attention layer where kv_src applies, accumulator / layers-so-far is min-max normalised per image, taken
   * nearest from 16 x 16 to the layer's resolution and thresholded >= masa_thres: the source map gives the key classes of
   * image i's source rows, the target map the query classes of its target rows.  A constant map gives class 0 everywhere
   * (the reference divides 0 by 0 there).  While the pass has collected no map, such a layer runs unmasked.  No host wait.
   * masa_ws: caller-owned device memory, 16-byte aligned, of at least
   *     2 n * 256 * 4  +  4 n * 4096  +  2 n * heads * 256 * 77 * 4   bytes
   * (accumulator, class array, probabilities); the executor zeroes the accumulator at the start of the pass.
   * h_masa_dump: optional HOST array of n_masa_dump device pointers, one per self-attention layer where kv_src applies, in
   * call order: the class array [B][N] of that layer is written THERE (and read from there) instead of into masa_ws; a layer
   * that ran unmasked leaves its buffer untouched. */
  int masa_auto;
  float masa_thres;
  int masa_images;
  const int32_t* masa_ref_tokens;
  int n_masa_ref;
  const int32_t* masa_cur_tokens;
  int n_masa_cur;
  void* masa_ws;
  size_t masa_ws_bytes;
  uint8_t* const* h_masa_dump;
  int n_masa_dump;
} hedit_p2p_plan;

typedef struct {
  float sqrt_ab_t, sqrt_1m_ab_t, sqrt_ab_prev, dir_coef, noise_coef;
  float w_src, w_hat, w_tar, coeff, w_rec;
} hedit_step_coef;

const char* hedit_last_error(void);
int hedit_version(void);

/* ---- UNet ------------------------------------------------------------------------------- */
int hedit_unet_create(const hedit_unet_cfg* cfg, hedit_unet** out);
void hedit_unet_destroy(hedit_unet* h);
/* number of parameters the handle expects; name of the i-th one (diffusers state_dict key) */
int hedit_unet_num_params(const hedit_unet* h);
const char* hedit_unet_param_name(const hedit_unet* h, int i);
/* torch shape of the i-th parameter: *ndim in 1..4, dims4[0..ndim) */
int hedit_unet_param_shape(const hedit_unet* h, int i, int* ndim, int* dims4);
/* hand one fp32 parameter tensor (torch layout, device memory) to the library, which packs it
 * into its own bf16/fp32 GEMM layout on `stream` */
int hedit_unet_load(hedit_unet* h, const char* name, const float* w, size_t numel, void* stream);
/* 1 if parameter i is kept as an unscaled bf16 copy: a bf16-rounded source gives the same packed bits (the weight
 * broadcast of the multi-GPU start-up sends those tensors as bf16, the rest as fp32) */
int hedit_unet_param_bf16_exact(const hedit_unet* h, int i);
/* 0 when every parameter has been loaded, else the count still missing */
int hedit_unet_missing(const hedit_unet* h);
size_t hedit_unet_workspace_bytes(hedit_unet* h, int B, int height, int width);
/* x: fp32 [B][Cin][H][W]; t: scalar timestep shared by the batch; ctx: fp32 [B][77][ctx_dim];
 * eps_out: fp32 [B][Cout][H][W] */
int hedit_unet_forward(hedit_unet* h, const float* x, float t, const float* ctx, int B, int height,
                       int width, const hedit_p2p_plan* plan, float* eps_out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The same evaluation for a batch whose rows share latents -- classifier-free guidance and the h-Edit passes evaluate each
 * latent under several contexts in one call.  x: fp32 [D][Cin][H][W], the D distinct latents (16-byte aligned);
 * row_latent: HOST array of B ints in [0, D): row r evaluates x[row_latent[r]] under ctx[r].  ctx, plan, eps_out and the
 * workspace are per row as above, and row r of eps_out has the bits hedit_unet_forward gives for that latent and context.
 * What precedes the first cross-attention depends on the latent and t only, so it runs once per distinct latent whenever
 * nothing there looks across rows: no hook, and no feature / key-value / query-key injection or self-map store of the plan
 * that reaches the first block; otherwise the latents are spread to one per row first.  The map travels in the kernel
 * arguments (nothing is uploaded, the host never waits); B <= 512.  hedit_unet_workspace_bytes(h, B, ..) covers any map. */
int hedit_unet_forward_shared(hedit_unet* h, const float* x, int D, const int* row_latent, float t, const float* ctx, int B,
                              int height, int width, const hedit_p2p_plan* plan, float* eps_out, void* workspace,
                              size_t workspace_bytes, void* stream);
/* A bound text context.  The context rows of an edit are fixed over its sampling steps, while hedit_unet_forward starts every call
 * by padding them to bf16 [B * 80][ctx_dim] and projecting them onto the stacked attn2 key / value matrices of all transformer
 * blocks (two GEMMs: 368 GFLOP at 120 rows of SD-1.5).  hedit_unet_context_create runs exactly those three launches once, on
 * `stream`, for ctx fp32 [B][77][ctx_dim], into device memory the object owns (allocated here, never inside a forward:
 * 2 * B * 80 * (ctx_n + ctx_dim / 2) * 2 bytes, 4 MB per row and 0.48 GB at 120 rows for SD-1.5; HEDIT_ERR_STATE while `stream`
 * is capturing, HEDIT_ERR_HIP when the memory is not to be had).  hedit_unet_forward_bound / hedit_unet_forward_shared_bound are
 * hedit_unet_forward / hedit_unet_forward_shared with the object in place of `ctx`: they skip the three launches, read the
 * object's buffers, and give the same bits.  hedit_unet_workspace_bytes(h, B, ..) is enough for either form.
 * Contract: the object is a SNAPSHOT of the rows and of the handle's weights at create time.  Changing the fp32 tensor, or
 * loading parameters, afterwards does not change it; nothing compares pointers to guess whether a tensor is "the same".  A call
 * with another B than the object was created for, or with an object of another handle, returns HEDIT_ERR_ARG, and so does a call
 * while an attention hook is set (the hook path, hedit_unet_forward_keep, _vjp and _backward_ctx take the fp32 rows).  The calls
 * that read the object must be ordered after its creation (the same stream, or an event).  hedit_unet_context_destroy waits for
 * the device, accepts NULL, and may run before or after hedit_unet_destroy of the handle. */
typedef struct hedit_unet_context hedit_unet_context;
int hedit_unet_context_create(hedit_unet* h, const float* ctx, int B, void* stream, hedit_unet_context** out);
void hedit_unet_context_destroy(hedit_unet_context* cx);
int hedit_unet_forward_bound(hedit_unet* h, const float* x, float t, const hedit_unet_context* cx, int B, int height, int width,
                             const hedit_p2p_plan* plan, float* eps_out, void* workspace, size_t workspace_bytes, void* stream);
int hedit_unet_forward_shared_bound(hedit_unet* h, const float* x, int D, const int* row_latent, float t,
                                    const hedit_unet_context* cx, int B, int height, int width, const hedit_p2p_plan* plan,
                                    float* eps_out, void* workspace, size_t workspace_bytes, void* stream);
/* Host-language attention controller -- the reference's hook point, text-guided/p2p/ptp_utils.py:98-106
 * (`self.controller(attention_probs, is_cross, self.place_in_unet, save_attn)` between the softmax and the product with V).
 * With a hook set, every attention layer of hedit_unet_forward writes its probabilities to HBM as fp32
 * [batch_heads = B * heads][n_query][n_key] (batch-major like `head_to_batch_dim`; n_key = 77 for the context), calls
 * fn -- which may rewrite them in place with work queued on `stream` -- and multiplies the result with V.  place: 0 down,
 * 1 mid, 2 up; layer counts the calls of one forward.  fn returns 0, anything else aborts the forward.  The in-kernel
 * edits of the plan are NOT applied on this path (pass plan = NULL or a mode-0 plan); fn = NULL restores the fused kernels.
 * hedit_unet_workspace_bytes accounts for the probabilities while a hook is set. */
typedef int (*hedit_attn_hook_fn)(void* user, float* probs, int batch_heads, int n_query, int n_key, int is_cross, int place,
                                  int layer, void* stream);
int hedit_unet_set_attn_hook(hedit_unet* h, hedit_attn_hook_fn fn, void* user);
/* number of cross-attention layers with <= 32*32 tokens (= plan.n_store) and their geometry */
int hedit_unet_num_store_layers(const hedit_unet* h, int height, int width);
int hedit_unet_store_layer_info(const hedit_unet* h, int height, int width, int i, int* tokens,
                                int* place /*0 down,1 mid,2 up*/);

/* Input gradient of the network: d_x = (d eps / d x)^T d_eps of a PLAIN pass (no plan, no hook) -- what Noise Map Guidance
 * differentiates (text-guided/inversion/p2p_baselines.py:195-293).  With respect to x only: nothing for ctx, t or the weights.
 * hedit_unet_create_grad: hedit_unet_create (same parameters, same names) whose hedit_unet_load also fills the input-gradient
 *   twins (transposed linear weights, dgrad-packed convolutions) and, at the width the forward-only handle runs as chain
 *   kernels, the unfused weights.  in_channels <= 4.  Such a handle serves hedit_unet_forward as before.
 * hedit_unet_forward_keep: the network through the unfused kernels with every block recorded inside `workspace`
 *   (hedit_unet_grad_workspace_bytes, which also covers the backward's temporaries); eps is within the forward's tolerance of
 *   hedit_unet_forward's, not its bits.  The tape lives until the next forward_keep / vjp / release on the handle; the
 *   workspace must stay untouched meanwhile.
 * hedit_unet_backward: one pass over the tape, which it leaves intact (any number of cotangents per forward; the same bits
 *   each time).  d_eps fp32 [B][Cout][H][W] -> d_x fp32 [B][Cin][H][W].  Batch rows are the bits of single calls.
 * hedit_unet_vjp: both in one call, nothing kept.
 * hedit_unet_create_grad_ctx: hedit_unet_create_grad whose load also fills [wk2_all | wv2_all]^T, the transposed stack of
 *   every block's attn2.to_k / to_v ([cross_attention_dim][2 * sum of the blocks' widths]) -- what the gradient with respect
 *   to the TEXT CONTEXT needs (null-text inversion).  hedit_unet_grad_workspace_bytes on such a handle also covers
 *   hedit_unet_backward_ctx; on a hedit_unet_create_grad handle it is what it was.
 * hedit_unet_backward_ctx: hedit_unet_backward over the same tape that also forms dK / dV of every cross-attention
 *   (csrc/attnbwd.hip, the context form) and from them d_ctx fp32 [B][77][cross_attention_dim] in ONE fp32 GEMM chain per
 *   element (never rounded to 16 bits).  d_x may be NULL: the walk then stops above the first transformer block; d_ctx has
 *   the same bits either way, d_x the bits of hedit_unet_backward.  HEDIT_ERR_STATE on a handle without the context weights.
 * HEDIT_ERR_STATE: a forward-only handle, a backward without a tape, or a set attention hook. */
int hedit_unet_create_grad(const hedit_unet_cfg* cfg, hedit_unet** out);
int hedit_unet_create_grad_ctx(const hedit_unet_cfg* cfg, hedit_unet** out);
int hedit_unet_backward_ctx(hedit_unet* h, const float* d_eps, float* d_x, float* d_ctx, void* workspace, void* stream);
size_t hedit_unet_grad_workspace_bytes(hedit_unet* h, int B, int height, int width);
int hedit_unet_forward_keep(hedit_unet* h, const float* x, float t, const float* ctx, int B, int height, int width, float* eps,
                            void* workspace, size_t workspace_bytes, void* stream);
int hedit_unet_backward(hedit_unet* h, const float* d_eps, float* d_x, void* workspace, void* stream);
void hedit_unet_release(hedit_unet* h);
int hedit_unet_vjp(hedit_unet* h, const float* x, float t, const float* ctx, const float* d_eps, int B, int height, int width,
                   float* d_x, float* eps, void* workspace, size_t workspace_bytes, void* stream);

/* Sampled launch timing for bench.py's roofline: while enabled, every kernel launch of
 * hedit_unet_forward is bracketed by a HIP event pair on the launch stream (up to max_records
 * launches).  kind: 0 conv3x3 GEMM, 1 linear/1x1 GEMM, 2 self-attention, 3 cross-attention,
 * 4 Group/LayerNorm, 5 other.  total_flops is the ALGORITHMIC count (2MNK; 4 B N Nk C for
 * attention).  Call hedit_prof_collect only after synchronising the stream. */
int hedit_prof_enable(hedit_unet* h, int on, int max_records);
int hedit_prof_reset(hedit_unet* h);
int hedit_prof_collect(hedit_unet* h, int kind, double* total_ms, double* total_flops, int64_t* count);
/* algorithmic HBM bytes of the sampled launches of a class: every operand read once, every result written once
 * (what roofline.traffic, a PMC measurement, is compared with) */
int hedit_prof_collect_bytes(hedit_unet* h, int kind, double* total_bytes);
/* one row of 8 doubles per sampled launch, in launch order: kind, ms, flops, bytes, M, N, K, tag (GEMM launches only:
 * mode | 8 GEGLU | 16 residual | 32 split-K | 64 chunked K); after synchronising the stream */
int hedit_prof_records(hedit_unet* h, double* rows, int max_rows, int* n_rows);

/* ---- sampler steps ------------------------------------------------------------------------
 * Batched tensors are [row][image][elems]: for one image this is exactly the reference layout.
 *   eps of the base pass: rows = 4 -> [x_o|null, x_e|null, x_o|src, x_e|src] (P2P loops),
 *                         rows = 2 -> [x_e|null, x_e|src] (no-P2P loops)
 *   xt / x_prev: [2][n_img][elems] = (x^orig, x^edit);   z: [n_img][elems] (may be NULL)
 *   step_update: the four eps operands are pointers to image 0, image i sits stride_img floats
 *   further; x_k / x_base / x_out: [n_img][elems].
 *   local_blend: h_maps = HOST array of n_maps device pointers to 16x16 cross maps, each
 *   [n_img][2][heads][256][77]; alpha_layers [n_img][2][77]; enabled [n_img] or NULL. */
int hedit_step_base(const float* eps, const float* xt, const float* z, float* x_prev, int n_img,
                    int elems, int eps_rows_per_img, const hedit_step_coef* c, void* stream);
/* Paired CFG + reverse step of the gradient-free comparison editors (EF, PnP-Inv, NP;
 * text-guided/inversion/p2p_baselines.py:165-181): source and target latent advance from the same UNet pass, each
 * kind with its own coefficient set -- c[k].w_src is kind k's guidance weight, dir_coef / noise_coef its stochasticity.
 *   e_u, e_c, xt, x_next: [n_kinds][n_img][elems], kind 0 = source (reconstruction), kind 1 = target (edit);
 *   n_kinds = 1: one latent per image (EF without P2P);  z: [n_img][elems], shared by both kinds, or NULL;
 *   c: HOST array of n_kinds coefficient sets.
 * x_next = sqrt_ab_prev (x - sqrt_1m_ab_t e) / sqrt_ab_t + dir_coef e + noise_coef z,  e = e_u + w_src (e_c - e_u):
 * the arithmetic of hedit_step_base element by element (same bits on equal coefficients). */
int hedit_step_pair(const float* e_u, const float* e_c, const float* xt, const float* z, float* x_next, int n_img,
                    int elems, int n_kinds, const hedit_step_coef* c, void* stream);
/* inversion step: e_u, e_c, xt, x_prev (in/out), z_out: [n_img][elems]; sigma = c->noise_coef > 0; the CFG mix
 * uses c->w_src (pass e_c = e_u for an unconditional inversion). */
int hedit_step_invert(const float* e_u, const float* e_c, const float* xt, float* x_prev, float* z_out,
                      int n_img, int elems, const hedit_step_coef* c, void* stream);
int hedit_step_update(const float* e_u_src, const float* e_c_src, const float* e_u_tar,
                      const float* e_c_tar, int64_t stride_img, const float* x_k,
                      const float* x_base, float* x_out, int n_img, int elems, int k_gt0,
                      const hedit_step_coef* c, void* stream);
/* Style guidance of the text + style loop (text-guided-n-style/inversion/h_edit.py:160-185), the latent-side
 * arithmetic either side of the decoder / image-encoder pass:
 *   step_tweedie: z0 = (x - sqrt(1-ab) e_tar) / sqrt(ab) * inv_scale, e_tar = e_u_tar + w_tar (e_c_tar - e_u_tar)
 *                 (reverse_step_pred_x0, inversion_utils.py:128-140, and the 1/0.18215 of h_edit.py:173)
 *   step_style:   x_out = x - rho g, g = chain * g_z, rho = rms(correction) / rms(g) * weight per image
 *                 (h_edit.py:179-183; g_z = d loss / d z0 from hedit_vae_decode_vjp behind the image encoder,
 *                 chain = inv_scale / sqrt(ab))
 * eps operands as in step_update: pointer to image 0, image i at + i * stride_img; x / z0 / g_z / x_out [n_img][elems] */
int hedit_step_tweedie(const float* e_u_tar, const float* e_c_tar, int64_t stride_img, const float* x, float* z0,
                       int n_img, int elems, float w_tar, float sqrt_ab, float sqrt_1m_ab, float inv_scale, void* stream);
int hedit_step_style(const float* e_u_src, const float* e_c_src, const float* e_u_tar, const float* e_c_tar,
                     int64_t stride_img, const float* x, const float* g_z, float* x_out, int n_img, int elems,
                     float w_hat, float w_tar, float chain, float weight, void* stream);
/* Style step of the Edit Friendly comparison editor (text-guided-n-style/inversion/ef.py:91-124).  The loss is differentiated
 * through a plain UNet pass of 2 n rows [x | uncond] * n, [x | tar] * n (hedit_unet_forward_keep): z0 = hedit_step_tweedie of
 * its eps with ab at t, g_z = d loss / d z0.  With a = inv_scale / sqrt(ab_t), c = -a sqrt(1 - ab_t):
 *   step_ef_seed:  d_eps [2 n][elems], the cotangent for hedit_unet_backward: row i = (1 - w_tar) c g_z[i],
 *                  row n + i = w_tar c g_z[i]   (`a` is not part of it: the direct term is added by step_ef_style)
 *   step_ef_style: dx [2 n][elems] = what hedit_unet_backward returned; g = (dx[i] + dx[n + i]) + a g_z[i];
 *                  rho = rms(e_c - e_u) / rms(g) * weight per image, no epsilon (a zero gradient gives the reference's
 *                  inf / nan); x_out = x_prev - rho g.  x_out may be x_prev.  Row i of a batch has the bits of a single call.
 * e_u / e_c: pointer to image 0, image i at + i * stride_img; g_z / x_prev / x_out [n_img][elems]. */
int hedit_step_ef_seed(const float* g_z, float* d_eps, int n_img, int elems, float w_tar, float a, float c, void* stream);
int hedit_step_ef_style(const float* e_u, const float* e_c, int64_t stride_img, const float* dx, const float* g_z,
                        const float* x_prev, float* x_out, int n_img, int elems, float a, float weight, void* stream);
/* A sparse linear map along one axis of a [outer][n_in][inner] fp32 tensor: out[o][i][x] = sum_j val[i][j] in[o][idx[i][j]][x]
 * (tables [n_out][nnz], fixed summation order).  With torch's bicubic weights it replaces F.interpolate(im, (224, 224),
 * mode="bicubic") in front of the style encoder (text-guided-n-style/clip_guidance/base_clip.py:57-58) and, with the
 * transposed table, its backward -- repeatable and batch-invariant, where torch's bicubic backward uses atomics. */
int hedit_axis_mix(const float* in, float* out, const int32_t* idx, const float* val, int nnz, int64_t outer, int n_in, int n_out,
                   int inner, void* stream);
int hedit_local_blend(float* const* h_maps, int n_maps, int heads, const float* alpha_layers,
                      const int32_t* enabled, float* xt, int n_img, int C, int H, int W, float th,
                      void* stream);
/* the same with LocalBlend's substruct_words (ptp_classes.py:28-38,64-68): substruct_layers [n_img][2][77] marks the words
 * whose (un-pooled) map, thresholded with th_sub = th[1], is cut out of the blend mask */
int hedit_local_blend_sub(float* const* h_maps, int n_maps, int heads, const float* alpha_layers,
                          const float* substruct_layers, const int32_t* enabled, float* xt, int n_img, int C, int H,
                          int W, float th, float th_sub, void* stream);
/* aggregate_attention (p2p/ptp_classes.py:298-309) for every image of a lock-step batch and both prompts of each pair, in
 * one launch.  h_maps = HOST array of n_maps (<= 16) device pointers to accumulated maps, each
 * [n_img][2][heads][tokens][cols] fp32 (cols = 77 for cross maps, tokens for self maps; the caller has selected them by
 * place and tokens == res * res); out [n_img][2][tokens][cols].  Per element, in fp32:
 *   out = (t_0,0 + t_0,1 + ... + t_L-1,H-1) / (n_maps * heads),   t_l,h = map_l[.., h, ..] / cur_step (a true division),
 * summed left to right, map-major then head-ascending: image i of a batch has the bits of a single-image call.
 * Refused before anything is launched: n_maps < 1 (or > 16), cur_step < 1, heads < 1, cols < 1, tokens < 1, null pointers. */
int hedit_attn_aggregate(float* const* h_maps, int n_maps, int heads, int tokens, int cols, int n_img, int cur_step,
                         float* out, void* stream);

/* ---- image autoencoder (SD-1.x AutoencoderKL): the steps either side of the editing loop ---------
 * replaces `model.vae.encode(image).latent_dist.mode()` (text-guided/main_p2p.py:159; also
 * p2p/ptp_classes.py:351-373) and `model.vae.decode(1 / 0.18215 * latents).sample`
 * (text-guided/main_p2p.py:263).  The 0.18215 scaling stays with the caller, as in the reference.
 * Parameters are addressed by their diffusers state_dict names (hedit_vae_param_name enumerates
 * them); fp32 device tensors in, packed to bf16 GEMM layouts on load.  Activations bf16 NHWC. */
typedef struct hedit_vae hedit_vae;
typedef struct hedit_vae_cfg {
  int in_channels;              /* 3 */
  int latent_channels;          /* 4 */
  int n_levels;                 /* number of entries used in block_out_channels (<= 4) */
  int block_out_channels[4];    /* 128,256,512,512; multiples of 64 */
  int layers_per_block;         /* 2 */
  int norm_num_groups;          /* 32 */
} hedit_vae_cfg;
int hedit_vae_create(const hedit_vae_cfg* cfg, hedit_vae** out);
void hedit_vae_destroy(hedit_vae* h);
int hedit_vae_num_params(const hedit_vae* h);
const char* hedit_vae_param_name(const hedit_vae* h, int i);
int hedit_vae_param_shape(const hedit_vae* h, int i, int* ndim, int* dims4);
int hedit_vae_load(hedit_vae* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_vae_missing(const hedit_vae* h);
/* workspace for a decode (encode = 0), an encode (encode = 1) or a decode_vjp (encode = 2) of B images
 * whose LATENT is h x w */
size_t hedit_vae_workspace_bytes(hedit_vae* h, int B, int latent_h, int latent_w, int encode);
/* z: fp32 [B][latent_channels][h][w] (already divided by the scaling factor)
 * -> image fp32 [B][in_channels][h*f][w*f], f = 2^(n_levels-1) */
int hedit_vae_decode(hedit_vae* h, const float* z, int B, int latent_h, int latent_w, float* image,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Vector-Jacobian product of the decoder: d_z = (d image / d z)^T d_image, what
 * `torch.autograd.grad(loss, latents)` pulls through `vae.decode` inside the reference's style-guidance
 * closure (text-guided-n-style/inversion/h_edit.py:146-185: x0 -> model.vae.decode -> image encoder ->
 * loss -> autograd.grad).  One call runs the forward (keeping block inputs and GroupNorm statistics
 * in the workspace) and the backward; no state survives the call.
 * z [B][latent_channels][h][w], d_image [B][in_channels][h*f][w*f] -> d_z like z; image (optional, may be
 * NULL) receives the decoded image as hedit_vae_decode would. */
int hedit_vae_decode_vjp(hedit_vae* h, const float* z, const float* d_image, int B, int latent_h, int latent_w,
                         float* d_z, float* image, void* workspace, size_t workspace_bytes, void* stream);
/* The same product in two calls, so that the caller's image encoder can run between them without a second
 * decoder forward: decode_keep = hedit_vae_decode that leaves its tape in the workspace (sized with
 * hedit_vae_workspace_bytes(.., 2)); decode_backward consumes it.  One outstanding forward per handle: a
 * further decode_keep drops the previous tape; the workspace must not be written in between. */
int hedit_vae_decode_keep(hedit_vae* h, const float* z, int B, int latent_h, int latent_w, float* image,
                          void* workspace, size_t workspace_bytes, void* stream);
int hedit_vae_decode_backward(hedit_vae* h, const float* d_image, float* d_z, void* workspace, void* stream);
/* image fp32 [B][in_channels][H][W] -> mean of the latent distribution, fp32 [B][latent_channels][H/f][W/f] */
int hedit_vae_encode(hedit_vae* h, const float* image, int B, int height, int width, float* mean,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- single kernels (parity tests) ------------------------------------------------------- */
/* C[M][N] = A . W^T (+bias)(+residual); mode 0 linear, 1 conv3x3 s1, 2 conv3x3 s2, 3 conv3x3 on
 * 2x nearest-upsampled input.  bf16 in/out.  splits: 0 = auto.  partial_ws may be NULL if the
 * call resolves to one split (query with hedit_k_gemm_ws_bytes). */
size_t hedit_k_gemm_ws_bytes(int M, int N, int K, int splits);
/* Batch-independent summation order.  The fp32 result of a contraction is DEFINED by a K-chunking that depends
 * on the layer's nominal shape only (per-image extent x 4 on the batch dimension): chunk sums are MFMA chains,
 * added in order.  hedit_k_gemm_canonical_chunk returns the chunk length in 64-deep K-tiles (0 = one chain);
 * hedit_k_gemm_plan_splits how many split-K slabs a launch of the ACTUAL shape uses to execute it (1 = chunks
 * folded in registers).  Both forms give the same bits, which hedit_k_gemm exposes for the tests:
 * splits > 0: that many slabs + reduce; splits < 0: the same chunking folded in one launch; 0: one plain chain. */
int hedit_k_gemm_canonical_chunk(int M_nominal, int N_nominal, int K);
int hedit_k_gemm_plan_splits(int M, int N, int K, int chunk_kt);
int hedit_k_gemm(const void* A, const void* W, const float* bias, const void* residual, void* C,
                 int M, int N, int K, int lda, int ldc, int ldr, int mode, int Hin, int Win,
                 int Cin, int Hout, int Wout, int splits, void* partial_ws, void* stream);
/* GroupNorm statistics taken by the producer (csrc/gnstat.h) -- what replaces the statistics pass of torch's GroupNorm in
 * the ResNet blocks of the pixel UNet (reference face-swapping/diffusion/diffusion.py:27-33 Normalize, :115-134 ResnetBlock).
 * hedit_k_conv_gn = hedit_k_gemm for a 3x3 convolution (mode 1..3; M % 128 == 0, N % 128 == 0 with the 128-column tile) that
 *   also writes gn_part[M / 128][N / 2][2] (fp32): (sum, sum of squares) of the stored bf16 output per unit of 128 rows and
 *   pair of adjacent channels, in a fixed summation tree -- the same bits whether the launch runs as one chain, folds its
 *   canonical chunks in registers (splits < 0) or goes through split-K slabs (splits > 0), and whatever shares the batch.
 * hedit_k_groupnorm_from_parts: y = GroupNorm(x) (+SiLU) for x [B][HW][C] = the channel concatenation of tensors with pair
 *   statistics part_a (ca channels) and part_b (cb channels, or null / 0); HW >= 1024, HW % 128 == 0, (C / G) even.
 *   ws: B * 512 bytes. */
int hedit_k_conv_gn(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int ldc,
                    int ldr, int mode, int Hin, int Win, int Cin, int Hout, int Wout, int splits, void* partial_ws, float* gn_part,
                    void* stream);
int hedit_k_groupnorm_from_parts(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                                 float eps, int silu, const float* part_a, int ca, const float* part_b, int cb, void* ws,
                                 void* stream);
/* FF1 of the transformer feed-forward with the GEGLU fused into the GEMM epilogue (diffusers
 * GEGLU.forward: hidden, gate = proj(x).chunk(2, -1); out = hidden * gelu(gate)).
 * hedit_k_pack_geglu interleaves the fp32 [2*inner][K] projection weight (and [2*inner] bias) of the
 * checkpoint layout into the row order the kernel wants; hedit_k_gemm_geglu then computes
 * C[M][inner] (bf16) from A[M][K] (bf16).  inner % 16 == 0, K % 8 == 0. */
int hedit_k_pack_geglu(const float* w, const float* bias, void* w_packed_bf16, float* bias_packed,
                       int inner, int K, void* stream);
int hedit_k_gemm_geglu(const void* A, const void* w_packed, const float* bias_packed, void* C, int M,
                       int inner, int K, int lda, int ldc, void* stream);
/* The token-local tail of a BasicTransformerBlock in one launch (csrc/ffn.hip), for C == hedit_k_ffn_channels() (320).
 * hedit_k_ffn_fused: out[M][C] = x + ff.net.2( GEGLU( ff.net.0.proj( LayerNorm(x) ) ) )  -- replaces diffusers'
 *   `hidden_states = self.ff(self.norm3(hidden_states)) + hidden_states` (oracle/sd_unet.py transformer block).
 * hedit_k_ffn_chain: the same with the linear layers either side of it,
 *   t2 = attn2.to_out.0(a) + t1;  t3 = t2 + ff(norm3(t2));  out = proj_out(t3) + x
 *   (oracle/sd_unet.py: the cross-attention output projection + residual in front, Transformer2DModel.proj_out +
 *   residual behind), x / t1 / a / out bf16 with row strides that are multiples of 8.
 * hedit_k_ffn_pack turns the checkpoint tensors w1 = ff.net.0.proj.weight [8C][C], b1 = ff.net.0.proj.bias [8C],
 * w2 = ff.net.2.weight [C][4C] (and w_pre = attn2.to_out.0.weight [C][C], w_post = proj_out.weight [C][C], both or
 * neither; fp32, device) into the weight stream (hedit_k_ffn_stream_bytes(with_outer_layers)) and the packed FF1 bias
 * (hedit_k_ffn_bias_bytes). */
int hedit_k_ffn_channels(void);
size_t hedit_k_ffn_stream_bytes(int with_outer_layers);
size_t hedit_k_ffn_bias_bytes(void);
int hedit_k_ffn_pack(const float* w1, const float* b1, const float* w2, const float* w_pre, const float* w_post, void* stream_out,
                     float* bias1_out, void* stream);
int hedit_k_ffn_fused(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps, const void* w_stream,
                      const float* bias1_packed, const float* bias2, void* out, int64_t ldo, int M, int C, void* stream);
int hedit_k_ffn_chain(const void* a, int64_t lda, const void* t1, int64_t ldt1, const void* x, int64_t ldx, const float* bias_pre,
                      const float* gamma, const float* beta, float eps, const void* w_stream, const float* bias1_packed,
                      const float* bias2, const float* bias_post, void* out, int64_t ldo, int M, int C, void* stream);
/* The projections around an attention of the same level in one launch (csrc/linchain.hip), two forms:
 *   n_out = 1 (gn_ss == NULL):  mid = attn1.to_out.0(a) + r1 (written to out_mid);  out[M][C] = attn2.to_q( norm2(mid) )
 *   n_out = 3 (gn_ss set):      mid = proj_in( a * scale + shift ) (GroupNorm applied on the fly; written to out_mid);
 *                               q, k = attn1.to_q / to_k ( norm1(mid) ) -> out_q, out_k;  out[C][ldo] = attn1.to_v(norm1(mid))^T
 *   (oracle/sd_unet.py: Transformer2DModel.norm / proj_in and BasicTransformerBlock attn1 / attn2 projections).
 * hedit_k_lin_chain_pack: checkpoint tensors [C][C] (fp32, device) -> weight stream; scale0 multiplies w0 (the softmax
 * scale folded into the query projection); w1, w2: both (n_out = 3) or neither.
 * hedit_k_groupnorm_affine: ss_out [B][C][2] = (scale, shift) per image and channel of GroupNorm(x). */
size_t hedit_k_lin_chain_stream_bytes(int n_out);
int hedit_k_lin_chain_pack(const float* w_pre, const float* w0, const float* w1, const float* w2, float scale0, void* stream_out,
                           void* stream);
int hedit_k_lin_chain(const void* a, int64_t lda, const void* r1, int64_t ldr1, const float* gn_ss, int rows_per_image,
                      const float* bias_pre, const float* gamma, const float* beta, float eps, const void* w_stream, void* out_mid,
                      int64_t ldmid, void* out_q, int64_t ldq, void* out_k, int64_t ldk, void* out, int64_t ldo, int M, int C,
                      void* stream);
/* Test entry (tests/test_gpu_chain_hazard.py): hedit_k_lin_chain with the kernel's wait schedule chosen -- sched 0 = the
 * product's (counted vmcnt windows around the bursts between the layers), 1 = every wait drained to vmcnt(0) lgkmcnt(0)
 * in front of its barrier: same arithmetic, no reliance on queue order or timing, i.e. the bits the product schedule must
 * reproduce under any memory load.  Never called by the executor. */
int hedit_k_lin_chain_sched(const void* a, int64_t lda, const void* r1, int64_t ldr1, const float* gn_ss, int rows_per_image,
                            const float* bias_pre, const float* gamma, const float* beta, float eps, const void* w_stream, void* out_mid,
                            int64_t ldmid, void* out_q, int64_t ldq, void* out_k, int64_t ldk, void* out, int64_t ldo, int M, int C,
                            int sched, void* stream);
/* The 16-bit storage format of this build: 0 = bfloat16 (libhedit_hip.so: the default, BASELINE configs[1], every benchmark
 * figure), 1 = IEEE half (libhedit_hip_f16.so, `build.py --f16`: the same kernels with -DHEDIT_STORE_F16).  Wherever this header
 * says "bf16" for a buffer of a kernel-level entry or for the P2P mix tables, read "the storage format of the build"; the
 * executors' own boundaries (images, latents, eps, checkpoints) are fp32 in either build. */
int hedit_storage_is_f16(void);
/* Test switch (tests/test_gpu_ring_hazard.py), process-wide, 0 by default and in every product path.
 * bit 0: the kernels whose operand rings are retired by COUNTED s_waitcnt vmcnt(N) -- igemm_kernel's three-stage ring and
 *        row-sharing 3x3 loop, ffn_chain_kernel, self_attn_kernel -- launch their drained twin: every ring wait is vmcnt(0)
 *        (and lgkmcnt(0)) in front of its barrier, same arithmetic in the same order.  The product schedule must reproduce
 *        those bits under any memory load.  (lin_chain_kernel has its own entry above.)
 * bit 1: self-attention takes the exact online-softmax pass only (no pinned-shift pass) -- the reference bits of the
 *        denominator-check / redo logic.
 * bit 2: the pixel UNet (hedit_ddpm_forward) takes the OTHER of its two GroupNorm statistics paths (statistics pass over the
 *        tensor / pair statistics from the producing convolution's epilogue, csrc/gnstat.h): tests/test_gpu_gn_stats.py
 *        compares the two on one library.
 * bit 3: gemm launches that would run a persistent kernel (csrc/pgemm.hip, csrc/pconv.hip) run the one-shot igemm_kernel of the
 *        same tile instead -- the same bits by construction; tools/pgemm_ab.py / tools/pconv_ab.py compare them (torch.equal)
 *        and time both on one box.
 * bit 4: the one-launch GroupNorm of images below 32 x 32 (csrc/norm.hip) launches its kept first form, gn_small_narrow_kernel
 *        (4 bytes per lane, grid (group, image)), instead of gn_small_kernel (wide vectors through LDS, the groups of an image on
 *        one XCD) -- the same bits by construction; tests/test_gpu_gn_small_bits.py compares them (torch.equal) and
 *        tools/gn_small_bench.py times both on one box. */
int hedit_test_set_flags(int flags);
size_t hedit_k_groupnorm_ws_bytes(int B, int HW, int C);
int hedit_k_groupnorm_affine(const void* x, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, void* ws,
                             float* ss_out, void* stream);
int hedit_k_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int B, int HW,
                      int C, int G, float eps, int silu, void* ws, void* stream);
int hedit_k_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                      int C, float eps, void* stream);
int hedit_k_geglu(const void* x, void* y, int64_t rows, int inner, void* stream);
int hedit_k_self_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt,
                      void* out, int ldo, int B, int N, int heads, int d, const int32_t* qk_src, const int32_t* kv_src,
                      void* stream);
/* class-matched mutual self-attention (hedit_p2p_plan.masa_rows): operands as hedit_k_self_attn; only the n_rows batch rows
 * listed in `rows` are computed and written.  Row b reads k, v and the key classes cls_k [B][N] of row kv_src[b] and the query
 * classes cls_q [B][N] of row b; bytes 0 / 1.  d in {32, 40, 64, 80, 160}, N % 64 == 0, 64 <= N <= 4096. */
int hedit_k_masked_self_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt, void* out, int ldo,
                             int B, int N, int heads, int d, const int32_t* rows, int n_rows, const int32_t* kv_src,
                             const uint8_t* cls_q, const uint8_t* cls_k, void* stream);
/* the two small kernels of hedit_p2p_plan.masa_auto: acc [rows][256] += head mean of the summed token columns of
 * probs [rows * heads][256][77] (the first rows / 2 rows sum the ref tokens, the others the cur tokens); and
 * acc [2 n][256] / count -> cls [4 n][res * res] as described at masa_auto (res <= 64) */
int hedit_k_masa_accumulate(const float* probs, int heads, int rows, const int32_t* ref_tokens, int n_ref,
                            const int32_t* cur_tokens, int n_cur, float* acc, void* stream);
int hedit_k_masa_auto_mask(const float* acc, int count, int n, int res, float thres, uint8_t* cls, void* stream);
int hedit_k_cross_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt,
                       void* out, int ldo, int B, int N, int heads, int d,
                       const hedit_p2p_plan* plan, float* store, void* stream);
/* the two kernels of the hook path: probs = softmax2(q k^T) as fp32 [B*heads][N][M] (q pre-scaled by scale * log2 e;
 * k: [B*kstride][ldk], the first M rows of every batch item count), then out = probs . v (vt: [heads*d][B*kstride]) */
int hedit_k_attn_probs(const void* q, int ldq, const void* k, int ldk, float* probs, int B, int N, int M, int kstride,
                       int heads, int d, void* stream);
int hedit_k_attn_apply(const float* probs, const void* vt, int64_t ldvt, void* out, int ldo, int B, int N, int M,
                       int kstride, int heads, int d, void* stream);
int hedit_k_pack_conv3x3(const float* w_oihw, void* out, int O, int I, void* stream);
int hedit_k_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);
/* The pieces of the image decoder's input-gradient pass (csrc/grad.hip; tests/test_gpu_grad_kernels.py), one launcher each,
 * and the forward kernels that feed them statistics and probabilities.  x / y / dy / dx / add / p / ds / du / src / dst and the
 * packed weights are bf16, NHWC where they are images; scores, dp, statistics and checkpoint weights are fp32.
 * hedit_k_groupnorm_stats: hedit_k_groupnorm that also writes stats [B][G][2] = (mean, rstd) per image and group, the buffer
 *   the backward pass is given; same ws, the same bits in y.
 * hedit_k_groupnorm_bwd: dx = d GroupNorm(+SiLU)(x) / dx applied to dy (+ add, or NULL): t = dz gamma,
 *   dx = rstd (t - mean_g(t) - xh mean_g(t xh)).  C % 8 == 0, C % G == 0, G <= 64, C / 8 a divisor of 256;
 *   ws of hedit_k_groupnorm_bwd_ws_bytes.
 * hedit_k_softmax_rows: p [rows][N] = softmax(scale * s) by rows, N % 4 == 0.  hedit_k_softmax_blockdiag: images of T tokens
 *   stacked along both axes of s [rows][ld]: the softmax inside each image's diagonal block, exact zeros elsewhere
 *   (T % 4, ld % 4, rows % T == 0).  hedit_k_softmax_bwd: ds = scale * p * (dp - rowsum(dp * p)), N % 4 == 0.
 * hedit_k_transpose: dst [C][R] = src [R][C]^T, R % 64 == 0 and C % 64 == 0.
 * hedit_k_sum2x2: dx [B][H][W][C] = the 2x2 block sums of du [B][2H][2W][C] (backward of the nearest 2x upsample), C % 8 == 0.
 * Weights of the input-gradient GEMMs from the checkpoint's fp32 tensors: hedit_k_pack_conv3x3_dgrad OIHW -> bf16 [I][9][O]
 *   with the taps flipped (the weight of hedit_k_gemm mode 1 with the channel counts swapped); hedit_k_pack_linear_t
 *   [O][I] -> bf16 [I][O]; hedit_k_flip_oihw k x k OIHW -> fp32 IOHW with the taps flipped. */
int hedit_k_groupnorm_stats(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                            float eps, int silu, void* ws, float* stats, void* stream);
size_t hedit_k_groupnorm_bwd_ws_bytes(int B, int HW, int C);
int hedit_k_groupnorm_bwd(const void* x, const void* dy, const void* add, void* dx, const float* gamma, const float* beta,
                          const float* stats, int B, int HW, int C, int G, int silu, void* ws, void* stream);
int hedit_k_softmax_rows(const float* s, void* p, int64_t rows, int N, float scale, void* stream);
int hedit_k_softmax_blockdiag(const float* s, void* p, int64_t rows, int T, int ld, float scale, void* stream);
int hedit_k_softmax_bwd(const void* p, const float* dp, void* ds, int64_t rows, int N, float scale, void* stream);
int hedit_k_transpose(const void* src, void* dst, int R, int C, void* stream);
int hedit_k_sum2x2(const void* du, void* dx, int B, int H, int W, int C, void* stream);
int hedit_k_pack_conv3x3_dgrad(const float* w_oihw, void* out, int O, int I, void* stream);
int hedit_k_pack_linear_t(const float* w, void* out, int O, int I, void* stream);
int hedit_k_flip_oihw(const float* w_oihw, float* out, int O, int I, int k, void* stream);
/* The two pieces the pixel UNet's input-gradient pass adds to those (csrc/s2dgrad.hip; tests/test_gpu_ddpm_grad.py).
 * hedit_k_conv3x3_s2_dgrad: dx [B][Hin][Win][I] = the input gradient of the stride-2 3x3 convolution with padding (0,1,0,1)
 *   (hedit_k_gemm mode 2 with asym; Hout = Hin / 2) applied to dy [B][Hin/2][Win/2][O].  Four sub-convolutions by the parity
 *   of the dx pixel (4 / 2 / 2 / 1 taps), one fp32 MFMA chain per element in an order fixed by the layer's shape.  w_packed =
 *   hedit_k_pack_conv3x3_s2_dgrad of the OIHW fp32 weight: bf16 [I][9][O], taps in place.  O % 64 == 0, I % 64 == 0, Hin, Win even.
 * hedit_k_slice_add: dst [rows][c] = src [rows][ld] columns [off, off + c) (accumulate == 0), or dst = the fp32 sum of dst
 *   and those columns rounded once (accumulate != 0): backward of the skip concatenation.  c, off, ld multiples of 8. */
int hedit_k_pack_conv3x3_s2_dgrad(const float* w_oihw, void* out, int O, int I, void* stream);
int hedit_k_conv3x3_s2_dgrad(const void* dy, const void* w_packed, void* dx, int B, int Hin, int Win, int O, int I, void* stream);
int hedit_k_slice_add(const void* src, int ld, int off, int c, void* dst, int64_t rows, int accumulate, void* stream);
/* The pieces the SD UNet's input-gradient pass adds to those (tests/test_gpu_unet_grad.py).  All 16-bit tensors in the
 * storage format of the build.
 * hedit_k_attn_bwd: multi-head self-attention backward without a T x T tensor and without atomics (csrc/attnbwd.hip).
 *   q, k as hedit_k_self_attn takes them ([B*N][ld], head h at column h*d, q pre-scaled by scale*log2(e)); v ROW-MAJOR
 *   [B*N][ldv] (not V^T); o = the forward's output and dout = its gradient, [B*N][ld].  dq [B*N][lddq] is the gradient with
 *   respect to the PRE-SCALED q; dk, dv are dense [B*N][heads*d].  ws of hedit_k_attn_bwd_ws_bytes.  d in {32, 40, 64, 80,
 *   160}, N % 64 == 0, every row stride a multiple of 8 and >= heads*d.
 * hedit_k_cross_attn_bwd_q: the query gradient of the attention over the 77 context rows (k, v [B*80][ld]; rows 77 .. 79 of an
 *   image are never read); the context is not differentiated.
 * hedit_k_cross_attn_bwd_kv: the other half, dk and dv [B*80][lddkv] at head column h*d (dk with respect to the unscaled k).
 *   The queries are split into chunks whose length depends on N alone (128; the last may be shorter): a block per (image,
 *   head, chunk) writes an fp32 partial, a second kernel sums the chunks in ascending order and rounds once -- no atomics,
 *   batch rows are the bits of single calls.  Rows 77 .. 79 of k, v are never read; those rows of dk, dv are written as exact
 *   zeros.  ws of hedit_k_cross_attn_bwd_kv_ws_bytes (16-byte aligned): the (lse, delta) statistics, then the partials.
 * hedit_k_layernorm_bwd: dx = d LayerNorm(x) / dx applied to dy (+ add, or NULL, summed in fp32 with one rounding); mean and
 *   rstd recomputed from x in fp32.  C % 8 == 0, C <= 1536.
 * hedit_k_geglu_bwd: x = [value | gate] [rows][2 inner] as hedit_k_geglu takes it, dy [rows][inner] the gradient of
 *   value * gelu(gate) -> dx [rows][2 inner], with the analytic derivative of the exact (erf) GELU.  inner % 8 == 0.
 * hedit_k_conv3x3_s2_dgrad_pad1: hedit_k_conv3x3_s2_dgrad for padding 1 all round (hedit_k_gemm mode 2 without asym): the
 *   parities mirrored, 1 / 2 / 2 / 4 taps; the same packed weight and the same conditions.
 * hedit_k_groupnorm_bwd_any: hedit_k_groupnorm_bwd for the widths of skip concatenations, as the executors call it: C / 8 need
 *   not divide 256 (the spare threads idle), and rows of more than 2048 channels (C / 8 in 257 .. 512: SD-1.5's 2560) run
 *   512-thread blocks.  Same arithmetic; the same ws size function. */
size_t hedit_k_attn_bwd_ws_bytes(int B, int N, int heads);
int hedit_k_attn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                     const void* dout, int lddo, void* dq, int lddq, void* dk, void* dv, int B, int N, int heads, int d,
                     void* ws, void* stream);
int hedit_k_cross_attn_bwd_q(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                             const void* dout, int lddo, void* dq, int lddq, int B, int N, int heads, int d, void* stream);
size_t hedit_k_cross_attn_bwd_kv_ws_bytes(int B, int N, int heads, int d);
int hedit_k_cross_attn_bwd_kv(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                              const void* dout, int lddo, void* dk, void* dv, int lddkv, int B, int N, int heads, int d, void* ws,
                              void* stream);
int hedit_k_layernorm_bwd(const void* x, const void* dy, const void* add, void* dx, const float* gamma, int64_t rows, int C,
                          float eps, void* stream);
int hedit_k_groupnorm_bwd_any(const void* x, const void* dy, const void* add, void* dx, const float* gamma, const float* beta,
                              const float* stats, int B, int HW, int C, int G, int silu, void* ws, void* stream);
int hedit_k_geglu_bwd(const void* x, const void* dy, void* dx, int64_t rows, int inner, void* stream);
int hedit_k_conv3x3_s2_dgrad_pad1(const void* dy, const void* w_packed, void* dx, int B, int Hin, int Win, int O, int I,
                                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel-space DDPM UNet of the face-swapping task: `Model.forward(x, t)` of
 * face-swapping/diffusion/diffusion.py:192-341, evaluated by face-swapping/inversion/h_edit_R.py:71,96,118
 * and inversion/sde_inversion.py:121.  Parameters by the state_dict names of that class
 * (temb.dense.0.weight, down.{i}.block.{j}.conv1.weight, down.{i}.attn.{j}.q.weight, mid.attn_1.proj_out.bias,
 * up.{i}.upsample.conv.weight, norm_out.weight, ...), fp32 device tensors in torch layouts.
 * attn_level[i] != 0 <=> the level's resolution is in the config's attn_resolutions. */
typedef struct hedit_ddpm hedit_ddpm;
typedef struct {
  int in_channels, out_ch, ch, n_levels;
  int ch_mult[8];
  int attn_level[8];
  int num_res_blocks, image_size;
} hedit_ddpm_cfg;
int hedit_ddpm_create(const hedit_ddpm_cfg* cfg, hedit_ddpm** out);
void hedit_ddpm_destroy(hedit_ddpm* h);
int hedit_ddpm_num_params(const hedit_ddpm* h);
const char* hedit_ddpm_param_name(const hedit_ddpm* h, int i);
int hedit_ddpm_param_shape(const hedit_ddpm* h, int i, int* ndim, int* dims4);
int hedit_ddpm_load(hedit_ddpm* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_ddpm_missing(const hedit_ddpm* h);
size_t hedit_ddpm_workspace_bytes(hedit_ddpm* h, int B);
/* x fp32 [B][in_channels][S][S], one timestep t for the batch (the reference passes ones(n) * t)
 * -> eps fp32 [B][out_ch][S][S] */
int hedit_ddpm_forward(hedit_ddpm* h, const float* x, float t, int B, float* eps, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Input gradient of the eps-network: d_x = (d eps / d x)^T d_eps, what `torch.autograd.grad(loss, xt)` pulls through
 * `model(xt, t)` in the face task's Edit Friendly mode (face-swapping/inversion/ef.py:64-66,95,106).  No weight gradient,
 * none w.r.t. t.
 * hedit_ddpm_create_grad = hedit_ddpm_create with the input-gradient weight twins attached (about as much device memory
 *   again; filled by the same hedit_ddpm_load calls).  Every entry above works on such a handle unchanged.
 * hedit_ddpm_forward_keep = hedit_ddpm_forward that leaves its tape (block inputs, conv1 outputs, GroupNorm statistics,
 *   attention q / k) in the workspace, sized with hedit_ddpm_grad_workspace_bytes.  The taped forward takes every
 *   GroupNorm's statistics itself, so where hedit_ddpm_forward takes them from the producing convolution (H*W >= 1024 and
 *   C % 128 == 0) eps can differ from it in the last bits; elsewhere the bits are equal.
 * hedit_ddpm_backward: d_eps [B][out_ch][S][S] -> d_x [B][in_channels][S][S], any number of times on one kept forward
 *   (ef.py:95 retain_graph=True, :106); the same cotangent gives the same bits.  One outstanding forward per handle: the
 *   next forward_keep, hedit_ddpm_release or hedit_ddpm_destroy drops the tape; the workspace must not be written in between.
 * hedit_ddpm_vjp: forward_keep + one backward + release in one call, the same bits.
 * A batch's rows are the bits of single calls, as everywhere. */
int hedit_ddpm_create_grad(const hedit_ddpm_cfg* cfg, hedit_ddpm** out);
size_t hedit_ddpm_grad_workspace_bytes(hedit_ddpm* h, int B);
int hedit_ddpm_forward_keep(hedit_ddpm* h, const float* x, float t, int B, float* eps, void* workspace,
                            size_t workspace_bytes, void* stream);
int hedit_ddpm_backward(hedit_ddpm* h, const float* d_eps, float* d_x, void* workspace, void* stream);
void hedit_ddpm_release(hedit_ddpm* h);
int hedit_ddpm_vjp(hedit_ddpm* h, const float* x, float t, const float* d_eps, int B, float* d_x, float* eps, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Identity reward of the face-swapping task: `IDLoss.get_cosine_loss(image)` of face-swapping/arcface/
 * arcface_model.py:40-67 (crop [35:223, 32:220] -> adaptive average pool 112 -> IR-SE50, model_irse.py:9-48 /
 * helpers.py:28-119 -> l2-normalised feature -> 1 - cos against the reference face's feature) fused with the gradient
 * w.r.t. the image that inversion/h_edit_R.py:103-106 takes from it with torch.autograd.grad.  fp32-quality
 * arithmetic (three-term split-bf16 products with fp32 accumulation, fp32 activations).  Parameters by the
 * reference's state_dict names (`input_layer.0.weight`, `body.3.res_layer.4.running_var`, `output_layer.3.weight`,
 * ...; the integer `num_batches_tracked` buffers are not parameters), fp32 device tensors in torch layouts;
 * hedit_irse50_finalize folds the BatchNorms and packs the GEMM operands once after loading. */
typedef struct hedit_irse hedit_irse;
int hedit_irse50_create(hedit_irse** out);
void hedit_irse50_destroy(hedit_irse* h);
int hedit_irse50_num_params(const hedit_irse* h);
const char* hedit_irse50_param_name(const hedit_irse* h, int i);
int hedit_irse50_param_shape(const hedit_irse* h, int i, int* ndim, int* dims4);
int hedit_irse50_load(hedit_irse* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_irse50_missing(const hedit_irse* h);
int hedit_irse50_finalize(hedit_irse* h, void* stream);
size_t hedit_irse50_workspace_bytes(hedit_irse* h, int B);
/* image fp32 [B][3][256][256] in [-1, 1] -> feat fp32 [B][512] = F.normalize(IDLoss.extract_feats(image)) */
int hedit_irse50_features(hedit_irse* h, const float* image, int B, float* feat, void* workspace,
                          size_t workspace_bytes, void* stream);
/* loss[b] = 1 - cos(feature(image_b), ref_feat); d_image [B][3][256][256] = d(scale * sum_b loss[b]) / d image
 * (scale = 1 / B: the reference's batch mean).  ref_feat: l2-normalised [512] (ref_per_image = 0) or [B][512]. */
int hedit_irse50_cos_fwd_bwd(hedit_irse* h, const float* image, const float* ref_feat, int ref_per_image, int B,
                             float scale, float* loss, float* d_image, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Perceptual reward of the face-swapping task: `LPIPS_Loss.get_lpips_loss(x)` of face-swapping/arcface/
 * arcface_model.py:69-94 = lpips.LPIPS(net='vgg')(x, src).mean() (lpips==0.1.4: ScalingLayer, VGG16 taps relu1_2 ...
 * relu5_3, channel-unit normalisation, squared difference, 1x1 lin weights, spatial mean, sum over taps) fused with
 * the gradient w.r.t. x that inversion/h_edit_R.py:124-132 takes with torch.autograd.grad.  Parameters by the lpips
 * state_dict names (`net.slice1.0.weight` ... `net.slice5.28.bias`, `lin0.model.1.weight` ... `lin4.model.1.weight`),
 * fp32 device tensors in torch layouts.  Image height / width: multiples of 16. */
typedef struct hedit_lpips hedit_lpips;
int hedit_lpips_create(hedit_lpips** out);
void hedit_lpips_destroy(hedit_lpips* h);
int hedit_lpips_num_params(const hedit_lpips* h);
const char* hedit_lpips_param_name(const hedit_lpips* h, int i);
int hedit_lpips_param_shape(const hedit_lpips* h, int i, int* ndim, int* dims4);
int hedit_lpips_load(hedit_lpips* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_lpips_missing(const hedit_lpips* h);
int hedit_lpips_finalize(hedit_lpips* h, void* stream);
size_t hedit_lpips_feature_floats(int height, int width);
size_t hedit_lpips_workspace_bytes(hedit_lpips* h, int B, int height, int width);
/* src fp32 [B][3][H][W] in [-1, 1] -> feats fp32 [B][hedit_lpips_feature_floats(H, W)] (normalised tap features) */
int hedit_lpips_source(hedit_lpips* h, const float* src, int B, int height, int width, float* feats,
                       void* workspace, size_t workspace_bytes, void* stream);
/* loss[b] = LPIPS(x_b, source); d_x = d(scale * sum_b loss[b]) / d x (scale = 1 / B: the reference's batch mean).
 * src_feats: one source shared by the batch (src_per_image = 0) or one per image. */
int hedit_lpips_fwd_bwd(hedit_lpips* h, const float* x, const float* src_feats, int src_per_image, int B, int height,
                        int width, float scale, float* loss, float* d_x, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Style encoder of the text + style task: `CLIPEncoder.get_gram_matrix_residual` of text-guided-n-style/clip_guidance/
 * base_clip.py:55-66 on the prefix of the CLIP ViT it exercises (clip/model.py:195-237,339-365: patch embedding, class +
 * positional embedding, ln_pre, the first `layers` ResidualAttentionBlocks): Gram matrix F^T F of the last block's patch
 * tokens, its residual against the style reference's Gram matrix and the Frobenius norm, fused with the gradient w.r.t.
 * the CLIP-normalised, resized image (what inversion/h_edit.py:170-179 pulls back into the decoder).  Parameters by the
 * OpenAI CLIP state_dict names (`visual.conv1.weight`, `visual.transformer.resblocks.{i}.attn.in_proj_weight`, ...).
 * width / heads = 64; at most 200 tokens. */
typedef struct hedit_vit hedit_vit;
typedef struct { int width, layers, heads, patch_size, input_resolution; } hedit_vit_cfg;
int hedit_vit_create(const hedit_vit_cfg* cfg, hedit_vit** out);
void hedit_vit_destroy(hedit_vit* h);
int hedit_vit_num_params(const hedit_vit* h);
const char* hedit_vit_param_name(const hedit_vit* h, int i);
int hedit_vit_param_shape(const hedit_vit* h, int i, int* ndim, int* dims4);
int hedit_vit_load(hedit_vit* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_vit_missing(const hedit_vit* h);
int hedit_vit_finalize(hedit_vit* h, void* stream);
size_t hedit_vit_workspace_bytes(hedit_vit* h, int B);
/* image fp32 [B][3][R][R] (CLIP-normalised, R = input_resolution) -> gram fp32 [B][width][width] */
int hedit_vit_gram(hedit_vit* h, const float* image, int B, float* gram, void* workspace, size_t workspace_bytes,
                   void* stream);
/* loss[b] = |Gram(image_b) - gram_ref|_F; d_image = d(scale * sum_b loss[b]) / d image.  gram_ref [width][width]
 * shared by the batch (ref_per_image = 0) or [B][width][width]. */
int hedit_vit_gram_fwd_bwd(hedit_vit* h, const float* image, const float* gram_ref, int ref_per_image, int B, float scale,
                           float* loss, float* d_image, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prompt encoder: `CLIP.encode_text` of text-guided-n-style/clip_guidance/clip/model.py:367-380 = transformers'
 * CLIPTextModel of SD-1.x.  Token + positional embedding, `layers` pre-LN residual blocks with a causal mask (fused q/k/v
 * projection, QuickGELU MLP), ln_final; forward only.  fp32 stream, split-bf16 contractions with fp32 accumulation; the
 * result is batch-invariant bit for bit, position i depends on the tokens 0..i alone, and both storage builds give the
 * same bits.  Parameters by the OpenAI CLIP state_dict names (`token_embedding.weight`, `positional_embedding`,
 * `transformer.resblocks.{i}.attn.in_proj_weight`, ..., `ln_final.weight`, `text_projection` [width][proj_dim] when
 * proj_dim > 0), fp32 device tensors; the token table stays fp32.  width / heads = 64; context_length <= 200; proj_dim 0
 * (no text_projection) or a multiple of 4. */
typedef struct hedit_text hedit_text;
typedef struct { int width, layers, heads, vocab_size, context_length, proj_dim; } hedit_text_cfg;
int hedit_text_create(const hedit_text_cfg* cfg, hedit_text** out);
void hedit_text_destroy(hedit_text* h);
int hedit_text_num_params(const hedit_text* h);
const char* hedit_text_param_name(const hedit_text* h, int i);
int hedit_text_param_shape(const hedit_text* h, int i, int* ndim, int* dims4);
int hedit_text_load(hedit_text* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_text_missing(const hedit_text* h);
int hedit_text_finalize(hedit_text* h, void* stream);
size_t hedit_text_workspace_bytes(hedit_text* h, int B, int L);
/* ids int32 [B][L] (device, 1 <= L <= context_length; an id outside the table is clamped, never read out of bounds) ->
 * hidden fp32 [B][L][width] after ln_final, or NULL;  pooled fp32 [B][proj_dim ? proj_dim : width] = the ln_final row at
 * pool_index[b] (int32 [B], device), times text_projection when there is one, or NULL (then pool_index may be NULL).
 * HEDIT_ERR_ARG, before anything is launched, for L or B out of range, a workspace below
 * hedit_text_workspace_bytes(h, B, L), `pooled` without `pool_index`, or nothing to write. */
int hedit_text_encode(hedit_text* h, const int32_t* ids, int B, int L, float* hidden, const int32_t* pool_index,
                      float* pooled, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CLIP image tower: `CLIP.encode_image` of text-guided-n-style/clip_guidance/clip/model.py:202-236 = transformers'
 * CLIPVisionModelWithProjection, the model of the PIE-Bench evaluator's CLIP score (text-guided/evaluation/
 * matrics_calculator.py:274).  Patch embedding, class token + positional embedding, ln_pre, `layers` pre-LN residual
 * blocks with bidirectional attention and a QuickGELU MLP, ln_post on the class row, times `visual.proj`; forward only.
 * fp32 stream, split-bf16 contractions with fp32 accumulation; attention walks the keys in LDS tiles of 128 with an online
 * softmax whose tile order is a function of the token count alone, so the result is batch-invariant bit for bit, does not
 * depend on the slice count of the attention grid, and both storage builds give the same bits.  Parameters by the OpenAI
 * CLIP state_dict names (`visual.conv1.weight`, `visual.class_embedding`, `visual.positional_embedding`, `visual.ln_pre.*`,
 * `visual.transformer.resblocks.{i}.attn.in_proj_weight`, ..., `visual.ln_post.*`, `visual.proj` [width][embed_dim]), fp32
 * device tensors.  width / heads = 64; (input_resolution / patch_size)^2 + 1 <= 577 tokens; embed_dim a multiple of 4. */
#define HEDIT_CLIPIMG_MAX_BATCH 256
typedef struct hedit_clipimg hedit_clipimg;
typedef struct { int width, layers, heads, patch_size, input_resolution, embed_dim; } hedit_clipimg_cfg;
int hedit_clipimg_create(const hedit_clipimg_cfg* cfg, hedit_clipimg** out);
void hedit_clipimg_destroy(hedit_clipimg* h);
int hedit_clipimg_num_params(const hedit_clipimg* h);
const char* hedit_clipimg_param_name(const hedit_clipimg* h, int i);
int hedit_clipimg_param_shape(const hedit_clipimg* h, int i, int* ndim, int* dims4);
int hedit_clipimg_load(hedit_clipimg* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_clipimg_missing(const hedit_clipimg* h);
int hedit_clipimg_finalize(hedit_clipimg* h, void* stream);
/* A TEST KNOB, not something a user ever needs: slices > 0 sets the number of workgroups the query rows of one (image, head)
 * are dealt to (clamped to the number of 32-row passes); 0, the default: one per pass.  It sizes the attention grid only --
 * the output bits do not depend on it, which is what the tests use it to show. */
int hedit_clipimg_set_slices(hedit_clipimg* h, int slices);
size_t hedit_clipimg_workspace_bytes(hedit_clipimg* h, int B);
/* image fp32 [B][3][R][R] (device; resized, CLIP-normalised) -> out fp32 [B][embed_dim], not normalised.  HEDIT_ERR_ARG,
 * before anything is launched, for B outside [1, HEDIT_CLIPIMG_MAX_BATCH] or a workspace below
 * hedit_clipimg_workspace_bytes(h, B); creation refuses width / heads != 64 and more than 577 tokens the same way. */
int hedit_clipimg_encode(hedit_clipimg* h, const float* image, int B, float* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * SqueezeNet-LPIPS, the `lpips*` columns of the PIE-Bench evaluator: LearnedPerceptualImagePatchSimilarity(net_type=
 * 'squeeze') of text-guided/evaluation/matrics_calculator.py:276,329-347.  ScalingLayer (compiled in), torchvision
 * squeezenet1_1.features with taps after features 1, 4, 7, 9, 10, 11, 12, every tap divided by its channel L2 norm + 1e-10,
 * squared difference, 1x1 lin weights, spatial mean, sum over the seven taps; forward only.  Exact fp32 (direct FMA and the
 * fp32 matrix instruction), fused Fire modules, no float atomics: dist[n] is bit-identical to the N = 1 call, symmetric in
 * (a, b) bit for bit, exactly 0 for a = b, and both storage builds give the same bits.  Parameters by the torchvision names
 * (`features.0.weight`, `features.{i}.squeeze|expand1x1|expand3x3.weight/.bias`, i in 3 4 6 7 9 10 11 12) and
 * `lin{k}.model.1.weight` (k = 0..6), fp32 device tensors in torch layouts. */
#define HEDIT_SQLPIPS_MAX_BATCH 64
typedef struct hedit_sqlpips hedit_sqlpips;
int hedit_sqlpips_create(hedit_sqlpips** out);
void hedit_sqlpips_destroy(hedit_sqlpips* h);
int hedit_sqlpips_num_params(const hedit_sqlpips* h);
const char* hedit_sqlpips_param_name(const hedit_sqlpips* h, int i);
int hedit_sqlpips_param_shape(const hedit_sqlpips* h, int i, int* ndim, int* dims4);
int hedit_sqlpips_load(hedit_sqlpips* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_sqlpips_missing(const hedit_sqlpips* h);
int hedit_sqlpips_finalize(hedit_sqlpips* h, void* stream);
size_t hedit_sqlpips_workspace_bytes(hedit_sqlpips* h, int N, int height, int width);
/* a, b fp32 [N][3][H][W] in [-1, 1] (device) -> dist fp32 [N], dist[n] = LPIPS(a_n, b_n).  HEDIT_ERR_STATE for a handle
 * that is not finalized, HEDIT_ERR_ARG for H or W outside [32, 4096] (no multiple-of-16 rule), N outside
 * [1, HEDIT_SQLPIPS_MAX_BATCH] or a workspace below hedit_sqlpips_workspace_bytes(h, N, H, W): all before anything is
 * launched. */
int hedit_sqlpips_distance(hedit_sqlpips* h, const float* a, const float* b, int N, int height, int width, float* dist,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DINO ViT key extractor and the key self-similarity distance, the `structure_distance*` columns of the PIE-Bench
 * evaluator (text-guided/evaluation/matrics_calculator.py:12-246,390-410): the images, as 0..255 floats times their masks,
 * are resized to input_resolution (bilinear, align_corners = False, no antialias), normalised with the ImageNet constants on
 * the 0..255 values, and run through the public DINO ViT (conv patch embedding with bias, cls_token + pos_embed, pre-LN
 * blocks with LayerNorm eps 1e-6, fused qkv, exact GELU) up to the keys of block `key_layer`; then S = K K^T /
 * max(|k_i| |k_j|, 1e-8) and dist = mean((S_a - S_b)^2).  Forward only.  Blocks 0 .. key_layer - 1 run whole, block
 * key_layer runs norm1 and the key third of qkv; nothing after that has a parameter slot.  fp32 stream, split-bf16
 * linear layers with fp32 accumulation, attention and both Gram matrices on the exact fp32 matrix instruction with an
 * order that is a function of the token count alone, no float atomics: dist[n] and keys[b] are bit-identical to the single
 * calls, dist is symmetric in (a, b) bit for bit and exactly 0 for a = b, and both storage builds give the same bits.
 * Parameters by the DINO state_dict names (`cls_token`, `pos_embed`, `patch_embed.proj.weight/.bias`,
 * `blocks.{i}.norm1|norm2.*`, `blocks.{i}.attn.qkv|proj.*`, `blocks.{i}.mlp.fc1|fc2.*`), fp32 device tensors.
 * width / heads = 64; (input_resolution / patch_size)^2 + 1 <= 1025 tokens. */
#define HEDIT_DINO_MAX_PAIRS 64
typedef struct hedit_dino hedit_dino;
typedef struct { int width, layers, heads, patch_size, input_resolution, key_layer; } hedit_dino_cfg;
/* HEDIT_ERR_ARG, before anything is allocated, for width / heads != 64, input_resolution % patch_size != 0, key_layer
 * outside [0, layers), or more than 1025 tokens */
int hedit_dino_create(const hedit_dino_cfg* cfg, hedit_dino** out);
void hedit_dino_destroy(hedit_dino* h);
int hedit_dino_num_params(const hedit_dino* h);
const char* hedit_dino_param_name(const hedit_dino* h, int i);
int hedit_dino_param_shape(const hedit_dino* h, int i, int* ndim, int* dims4);
int hedit_dino_load(hedit_dino* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_dino_missing(const hedit_dino* h);
int hedit_dino_finalize(hedit_dino* h, void* stream);
/* A TEST KNOB: slices > 0 sets the number of workgroups the query rows of one (image, head) are dealt to (clamped to the
 * number of 128-row passes); 0, the default: one per pass.  The output bits do not depend on it. */
int hedit_dino_set_slices(hedit_dino* h, int slices);
/* bytes hedit_dino_structure_distance needs for N pairs of S x S images; enough for hedit_dino_keys of B <= 2 N images */
size_t hedit_dino_workspace_bytes(hedit_dino* h, int N, int S);
/* image fp32 [B][3][S][S] (device; 0..255, already times its mask) -> keys fp32 [B][L][W] of block key_layer, bias
 * included.  HEDIT_ERR_STATE for a handle that is not finalized; HEDIT_ERR_ARG for B outside [1, 2 HEDIT_DINO_MAX_PAIRS],
 * S outside [patch_size, 4096] or a workspace that is too small: all before anything is launched. */
int hedit_dino_keys(hedit_dino* h, const float* image, int B, int S, float* keys, void* workspace, size_t workspace_bytes,
                    void* stream);
/* a, b fp32 [N][3][S][S] as above -> dist fp32 [N].  The same checks with N in [1, HEDIT_DINO_MAX_PAIRS]. */
int hedit_dino_structure_distance(hedit_dino* h, const float* a, const float* b, int N, int S, float* dist, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Face-parsing network of the face-swapping task: `FaceParsing()` of face-swapping/arcface/face_parsing_model.py
 * (CelebAMask-HQ U-Net, feature_scale 4: filters 16/32/64/128/256, transposed-convolution up-sampling, BatchNorm,
 * 19 classes, argmax) as main_edit.py:120-127 / :184 runs it.  Parameters by the reference's state_dict names
 * (`conv1.conv1.0.weight`, `up_concat4.up.weight`, `final.bias`, ...; the integer `num_batches_tracked` buffers are
 * not parameters), fp32 device tensors in torch layouts; hedit_faceparse_finalize packs the GEMM operands once.
 * batch_stats = 1: every BatchNorm uses the (mean, biased variance) of each image over H x W -- the reference's model is
 * never put in eval mode and is called with one image; results are bit-identical whatever the batch.  batch_stats = 0:
 * the running statistics (eval mode).  H and W: positive multiples of 16. */
typedef struct hedit_faceparse hedit_faceparse;
int hedit_faceparse_create(hedit_faceparse** out);
void hedit_faceparse_destroy(hedit_faceparse* h);
int hedit_faceparse_num_params(const hedit_faceparse* h);
const char* hedit_faceparse_param_name(const hedit_faceparse* h, int i);
int hedit_faceparse_param_shape(const hedit_faceparse* h, int i, int* ndim, int* dims4);
int hedit_faceparse_load(hedit_faceparse* h, const char* name, const float* dev_w, size_t numel, void* stream);
int hedit_faceparse_missing(const hedit_faceparse* h);
int hedit_faceparse_finalize(hedit_faceparse* h, void* stream);
size_t hedit_faceparse_workspace_bytes(hedit_faceparse* h, int B, int height, int width);
/* image fp32 [B][3][H][W] in [-1, 1] -> labels int64 [B][1][H][W] */
int hedit_faceparse_labels(hedit_faceparse* h, const float* image, int B, int height, int width, int batch_stats,
                           int64_t* labels, void* workspace, size_t workspace_bytes, void* stream);

/* Soft face mask of the face-swapping post-processing (main_edit.py:185-191): encode_segmentation's face + mouth map
 * (face_utils.py: ids {1..7, 10, 11, 12}, the mouth 10 counted twice) through SoftErosion(kernel_size, threshold,
 * iterations): iterations - 1 rounds of min(x, blur(x)), one more blur (zero-padded, normalised kernel_size^2 cone), then
 * hard = x >= threshold -> 1, other pixels divided by their maximum.  The maximum is taken per image (the reference calls
 * with one image).  No pixel below the threshold: soft = 1 everywhere; a maximum of 0: soft = 0 there.
 * labels int64 [B][1][H][W] -> soft fp32, hard uint8 [B][1][H][W]; kernel_size odd in [3, 31] (1 makes the cone 0 / 0),
 * iterations >= 1. */
size_t hedit_face_mask_workspace_bytes(int B, int height, int width);
int hedit_face_mask(const int64_t* labels, int B, int height, int width, int kernel_size, float threshold, int iterations,
                    float* soft, uint8_t* hard, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel metrics of the PIE-Bench evaluator (the psnr*, mse*, ssim* columns): torchmetrics' MeanSquaredError,
 * PeakSignalNoiseRatio(data_range=1) and StructuralSimilarityIndexMeasure(data_range=1) as
 * text-guided/evaluation/matrics_calculator.py:272-279 instantiates them, for N pairs and all three parts in one call.
 * pred, gt: uint8 [N][H][W][3] (what np.array(PIL image) holds); mask_pred, mask_gt: uint8 [N][H][W] with values 0 / 1, either may
 * be null = all ones.  out: double [N][3][3] = parts (whole, edit, unedit) x (mse, psnr, ssim): whole ignores the masks, edit
 * multiplies each image by its mask, unedit by 1 - mask; with both masks null the edit and unedit rows are NaN.
 * a = float(u8) / 255.0f times the mask and d = a - b in fp32; everything after that in fp64: mse = sum d d / (3 H W),
 * psnr = 10 log10(1 / mse) (+inf for mse 0), ssim = the mean over the (H - 10) x (W - 10) x 3 windows inside the image of the
 * 11-tap Gaussian (sigma 1.5, the evaluator's fp32 taps, separable) SSIM quotient with c1 = 1e-4, c2 = 9e-4.  Equal images
 * give exactly 0, +inf and 1.  Two launches, no atomics, fixed reduction order, nothing synchronises; out[n] has the bits of
 * the N = 1 call on pair n, in either storage build.  HEDIT_ERR_ARG for H or W outside [11, 16384], N outside
 * [1, HEDIT_PIXEL_METRICS_MAX_BATCH], a null pred / gt / out / workspace, an out or workspace that is not 8-byte aligned, or a
 * workspace below hedit_pixel_metrics_workspace_bytes(N, H, W) (0 for sizes out of range): all before anything is launched. */
#define HEDIT_PIXEL_METRICS_MAX_BATCH 64
size_t hedit_pixel_metrics_workspace_bytes(int N, int height, int width);
int hedit_pixel_metrics(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask_pred, const uint8_t* mask_gt, int N, int height,
                        int width, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image preprocessing of the evaluator's CLIP metrics (csrc/imgprep.hip): PIL's Image.resize on 8-bit RGB, a crop and a
 * per-channel look-up, bit for bit.  src: uint8 [B][H][W][3] (what np.array(PIL image) holds).  The image is resampled to
 * resized_height x resized_width by Pillow's two passes (horizontal, then vertical, the intermediate rounded and clamped to
 * uint8; 22-bit fixed-point taps, int32 accumulator starting at 1 << 21, clamp(acc >> 22, 0, 255)), of which only the window
 * [top, top + crop_height) x [left, left + crop_width) is computed.  out: fp32 [B][3][crop_height][crop_width] =
 * lut[channel][pixel], lut fp32 [3][256]; out_u8 (may be null): the pixels themselves, uint8 [B][crop_height][crop_width][3].
 * The filter is the caller's: taps_x int32 [resized_width][ksize_x] and bounds_x int32 [resized_width][2] = (first source
 * index, count <= ksize_x) per output column, taps_y / bounds_y / ksize_y likewise per output row, all in device memory
 * (hedit/image_prep.py builds Pillow's bilinear and bicubic tables).  A null taps / bounds pair means that axis keeps its size
 * (Pillow skips the pass).  row0, nrows: the source rows the crop's vertical taps read, [min first, max first + count) over
 * the crop's rows (top, crop_height when the height is unchanged); a pair of the table that leaves that range is cut to it.
 * Two launches through a uint8 workspace [B][nrows][crop_width][3], no atomics, nothing synchronises; image b has the bits of
 * the B = 1 call, in either storage build.  HEDIT_ERR_ARG, before anything is launched, for a null src / lut / out /
 * workspace, B outside [1, HEDIT_IMAGE_PREP_MAX_BATCH], H, W or a resized size outside [1, 16384], a crop that leaves the
 * resized image, a null table for an axis whose size changes, ksize outside [1, HEDIT_IMAGE_PREP_MAX_TAPS], source rows that
 * leave the image, or a workspace below hedit_image_prep_workspace_bytes(B, nrows, crop_width) (0 for arguments out of range). */
#define HEDIT_IMAGE_PREP_MAX_BATCH 64
#define HEDIT_IMAGE_PREP_MAX_TAPS 1024
size_t hedit_image_prep_workspace_bytes(int B, int nrows, int crop_width);
int hedit_image_prep(const uint8_t* src, int B, int height, int width, int resized_height, int resized_width, int top, int left,
                     int crop_height, int crop_width, const int32_t* taps_x, const int32_t* bounds_x, int ksize_x,
                     const int32_t* taps_y, const int32_t* bounds_y, int ksize_y, int row0, int nrows, const float* lut, float* out,
                     uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream);

/* The head of the evaluator's local_clip column (clip_directional_loss with the DirectionMetric of
 * text-guided/evaluation/local_clip_evaluation.py), P pairs in one launch, one workgroup per pair.
 * txt: fp32 [P][2][T][E], the T template prompts of the source prompt (index 0) and of the target prompt (index 1) as the text
 * tower returns them; img: fp32 [P][2][E], source image then target image; out: double [P].  In fp64 after the loads:
 * s^_j = s_j / |s_j|, t^_j = t_j / |t_j|; d = sum_j (t^_j - s^_j) / T with j in index order; D = d / |d|; a^ = a / |a|,
 * b^ = b / |b|; e = b^ - a^; e^ = e / (|e| + 1e-7); out = e^ . D / (max(|e^|, 1e-8) max(|D|, 1e-8)).  Every reduction over E
 * is a fixed tree that depends on E alone: out[p] has the bits of the P = 1 call, in either storage build.  Equal image
 * features give exactly 0.0, equal prompt features NaN (the reference's 0 / 0).  HEDIT_ERR_ARG, before the launch, for a null
 * pointer, P outside [1, 64], T outside [1, 256], E not a multiple of 4 or above 4096, or an out that is not 8-byte aligned. */
#define HEDIT_CLIP_DIRECTION_MAX_PAIRS 64
#define HEDIT_CLIP_DIRECTION_MAX_TEMPLATES 256
#define HEDIT_CLIP_DIRECTION_MAX_DIM 4096
int hedit_clip_direction(const float* txt, const float* img, int P, int T, int E, double* out, void* stream);

/* ---- single kernels (parity tests), precise family ------------------------------------------------
 * The kernels of the "precise" path (csrc/pnet.hip, encoder.hip, the attention / LayerNorm gradient kernels of vit.hip) one
 * by one, for tests/test_gpu_precise_kernels.py.  Thin wrappers: no product kernel and no dispatch is changed by them.  All
 * pointers are device pointers unless said otherwise; activations are fp32, the split operands bfloat16 in BOTH storage
 * builds.  Integer ops are the P_* values of csrc/kernels.h: 0 copy, 1 affine p x + q, 2 PReLU, 3 PReLU gradient, 4 ReLU,
 * 5 ReLU gradient, 6 QuickGELU, 7 QuickGELU gradient, 8 affine + ReLU, 9 exact GELU.
 *
 * hedit_k_split3_geometry: the operand geometry of C channels (host pointers): Cs = the stride between the three parts
 *   (C when 3 C <= 64 or 3 C % 64 == 0, else C rounded up to 64), Kp = 3 Cs rounded up to 64 = the operand's row length.
 * hedit_k_split3: x fp32 [rows_in][ldx] (ldx >= C) -> out bf16 [rows_out][Kp]: columns [0, C) hi, [Cs, Cs + C) hi,
 *   [2 Cs, 2 Cs + C) lo of v = op(x) (worder = 1: hi, lo, hi), every other column exact zero.  hi = bf16(v), lo = bf16(v - hi).
 *   z: the pre-activation of the *_GRAD ops (same geometry and ldx as x), else unused.  p, q [C] (q may be null for the
 *   activations; both are needed by the affine ops), or [B][C] with pq_img = 1 (affine ops only).  geo 0: rows_out = rows_in;
 *   geo 1: x is [B][H][W] pixels, out the pixels (2 oy, 2 ox): rows_out = B (H / 2)(W / 2), H and W EVEN (no caller has odd
 *   ones; an odd size is not supported); geo 2: out is [B][2H][2W], pixel (2 y, 2 x) = pixel (y, x) of x, the others exact
 *   zero.  B, H, W describe x and are read only with geo != 0 or pq_img.  Eight columns per thread when C % 8 == 0,
 *   Cs % 8 == 0 and ldx % 4 == 0 (x, z 16-byte aligned), else one: same bits.
 * hedit_k_pack_split3_w: w fp32 OIHW [O][I][k][k] (k = 1 or 3) -> bf16 [rows_out][k k][Kp], parts (hi, lo, hi) of
 *   w[o][i][tap] * scale[o] (scale null: 1).  dgrad 0: row o, channel i (Cs, Kp of I, rows_out >= O); dgrad 1: row i,
 *   channel o, tap k k - 1 - tap (Cs, Kp of O, rows_out >= I).  perm_hw > 0: the input index i of the packed operand counts
 *   (hw, ch) with ch < perm_c and addresses w's input ch * perm_hw + hw (a Linear behind an NCHW flatten).  Rows beyond the
 *   real count and every padding column are exact zeros.
 * hedit_k_precise_conv: one layer as the executors run it (op_split, then pgemm of csrc/pnet.h on an arena over `ws`):
 *   x fp32 [B * Hin * Win][Cin], Cin = dgrad ? O : I, through hedit_k_split3's op / p / q / pq_img / z / geo (ldx = Cin), times
 *   the weight packed as above from w_oihw (+ scale, perm_hw, perm_c).  With (Hs, Ws) = the size after geo: mode 0 a linear
 *   layer over the B Hs Ws rows (k = 1), mode 1 a 3x3 stride-1 pad-1 convolution, mode 2 a 3x3 stride-2 pad-1 one (Hs, Ws
 *   even).  out fp32 [M][rows], rows = (dgrad ? I : O) rounded up to 4 (the padding columns are exact zeros), M = B Hs Ws
 *   (mode 2: a quarter).  The summation order is the canonical one of M / B rows per image: *chunk_kt and *splits (host
 *   pointers, may be null) return gemm_canonical_chunk's and gemm_plan_splits' answers for the launch.  ws: at least
 *   hedit_k_precise_conv_ws_bytes, 256-byte aligned.
 *
 * pnet.hip, one entry per launcher (C = channels, NHWC fp32 activations):
 *   bn_affine: p[i] = g / sqrt(v + eps), q[i] = b - m p for i < C rep, channel i % C.  bn_fold_bias: p likewise,
 *     q = (bias - m) p + b (bias null: 0).
 *   act: y = act(x + q[c]) over `total` elements, op 2 (PReLU, slope p[c]) or 4 (ReLU); q may be null.
 *   se_nslab(HW): pixel slabs of the SE reductions.  se_pool: part[b][slab][c] = sum over the slab's pixels of u [B][HW][C].
 *     se_fc: pool = (sum of the slabs in order) / HW + bias; h [B][R] = relu(W1 pool), s [B][C] = sigmoid(W2 h); w1 [R][C],
 *     w2 [C][R], C <= 512, R <= 32.  se_combine: Y = (u + bias) s[b][c] + shortcut, shortcut = sc + sc_bias (sc given) or
 *     X [B][Ho stride][Wo stride][C] at (stride y, stride x).  se_bwd_reduce: part[b][slab][c] = sum dY (u + bias).
 *     se_fc_bwd: r [B][C] = W1^T((W2^T(gs s (1 - s))) [h > 0]) / HW with gs the slab sum.
 *   unit_bwd_combine: dX [B][H][W][C] = p[c] dxa + (y, x both multiples of stride ? dsc[b][y / stride][x / stride][c] : 0).
 *   scale_cols: y[i] = x[i] p[i % n].
 *   face_pool: img [B][3][256][256] -> [B][112][112][3]: adaptive average pool of the crop [35:223, 32:220].  face_pool_bwd:
 *     g [B 112 112][ldg] (the first three columns) -> dimg [B][3][256][256], zero outside the crop.
 *   cos_head: f = raw + bias [B][D <= 512]; e = f / |f|; e2 = e / max(|e|, 1e-12) -> feat (or null); with ref
 *     [B][ref_stride] (ref_stride 0: shared): loss[b] = 1 - <e2, ref>, df = d(scale loss_b) / d raw (either may be null).
 *   lpips_prep: img [B][3][H][W] -> [B H W][3] = (img - shift_c) / scale_c; lpips_prep_bwd: g [B H W][ldg] -> dimg = g / scale_c.
 *     shift3, scale3: HOST pointers to three floats.
 *   maxpool2: z [B][H][W][C] (H, W even) -> zp [B][H/2][W/2][C], idx uint8 = the winner 2 dy + dx (the first of equals).
 *     maxpool2_bwd: G [B][H][W][C] = add (or 0) + (the pixel won ? gp : 0).
 *   lpips_head: F = relu(z + bias) [B HW][C <= 512], Fn = F / (|F| + 1e-10).  src null: fn_out = Fn.  Else with src
 *     [..][HW][C] (image b at src + b src_img_stride, 0 = shared): dpix[pixel] = sum_c w_c (Fn - src)^2 and, if dF is given,
 *     dF = d(gscale sum_pixels dpix) / dF.
 *   lpips_reduce: acc[b] (first) = or += mean over the HW pixels of dpix.
 * encoder.hip: patchify (bwd = 1: X -> img), tokens, gather_rows, ln (stats [rows][2] = (mean, rstd) or null),
 *   add_bias_res -- the layouts in csrc/kernels.h.
 * vit.hip (head dimension 64, L <= 200 tokens, W = 64 * heads): ln_bwd: dx = add (or 0) + the LayerNorm input gradient from
 *   the kept (mean, rstd).  attn_fwd: qkv [B L][3W] raw + bias [3W] -> A [B L][W], lse [B][heads][L] of the scaled scores.
 *   attn_bwd: dq, dk, dv into dqkv [B L][3W] (every element written).  slices: the grid's third dimension (query rows or
 *   keys per workgroup), 0 = what the executor picks from heads and B, else 1 .. 4: the bits do not depend on it.
 *   drop_cls: dE [B][L-1][W] = dT [B][1 + l].  gram_bwd: dT [L][W] row 0 = 0, row 1 + l = (2 scale / *nrm) FR[l]
 *   (0 when *nrm is 0); nrm a device pointer. */
int hedit_k_split3_geometry(int C, int* Cs, int* Kp);
int hedit_k_split3(const float* x, int ldx, const float* z, const float* p, const float* q, int pq_img, int op, void* out, int Kp,
                   int Cs, int C, int geo, int B, int H, int W, int worder, int64_t rows_out, void* stream);
int hedit_k_pack_split3_w(const float* w, const float* scale, void* out, int O, int I, int k, int dgrad, int Cs, int Kp, int rows_out,
                          int perm_hw, int perm_c, void* stream);
size_t hedit_k_precise_conv_ws_bytes(int O, int I, int k, int dgrad, int mode, int geo, int B, int Hin, int Win);
int hedit_k_precise_conv(const float* x, int op, const float* p, const float* q, int pq_img, const float* z, int geo,
                         const float* w_oihw, const float* scale, int O, int I, int k, int perm_hw, int perm_c, int dgrad, int mode,
                         int B, int Hin, int Win, float* out, int* chunk_kt, int* splits, void* ws, size_t ws_bytes, void* stream);
int hedit_k_bn_affine(const float* g, const float* b, const float* m, const float* v, float eps, float* p, float* q, int C, int rep,
                      void* stream);
int hedit_k_bn_fold_bias(const float* bias, const float* g, const float* b, const float* m, const float* v, float eps, float* p,
                         float* q, int C, void* stream);
int hedit_k_act(const float* x, const float* p, const float* q, float* y, int64_t total, int C, int op, void* stream);
int hedit_k_se_nslab(int HW);
int hedit_k_se_pool(const float* u, float* part, int B, int HW, int C, void* stream);
int hedit_k_se_fc(const float* part, const float* bias, const float* w1, const float* w2, float* hbuf, float* sbuf, int B, int HW,
                  int C, int R, void* stream);
int hedit_k_se_combine(const float* u, const float* bias, const float* s, const float* sc, const float* sc_bias, const float* X,
                       int stride, float* Y, int B, int Ho, int Wo, int C, void* stream);
int hedit_k_se_bwd_reduce(const float* dY, const float* u, const float* bias, float* part, int B, int HW, int C, void* stream);
int hedit_k_se_fc_bwd(const float* part, const float* sbuf, const float* hbuf, const float* w1, const float* w2, float* rbuf, int B,
                      int C, int R, int HW, void* stream);
int hedit_k_unit_bwd_combine(const float* dxa, const float* p, const float* dsc, int stride, float* dX, int B, int H, int W, int C,
                             void* stream);
int hedit_k_scale_cols(const float* x, const float* p, float* y, int64_t total, int n, void* stream);
int hedit_k_face_pool(const float* img, float* out, int B, void* stream);
int hedit_k_face_pool_bwd(const float* g, int ldg, float* dimg, int B, void* stream);
int hedit_k_cos_head(const float* raw, const float* bias, const float* ref, int ref_stride, float* feat, float* loss, float* df,
                     int B, int D, float scale, void* stream);
int hedit_k_lpips_prep(const float* img, float* out, const float* shift3, const float* scale3, int B, int H, int W, void* stream);
int hedit_k_lpips_prep_bwd(const float* g, int ldg, float* dimg, const float* scale3, int B, int H, int W, void* stream);
int hedit_k_maxpool2(const float* z, float* zp, uint8_t* idx, int B, int H, int W, int C, void* stream);
int hedit_k_maxpool2_bwd(const float* gp, const uint8_t* idx, const float* add, float* G, int B, int H, int W, int C, void* stream);
int hedit_k_lpips_head(const float* z, const float* bias, const float* src, int64_t src_img_stride, const float* w, float* fn_out,
                       float* dpix, float* dF, int B, int HW, int C, float gscale, void* stream);
int hedit_k_lpips_reduce(const float* dpix, float* acc, int B, int HW, int first, void* stream);
int hedit_k_enc_patchify(const float* img, float* X, int B, int R, int p, int bwd, void* stream);
int hedit_k_enc_tokens(const float* E, const float* cbias, const float* cls, const float* pos, float* T, int B, int L, int W,
                       void* stream);
int hedit_k_enc_gather_rows(const float* T, const int32_t* idx, float* R, int B, int L, int W, void* stream);
int hedit_k_enc_ln(const float* x, const float* g, const float* b, float* y, float* stats, int64_t rows, int W, float eps,
                   void* stream);
int hedit_k_enc_add_bias_res(const float* raw, const float* bias, const float* res, float* out, int64_t total, int W, void* stream);
int hedit_k_vit_ln_bwd(const float* x, const float* dy, const float* g, const float* stats, const float* add, float* dx, int64_t rows,
                       int W, void* stream);
int hedit_k_vit_attn_fwd(const float* qkv, const float* bias, float* A, float* lse, int B, int L, int heads, int slices,
                         void* stream);
int hedit_k_vit_attn_bwd(const float* qkv, const float* bias, const float* A, const float* dA, const float* lse, float* dqkv, int B,
                         int L, int heads, int slices, void* stream);
int hedit_k_vit_drop_cls(const float* dT, float* dE, int B, int L, int W, void* stream);
int hedit_k_vit_gram_bwd(const float* FR, const float* nrm, float* dT, int L, int W, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
