// C-ABI glue: error reporting, sampler-step entry points and the single-kernel entry points the
// parity tests call (see include/hedit.h).
#include "../../include/hedit.h"
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <utility>

#include "common.h"
#include "kernels.h"
#include "pnet.h"

static thread_local std::string g_last_error;
void hedit_set_error(const std::string& msg) { g_last_error = msg; }

int hedit_abi_catch() noexcept {
  try {
    try {
      throw;
    } catch (const std::bad_alloc&) {
      g_last_error = "out of host memory inside libhedit_hip";
    } catch (const std::exception& e) {
      g_last_error = std::string("C++ exception inside libhedit_hip: ") + e.what();
    } catch (...) {
      g_last_error = "unknown C++ exception inside libhedit_hip";
    }
  } catch (...) {
    // even the message could not be stored; the code alone reports the failure
  }
  return HEDIT_ERR_STATE;
}

#include <atomic>
static std::atomic<int> g_test_flags{0};
int hedit_test_flags() { return g_test_flags.load(std::memory_order_relaxed); }

namespace {
std::mutex g_dev_mu;
std::set<std::pair<const void*, int>> g_lds_set;      // (kernel, device) pairs whose dynamic-LDS limit was raised
std::map<int, int> g_cus;                              // device -> CU count
}  // namespace

int hedit_dyn_lds(const void* kernel, int bytes) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (g_lds_set.count({kernel, dev})) return HEDIT_OK;
  HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  g_lds_set.insert({kernel, dev});
  return HEDIT_OK;
}

int hedit_cu_count(int* cus) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto it = g_cus.find(dev);
  if (it == g_cus.end()) {
    int n = 0;
    HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    it = g_cus.emplace(dev, n).first;
  }
  *cus = it->second;
  return HEDIT_OK;
}

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline StepCoef to_coef(const hedit_step_coef* c) {
  StepCoef k;
  k.sqrt_ab_t = c->sqrt_ab_t; k.sqrt_1m_ab_t = c->sqrt_1m_ab_t; k.sqrt_ab_prev = c->sqrt_ab_prev;
  k.dir_coef = c->dir_coef; k.noise_coef = c->noise_coef;
  k.w_src = c->w_src; k.w_hat = c->w_hat; k.w_tar = c->w_tar; k.coeff = c->coeff; k.w_rec = c->w_rec;
  return k;
}

extern "C" {

const char* hedit_last_error(void) { return g_last_error.c_str(); }
int hedit_version(void) { return 1; }

int hedit_step_base(const float* eps, const float* xt, const float* z, float* x_prev, int n_img, int elems,
                    int eps_rows_per_img, const hedit_step_coef* c, void* stream) try {
  ARG_CHECK(eps && xt && x_prev && c && n_img > 0 && elems > 0, "step_base args");
  return step_base_launch(eps, xt, z, x_prev, n_img, elems, eps_rows_per_img, to_coef(c), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_pair(const float* e_u, const float* e_c, const float* xt, const float* z, float* x_next, int n_img, int elems,
                    int n_kinds, const hedit_step_coef* c, void* stream) try {
  ARG_CHECK(e_u && e_c && xt && x_next && c && n_img > 0 && elems > 0 && (n_kinds == 1 || n_kinds == 2), "step_pair args");
  const StepCoef k[2] = {to_coef(c), to_coef(c + (n_kinds - 1))};
  return step_pair_launch(e_u, e_c, xt, z, x_next, n_img, elems, n_kinds, k, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_invert(const float* e_u, const float* e_c, const float* xt, float* x_prev, float* z_out, int n_img,
                      int elems, const hedit_step_coef* c, void* stream) try {
  ARG_CHECK(e_u && e_c && xt && x_prev && z_out && c && n_img > 0 && elems > 0, "step_invert args");
  return step_invert_launch(e_u, e_c, xt, x_prev, z_out, n_img, elems, to_coef(c), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_update(const float* e_u_src, const float* e_c_src, const float* e_u_tar, const float* e_c_tar,
                      int64_t stride_img, const float* x_k, const float* x_base, float* x_out, int n_img,
                      int elems, int k_gt0, const hedit_step_coef* c, void* stream) try {
  ARG_CHECK(e_u_src && e_c_src && e_u_tar && e_c_tar && x_k && x_base && x_out && c, "step_update args");
  return step_update_launch(e_u_src, e_c_src, e_u_tar, e_c_tar, (long)stride_img, x_k, x_base, x_out, n_img,
                            elems, k_gt0, to_coef(c), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_tweedie(const float* e_u_tar, const float* e_c_tar, int64_t stride_img, const float* x, float* z0,
                       int n_img, int elems, float w_tar, float sqrt_ab, float sqrt_1m_ab, float inv_scale, void* stream) try {
  ARG_CHECK(e_u_tar && e_c_tar && x && z0 && sqrt_ab > 0.f, "step_tweedie args");
  return step_tweedie_launch(e_u_tar, e_c_tar, (long)stride_img, x, z0, n_img, elems, w_tar, sqrt_ab, sqrt_1m_ab, inv_scale,
                             S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_style(const float* e_u_src, const float* e_c_src, const float* e_u_tar, const float* e_c_tar,
                     int64_t stride_img, const float* x, const float* g_z, float* x_out, int n_img, int elems, float w_hat,
                     float w_tar, float chain, float weight, void* stream) try {
  ARG_CHECK(e_u_src && e_c_src && e_u_tar && e_c_tar && x && g_z && x_out, "step_style args");
  return step_style_launch(e_u_src, e_c_src, e_u_tar, e_c_tar, (long)stride_img, x, g_z, x_out, n_img, elems, w_hat, w_tar,
                           chain, weight, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_ef_seed(const float* g_z, float* d_eps, int n_img, int elems, float w_tar, float a, float c, void* stream) try {
  ARG_CHECK(g_z && d_eps && n_img >= 1 && elems >= 1, "step_ef_seed args");
  (void)a;      // the direct term a * g_z belongs to step_ef_style: the seed carries the path through eps only
  return step_ef_seed_launch(g_z, d_eps, n_img, elems, w_tar, c, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_step_ef_style(const float* e_u, const float* e_c, int64_t stride_img, const float* dx, const float* g_z,
                        const float* x_prev, float* x_out, int n_img, int elems, float a, float weight, void* stream) try {
  ARG_CHECK(e_u && e_c && dx && g_z && x_prev && x_out && n_img >= 1 && elems >= 1, "step_ef_style args");
  return step_ef_style_launch(e_u, e_c, (long)stride_img, dx, g_z, x_prev, x_out, n_img, elems, a, weight, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_local_blend(float* const* h_maps, int n_maps, int heads, const float* alpha_layers,
                      const int32_t* enabled, float* xt, int n_img, int C, int H, int W, float th, void* stream) try {
  ARG_CHECK(h_maps && alpha_layers && xt, "local_blend args");
  return local_blend_launch(const_cast<const float* const*>(h_maps), n_maps, heads, alpha_layers, nullptr, enabled, xt, n_img, C, H, W, th,
                            0.f, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_local_blend_sub(float* const* h_maps, int n_maps, int heads, const float* alpha_layers, const float* substruct_layers,
                          const int32_t* enabled, float* xt, int n_img, int C, int H, int W, float th, float th_sub, void* stream) try {
  ARG_CHECK(h_maps && alpha_layers && substruct_layers && xt, "local_blend_sub args");
  return local_blend_launch(const_cast<const float* const*>(h_maps), n_maps, heads, alpha_layers, substruct_layers, enabled, xt, n_img, C,
                            H, W, th, th_sub, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_attn_aggregate(float* const* h_maps, int n_maps, int heads, int tokens, int cols, int n_img, int cur_step, float* out,
                         void* stream) try {
  ARG_CHECK(h_maps, "attn_aggregate: h_maps is null");
  ARG_CHECK(out, "attn_aggregate: out is null");
  return attn_aggregate_launch(const_cast<const float* const*>(h_maps), n_maps, heads, tokens, cols, n_img, cur_step, out, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_axis_mix(const float* in, float* out, const int32_t* idx, const float* val, int nnz, int64_t outer, int n_in, int n_out, int inner,
                   void* stream) try {
  ARG_CHECK(in && out && idx && val, "axis_mix args");
  return axis_mix_launch(in, out, idx, val, nnz, (long)outer, n_in, n_out, inner, S(stream));
} catch (...) { return hedit_abi_catch(); }

size_t hedit_k_gemm_ws_bytes(int M, int N, int K, int splits) try {
  const int s = gemm_pick_splits(M, N, K, splits);
  return gemm_partial_bytes(M, N, s);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* the canonical (batch-independent) chunking of a layer and the slab count a launch of the actual shape uses */
int hedit_k_gemm_canonical_chunk(int M_nominal, int N_nominal, int K) { return gemm_canonical_chunk(M_nominal, N_nominal, K); }
int hedit_k_gemm_plan_splits(int M, int N, int K, int chunk_kt) { return gemm_plan_splits(M, N, K, chunk_kt); }

int hedit_k_gemm(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N,
                 int K, int lda, int ldc, int ldr, int mode, int Hin, int Win, int Cin, int Hout, int Wout,
                 int splits, void* partial_ws, void* stream) try {
  ARG_CHECK(A && W && C, "gemm args");
  GemmParams p{};
  p.A = reinterpret_cast<const bf16_t*>(A);
  p.W = reinterpret_cast<const bf16_t*>(W);
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.mode = mode;
  p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Hout = Hout; p.Wout = Wout;
  p.bias = bias;
  p.residual = reinterpret_cast<const bf16_t*>(residual);
  p.ldr = ldr;
  p.C = reinterpret_cast<bf16_t*>(C);
  p.ldc = ldc;
  if (splits < 0) {
    // the same chunking as `-splits` slabs, folded in registers by one launch (bit-identical by construction)
    const int kt = K / 64;
    const int s = gemm_pick_splits(M, N, K, -splits);
    p.chunk_kt = (kt + s - 1) / s;
    return gemm_launch(p, 1, nullptr, S(stream));
  }
  const int s = gemm_pick_splits(M, N, K, splits);
  return gemm_launch(p, s, reinterpret_cast<float*>(partial_ws), S(stream));
} catch (...) { return hedit_abi_catch(); }

/* hedit_k_gemm for a convolution (mode 1..3) that also writes the GroupNorm pair statistics of its output (csrc/gnstat.h) */
int hedit_k_conv_gn(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int ldc,
                    int ldr, int mode, int Hin, int Win, int Cin, int Hout, int Wout, int splits, void* partial_ws, float* gn_part,
                    void* stream) try {
  ARG_CHECK(A && W && C && gn_part, "conv_gn args");
  GemmParams p{};
  p.A = reinterpret_cast<const bf16_t*>(A);
  p.W = reinterpret_cast<const bf16_t*>(W);
  p.M = M; p.N = N; p.K = K; p.lda = Cin; p.mode = mode;
  p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Hout = Hout; p.Wout = Wout;
  p.bias = bias;
  p.residual = reinterpret_cast<const bf16_t*>(residual);
  p.ldr = ldr;
  p.C = reinterpret_cast<bf16_t*>(C);
  p.ldc = ldc;
  p.gn_part = gn_part;
  if (splits < 0) {
    const int kt = K / 64;
    const int s = gemm_pick_splits(M, N, K, -splits);
    p.chunk_kt = (kt + s - 1) / s;
    return gemm_launch(p, 1, nullptr, S(stream));
  }
  const int s = gemm_pick_splits(M, N, K, splits);
  return gemm_launch(p, s, reinterpret_cast<float*>(partial_ws), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_groupnorm_from_parts(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                                 float eps, int silu, const float* part_a, int ca, const float* part_b, int cb, void* ws,
                                 void* stream) try {
  ARG_CHECK(x && y && gamma && beta && part_a && ws, "groupnorm_from_parts args");
  return groupnorm_from_parts_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), gamma, beta, B, HW, C, G,
                                     eps, silu, part_a, ca, part_b, cb, reinterpret_cast<float*>(ws), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_geglu(const float* w, const float* bias, void* w_packed_bf16, float* bias_packed, int inner, int K,
                       void* stream) try {
  ARG_CHECK(w && w_packed_bf16, "pack_geglu args");
  int rc = pack_geglu_rows_launch(w, reinterpret_cast<bf16_t*>(w_packed_bf16), nullptr, 2 * inner, K, S(stream));
  if (rc != HEDIT_OK || !bias) return rc;
  ARG_CHECK(bias_packed, "pack_geglu: bias_packed");
  return pack_geglu_rows_launch(bias, nullptr, bias_packed, 2 * inner, 1, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_gemm_geglu(const void* A, const void* w_packed, const float* bias_packed, void* C, int M, int inner, int K,
                       int lda, int ldc, void* stream) try {
  ARG_CHECK(A && w_packed && C, "gemm_geglu args");
  GemmParams p{};
  p.A = reinterpret_cast<const bf16_t*>(A);
  p.W = reinterpret_cast<const bf16_t*>(w_packed);
  p.M = M; p.N = 2 * inner; p.K = K; p.lda = lda; p.mode = 0;
  p.bias = bias_packed;
  p.C = reinterpret_cast<bf16_t*>(C);
  p.ldc = ldc;
  p.geglu = 1;
  return gemm_launch(p, 1, nullptr, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_ffn_channels(void) { return ffn_fused_channels(); }
size_t hedit_k_ffn_stream_bytes(int with_outer_layers) { return ffn_stream_bytes(with_outer_layers, with_outer_layers); }
size_t hedit_k_ffn_bias_bytes(void) { return ffn_bias_bytes(); }

int hedit_k_ffn_pack(const float* w1, const float* b1, const float* w2, const float* w_pre, const float* w_post, void* stream_out,
                     float* bias1_out, void* stream) try {
  ARG_CHECK(w1 && b1 && w2 && stream_out && bias1_out && ((w_pre == nullptr) == (w_post == nullptr)), "ffn_pack args");
  const int outer = w_pre != nullptr;
  bf16_t* so = reinterpret_cast<bf16_t*>(stream_out);
  int rc = ffn_pack_launch(w1, 1, outer, outer, so, S(stream));
  if (rc == HEDIT_OK) rc = ffn_pack_launch(w2, 2, outer, outer, so, S(stream));
  if (rc == HEDIT_OK && outer) rc = ffn_pack_launch(w_pre, 0, 1, 1, so, S(stream));
  if (rc == HEDIT_OK && outer) rc = ffn_pack_launch(w_post, 3, 1, 1, so, S(stream));
  if (rc != HEDIT_OK) return rc;
  return ffn_pack_bias_launch(b1, bias1_out, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_ffn_fused(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps, const void* w_stream,
                      const float* bias1_packed, const float* bias2, void* out, int64_t ldo, int M, int C, void* stream) try {
  FfnParams f{};
  f.x = reinterpret_cast<const bf16_t*>(x); f.ldx = (long)ldx; f.gamma = gamma; f.beta = beta; f.eps = eps;
  f.stream = reinterpret_cast<const bf16_t*>(w_stream); f.bias1p = bias1_packed; f.bias2 = bias2;
  f.out = reinterpret_cast<bf16_t*>(out); f.ldo = (long)ldo; f.M = M; f.C = C;
  return ffn_fused_launch(f, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_ffn_chain(const void* a, int64_t lda, const void* t1, int64_t ldt1, const void* x, int64_t ldx, const float* bias_pre,
                      const float* gamma, const float* beta, float eps, const void* w_stream, const float* bias1_packed, const float* bias2,
                      const float* bias_post, void* out, int64_t ldo, int M, int C, void* stream) try {
  ARG_CHECK(a && t1 && x, "ffn_chain args");
  FfnParams f{};
  f.a = reinterpret_cast<const bf16_t*>(a); f.lda = (long)lda;
  f.x = reinterpret_cast<const bf16_t*>(t1); f.ldx = (long)ldt1;
  f.r2 = reinterpret_cast<const bf16_t*>(x); f.ldr2 = (long)ldx;
  f.bias_pre = bias_pre; f.bias_post = bias_post;
  f.gamma = gamma; f.beta = beta; f.eps = eps;
  f.stream = reinterpret_cast<const bf16_t*>(w_stream); f.bias1p = bias1_packed; f.bias2 = bias2;
  f.out = reinterpret_cast<bf16_t*>(out); f.ldo = (long)ldo; f.M = M; f.C = C;
  return ffn_fused_launch(f, S(stream));
} catch (...) { return hedit_abi_catch(); }

size_t hedit_k_lin_chain_stream_bytes(int n_out) { return lin_chain_stream_bytes(n_out == 3 ? 4 : 2); }

int hedit_k_lin_chain_pack(const float* w_pre, const float* w0, const float* w1, const float* w2, float scale0, void* stream_out,
                           void* stream) try {
  ARG_CHECK(w_pre && w0 && stream_out && ((w1 == nullptr) == (w2 == nullptr)), "lin_chain_pack args");
  const int layers = w1 ? 4 : 2;
  bf16_t* so = reinterpret_cast<bf16_t*>(stream_out);
  int rc = lin_chain_pack_launch(w_pre, 0, 1.f, layers, so, S(stream));
  if (rc == HEDIT_OK) rc = lin_chain_pack_launch(w0, 1, scale0, layers, so, S(stream));
  if (rc == HEDIT_OK && w1) rc = lin_chain_pack_launch(w1, 2, 1.f, layers, so, S(stream));
  if (rc == HEDIT_OK && w1) rc = lin_chain_pack_launch(w2, 3, 1.f, layers, so, S(stream));
  return rc;
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lin_chain(const void* a, int64_t lda, const void* r1, int64_t ldr1, const float* gn_ss, int rows_per_image,
                      const float* bias_pre, const float* gamma, const float* beta, float eps, const void* w_stream, void* out_mid,
                      int64_t ldmid, void* out_q, int64_t ldq, void* out_k, int64_t ldk, void* out, int64_t ldo, int M, int C,
                      void* stream) try {
  LinChainParams c{};
  c.a = reinterpret_cast<const bf16_t*>(a); c.lda = (long)lda; c.r1 = reinterpret_cast<const bf16_t*>(r1); c.ldr1 = (long)ldr1;
  c.bias_pre = bias_pre; c.gamma = gamma; c.beta = beta; c.eps = eps; c.stream = reinterpret_cast<const bf16_t*>(w_stream);
  c.out_mid = reinterpret_cast<bf16_t*>(out_mid); c.ldmid = (long)ldmid; c.out = reinterpret_cast<bf16_t*>(out); c.ldo = (long)ldo;
  c.M = M; c.C = C; c.gn_ss = gn_ss; c.rows_per_image = rows_per_image;
  c.out_q = reinterpret_cast<bf16_t*>(out_q); c.ldq = (long)ldq; c.out_k = reinterpret_cast<bf16_t*>(out_k); c.ldk = (long)ldk;
  return lin_chain_launch(c, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_storage_is_f16(void) { return HEDIT_F16; }

int hedit_test_set_flags(int flags) try {
  ARG_CHECK(flags >= 0 && flags <= 31, "hedit_test_set_flags: bit 0 drained ring waits, bit 1 exact self-attention pass, bit 2 pixel-UNet GroupNorm statistics path flipped, bit 3 no persistent linear kernel, bit 4 narrow one-launch GroupNorm");
  g_test_flags.store(flags, std::memory_order_relaxed);
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lin_chain_sched(const void* a, int64_t lda, const void* r1, int64_t ldr1, const float* gn_ss, int rows_per_image,
                            const float* bias_pre, const float* gamma, const float* beta, float eps, const void* w_stream, void* out_mid,
                            int64_t ldmid, void* out_q, int64_t ldq, void* out_k, int64_t ldk, void* out, int64_t ldo, int M, int C,
                            int sched, void* stream) try {
  LinChainParams c{};
  c.a = reinterpret_cast<const bf16_t*>(a); c.lda = (long)lda; c.r1 = reinterpret_cast<const bf16_t*>(r1); c.ldr1 = (long)ldr1;
  c.bias_pre = bias_pre; c.gamma = gamma; c.beta = beta; c.eps = eps; c.stream = reinterpret_cast<const bf16_t*>(w_stream);
  c.out_mid = reinterpret_cast<bf16_t*>(out_mid); c.ldmid = (long)ldmid; c.out = reinterpret_cast<bf16_t*>(out); c.ldo = (long)ldo;
  c.M = M; c.C = C; c.gn_ss = gn_ss; c.rows_per_image = rows_per_image;
  c.out_q = reinterpret_cast<bf16_t*>(out_q); c.ldq = (long)ldq; c.out_k = reinterpret_cast<bf16_t*>(out_k); c.ldk = (long)ldk;
  return lin_chain_launch_sched(c, sched, S(stream));
} catch (...) { return hedit_abi_catch(); }

size_t hedit_k_groupnorm_ws_bytes(int B, int HW, int C) { return groupnorm_ws_bytes(B, HW, C); }

int hedit_k_groupnorm_affine(const void* x, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, void* ws,
                             float* ss_out, void* stream) try {
  ARG_CHECK(x && gamma && beta && ws && ss_out, "groupnorm_affine args");
  const float* ss = nullptr;
  int rc = groupnorm_affine_launch(reinterpret_cast<const bf16_t*>(x), gamma, beta, B, HW, C, G, eps, reinterpret_cast<float*>(ws), S(stream), &ss);
  if (rc != HEDIT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ss_out, ss, (size_t)B * C * 2 * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_k_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                      float eps, int silu, void* ws, void* stream) try {
  ARG_CHECK(x && y && gamma && beta && ws, "groupnorm args");
  return groupnorm_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), gamma, beta, B, HW, C, G,
                          eps, silu, reinterpret_cast<float*>(ws), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                      void* stream) try {
  ARG_CHECK(x && y && gamma && beta, "layernorm args");
  return layernorm_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), gamma, beta, (long)rows, C, eps, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_geglu(const void* x, void* y, int64_t rows, int inner, void* stream) try {
  ARG_CHECK(x && y, "geglu args");
  return geglu_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), (long)rows, inner, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_self_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt, void* out, int ldo,
                      int B, int N, int heads, int d, const int32_t* qk_src, const int32_t* kv_src, void* stream) try {
  ARG_CHECK(q && k && vt && out, "self_attn args");
  SelfAttnParams p{};
  p.q = reinterpret_cast<const bf16_t*>(q); p.ldq = ldq;
  p.k = reinterpret_cast<const bf16_t*>(k); p.ldk = ldk;
  p.vt = reinterpret_cast<const bf16_t*>(vt); p.ldvt = (long)ldvt;
  p.out = reinterpret_cast<bf16_t*>(out); p.ldo = ldo;
  p.B = B; p.N = N; p.heads = heads; p.d = d; p.qk_src = qk_src; p.kv_src = kv_src;
  return self_attn_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_masked_self_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt, void* out, int ldo,
                             int B, int N, int heads, int d, const int32_t* rows, int n_rows, const int32_t* kv_src,
                             const uint8_t* cls_q, const uint8_t* cls_k, void* stream) try {
  ARG_CHECK(q && k && vt && out && rows && kv_src && cls_q && cls_k, "masked_self_attn args");
  MaskedSelfAttnParams p{};
  p.q = reinterpret_cast<const bf16_t*>(q); p.ldq = ldq;
  p.k = reinterpret_cast<const bf16_t*>(k); p.ldk = ldk;
  p.vt = reinterpret_cast<const bf16_t*>(vt); p.ldvt = (long)ldvt;
  p.out = reinterpret_cast<bf16_t*>(out); p.ldo = ldo;
  p.B = B; p.N = N; p.heads = heads; p.d = d;
  p.rows = rows; p.n_rows = n_rows; p.kv_src = kv_src; p.cls_q = cls_q; p.cls_k = cls_k;
  return masked_self_attn_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_masa_accumulate(const float* probs, int heads, int rows, const int32_t* ref_tokens, int n_ref,
                            const int32_t* cur_tokens, int n_cur, float* acc, void* stream) try {
  return masa_accumulate_launch(probs, heads, rows, ref_tokens, n_ref, cur_tokens, n_cur, acc, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_masa_auto_mask(const float* acc, int count, int n, int res, float thres, uint8_t* cls, void* stream) try {
  return masa_auto_mask_launch(acc, count, n, res, thres, cls, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_cross_attn(const void* q, int ldq, const void* k, int ldk, const void* vt, int64_t ldvt, void* out, int ldo,
                       int B, int N, int heads, int d, const hedit_p2p_plan* plan, float* store, void* stream) try {
  ARG_CHECK(q && k && vt && out && plan, "cross_attn args");
  CrossAttnParams p{};
  p.q = reinterpret_cast<const bf16_t*>(q); p.ldq = ldq;
  p.k = reinterpret_cast<const bf16_t*>(k); p.ldk = ldk;
  p.vt = reinterpret_cast<const bf16_t*>(vt); p.ldvt = (long)ldvt;
  p.out = reinterpret_cast<bf16_t*>(out); p.ldo = ldo;
  p.B = B; p.N = N; p.heads = heads; p.d = d;
  p.n_pairs = plan->n_pairs; p.pair_src = plan->pair_src; p.pair_tar = plan->pair_tar;
  p.mixT = reinterpret_cast<const bf16_t*>(plan->mixT); p.bvec = plan->bvec;
  p.singles = plan->singles; p.n_single = plan->n_single;
  p.store = store;
  return cross_attn_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_attn_probs(const void* q, int ldq, const void* k, int ldk, float* probs, int B, int N, int M, int kstride,
                       int heads, int d, void* stream) try {
  ARG_CHECK(q && k && probs, "attn_probs args");
  AttnProbsParams p{};
  p.q = reinterpret_cast<const bf16_t*>(q); p.ldq = ldq;
  p.k = reinterpret_cast<const bf16_t*>(k); p.ldk = ldk;
  p.probs = probs; p.B = B; p.N = N; p.M = M; p.kstride = kstride; p.heads = heads; p.d = d;
  return attn_probs_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_attn_apply(const float* probs, const void* vt, int64_t ldvt, void* out, int ldo, int B, int N, int M,
                       int kstride, int heads, int d, void* stream) try {
  ARG_CHECK(probs && vt && out, "attn_apply args");
  AttnProbsParams p{};
  p.probs = const_cast<float*>(probs);
  p.vt = reinterpret_cast<const bf16_t*>(vt); p.ldvt = (long)ldvt;
  p.out = reinterpret_cast<bf16_t*>(out); p.ldo = ldo;
  p.B = B; p.N = N; p.M = M; p.kstride = kstride; p.heads = heads; p.d = d;
  return attn_apply_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_conv3x3(const float* w, void* out, int O, int I, void* stream) try {
  ARG_CHECK(w && out, "pack args");
  return pack_conv3x3_launch(w, reinterpret_cast<bf16_t*>(out), O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_f32_to_bf16(const float* x, void* y, int64_t n, void* stream) try {
  ARG_CHECK(x && y, "cast args");
  return f32_to_bf16_launch(x, reinterpret_cast<bf16_t*>(y), (long)n, S(stream));
} catch (...) { return hedit_abi_catch(); }

// ---- the decoder's backward pieces (grad.hip) and the forward kernels that feed them statistics and probabilities
int hedit_k_groupnorm_stats(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                            float eps, int silu, void* ws, float* stats, void* stream) try {
  ARG_CHECK(x && y && gamma && beta && ws && stats, "groupnorm_stats args");
  return groupnorm_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), gamma, beta, B, HW, C, G,
                          eps, silu, reinterpret_cast<float*>(ws), S(stream), stats);
} catch (...) { return hedit_abi_catch(); }

size_t hedit_k_groupnorm_bwd_ws_bytes(int B, int HW, int C) { return groupnorm_bwd_ws_bytes(B, HW, C); }

int hedit_k_groupnorm_bwd(const void* x, const void* dy, const void* add, void* dx, const float* gamma, const float* beta,
                          const float* stats, int B, int HW, int C, int G, int silu, void* ws, void* stream) try {
  ARG_CHECK(x && dy && dx && gamma && beta && stats && ws, "groupnorm_bwd args");
  return groupnorm_bwd_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<const bf16_t*>(dy),
                              reinterpret_cast<const bf16_t*>(add), reinterpret_cast<bf16_t*>(dx), gamma, beta, stats, B, HW, C,
                              G, silu, reinterpret_cast<float*>(ws), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_softmax_rows(const float* s, void* p, int64_t rows, int N, float scale, void* stream) try {
  ARG_CHECK(s && p, "softmax_rows args");
  return softmax_rows_launch(s, reinterpret_cast<bf16_t*>(p), (long)rows, N, scale, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_softmax_blockdiag(const float* s, void* p, int64_t rows, int T, int ld, float scale, void* stream) try {
  ARG_CHECK(s && p, "softmax_blockdiag args");
  return softmax_blockdiag_launch(s, reinterpret_cast<bf16_t*>(p), (long)rows, T, ld, scale, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_softmax_bwd(const void* p, const float* dp, void* ds, int64_t rows, int N, float scale, void* stream) try {
  ARG_CHECK(p && dp && ds, "softmax_bwd args");
  return softmax_bwd_launch(reinterpret_cast<const bf16_t*>(p), dp, reinterpret_cast<bf16_t*>(ds), (long)rows, N, scale, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_transpose(const void* src, void* dst, int R, int C, void* stream) try {
  ARG_CHECK(src && dst, "transpose args");
  return transpose_bf16_launch(reinterpret_cast<const bf16_t*>(src), reinterpret_cast<bf16_t*>(dst), R, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_sum2x2(const void* du, void* dx, int B, int H, int W, int C, void* stream) try {
  ARG_CHECK(du && dx, "sum2x2 args");
  return sum2x2_launch(reinterpret_cast<const bf16_t*>(du), reinterpret_cast<bf16_t*>(dx), B, H, W, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_conv3x3_dgrad(const float* w, void* out, int O, int I, void* stream) try {
  ARG_CHECK(w && out, "pack args");
  return pack_conv3x3_dgrad_launch(w, reinterpret_cast<bf16_t*>(out), O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_conv3x3_s2_dgrad(const float* w, void* out, int O, int I, void* stream) try {
  ARG_CHECK(w && out, "pack args");
  return pack_conv3x3_s2_dgrad_launch(w, reinterpret_cast<bf16_t*>(out), O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_conv3x3_s2_dgrad(const void* dy, const void* w_packed, void* dx, int B, int Hin, int Win, int O, int I, void* stream) try {
  ARG_CHECK(dy && w_packed && dx, "conv3x3_s2_dgrad args");
  return conv3x3_s2_dgrad_launch(reinterpret_cast<const bf16_t*>(dy), reinterpret_cast<const bf16_t*>(w_packed),
                                 reinterpret_cast<bf16_t*>(dx), B, Hin, Win, O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_slice_add(const void* src, int ld, int off, int c, void* dst, int64_t rows, int accumulate, void* stream) try {
  ARG_CHECK(src && dst && rows >= 0, "slice_add args");
  return slice_add_launch(reinterpret_cast<const bf16_t*>(src), ld, off, c, reinterpret_cast<bf16_t*>(dst), (long)rows, accumulate,
                          S(stream));
} catch (...) { return hedit_abi_catch(); }

// ---- the pieces of the SD UNet's input-gradient pass (attnbwd.hip, grad.hip, s2dgrad.hip)
size_t hedit_k_attn_bwd_ws_bytes(int B, int N, int heads) { return attn_bwd_ws_bytes(B, N, heads); }

static AttnBwdParams attn_bwd_params(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                                     const void* dout, int lddo, void* dq, int lddq, int B, int N, int heads, int d) {
  AttnBwdParams p{};
  p.q = reinterpret_cast<const bf16_t*>(q); p.ldq = ldq;
  p.k = reinterpret_cast<const bf16_t*>(k); p.ldk = ldk;
  p.v = reinterpret_cast<const bf16_t*>(v); p.ldv = ldv;
  p.o = reinterpret_cast<const bf16_t*>(o); p.ldo = ldo;
  p.dout = reinterpret_cast<const bf16_t*>(dout); p.lddo = lddo;
  p.dq = reinterpret_cast<bf16_t*>(dq); p.lddq = lddq;
  p.B = B; p.N = N; p.heads = heads; p.d = d;
  return p;
}

int hedit_k_attn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                     const void* dout, int lddo, void* dq, int lddq, void* dk, void* dv, int B, int N, int heads, int d,
                     void* ws, void* stream) try {
  ARG_CHECK(q && k && v && o && dout && dq && dk && dv && ws, "attn_bwd args");
  AttnBwdParams p = attn_bwd_params(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, B, N, heads, d);
  p.dk = reinterpret_cast<bf16_t*>(dk); p.dv = reinterpret_cast<bf16_t*>(dv); p.lddkv = heads * d;
  p.stats = reinterpret_cast<float*>(ws);
  p.M = N; p.kstride = N;
  return attn_bwd_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_cross_attn_bwd_q(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                             const void* dout, int lddo, void* dq, int lddq, int B, int N, int heads, int d, void* stream) try {
  ARG_CHECK(q && k && v && o && dout && dq, "cross_attn_bwd_q args");
  AttnBwdParams p = attn_bwd_params(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, B, N, heads, d);
  p.M = HEDIT_MAXW; p.kstride = HEDIT_CTXP;
  return attn_bwd_launch(p, S(stream));
} catch (...) { return hedit_abi_catch(); }

size_t hedit_k_cross_attn_bwd_kv_ws_bytes(int B, int N, int heads, int d) {
  if (B < 1 || N < 1 || heads < 1 || d < 1) return 0;
  return attn_bwd_ws_bytes(B, N, heads) + attn_bwd_ctx_kv_ws_bytes(B, N, heads, d);
}

int hedit_k_cross_attn_bwd_kv(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                              const void* dout, int lddo, void* dk, void* dv, int lddkv, int B, int N, int heads, int d, void* ws,
                              void* stream) try {
  ARG_CHECK(q && k && v && o && dout && dk && dv && ws, "cross_attn_bwd_kv args");
  ARG_CHECK(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "cross_attn_bwd_kv: the workspace must be 16-byte aligned");
  AttnBwdParams p = attn_bwd_params(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, nullptr, 0, B, N, heads, d);
  p.M = HEDIT_MAXW; p.kstride = HEDIT_CTXP;
  p.stats = reinterpret_cast<float*>(ws);
  const int rc = attn_bwd_launch(p, S(stream));      // (lse, delta) per query; no dq
  if (rc != HEDIT_OK) return rc;
  p.dk = reinterpret_cast<bf16_t*>(dk); p.dv = reinterpret_cast<bf16_t*>(dv); p.lddkv = lddkv;
  return attn_bwd_ctx_kv_launch(p, p.stats + attn_bwd_ws_bytes(B, N, heads) / sizeof(float), S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_groupnorm_bwd_any(const void* x, const void* dy, const void* add, void* dx, const float* gamma, const float* beta,
                              const float* stats, int B, int HW, int C, int G, int silu, void* ws, void* stream) try {
  ARG_CHECK(x && dy && dx && gamma && beta && stats && ws, "groupnorm_bwd_any args");
  return groupnorm_bwd_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<const bf16_t*>(dy),
                              reinterpret_cast<const bf16_t*>(add), reinterpret_cast<bf16_t*>(dx), gamma, beta, stats, B, HW, C,
                              G, silu, reinterpret_cast<float*>(ws), S(stream), true);
} catch (...) { return hedit_abi_catch(); }

int hedit_k_layernorm_bwd(const void* x, const void* dy, const void* add, void* dx, const float* gamma, int64_t rows, int C,
                          float eps, void* stream) try {
  ARG_CHECK(x && dy && dx && gamma, "layernorm_bwd args");
  return layernorm_bwd_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<const bf16_t*>(dy),
                              reinterpret_cast<const bf16_t*>(add), reinterpret_cast<bf16_t*>(dx), gamma, (long)rows, C, eps, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_geglu_bwd(const void* x, const void* dy, void* dx, int64_t rows, int inner, void* stream) try {
  ARG_CHECK(x && dy && dx, "geglu_bwd args");
  return geglu_bwd_launch(reinterpret_cast<const bf16_t*>(x), reinterpret_cast<const bf16_t*>(dy), reinterpret_cast<bf16_t*>(dx),
                          (long)rows, inner, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_conv3x3_s2_dgrad_pad1(const void* dy, const void* w_packed, void* dx, int B, int Hin, int Win, int O, int I,
                                  void* stream) try {
  ARG_CHECK(dy && w_packed && dx, "conv3x3_s2_dgrad_pad1 args");
  return conv3x3_s2_dgrad_pad1_launch(reinterpret_cast<const bf16_t*>(dy), reinterpret_cast<const bf16_t*>(w_packed),
                                      reinterpret_cast<bf16_t*>(dx), B, Hin, Win, O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_linear_t(const float* w, void* out, int O, int I, void* stream) try {
  ARG_CHECK(w && out, "pack args");
  return pack_linear_t_launch(w, reinterpret_cast<bf16_t*>(out), O, I, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_flip_oihw(const float* w, float* out, int O, int I, int k, void* stream) try {
  ARG_CHECK(w && out, "flip args");
  return flip_oihw_launch(w, out, O, I, k, S(stream));
} catch (...) { return hedit_abi_catch(); }

// ---- single kernels (parity tests), precise family: pnet.hip / encoder.hip launchers and one layer as the executors run it (pnet.h)
int hedit_k_split3_geometry(int C, int* Cs, int* Kp) try {
  ARG_CHECK(C >= 1 && Cs && Kp, "split3_geometry args");
  *Cs = split_cs(C);
  *Kp = split_kp(C);
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_k_split3(const float* x, int ldx, const float* z, const float* p, const float* q, int pq_img, int op, void* out, int Kp, int Cs,
                   int C, int geo, int B, int H, int W, int worder, int64_t rows_out, void* stream) try {
  ARG_CHECK(x && out && rows_out >= 1 && ldx >= C && geo >= 0 && geo <= 2 && op >= P_COPY && op <= P_GELU, "split3 args");
  ARG_CHECK(geo != 1 || (H % 2 == 0 && W % 2 == 0), "split3: geo 1 needs even H and W");
  Split3Params s{};
  s.x = x; s.ldx = ldx; s.z = z; s.p = p; s.q = q; s.pq_img = pq_img; s.op = op;
  s.out = reinterpret_cast<bf16_t*>(out); s.Kp = Kp; s.Cs = Cs; s.C = C; s.geo = geo; s.B = B; s.H = H; s.W = W; s.worder = worder;
  return split3_launch(s, (long)rows_out, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_pack_split3_w(const float* w, const float* scale, void* out, int O, int I, int k, int dgrad, int Cs, int Kp, int rows_out,
                          int perm_hw, int perm_c, void* stream) try {
  ARG_CHECK(w && out && O >= 1 && I >= 1 && (k == 1 || k == 3) && rows_out >= (dgrad ? I : O), "pack_split3_w args");
  return pack_split3_w_launch(w, scale, reinterpret_cast<bf16_t*>(out), O, I, k, dgrad, Cs, Kp, rows_out, perm_hw, perm_c, S(stream));
} catch (...) { return hedit_abi_catch(); }

// op_split + pgemm of pnet.h on an arena over ws; the weight is packed as make_pconv packs the side that is used
static int precise_conv_run(const float* x, int op, const float* p, const float* q, int pq_img, const float* z, int geo, const float* w,
                            const float* scale, int O, int I, int k, int perm_hw, int perm_c, int dgrad, int mode, int B, int Hin, int Win,
                            float* out, int* chunk_kt, int* splits, void* ws, size_t ws_bytes, hipStream_t st, bool dry, size_t* peak) {
  ARG_CHECK(O >= 1 && I >= 1 && B >= 1 && Hin >= 1 && Win >= 1 && geo >= 0 && geo <= 2 && mode >= 0 && mode <= 2, "precise_conv shape");
  ARG_CHECK(k == (mode == 0 ? 1 : 3), "precise_conv: k = 1 with mode 0, 3 with the convolution modes");
  ARG_CHECK(geo != 1 || (Hin % 2 == 0 && Win % 2 == 0), "precise_conv: geo 1 needs even H and W");
  const int Hs = geo == 1 ? Hin / 2 : (geo == 2 ? Hin * 2 : Hin), Ws = geo == 1 ? Win / 2 : (geo == 2 ? Win * 2 : Win);
  ARG_CHECK(mode != 2 || (Hs % 2 == 0 && Ws % 2 == 0), "precise_conv: mode 2 needs an even image");
  PF f{B, st, Arena{}};
  f.ar.dry = dry;
  f.ar.base = reinterpret_cast<char*>(ws);
  f.ar.cap = ws_bytes;
  const int Cin = dgrad ? O : I;
  PConv c;
  c.O = O; c.I = I; c.k = k;
  c.rows_f = (O + 3) / 4 * 4;
  c.rows_b = (I + 3) / 4 * 4;
  const int rows = dgrad ? c.rows_b : c.rows_f;
  bf16_t *wp, *A;
  TRY(aalloc(f, &wp, (size_t)rows * k * k * split_kp(Cin)));
  if (!dry) TRY(pack_split3_w_launch(w, scale, wp, O, I, k, dgrad, split_cs(Cin), split_kp(Cin), rows, perm_hw, perm_c, st));
  (dgrad ? c.wb : c.wf) = wp;
  TRY(op_split(f, x, Cin, op, p, q, pq_img, z, geo, Hin, Win, (long)B * Hin * Win, &A));
  const long M = (long)B * Hs * Ws / (mode == 2 ? 4 : 1);
  float* o;
  TRY(pgemm(f, A, c, dgrad != 0, mode, Hs, Ws, M, &o));
  const int K = (mode == 0 ? 1 : 9) * split_kp(Cin);
  const int ck = gemm_canonical_chunk((int)(M / B) * GEMM_NOMINAL_BATCH, rows, K);
  if (chunk_kt) *chunk_kt = ck;
  if (splits) *splits = gemm_plan_splits((int)M, rows, K, ck);
  if (!dry) HIP_TRY(hipMemcpyAsync(out, o, (size_t)M * rows * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

size_t hedit_k_precise_conv_ws_bytes(int O, int I, int k, int dgrad, int mode, int geo, int B, int Hin, int Win) try {
  size_t peak = 0;
  const int rc = precise_conv_run(nullptr, P_COPY, nullptr, nullptr, 0, nullptr, geo, nullptr, nullptr, O, I, k, 0, 0, dgrad, mode, B, Hin, Win,
                                  nullptr, nullptr, nullptr, nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

int hedit_k_precise_conv(const float* x, int op, const float* p, const float* q, int pq_img, const float* z, int geo, const float* w_oihw,
                         const float* scale, int O, int I, int k, int perm_hw, int perm_c, int dgrad, int mode, int B, int Hin, int Win,
                         float* out, int* chunk_kt, int* splits, void* ws, size_t ws_bytes, void* stream) try {
  ARG_CHECK(x && w_oihw && out && ws, "precise_conv args");
  ARG_CHECK(reinterpret_cast<uintptr_t>(ws) % 256 == 0, "precise_conv: the workspace must be 256-byte aligned");
  TRY(gemm_prepare());
  return precise_conv_run(x, op, p, q, pq_img, z, geo, w_oihw, scale, O, I, k, perm_hw, perm_c, dgrad, mode, B, Hin, Win, out, chunk_kt,
                          splits, ws, ws_bytes, S(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

int hedit_k_bn_affine(const float* g, const float* b, const float* m, const float* v, float eps, float* p, float* q, int C, int rep,
                      void* stream) try {
  ARG_CHECK(g && b && m && v && p && q && C >= 1 && rep >= 1, "bn_affine args");
  return bn_affine_launch(g, b, m, v, eps, p, q, C, rep, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_bn_fold_bias(const float* bias, const float* g, const float* b, const float* m, const float* v, float eps, float* p, float* q,
                         int C, void* stream) try {
  ARG_CHECK(g && b && m && v && p && q && C >= 1, "bn_fold_bias args");
  return bn_fold_bias_launch(bias, g, b, m, v, eps, p, q, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_act(const float* x, const float* p, const float* q, float* y, int64_t total, int C, int op, void* stream) try {
  ARG_CHECK(x && y && total >= 1 && C >= 1 && ((op == P_PRELU && p) || op == P_RELU), "act args");
  return act_launch(x, p, q, y, (long)total, C, op, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_se_nslab(int HW) { return se_nslab(HW); }

int hedit_k_se_pool(const float* u, float* part, int B, int HW, int C, void* stream) try {
  ARG_CHECK(u && part && B >= 1 && HW >= 1 && C >= 1, "se_pool args");
  return se_pool_launch(u, part, B, HW, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_se_fc(const float* part, const float* bias, const float* w1, const float* w2, float* hbuf, float* sbuf, int B, int HW, int C,
                  int R, void* stream) try {
  ARG_CHECK(part && bias && w1 && w2 && hbuf && sbuf && B >= 1 && HW >= 1, "se_fc args");
  return se_fc_launch(part, bias, w1, w2, hbuf, sbuf, B, HW, C, R, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_se_combine(const float* u, const float* bias, const float* s, const float* sc, const float* sc_bias, const float* X, int stride,
                       float* Y, int B, int Ho, int Wo, int C, void* stream) try {
  ARG_CHECK(u && bias && s && Y && (sc ? sc_bias != nullptr : X != nullptr) && stride >= 1, "se_combine args");
  return se_combine_launch(u, bias, s, sc, sc_bias, X, stride, Y, B, Ho, Wo, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_se_bwd_reduce(const float* dY, const float* u, const float* bias, float* part, int B, int HW, int C, void* stream) try {
  ARG_CHECK(dY && u && bias && part && B >= 1 && HW >= 1 && C >= 1, "se_bwd_reduce args");
  return se_bwd_reduce_launch(dY, u, bias, part, B, HW, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_se_fc_bwd(const float* part, const float* sbuf, const float* hbuf, const float* w1, const float* w2, float* rbuf, int B, int C,
                      int R, int HW, void* stream) try {
  ARG_CHECK(part && sbuf && hbuf && w1 && w2 && rbuf && B >= 1 && HW >= 1, "se_fc_bwd args");
  return se_fc_bwd_launch(part, sbuf, hbuf, w1, w2, rbuf, B, C, R, HW, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_unit_bwd_combine(const float* dxa, const float* p, const float* dsc, int stride, float* dX, int B, int H, int W, int C,
                             void* stream) try {
  ARG_CHECK(dxa && p && dsc && dX && stride >= 1 && H % stride == 0 && W % stride == 0, "unit_bwd_combine args");
  return unit_bwd_combine_launch(dxa, p, dsc, stride, dX, B, H, W, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_scale_cols(const float* x, const float* p, float* y, int64_t total, int n, void* stream) try {
  ARG_CHECK(x && p && y && total >= 1 && n >= 1, "scale_cols args");
  return scale_cols_launch(x, p, y, (long)total, n, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_face_pool(const float* img, float* out, int B, void* stream) try {
  ARG_CHECK(img && out && B >= 1, "face_pool args");
  return face_pool_launch(img, out, B, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_face_pool_bwd(const float* g, int ldg, float* dimg, int B, void* stream) try {
  ARG_CHECK(g && dimg && ldg >= 3 && B >= 1, "face_pool_bwd args");
  return face_pool_bwd_launch(g, ldg, dimg, B, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_cos_head(const float* raw, const float* bias, const float* ref, int ref_stride, float* feat, float* loss, float* df, int B,
                     int D, float scale, void* stream) try {
  ARG_CHECK(raw && bias && B >= 1 && D >= 1, "cos_head args");
  return cos_head_launch(raw, bias, ref, ref_stride, feat, loss, df, B, D, scale, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lpips_prep(const float* img, float* out, const float* shift3, const float* scale3, int B, int H, int W, void* stream) try {
  ARG_CHECK(img && out && shift3 && scale3, "lpips_prep args");
  return lpips_prep_launch(img, out, shift3, scale3, B, H, W, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lpips_prep_bwd(const float* g, int ldg, float* dimg, const float* scale3, int B, int H, int W, void* stream) try {
  ARG_CHECK(g && dimg && scale3 && ldg >= 3, "lpips_prep_bwd args");
  return lpips_prep_bwd_launch(g, ldg, dimg, scale3, B, H, W, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_maxpool2(const float* z, float* zp, uint8_t* idx, int B, int H, int W, int C, void* stream) try {
  ARG_CHECK(z && zp && idx, "maxpool2 args");
  return maxpool2_launch(z, zp, idx, B, H, W, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_maxpool2_bwd(const float* gp, const uint8_t* idx, const float* add, float* G, int B, int H, int W, int C, void* stream) try {
  ARG_CHECK(gp && idx && G && H % 2 == 0 && W % 2 == 0, "maxpool2_bwd args");
  return maxpool2_bwd_launch(gp, idx, add, G, B, H, W, C, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lpips_head(const float* z, const float* bias, const float* src, int64_t src_img_stride, const float* w, float* fn_out,
                       float* dpix, float* dF, int B, int HW, int C, float gscale, void* stream) try {
  ARG_CHECK(z && bias && (src ? (w && dpix) : fn_out != nullptr), "lpips_head args");
  return lpips_head_launch(z, bias, src, (long)src_img_stride, w, fn_out, dpix, dF, B, HW, C, gscale, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_lpips_reduce(const float* dpix, float* acc, int B, int HW, int first, void* stream) try {
  ARG_CHECK(dpix && acc && B >= 1 && HW >= 1, "lpips_reduce args");
  return lpips_reduce_launch(dpix, acc, B, HW, first, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_enc_patchify(const float* img, float* X, int B, int R, int p, int bwd, void* stream) try {
  ARG_CHECK(img && X && B >= 1 && p >= 1 && R >= p && R % p == 0, "enc_patchify args");
  return enc_patchify_launch(img, X, B, R, p, bwd, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_enc_tokens(const float* E, const float* cbias, const float* cls, const float* pos, float* T, int B, int L, int W,
                       void* stream) try {
  ARG_CHECK(E && cls && pos && T && B >= 1 && L >= 2 && W >= 1, "enc_tokens args");
  return enc_tokens_launch(E, cbias, cls, pos, T, B, L, W, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_enc_gather_rows(const float* T, const int32_t* idx, float* R, int B, int L, int W, void* stream) try {
  ARG_CHECK(T && R && B >= 1 && L >= 1 && W >= 1, "enc_gather_rows args");
  return enc_gather_rows_launch(T, idx, R, B, L, W, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_enc_ln(const float* x, const float* g, const float* b, float* y, float* stats, int64_t rows, int W, float eps,
                   void* stream) try {
  ARG_CHECK(x && g && b && y && rows >= 1 && W >= 1, "enc_ln args");
  return enc_ln_launch(x, g, b, y, stats, (long)rows, W, eps, S(stream));
} catch (...) { return hedit_abi_catch(); }

int hedit_k_enc_add_bias_res(const float* raw, const float* bias, const float* res, float* out, int64_t total, int W, void* stream) try {
  ARG_CHECK(raw && bias && out && total >= 1 && W >= 1, "enc_add_bias_res args");
  return enc_add_bias_res_launch(raw, bias, res, out, (long)total, W, S(stream));
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
