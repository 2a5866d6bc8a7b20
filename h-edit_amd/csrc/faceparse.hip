// The face-parsing network of the face-swapping task and the soft face mask made from its labels: `FaceParsing()` of the
// reference's face-swapping/arcface/face_parsing_model.py (the CelebAMask-HQ U-Net at feature_scale 4: filters
// 16/32/64/128/256, 19 classes, transposed-convolution up-sampling, BatchNorm) followed by encode_segmentation +
// SoftErosion(13, 0.9, 7) of arcface/face_utils.py, as main_edit.py:120-127 / :184-191 runs them on the source image.
//
// The reference never calls .eval() on this model, so its BatchNorms normalise with the statistics of the batch it is
// called with -- one image.  batch_stats = 1 reproduces that per image: (mean, biased variance) over H x W for every
// (image, channel), in a fixed slab order that depends on H x W only (bit-identical whatever the batch).  The conv biases in
// front of a batch-statistics BatchNorm cancel and are not applied; batch_stats = 0 uses the running statistics with the
// bias folded in (eval mode).
//
// Arithmetic: every convolution is the three-term split-bf16 GEMM of pnet.h (fp32 quality -- the final argmax decides on
// small logit margins); activations are fp32 NHWC.  The normalisation + ReLU of a layer is applied where its output is read:
// in the operand pass of the next GEMM (P_AFFINE_RELU), in the pooling kernel that also materialises the skip half of the
// level's concat buffer, or in the head that fuses the 1x1 classifier with the argmax.  The transposed convolution 2x2 s2 is
// a 1x1 GEMM with N = 4 Cout whose result is scattered into the right half of the concat buffer (torch.cat([skip, up])).
#include "pnet.h"

namespace {

constexpr float FP_BN_EPS = 1e-5f;
constexpr int FP_LEVELS = 5;
constexpr int FP_FILTERS[FP_LEVELS] = {16, 32, 64, 128, 256};   // [64, 128, 256, 512, 1024] / feature_scale 4
constexpr int FP_CLASSES = 19;
constexpr int FP_MAX_KSIZE = 31;                                  // SoftErosion kernel_size bound of hedit_face_mask

// ------------------------------------------------------------------------------------------------ network kernels
// image NCHW [B][C][HW] -> NHWC rows [B*HW][C]
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int HW, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long pix = i / C;
    const long b = pix / HW;
    y[i] = x[(b * C + c) * HW + (pix - b * HW)];
  }
}

// Per-(image, channel) statistics of z [B*HW][ldz], pass 1 of 2.  Block (channel slice, image, slab): cw channels x (256 / cw)
// pixel lanes.  Each thread takes the two-pass (mean, M2) of its pixels; the lanes are Chan-merged in lane order.  The slab
// partition is a function of HW only.  part: [B][nslab][C][3] = (count, mean, M2).
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const float* __restrict__ z, int ldz, int C, int HW, int nslab, int cw,
                                                            float* __restrict__ part) {
  __shared__ float sn[256], sm[256], s2[256];
  const int lanes = 256 / cw;
  const int cl = threadIdx.x % cw, r = threadIdx.x / cw;
  const int c = blockIdx.x * cw + cl, b = blockIdx.y, sl = blockIdx.z;
  const int per = (HW + nslab - 1) / nslab, p0 = sl * per, p1 = p0 + per < HW ? p0 + per : HW;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (c < C) {
    const float* zb = z + (long)b * HW * ldz + c;
    float s = 0.f;
    for (int p = p0 + r; p < p1; p += lanes) { s += zb[(long)p * ldz]; n += 1.f; }
    if (n > 0.f) {
      mean = s / n;
      for (int p = p0 + r; p < p1; p += lanes) { const float d = zb[(long)p * ldz] - mean; m2 += d * d; }
    }
  }
  sn[threadIdx.x] = n; sm[threadIdx.x] = mean; s2[threadIdx.x] = m2;
  __syncthreads();
  if (r == 0 && c < C) {
    for (int k = 1; k < lanes; ++k) {
      const int t = k * cw + cl;
      const float nb = sn[t];
      if (nb == 0.f) continue;
      const float nn = n + nb, d = sm[t] - mean;
      mean += d * (nb / nn);
      m2 += s2[t] + d * d * (n * nb / nn);
      n = nn;
    }
    float* o = part + (((long)b * nslab + sl) * C + c) * 3;
    o[0] = n; o[1] = mean; o[2] = m2;
  }
}

// pass 2: merge the slabs in order -> p = gamma / sqrt(var + eps), q = beta - mean p  ([B][C], var biased)
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int nslab, int C, int B, const float* __restrict__ g,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ p, float* __restrict__ q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int sl = 0; sl < nslab; ++sl) {
    const float* o = part + (((long)b * nslab + sl) * C + c) * 3;
    const float nb = o[0];
    if (nb == 0.f) continue;
    const float nn = n + nb, d = o[1] - mean;
    mean += d * (nb / nn);
    m2 += o[2] + d * d * (n * nb / nn);
    n = nn;
  }
  const float s = g[c] / sqrtf(m2 / n + eps);
  p[i] = s;
  q[i] = beta[c] - mean * s;
}

// y = relu(p z + q) for the 2 x 2 window of every pooled pixel: the four values go to the skip half of the concat buffer
// (row stride ldy), their maximum to the pooled tensor [B][H/2][W/2][C].  ReLU before the max: a negative gamma reverses
// the order of the pre-activations.
__global__ __launch_bounds__(256) void affine_relu_pool_kernel(const float* __restrict__ z, const float* __restrict__ p, const float* __restrict__ q,
                                                               int pq_img, float* __restrict__ y, int ldy, float* __restrict__ pooled, int B,
                                                               int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2;
  const long total = (long)B * Ho * Wo * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long pix = i / C;
    const int b = (int)(pix / ((long)Ho * Wo));
    const int r = (int)(pix - (long)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    const int pi = pq_img ? b * C + c : c;
    const float pp = p[pi], qq = q[pi];
    float best = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long row = ((long)b * H + oy * 2 + (k >> 1)) * W + ox * 2 + (k & 1);
      const float t = pp * z[row * C + c] + qq;
      const float v = t > 0.f ? t : 0.f;
      y[row * ldy + c] = v;
      best = k == 0 || v > best ? v : best;
    }
    pooled[i] = best;
  }
}

// ConvTranspose2d(k 2, s 2) as a 1x1 GEMM: t [B*Hin*Win][4 C], column (a * 2 + bb) * C + co = output pixel (2 iy + a, 2 ix + bb).
// Scatter + bias into y [B][2Hin][2Win] at column offset `off` (row stride ldy).
__global__ __launch_bounds__(256) void convt_scatter_kernel(const float* __restrict__ t, const float* __restrict__ bias, float* __restrict__ y,
                                                            int ldy, int off, int B, int Hin, int Win, int C) {
  const int Ho = Hin * 2, Wo = Win * 2;
  const long total = (long)B * Ho * Wo * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long pix = i / C;
    const int b = (int)(pix / ((long)Ho * Wo));
    const int r = (int)(pix - (long)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    const long src = ((long)b * Hin + (oy >> 1)) * Win + (ox >> 1);
    y[pix * ldy + off + c] = t[src * 4 * C + ((oy & 1) * 2 + (ox & 1)) * C + c] + bias[c];
  }
}

// torch ConvTranspose2d weight [Cin][Cout][2][2] -> GEMM rows [4 Cout][Cin], row (a * 2 + bb) * Cout + co
__global__ __launch_bounds__(256) void convt_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * Cout * Cin) return;
  const int ci = i % Cin, n = i / Cin;
  const int co = n % Cout, ab = n / Cout;
  out[i] = w[((long)ci * Cout + co) * 4 + ab];
}

// head: a = relu(p z + q) (C channels), logits = bias + W a (fp32, channels in order), label = first index of the maximum
// (torch.argmax), int64.  One thread per pixel.
template <int C, int K>
__global__ __launch_bounds__(256) void head_argmax_kernel(const float* __restrict__ z, const float* __restrict__ p, const float* __restrict__ q,
                                                          int pq_img, const float* __restrict__ w, const float* __restrict__ bias,
                                                          int64_t* __restrict__ labels, int B, int HW) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / HW);
    const float* zr = z + i * C;
    float a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int pi = pq_img ? b * C + c : c;
      const float t = p[pi] * zr[c] + q[pi];
      a[c] = t > 0.f ? t : 0.f;
    }
    int best = 0;
    float bv = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float s = bias[k];
#pragma unroll
      for (int c = 0; c < C; ++c) s += w[k * C + c] * a[c];
      if (k == 0 || s > bv) { bv = s; best = k; }
    }
    labels[i] = best;
  }
}

// ------------------------------------------------------------------------------------------------ mask kernels
// face + mouth of encode_segmentation (no_neck): 1 for ids {1..7, 10, 11, 12}, plus 1 more for the mouth (10)
__global__ __launch_bounds__(256) void mask_encode_kernel(const int64_t* __restrict__ labels, float* __restrict__ x, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int64_t l = labels[i];
    const bool face = (l >= 1 && l <= 7) || (l >= 10 && l <= 12);
    x[i] = (face ? 1.f : 0.f) + (l == 10 ? 1.f : 0.f);
  }
}

// SoftErosion's kernel: dist = sqrt((x - r)^2 + (y - r)^2), k = max(dist) - dist, k /= sum(k)  (K x K, one block)
__global__ __launch_bounds__(256) void cone_table_kernel(float* __restrict__ tab, int K) {
  __shared__ float d[FP_MAX_KSIZE * FP_MAX_KSIZE];
  __shared__ float mx, sum;
  const int r = K / 2, n = K * K;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float dy = (float)(i / K - r), dx = (float)(i % K - r);
    d[i] = sqrtf(dx * dx + dy * dy);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = d[0];
    for (int i = 1; i < n; ++i) m = d[i] > m ? d[i] : m;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += m - d[i];
    mx = m; sum = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) tab[i] = (mx - d[i]) / sum;
}

// y = blur(x) (zero-padded K x K correlation with the cone, taps in row-major order) or min(x, blur(x)).  16 x 16 tile per block.
__global__ __launch_bounds__(256) void cone_blur_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ tab, int K,
                                                        int H, int W, int with_min) {
  constexpr int T = 16, S = T + FP_MAX_KSIZE - 1;
  __shared__ float tile[S * S];
  __shared__ float tk[FP_MAX_KSIZE * FP_MAX_KSIZE];
  const int r = K / 2, span = T + K - 1;
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const float* xb = x + (long)b * H * W;
  for (int i = threadIdx.x; i < span * span; i += 256) {
    const int ty = i / span, tx = i - ty * span;
    const int gy = y0 + ty - r, gx = x0 + tx - r;
    tile[ty * S + tx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[(long)gy * W + gx] : 0.f;
  }
  for (int i = threadIdx.x; i < K * K; i += 256) tk[i] = tab[i];
  __syncthreads();
  const int ty = threadIdx.x / T, tx = threadIdx.x % T;
  const int gy = y0 + ty, gx = x0 + tx;
  if (gy >= H || gx >= W) return;
  float acc = 0.f;
  for (int ky = 0; ky < K; ++ky)
    for (int kx = 0; kx < K; ++kx) acc += tk[ky * K + kx] * tile[(ty + ky) * S + tx + kx];
  const float c = tile[(ty + r) * S + tx + r];
  y[(long)b * H * W + (long)gy * W + gx] = with_min ? (c < acc ? c : acc) : acc;
}

// per image: the maximum of the field over the pixels below the threshold (-1 if there is none).  One block per image.
__global__ __launch_bounds__(1024) void nonhard_max_kernel(const float* __restrict__ x, float thr, int HW, float* __restrict__ mx) {
  __shared__ float red[1024];
  const float* xb = x + (long)blockIdx.x * HW;
  float m = -1.f;
  for (int i = threadIdx.x; i < HW; i += 1024) {
    const float v = xb[i];
    if (!(v >= thr) && v > m) m = v;
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) mx[blockIdx.x] = red[0];
}

// hard = field >= thr -> soft 1; otherwise soft = field / (maximum below the threshold), 0 when that maximum is 0
__global__ __launch_bounds__(256) void mask_final_kernel(const float* __restrict__ x, const float* __restrict__ mx, float thr, int HW,
                                                         float* __restrict__ soft, uint8_t* __restrict__ hard, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const float v = x[i];
    const bool h = v >= thr;
    const float m = mx[i / HW];
    soft[i] = h ? 1.f : (m > 0.f ? v / m : 0.f);
    hard[i] = h ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct FBN { float *g, *b, *m, *v; };
struct FConv {
  int cin, cout;
  float *w, *bias;
  FBN bn;
  float *pe, *qe;      // eval mode: running statistics with the conv bias folded in
  PConv pc;
};
struct FBlock { FConv c1, c2; };     // unetConv2
struct FUp {
  int cin, cout;
  float *w, *bias, *wg;              // torch [Cin][Cout][2][2], [Cout]; GEMM rows [4 Cout][Cin]
  PConv pc;
  FBlock conv;
};

}  // namespace

struct HEDIT_HANDLE hedit_faceparse : ParamStore {
  FBlock enc[FP_LEVELS];             // conv1 .. conv4, center
  FUp up[FP_LEVELS - 1];             // up[l] = up_concat{l+1}: output at level l
  float *fw = nullptr, *fb = nullptr;
};

namespace {

FBN make_fbn(ParamStore* h, const std::string& pre, int C) {
  FBN b;
  b.g = vec(h, pre + ".weight", C);
  b.b = vec(h, pre + ".bias", C);
  b.m = vec(h, pre + ".running_mean", C);
  b.v = vec(h, pre + ".running_var", C);
  return b;
}

FConv make_fconv(ParamStore* h, const std::string& pre, int cin, int cout) {
  FConv c{};
  c.cin = cin; c.cout = cout;
  c.w = f32conv(h, pre + ".0.weight", cout, cin, 3);
  c.bias = vec(h, pre + ".0.bias", cout);
  c.bn = make_fbn(h, pre + ".1", cout);
  c.pe = dalloc<float>(h, cout);
  c.qe = dalloc<float>(h, cout);
  return c;
}

FBlock make_fblock(ParamStore* h, const std::string& pre, int cin, int cout) {
  FBlock b;
  b.c1 = make_fconv(h, pre + ".conv1", cin, cout);
  b.c2 = make_fconv(h, pre + ".conv2", cout, cout);
  return b;
}

int bn_nslab(int HW) {
  const int n = HW / 512;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}

// fp32 rows [rows][ldx] (C channels used) -> split bf16 operand
int op_split_ld(PF& f, const float* x, int C, int ldx, int op, const float* p, const float* q, int pq_img, int H, int W, long rows,
                bf16_t** out) {
  Split3Params s{};
  s.x = x; s.ldx = ldx; s.p = p; s.q = q; s.pq_img = pq_img; s.op = op;
  s.Kp = split_kp(C); s.Cs = split_cs(C); s.C = C; s.geo = 0; s.B = f.B; s.H = H; s.W = W;
  TRY(aalloc(f, out, (size_t)rows * s.Kp));
  s.out = *out;
  if (!f.dry()) TRY(split3_launch(s, rows, f.st));
  return HEDIT_OK;
}

// a layer's output z [B*HW][C] and the affine of its BatchNorm: (p, q) per (image, channel) or per channel
struct Act {
  float* z = nullptr;
  float *p = nullptr, *q = nullptr;      // arena-owned when pq_img
  int pq_img = 0;
  const float *pc = nullptr, *qc = nullptr;
  const float* P() const { return pq_img ? p : pc; }
  const float* Q() const { return pq_img ? q : qc; }
};

void act_free(PF& f, Act& a) {
  f.ar.free(a.z);
  if (a.pq_img) { f.ar.free(a.p); f.ar.free(a.q); }
  a = Act{};
}

// conv3x3 (operand A) -> z, and the BatchNorm affine: per-image statistics of z, or the folded running statistics
int conv_bn(PF& f, const FConv& c, const bf16_t* A, int H, int W, bool batch_stats, Act* out) {
  const int B = f.B, HW = H * W, C = c.cout;
  const long M = (long)B * HW;
  Act a;
  TRY(pgemm(f, A, c.pc, false, 1, H, W, M, &a.z));     // rows_f == C: every width here is a multiple of 4
  if (batch_stats) {
    const int nslab = bn_nslab(HW);
    int cw = 1;
    while (cw < C && cw < 64) cw *= 2;
    float* part;
    TRY(aalloc(f, &part, (size_t)B * nslab * C * 3));
    TRY(aalloc(f, &a.p, (size_t)B * C));
    TRY(aalloc(f, &a.q, (size_t)B * C));
    if (!f.dry()) {
      hipLaunchKernelGGL(bn_stats_part_kernel, dim3(cdiv(C, cw), B, nslab), dim3(256), 0, f.st, a.z, C, C, HW, nslab, cw, part);
      LAUNCH_CHECK();
      hipLaunchKernelGGL(bn_stats_final_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, f.st, part, nslab, C, B, c.bn.g, c.bn.b,
                         FP_BN_EPS, a.p, a.q);
      LAUNCH_CHECK();
    }
    f.ar.free(part);
    a.pq_img = 1;
  } else {
    a.pc = c.pe;
    a.qc = c.qe;
  }
  *out = a;
  return HEDIT_OK;
}

// unetConv2 on X (rows [B*H*W][ldx], C = blk.c1.cin channels, already activated) -> the second conv's output + affine
int block_fwd(PF& f, const FBlock& blk, const float* X, int ldx, int H, int W, bool batch_stats, Act* out) {
  const long M = (long)f.B * H * W;
  bf16_t* A;
  Act a1;
  TRY(op_split_ld(f, X, blk.c1.cin, ldx, P_COPY, nullptr, nullptr, 0, H, W, M, &A));
  TRY(conv_bn(f, blk.c1, A, H, W, batch_stats, &a1));
  f.ar.free(A);
  TRY(op_split_ld(f, a1.z, blk.c1.cout, blk.c1.cout, P_AFFINE_RELU, a1.P(), a1.Q(), a1.pq_img, H, W, M, &A));
  act_free(f, a1);
  TRY(conv_bn(f, blk.c2, A, H, W, batch_stats, out));
  f.ar.free(A);
  return HEDIT_OK;
}

// image fp32 [B][3][H][W] -> labels int64 [B][H][W]
int run(hedit_faceparse* h, const float* image, int B, int H, int W, bool batch_stats, int64_t* labels, void* ws, size_t ws_bytes,
        hipStream_t st, bool dry, size_t* peak) {
  PF f{B, st, Arena{}};
  f.ar.dry = dry;
  f.ar.base = reinterpret_cast<char*>(ws);
  f.ar.cap = ws_bytes;
  float* cat[FP_LEVELS - 1];            // [B][H_l][W_l][2 F_l]: [skip | up]
  for (int l = 0; l < FP_LEVELS - 1; ++l) TRY(aalloc(f, &cat[l], (size_t)B * (H >> l) * (W >> l) * 2 * FP_FILTERS[l]));
  float* X;
  TRY(aalloc(f, &X, (size_t)B * H * W * 3));
  if (!dry) {
    const long n = (long)B * H * W * 3;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, egrid(n), dim3(256), 0, st, image, X, 3, H * W, n);
    LAUNCH_CHECK();
  }
  int ldx = 3;
  Act a;
  for (int l = 0; l < FP_LEVELS - 1; ++l) {   // conv1 .. conv4, each followed by its pool
    const int Hl = H >> l, Wl = W >> l, F = FP_FILTERS[l];
    TRY(block_fwd(f, h->enc[l], X, ldx, Hl, Wl, batch_stats, &a));
    f.ar.free(X);
    TRY(aalloc(f, &X, (size_t)B * (Hl / 2) * (Wl / 2) * F));
    if (!dry) {
      hipLaunchKernelGGL(affine_relu_pool_kernel, egrid((long)B * (Hl / 2) * (Wl / 2) * F), dim3(256), 0, st, a.z, a.P(), a.Q(), a.pq_img,
                         cat[l], 2 * F, X, B, Hl, Wl, F);
      LAUNCH_CHECK();
    }
    act_free(f, a);
    ldx = F;
  }
  TRY(block_fwd(f, h->enc[FP_LEVELS - 1], X, ldx, H >> 4, W >> 4, batch_stats, &a));    // center
  f.ar.free(X);
  for (int l = FP_LEVELS - 2; l >= 0; --l) {  // up_concat4 .. up_concat1
    const FUp& u = h->up[l];
    const int Hin = H >> (l + 1), Win = W >> (l + 1), F = FP_FILTERS[l];
    const long Min = (long)B * Hin * Win;
    bf16_t* A;
    float* t;
    TRY(op_split_ld(f, a.z, u.cin, u.cin, P_AFFINE_RELU, a.P(), a.Q(), a.pq_img, Hin, Win, Min, &A));
    act_free(f, a);
    TRY(pgemm(f, A, u.pc, false, 0, Hin, Win, Min, &t));
    f.ar.free(A);
    if (!dry) {
      hipLaunchKernelGGL(convt_scatter_kernel, egrid(Min * 4 * F), dim3(256), 0, st, t, u.bias, cat[l], 2 * F, F, B, Hin, Win, F);
      LAUNCH_CHECK();
    }
    f.ar.free(t);
    TRY(block_fwd(f, u.conv, cat[l], 2 * F, 2 * Hin, 2 * Win, batch_stats, &a));
    f.ar.free(cat[l]);
  }
  if (!dry) {
    hipLaunchKernelGGL((head_argmax_kernel<FP_FILTERS[0], FP_CLASSES>), egrid((long)B * H * W), dim3(256), 0, st, a.z, a.P(), a.Q(), a.pq_img,
                       h->fw, h->fb, labels, B, H * W);
    LAUNCH_CHECK();
  }
  act_free(f, a);
  if (peak) *peak = f.ar.peak;
  return HEDIT_OK;
}

int shape_check(int B, int H, int W) {
  ARG_CHECK(B >= 1, "faceparse: B >= 1");
  if (H < 16 || W < 16 || H % 16 != 0 || W % 16 != 0) {
    hedit_set_error("bad argument: face parsing needs H and W that are positive multiples of 16 (got " + std::to_string(H) + " x " +
                    std::to_string(W) + ")");
    return HEDIT_ERR_ARG;
  }
  return HEDIT_OK;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

HEDIT_LIFECYCLE(faceparse, hedit_faceparse, "face parsing", no_pre_destroy)

extern "C" {

int hedit_faceparse_create(hedit_faceparse** out) try {
  ARG_CHECK(out, "null");
  TRY(gemm_prepare());
  hedit_faceparse* h = new hedit_faceparse();
  static const char* enc_names[FP_LEVELS] = {"conv1", "conv2", "conv3", "conv4", "center"};
  for (int l = 0; l < FP_LEVELS; ++l)
    h->enc[l] = make_fblock(h, enc_names[l], l == 0 ? 3 : FP_FILTERS[l - 1], FP_FILTERS[l]);
  for (int l = FP_LEVELS - 2; l >= 0; --l) {        // the reference's registration order: up_concat4 first
    FUp& u = h->up[l];
    const std::string pre = "up_concat" + std::to_string(l + 1);
    u.cin = FP_FILTERS[l + 1];
    u.cout = FP_FILTERS[l];
    u.conv = make_fblock(h, pre + ".conv", u.cin, u.cout);
    u.w = dalloc<float>(h, (size_t)u.cin * u.cout * 4);
    add_slot(h, pre + ".up.weight", Pack::F32, u.w, (size_t)u.cin * u.cout * 4, u.cin, u.cout, 4, u.cin, u.cout, 2, 2);
    u.bias = vec(h, pre + ".up.bias", u.cout);
    u.wg = dalloc<float>(h, (size_t)u.cin * u.cout * 4);
  }
  h->fw = f32conv(h, "final.weight", FP_CLASSES, FP_FILTERS[0], 1);
  h->fb = vec(h, "final.bias", FP_CLASSES);
  return handle_created(h, out);
} catch (...) { return hedit_abi_catch(); }

int hedit_faceparse_finalize(hedit_faceparse* h, void* stream) try {
  ARG_CHECK(h, "null");
  TRY(handle_loaded(h));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto conv = [&](FConv& c) -> int {
    TRY(bn_fold_bias_launch(c.bias, c.bn.g, c.bn.b, c.bn.m, c.bn.v, FP_BN_EPS, c.pe, c.qe, c.cout, st));
    return make_pconv(h, c.pc, c.w, nullptr, c.cout, c.cin, 3, 0, 0, st);
  };
  for (FBlock& b : h->enc) { TRY(conv(b.c1)); TRY(conv(b.c2)); }
  for (FUp& u : h->up) {
    TRY(conv(u.conv.c1));
    TRY(conv(u.conv.c2));
    hipLaunchKernelGGL(convt_weight_kernel, dim3(cdiv((long)4 * u.cout * u.cin, 256)), dim3(256), 0, st, u.w, u.wg, u.cin, u.cout);
    LAUNCH_CHECK();
    TRY(make_pconv(h, u.pc, u.wg, nullptr, 4 * u.cout, u.cin, 1, 0, 0, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (h->alloc_failed) { hedit_set_error("hipMalloc failed while packing the face-parsing weights"); return HEDIT_ERR_HIP; }
  h->finalized = true;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

size_t hedit_faceparse_workspace_bytes(hedit_faceparse* h, int B, int H, int W) try {
  if (!h || !h->finalized || shape_check(B, H, W) != HEDIT_OK) return 0;      // the GEMM geometry is set by finalize
  size_t peak = 0;
  const int rc = run(h, nullptr, B, H, W, true, nullptr, nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* image fp32 [B][3][H][W] in [-1, 1] -> labels int64 [B][1][H][W] = argmax of the 19 class logits */
int hedit_faceparse_labels(hedit_faceparse* h, const float* image, int B, int H, int W, int batch_stats, int64_t* labels, void* workspace,
                           size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && image && labels && workspace, "faceparse_labels args");
  TRY(shape_check(B, H, W));
  TRY(handle_finalized(h));
  return run(h, image, B, H, W, batch_stats != 0, labels, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

size_t hedit_face_mask_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  const size_t n = (size_t)B * H * W;
  return 2 * align256(n * sizeof(float)) + align256((size_t)B * sizeof(float)) + align256(FP_MAX_KSIZE * FP_MAX_KSIZE * sizeof(float));
}

/* labels int64 [B][1][H][W] -> soft fp32 / hard uint8 [B][1][H][W]: SoftErosion(kernel_size, threshold, iterations) of
 * face + mouth (encode_segmentation), with the maximum over the non-hard pixels taken per image */
int hedit_face_mask(const int64_t* labels, int B, int H, int W, int kernel_size, float threshold, int iterations, float* soft, uint8_t* hard,
                    void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(labels && soft && hard && workspace, "face_mask args");
  ARG_CHECK(B >= 1 && H >= 1 && W >= 1, "face_mask: shape");
  ARG_CHECK(kernel_size >= 3 && kernel_size <= FP_MAX_KSIZE && kernel_size % 2 == 1, "face_mask: odd kernel_size in [3, 31]");   // 1: a 0 / 0 kernel
  ARG_CHECK(iterations >= 1, "face_mask: iterations >= 1");
  ARG_CHECK(workspace_bytes >= hedit_face_mask_workspace_bytes(B, H, W), "face_mask: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long n = (long)B * H * W;
  char* ws = reinterpret_cast<char*>(workspace);
  float* x = reinterpret_cast<float*>(ws);
  float* y = reinterpret_cast<float*>(ws + align256(n * sizeof(float)));
  float* mx = reinterpret_cast<float*>(ws + 2 * align256(n * sizeof(float)));
  float* tab = reinterpret_cast<float*>(ws + 2 * align256(n * sizeof(float)) + align256((size_t)B * sizeof(float)));
  hipLaunchKernelGGL(mask_encode_kernel, egrid(n), dim3(256), 0, st, labels, x, n);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(cone_table_kernel, dim3(1), dim3(256), 0, st, tab, kernel_size);
  LAUNCH_CHECK();
  const dim3 g(cdiv(W, 16), cdiv(H, 16), B);
  for (int it = 0; it < iterations; ++it) {      // iterations - 1 rounds of min(x, blur(x)), then one blur
    hipLaunchKernelGGL(cone_blur_kernel, g, dim3(256), 0, st, x, y, tab, kernel_size, H, W, it < iterations - 1 ? 1 : 0);
    LAUNCH_CHECK();
    std::swap(x, y);
  }
  hipLaunchKernelGGL(nonhard_max_kernel, dim3(B), dim3(1024), 0, st, x, threshold, H * W, mx);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(mask_final_kernel, egrid(n), dim3(256), 0, st, x, mx, threshold, H * W, soft, hard, n);
  LAUNCH_CHECK();
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
