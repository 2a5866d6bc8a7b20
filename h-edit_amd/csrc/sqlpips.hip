// SqueezeNet-LPIPS as a native forward-only executor: the `lpips` columns of the PIE-Bench evaluator, the reference's
// LearnedPerceptualImagePatchSimilarity(net_type='squeeze') of text-guided/evaluation/matrics_calculator.py:276,329-347.
// The torchmetrics / lpips packages are absent offline; their published network is restated here: ScalingLayer ->
// torchvision squeezenet1_1.features cut into seven slices (taps after features 1, 4, 7, 9, 10, 11, 12) -> every tap
// divided by its channel L2 norm (+ 1e-10, as csrc/pnet.hip's lpips_head) -> squared difference -> non-negative 1x1 `lin`
// weights -> spatial mean -> sum over the taps.  Parameters by the torchvision names (`features.0.weight`,
// `features.3.squeeze.weight`, ..., `features.12.expand3x3.bias`) and `lin{k}.model.1.weight`.
//
// This is a different machine from lpips.hip (VGG16, forward + backward on the split-bf16 GEMMs): the network is 2.2 GFLOP
// per 512 x 512 image, so what it costs is launches and round trips, and the kernels here are fused and exact fp32:
//   stem   ScalingLayer + conv 3x3 stride 2 (no padding) + bias + ReLU, direct fp32 FMA (K = 27)            1 launch
//   pool   3x3 stride 2 ceil-mode max, a partial last window takes its in-range elements                     3 launches
//   fire   squeeze 1x1 + ReLU into LDS for an 8 x 8 tile and its one-pixel halo, then expand1x1 and expand3x3 from LDS,
//          bias + ReLU, written as the concatenated [e1 | e3] channels; the squeeze map never reaches memory  8 launches
//   head   per tap: both channel norms and sum_c lin[c] (a^ - b^)^2 per pixel, fixed-shape per-block partials  7 launches
//   sum    the partials in a fixed order, / (H_k W_k), tap 0 ... tap 6 in that order                           1 launch
// Every contraction of a Fire module runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bit for bit a k-ordered
// fmaf chain).  Activations are NHWC, both images of all N pairs go through the backbone as ONE batch of 2 N, and an
// image's arithmetic -- tile partition, K order, block partition of the head, reduction tree -- is a function of (H, W)
// alone: dist[n] of a batch is bit-identical to the N = 1 call, distance(a, b) to distance(b, a), and distance(a, a) is 0.
// No float atomics.  Nothing reads the 16-bit storage type: both storage builds give the same bits.
#include "exec.h"
#include "kernels.h"
#include "store.h"

namespace {

constexpr int NFIRE = 8, NTAP = 7;
// features index, input channels, squeeze channels, channels of EACH expand
constexpr int FIRE[NFIRE][4] = {{3, 64, 16, 64},    {4, 128, 16, 64},   {6, 128, 32, 128},  {7, 256, 32, 128},
                                {9, 256, 48, 192},  {10, 384, 48, 192}, {11, 384, 64, 256}, {12, 512, 64, 256}};
constexpr int TAP_C[NTAP] = {64, 128, 256, 384, 384, 512, 512};
// the tap a Fire module's output is (-1: none), and whether a pool follows that tap
inline int tap_after_fire(int f) { return f == 1 ? 1 : (f == 3 ? 2 : (f >= 4 ? f - 1 : -1)); }
constexpr int MIN_SIDE = 32, MAX_SIDE = 4096;

constexpr int TS = 8;                    // output tile edge of the Fire kernel
constexpr int HT = TS + 2;               // the tile with its halo
constexpr int HPIX = HT * HT;            // 100 halo pixels
constexpr int HCT = (HPIX + 15) / 16;    // in 7 column tiles of 16
constexpr int HEAD_PIX = 64;             // pixels per block of the head kernel: 4 waves x 16

inline int stem_out(int n) { return (n - 3) / 2 + 1; }
inline int pool_out(int n) { return (n - 3 + 1) / 2 + 1; }          // ceil((n - 3) / 2) + 1; the last window starts inside for n >= 3

// ---- stem: x [N][3][H][W] of a and of b (images 0..N-1 = a, N..2N-1 = b) -> out [2N][Ho][Wo][64]
// one thread = one pixel x 16 channels; k = (c, ky, kx) rising, one fmaf chain per output
__global__ __launch_bounds__(256) void sq_stem_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int H, int W, int Ho, int Wo,
                                                      const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ws[27 * 64];      // [k][c]
  __shared__ __attribute__((aligned(16))) float bs[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) ws[(i % 27) * 64 + i / 27] = w[i];
  if (threadIdx.x < 64) bs[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};     // the ScalingLayer buffers
  const long total = (long)2 * N * Ho * Wo * 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int g = (int)(i & 3);
    const long pix = i >> 2;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), img = (int)(pix / ((long)Wo * Ho));
    const float* src = (img < N ? a + (size_t)img * 3 * H * W : b + (size_t)(img - N) * 3 * H * W) + (size_t)(2 * oy) * W + 2 * ox;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll 1
    for (int cy = 0; cy < 9; ++cy) {                     // (c, ky); not unrolled: 48 weights in flight, not 432
      const int c = cy / 3, ky = cy - 3 * c;
      const float sh = c == 0 ? shift[0] : (c == 1 ? shift[1] : shift[2]), sc = c == 0 ? scale[0] : (c == 1 ? scale[1] : scale[2]);
      const float* row = src + ((size_t)c * H + ky) * W;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float v = (row[kx] - sh) / sc;
        const float* wk = ws + (cy * 3 + kx) * 64 + g * 16;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
          const f32x4 w4 = *reinterpret_cast<const f32x4*>(wk + j4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j4 * 4 + e] = fmaf(v, w4[e], acc[j4 * 4 + e]);
        }
      }
    }
    float* o = out + (size_t)pix * 64 + g * 16;
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bs + g * 16 + j4 * 4);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[j4 * 4 + e] + bb[e], 0.f);
      *reinterpret_cast<f32x4*>(o + j4 * 4) = v;
    }
  }
}

// ---- 3x3 stride-2 ceil-mode max pooling, NHWC, four channels per thread
__global__ __launch_bounds__(256) void sq_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int imgs, int H, int W, int Ho, int Wo, int C) {
  const int C4 = C / 4;
  const long total = (long)imgs * Ho * Wo * C4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long pix = i / C4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), img = (int)(pix / ((long)Wo * Ho));
    const float* xi = x + (size_t)img * H * W * C + c;
    f32x4 m = *reinterpret_cast<const f32x4*>(xi + ((size_t)(2 * oy) * W + 2 * ox) * C);       // the window's first element is in range
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = 2 * oy + ky;
      if (yy >= H) break;
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = 2 * ox + kx;
        if (xx >= W) break;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xi + ((size_t)yy * W + xx) * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    *reinterpret_cast<f32x4*>(y + (size_t)pix * C + c) = m;
  }
}

// ---- expand3x3 weight [E][S][3][3] -> [E][9][S]: the S channels of a tap contiguous
__global__ __launch_bounds__(256) void sq_pack_e3_kernel(const float* __restrict__ w, float* __restrict__ p, int E, int S) {
  const int total = E * S * 9;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int s = i % S, tap = (i / S) % 9, e = i / (9 * S);
    p[i] = w[((size_t)e * S + s) * 9 + tap];
  }
}

// ---- one Fire module.  x [imgs][H][W][Cin] -> out [imgs][H][W][2E] = [relu(e1(s)) | relu(e3(s))], s = relu(squeeze(x)).
// grid (tiles x, tiles y, imgs * Z), 4 waves.  Every product is D = Wt . X^T on v_mfma_f32_16x16x4_f32: the A operand holds
// 16 output channels (lane l: row l & 15), the B operand 16 pixels (lane l: column l & 15), and both read ONE 16-byte
// vector of 4 consecutive input channels at 4 (l >> 4) of a 16-channel chunk -- MFMA i of the chunk contracts element i, so
// the K order of a chunk is (i, l >> 4) and the chunks and taps rise: a fixed order.  A lane ends up with 4 consecutive
// channels of one pixel, one vector store.
//   phase 1: the squeeze map of the 10 x 10 halo tile into LDS (pixel-major rows of S + 4 floats), bias + ReLU applied;
//            a halo pixel OUTSIDE the image is 0 -- expand3x3 pads the post-ReLU squeeze map with zeros, not with
//            relu(bias), which a squeeze of a zero-padded input would give.
//   phase 2: the 2E / 16 row tiles of the two expands are dealt to the 4 Z waves of the tile (Z > 1 only sizes the grid
//            of small maps: every workgroup of a tile recomputes the squeeze map, no output element's arithmetic changes).
template <int NRT>
__global__ __launch_bounds__(256) void sq_fire_kernel(const float* __restrict__ x, int H, int W, int Cin, const float* __restrict__ wsq,
                                                      const float* __restrict__ bsq, const float* __restrict__ we1, const float* __restrict__ be1,
                                                      const float* __restrict__ we3, const float* __restrict__ be3, int E, int Z,
                                                      float* __restrict__ out) {
  constexpr int S = 16 * NRT, SP = S + 4;
  __shared__ __attribute__((aligned(16))) float sq[HPIX * SP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int tx0 = blockIdx.x * TS, ty0 = blockIdx.y * TS;
  const int img = blockIdx.z / Z, z = blockIdx.z % Z;
  const float* xi = x + (size_t)img * H * W * Cin;
  for (int ct = wv; ct < HCT; ct += 4) {                 // uniform over the wave: every MFMA runs with all lanes
    const int p = ct * 16 + r;
    const int y = ty0 + p / HT - 1, xx = tx0 + p % HT - 1;
    const bool inside = p < HPIX && y >= 0 && y < H && xx >= 0 && xx < W;
    const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y), xc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);       // a clamped read, its result is not used
    const float* bp = xi + ((size_t)yc * W + xc) * Cin + 4 * q;
    const float* ap = wsq + (size_t)r * Cin + 4 * q;
    f32x4 acc[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Cin; k0 += 16) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + k0);
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ap + (size_t)rt * 16 * Cin + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[rt], 0, 0, 0);
      }
    }
    if (p < HPIX) {
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(bsq + rt * 16 + 4 * q);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = inside ? fmaxf(acc[rt][i] + bb[i], 0.f) : 0.f;
        *reinterpret_cast<f32x4*>(sq + p * SP + rt * 16 + 4 * q) = v;
      }
    }
  }
  __syncthreads();
  const int nt = E / 16;
  int cen[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int op = m * 16 + r;
    cen[m] = (((op >> 3) + 1) * HT + (op & 7) + 1) * SP + 4 * q;
  }
  float* oi = out + (size_t)img * H * W * 2 * E;
  for (int t = z * 4 + wv; t < 2 * nt; t += 4 * Z) {     // uniform over the wave
    const bool is3 = t >= nt;
    const int rt = is3 ? t - nt : t;
    const int ntap = is3 ? 9 : 1;
    const float* ap = (is3 ? we3 + (size_t)(rt * 16 + r) * 9 * S : we1 + (size_t)(rt * 16 + r) * S) + 4 * q;
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < ntap; ++tap) {
      const int off = is3 ? ((tap / 3 - 1) * HT + tap % 3 - 1) * SP : 0;
#pragma unroll
      for (int k0 = 0; k0 < S; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ap + tap * S + k0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(sq + cen[m] + off + k0);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[m], 0, 0, 0);
        }
      }
    }
    const int c = rt * 16 + 4 * q;
    const f32x4 bb = *reinterpret_cast<const f32x4*>((is3 ? be3 : be1) + c);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int op = m * 16 + r;
      const int y = ty0 + (op >> 3), xx = tx0 + (op & 7);
      if (y < H && xx < W) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[m][i] + bb[i], 0.f);
        *reinterpret_cast<f32x4*>(oi + ((size_t)y * W + xx) * 2 * E + (is3 ? E : 0) + c) = v;
      }
    }
  }
}

// ---- head of one tap.  f [2N][HW][C]: pair n = images n and N + n.  One wave per pixel: both channel norms, then
// sum_c lin[c] (a_c / (|a| + eps) - b_c / (|b| + eps))^2; a wave adds its 16 pixels in rising order, the block its four
// waves as (w0 + w1) + (w2 + w3): part[n][block].  grid (ceil(HW / 64), N)
__global__ __launch_bounds__(256) void sq_head_kernel(const float* __restrict__ f, const float* __restrict__ lin, int N, int HW, int C,
                                                      float* __restrict__ part) {
  __shared__ float ws[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const float* fa = f + (size_t)n * HW * C;
  const float* fb = f + (size_t)(N + n) * HW * C;
  float sum = 0.f;
  for (int j = 0; j < HEAD_PIX / 4; ++j) {
    const long pix = (long)blockIdx.x * HEAD_PIX + wv * (HEAD_PIX / 4) + j;
    if (pix >= HW) break;                                // uniform over the wave
    float va[8], vb[8], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = lane + 64 * k;
      va[k] = c < C ? fa[pix * C + c] : 0.f;
      vb[k] = c < C ? fb[pix * C + c] : 0.f;
      sa += va[k] * va[k];
      sb += vb[k] * vb[k];
    }
    const float na = sqrtf(wave_sum(sa)) + 1e-10f, nb = sqrtf(wave_sum(sb)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = lane + 64 * k;
      if (c < C) {
        const float df = va[k] / na - vb[k] / nb;
        d += lin[c] * (df * df);
      }
    }
    sum += wave_sum(d);
  }
  if (lane == 0) ws[wv] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

struct SumArgs {
  const float* part[NTAP];
  int nblk[NTAP];
  int hw[NTAP];
};
// ---- dist[n] = sum_k (sum of the partials of tap k) / (H_k W_k): thread t adds the partials t, t + 256, ... in rising
// order, then a fixed binary tree over the 256 threads; the taps in rising order.  grid (N)
__global__ __launch_bounds__(256) void sq_sum_kernel(SumArgs a, float* __restrict__ dist) {
  __shared__ float s[256];
  const int n = blockIdx.x;
  float total = 0.f;
  for (int k = 0; k < NTAP; ++k) {
    float v = 0.f;
    for (int i = threadIdx.x; i < a.nblk[k]; i += 256) v += a.part[k][(size_t)n * a.nblk[k] + i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
      __syncthreads();
    }
    total += s[0] / (float)a.hw[k];
    __syncthreads();
  }
  if (threadIdx.x == 0) dist[n] = total;
}

struct Fire {
  int idx, cin, s, e;
  float *wsq, *bsq, *we1, *be1, *we3, *be3, *we3p;
};

}  // namespace

struct HEDIT_HANDLE hedit_sqlpips : ParamStore {
  float *w0 = nullptr, *b0 = nullptr;
  Fire fire[NFIRE];
  float* lin[NTAP] = {};
};

namespace {


int fire_launch(const Fire& f, const float* x, int imgs, int H, int W, float* out, hipStream_t st) {
  const int tx = cdiv(W, TS), ty = cdiv(H, TS), nt = f.e / 16;
  // small maps: the row tiles of a tile are dealt to Z workgroups.  A function of (H, W) and the layer alone.
  const int Z = tx * ty >= 64 || nt < 8 ? 1 : (nt >= 12 ? 4 : 2);
  const dim3 grid(tx, ty, imgs * Z), block(256);
#define SQ_FIRE(NRT)                                                                                                                     \
  hipLaunchKernelGGL(sq_fire_kernel<NRT>, grid, block, 0, st, x, H, W, f.cin, f.wsq, f.bsq, f.we1, f.be1, f.we3p, f.be3, f.e, Z, out)
  switch (f.s) {
    case 16: SQ_FIRE(1); break;
    case 32: SQ_FIRE(2); break;
    case 48: SQ_FIRE(3); break;
    default: SQ_FIRE(4); break;
  }
#undef SQ_FIRE
  LAUNCH_CHECK();
  return HEDIT_OK;
}

// a, b fp32 [N][3][H][W] -> dist [N]
int run(hedit_sqlpips* h, const float* a, const float* b, int N, int H0, int W0, float* dist, void* ws, size_t ws_bytes, hipStream_t st, bool dry,
        size_t* peak) {
  Arena ar;
  ar.dry = dry;
  ar.base = reinterpret_cast<char*>(ws);
  ar.cap = ws_bytes;
  const int imgs = 2 * N;
  SumArgs sa{};
  float* part[NTAP];
  // the partial sums of the seven heads live to the end; the maps come and go
  {
    int H = stem_out(H0), W = stem_out(W0);
    for (int k = 0; k < NTAP; ++k) {
      sa.hw[k] = H * W;
      sa.nblk[k] = cdiv((long)H * W, HEAD_PIX);
      TRY(aalloc(ar, &part[k], (size_t)N * sa.nblk[k]));
      sa.part[k] = part[k];
      if (k < 3) { H = pool_out(H); W = pool_out(W); }
    }
  }
  auto head = [&](int k, const float* f, int H, int W) -> int {
    if (dry) return HEDIT_OK;
    hipLaunchKernelGGL(sq_head_kernel, dim3(sa.nblk[k], N), dim3(256), 0, st, f, h->lin[k], N, H * W, TAP_C[k], part[k]);
    LAUNCH_CHECK();
    return HEDIT_OK;
  };
  auto pool = [&](float** cur, int* H, int* W, int C) -> int {
    const int Ho = pool_out(*H), Wo = pool_out(*W);
    float* y;
    TRY(aalloc(ar, &y, (size_t)imgs * Ho * Wo * C));
    if (!dry) {
      hipLaunchKernelGGL(sq_pool_kernel, dim3(ew_grid((long)imgs * Ho * Wo * C / 4)), dim3(256), 0, st, *cur, y, imgs, *H, *W, Ho, Wo, C);
      LAUNCH_CHECK();
    }
    ar.free(*cur);
    *cur = y;
    *H = Ho; *W = Wo;
    return HEDIT_OK;
  };
  int H = stem_out(H0), W = stem_out(W0);
  float* cur;
  TRY(aalloc(ar, &cur, (size_t)imgs * H * W * 64));
  if (!dry) {
    hipLaunchKernelGGL(sq_stem_kernel, dim3(ew_grid((long)imgs * H * W * 4)), dim3(256), 0, st, a, b, N, H0, W0, H, W, h->w0, h->b0, cur);
    LAUNCH_CHECK();
  }
  TRY(head(0, cur, H, W));
  TRY(pool(&cur, &H, &W, 64));
  for (int i = 0; i < NFIRE; ++i) {
    const Fire& f = h->fire[i];
    float* y;
    TRY(aalloc(ar, &y, (size_t)imgs * H * W * 2 * f.e));
    if (!dry) TRY(fire_launch(f, cur, imgs, H, W, y, st));
    ar.free(cur);
    cur = y;
    const int t = tap_after_fire(i);
    if (t >= 0) TRY(head(t, cur, H, W));
    if (t == 1 || t == 2) TRY(pool(&cur, &H, &W, 2 * f.e));
  }
  ar.free(cur);
  if (!dry) {
    hipLaunchKernelGGL(sq_sum_kernel, dim3(N), dim3(256), 0, st, sa, dist);
    LAUNCH_CHECK();
  }
  for (int k = 0; k < NTAP; ++k) ar.free(part[k]);
  if (peak) *peak = ar.peak;
  return HEDIT_OK;
}

bool sizes_ok(int N, int H, int W) {
  return N >= 1 && N <= HEDIT_SQLPIPS_MAX_BATCH && H >= MIN_SIDE && W >= MIN_SIDE && H <= MAX_SIDE && W <= MAX_SIDE;
}

}  // namespace

HEDIT_LIFECYCLE(sqlpips, hedit_sqlpips, "SqueezeNet-LPIPS", no_pre_destroy)

extern "C" {

int hedit_sqlpips_create(hedit_sqlpips** out) try {
  ARG_CHECK(out, "null");
  hedit_sqlpips* h = new hedit_sqlpips();
  h->w0 = f32conv(h, "features.0.weight", 64, 3, 3);
  h->b0 = vec(h, "features.0.bias", 64);
  for (int i = 0; i < NFIRE; ++i) {
    Fire& f = h->fire[i];
    f.idx = FIRE[i][0]; f.cin = FIRE[i][1]; f.s = FIRE[i][2]; f.e = FIRE[i][3];
    const std::string pre = "features." + std::to_string(f.idx);
    f.wsq = f32conv(h, pre + ".squeeze.weight", f.s, f.cin, 1);
    f.bsq = vec(h, pre + ".squeeze.bias", f.s);
    f.we1 = f32conv(h, pre + ".expand1x1.weight", f.e, f.s, 1);
    f.be1 = vec(h, pre + ".expand1x1.bias", f.e);
    f.we3 = f32conv(h, pre + ".expand3x3.weight", f.e, f.s, 3);
    f.be3 = vec(h, pre + ".expand3x3.bias", f.e);
    f.we3p = dalloc<float>(h, (size_t)f.e * f.s * 9);
  }
  for (int k = 0; k < NTAP; ++k) h->lin[k] = f32conv(h, "lin" + std::to_string(k) + ".model.1.weight", 1, TAP_C[k], 1);
  return handle_created(h, out);
} catch (...) { return hedit_abi_catch(); }

int hedit_sqlpips_finalize(hedit_sqlpips* h, void* stream) try {
  ARG_CHECK(h, "null");
  TRY(handle_loaded(h));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int i = 0; i < NFIRE; ++i) {
    const Fire& f = h->fire[i];
    hipLaunchKernelGGL(sq_pack_e3_kernel, dim3(ew_grid((long)f.e * f.s * 9)), dim3(256), 0, st, f.we3, f.we3p, f.e, f.s);
    LAUNCH_CHECK();
  }
  HIP_TRY(hipStreamSynchronize(st));
  h->finalized = true;
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

size_t hedit_sqlpips_workspace_bytes(hedit_sqlpips* h, int N, int height, int width) try {
  if (!h || !sizes_ok(N, height, width)) return 0;
  size_t peak = 0;
  const int rc = run(h, nullptr, nullptr, N, height, width, nullptr, nullptr, 0, nullptr, true, &peak);
  return dry_run_bytes(rc, peak);
} catch (...) { (void)hedit_abi_catch(); return 0; }

/* a, b fp32 [N][3][H][W] in [-1, 1] -> dist[n] = LPIPS(a_n, b_n).  Every argument is checked before the first launch. */
int hedit_sqlpips_distance(hedit_sqlpips* h, const float* a, const float* b, int N, int height, int width, float* dist, void* workspace,
                           size_t workspace_bytes, void* stream) try {
  ARG_CHECK(h && a && b && dist, "sqlpips_distance: null");
  TRY(handle_finalized(h));
  ARG_CHECK(height >= MIN_SIDE && width >= MIN_SIDE, "sqlpips_distance: height and width must be at least 32");
  ARG_CHECK(height <= MAX_SIDE && width <= MAX_SIDE, "sqlpips_distance: height and width must be at most 4096");
  ARG_CHECK(N >= 1 && N <= HEDIT_SQLPIPS_MAX_BATCH, "sqlpips_distance: 1 <= N <= 64");
  ARG_CHECK(workspace, "sqlpips_distance: null workspace");
  size_t need = 0;
  TRY(run(h, nullptr, nullptr, N, height, width, nullptr, nullptr, 0, nullptr, true, &need));
  if (workspace_bytes < need) {
    hedit_set_error("bad argument: sqlpips_distance: workspace too small (need " + std::to_string(need) + " bytes, got " +
                    std::to_string(workspace_bytes) + ")");
    return HEDIT_ERR_ARG;
  }
  return run(h, a, b, N, height, width, dist, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, nullptr);
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
