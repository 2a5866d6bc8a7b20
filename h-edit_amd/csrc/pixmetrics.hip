// The pixel columns of the PIE-Bench evaluator (psnr*, mse*, ssim*) as one native call on uint8 images: the formulas of the
// torchmetrics classes the reference instantiates (text-guided/evaluation/matrics_calculator.py:272-279) as
// evaluation/evaluation.py's MetricsCalculator restates them, for N pairs and all three parts (whole / edit / unedit) at once.
//
//   a = float(u8) / 255.0f (fp32), times the part's mask (1, mask, 1 - mask); d = a - b (fp32)
//   mse  = sum (double)d * (double)d / (3 H W)                                  psnr = 10 log10(1 / mse), +inf for mse == 0
//   ssim = mean over the (H - 10) x (W - 10) x 3 windows that lie inside the image of
//          (2 mu_a mu_b + c1)(2 s_ab + c2) / ((mu_a^2 + mu_b^2 + c1)(s_a + s_b + c2)),  c1 = 1e-4, c2 = 9e-4,
//          the five window moments (a, b, aa, bb, ab) under the separable 11-tap Gaussian (sigma 1.5; the fp32 taps the
//          evaluator normalises, widened to fp64), rows first, then columns, everything fp64
//
// Why fp64: the torch path's fp32 convolution and fp32 mean leave up to 1.4e-5 of noise in SSIM (cancellation in s - mu^2);
// in fp64 the result is a function of the uint8 images alone to ~1e-13, whatever the summation order.  aa, bb and ab go
// through ONE instruction sequence (moment(x, y) = sum w (x y)), so equal images give mse 0, psnr +inf and ssim 1 exactly.
//
//   tile      one block = 32 x 16 windows of one image: the 42 x 26 uint8 pixels of both images and both masks are staged in
//             LDS ONCE with aligned dword loads (rows of 3 W bytes start at any byte offset for odd W: every staged row keeps
//             its global skew, a dword that leaves the buffer is read byte by byte); each (part, channel) is then derived
//             from that copy: masked fp32 planes (+ the squared-difference sum of the pixels the tile owns) -> row pass ->
//             column pass + the quotient.  Per-block sums go through a fixed LDS tree to partial[n][quantity][tile].
//   finalise  one block per image sums the tile partials in a fixed order and writes the 3 x 3 results.
// No atomics, nothing synchronises, and the tile partition is a function of (H, W): out[n] of a batch has the bits of the
// N = 1 call on image n.  Nothing reads the 16-bit storage type: both storage builds give the same bits.
#include "../../include/hedit.h"
#include "common.h"

namespace {

constexpr int PM_HALO = 10;                            // an 11-tap window reaches 10 pixels past its first
constexpr int PM_TW = 32, PM_TH = 16;                  // windows per tile
constexpr int PM_SW = PM_TW + PM_HALO, PM_SH = PM_TH + PM_HALO;      // staged pixels: 42 x 26
constexpr int PM_PITCH = 132;                          // bytes per staged image row: 3 * 42 + a skew of up to 3, in whole dwords
constexpr int PM_MPITCH = 48;                          // bytes per staged mask row: 42 + 3, in whole dwords
constexpr int PM_FP = PM_SW + 1;                       // floats per row of the masked planes
constexpr int PM_THREADS = 256;
constexpr int PM_NQ = 6;                               // sums per image: parts (whole, edit, unedit) x (squared difference, ssim)
constexpr int PM_MIN_SIDE = 11, PM_MAX_SIDE = 16384;
static_assert(PM_PITCH % 4 == 0 && PM_PITCH >= 3 * PM_SW + 3 + 3 && PM_MPITCH % 4 == 0 && PM_MPITCH >= PM_SW + 3 + 3, "staging pitches");
static_assert(PM_NQ * PM_THREADS <= 5 * PM_SH * PM_TW, "the reduction tree lives in the row-pass buffer");

// the evaluator's _gauss(11, 1.5) before the outer product: exp(-(d / 1.5)^2 / 2) / sum in fp32, d = -5 ... 5
#define PM_TAPS {0x1.0d957p-10, 0x1.f1fdf8p-8, 0x1.26eb18p-5, 0x1.bff0fcp-4, 0x1.b43c3ep-3, 0x1.10656p-2, \
                 0x1.b43c3ep-3, 0x1.bff0fcp-4, 0x1.26eb18p-5, 0x1.f1fdf8p-8, 0x1.0d957p-10}

inline int tiles_x(int W) { return cdiv(W - PM_HALO, PM_TW); }
inline int tiles_y(int H) { return cdiv(H - PM_HALO, PM_TH); }

// rows x nbytes bytes starting at base[off0], row_stride apart -> lds, row r at lds + r * pitch + (its global address & 3).
// One aligned dword per lane; a dword that is not wholly inside [base, base + total) takes its in-range bytes one by one.
__device__ __forceinline__ void pm_stage(const uint8_t* __restrict__ base, size_t total, size_t off0, size_t row_stride, int rows, int nbytes,
                                         uint32_t* __restrict__ lds, int pitch) {
  const int per_row = pitch / 4;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), hi = lo + total;
  for (int i = threadIdx.x; i < rows * per_row; i += PM_THREADS) {
    const int r = i / per_row, j = i - r * per_row;
    const uintptr_t g0 = lo + off0 + (size_t)r * row_stride;
    const uintptr_t a = (g0 & ~(uintptr_t)3) + 4 * (uintptr_t)j;
    if (a >= g0 + (uintptr_t)nbytes) continue;
    uint32_t v = 0;
    if (a >= lo && a + 4 <= hi) {
      v = *reinterpret_cast<const uint32_t*>(a);
    } else {
      for (int k = 0; k < 4; ++k)
        if (a + k >= lo && a + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + k)) << (8 * k);
    }
    lds[r * per_row + j] = v;
  }
}

// sum_k w[k] (x_k y_k): the ONE sequence behind the aa, bb and ab moments
__device__ __forceinline__ double pm_mul(double x, double y) { return x * y; }

__global__ __launch_bounds__(PM_THREADS) void pixel_tile_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                const uint8_t* __restrict__ mask_pred, const uint8_t* __restrict__ mask_gt, int N,
                                                                int H, int W, int ntx, int ntiles, double* __restrict__ partial) {
  __shared__ uint32_t s_a[PM_SH * PM_PITCH / 4], s_b[PM_SH * PM_PITCH / 4];
  __shared__ uint32_t s_ma[PM_SH * PM_MPITCH / 4], s_mb[PM_SH * PM_MPITCH / 4];
  __shared__ float s_lut[256];
  __shared__ float s_fa[PM_SH * PM_FP], s_fb[PM_SH * PM_FP];
  __shared__ double s_h[5 * PM_SH * PM_TW];            // row-pass moments [m][row][col]; afterwards the reduction tree
  const double w[11] = PM_TAPS;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int ty = tile / ntx, tx = tile - ty * ntx;
  const int r0 = ty * PM_TH, c0 = tx * PM_TW;
  const int nwr = min(PM_TH, H - PM_HALO - r0), nwc = min(PM_TW, W - PM_HALO - c0);       // windows of this tile, >= 1
  const int rows = nwr + PM_HALO, cols = nwc + PM_HALO;                                   // staged pixels, inside the image
  // the pixels whose squared difference this tile adds: its 16 x 32 block, the last tile of a row / column to the image edge
  const int own_r = (r0 + nwr == H - PM_HALO) ? rows : PM_TH, own_c = (c0 + nwc == W - PM_HALO) ? cols : PM_TW;
  const bool masked = mask_pred != nullptr || mask_gt != nullptr;

  const size_t img_total = (size_t)N * H * W * 3, msk_total = (size_t)N * H * W;
  const size_t img_off = (((size_t)n * H + r0) * W + c0) * 3, msk_off = ((size_t)n * H + r0) * W + c0;
  pm_stage(pred, img_total, img_off, (size_t)W * 3, rows, cols * 3, s_a, PM_PITCH);
  pm_stage(gt, img_total, img_off, (size_t)W * 3, rows, cols * 3, s_b, PM_PITCH);
  if (mask_pred) pm_stage(mask_pred, msk_total, msk_off, (size_t)W, rows, cols, s_ma, PM_MPITCH);
  if (mask_gt) pm_stage(mask_gt, msk_total, msk_off, (size_t)W, rows, cols, s_mb, PM_MPITCH);
  s_lut[tid] = (float)tid / 255.0f;
  // the skew of staged row r: (address of its first byte) & 3
  const uint32_t ska0 = (uint32_t)((reinterpret_cast<uintptr_t>(pred) + img_off) & 3), skb0 = (uint32_t)((reinterpret_cast<uintptr_t>(gt) + img_off) & 3);
  const uint32_t skma0 = (uint32_t)((reinterpret_cast<uintptr_t>(mask_pred) + msk_off) & 3);
  const uint32_t skmb0 = (uint32_t)((reinterpret_cast<uintptr_t>(mask_gt) + msk_off) & 3);
  const uint32_t rs3 = (uint32_t)(((size_t)W * 3) & 3), rs1 = (uint32_t)(W & 3);
  const uint8_t* ba = reinterpret_cast<const uint8_t*>(s_a);
  const uint8_t* bb = reinterpret_cast<const uint8_t*>(s_b);
  const uint8_t* bma = reinterpret_cast<const uint8_t*>(s_ma);
  const uint8_t* bmb = reinterpret_cast<const uint8_t*>(s_mb);
  __syncthreads();

  double acc_d[3] = {0.0, 0.0, 0.0}, acc_s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    if (p > 0 && !masked) break;                       // block-uniform
    for (int ch = 0; ch < 3; ++ch) {
      // ---- masked fp32 planes of this (part, channel), and the squared differences of the owned pixels
      for (int i = tid; i < rows * cols; i += PM_THREADS) {
        const int r = i / cols, c = i - r * cols;
        float a = s_lut[ba[r * PM_PITCH + ((ska0 + r * rs3) & 3) + 3 * c + ch]];
        float b = s_lut[bb[r * PM_PITCH + ((skb0 + r * rs3) & 3) + 3 * c + ch]];
        if (p > 0) {
          const float ma = mask_pred ? (float)bma[r * PM_MPITCH + ((skma0 + r * rs1) & 3) + c] : 1.0f;
          const float mb = mask_gt ? (float)bmb[r * PM_MPITCH + ((skmb0 + r * rs1) & 3) + c] : 1.0f;
          a = a * (p == 1 ? ma : 1.0f - ma);
          b = b * (p == 1 ? mb : 1.0f - mb);
        }
        s_fa[r * PM_FP + c] = a;
        s_fb[r * PM_FP + c] = b;
        if (r < own_r && c < own_c) {
          const double d = (double)(a - b);
          acc_d[p] += d * d;
        }
      }
      __syncthreads();
      // ---- row pass: the five moments of every staged row at every window column
      for (int i = tid; i < rows * nwc; i += PM_THREADS) {
        const int r = i / nwc, c = i - r * nwc;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double x = (double)s_fa[r * PM_FP + c + k], y = (double)s_fb[r * PM_FP + c + k];
          m0 += w[k] * x;
          m1 += w[k] * y;
          m2 += w[k] * pm_mul(x, x);
          m3 += w[k] * pm_mul(y, y);
          m4 += w[k] * pm_mul(x, y);
        }
        s_h[(0 * PM_SH + r) * PM_TW + c] = m0;
        s_h[(1 * PM_SH + r) * PM_TW + c] = m1;
        s_h[(2 * PM_SH + r) * PM_TW + c] = m2;
        s_h[(3 * PM_SH + r) * PM_TW + c] = m3;
        s_h[(4 * PM_SH + r) * PM_TW + c] = m4;
      }
      __syncthreads();
      // ---- column pass and the quotient
      for (int i = tid; i < nwr * nwc; i += PM_THREADS) {
        const int r = i / nwc, c = i - r * nwc;
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 11; ++k) s += w[k] * s_h[(q * PM_SH + r + k) * PM_TW + c];
          m[q] = s;
        }
        const double mu_a = m[0], mu_b = m[1];
        const double va = m[2] - pm_mul(mu_a, mu_a), vb = m[3] - pm_mul(mu_b, mu_b), vab = m[4] - pm_mul(mu_a, mu_b);
        const double num = (2.0 * pm_mul(mu_a, mu_b) + 1e-4) * (2.0 * vab + 9e-4);
        const double den = (pm_mul(mu_a, mu_a) + pm_mul(mu_b, mu_b) + 1e-4) * (va + vb + 9e-4);
        acc_s[p] += num / den;
      }
      // the next plane pass writes s_fa / s_fb only; the barrier after it orders the next row pass behind this column pass
    }
  }
  __syncthreads();
  // ---- the block's six sums: a fixed tree over the 256 threads
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    s_h[(2 * p) * PM_THREADS + tid] = acc_d[p];
    s_h[(2 * p + 1) * PM_THREADS + tid] = acc_s[p];
  }
  __syncthreads();
  for (int s = PM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int q = 0; q < PM_NQ; ++q) s_h[q * PM_THREADS + tid] += s_h[q * PM_THREADS + tid + s];
    }
    __syncthreads();
  }
  if (tid < PM_NQ) partial[((size_t)n * PM_NQ + tid) * ntiles + tile] = s_h[tid * PM_THREADS];
}

// one block per image: the tile partials of each quantity in a fixed order (thread t takes tiles t, t + 256, ..., then the tree)
__global__ __launch_bounds__(PM_THREADS) void pixel_finalise_kernel(const double* __restrict__ partial, int ntiles, int H, int W, int masked,
                                                                    double* __restrict__ out) {
  __shared__ double s_r[PM_NQ * PM_THREADS];
  const int tid = threadIdx.x, n = blockIdx.x;
#pragma unroll
  for (int q = 0; q < PM_NQ; ++q) {
    const double* src = partial + ((size_t)n * PM_NQ + q) * ntiles;
    double s = 0.0;
    for (int t = tid; t < ntiles; t += PM_THREADS) s += src[t];
    s_r[q * PM_THREADS + tid] = s;
  }
  __syncthreads();
  for (int s = PM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int q = 0; q < PM_NQ; ++q) s_r[q * PM_THREADS + tid] += s_r[q * PM_THREADS + tid + s];
    }
    __syncthreads();
  }
  if (tid < 3) {
    double* o = out + ((size_t)n * 3 + tid) * 3;
    if (tid > 0 && !masked) {
      o[0] = o[1] = o[2] = __builtin_nan("");
    } else {
      const double mse = s_r[(2 * tid) * PM_THREADS] / (3.0 * (double)H * (double)W);
      o[0] = mse;
      o[1] = mse == 0.0 ? __builtin_inf() : 10.0 * log10(1.0 / mse);
      o[2] = s_r[(2 * tid + 1) * PM_THREADS] / (3.0 * (double)(H - PM_HALO) * (double)(W - PM_HALO));
    }
  }
}

bool sizes_ok(int N, int H, int W) {
  return N >= 1 && N <= HEDIT_PIXEL_METRICS_MAX_BATCH && H >= PM_MIN_SIDE && W >= PM_MIN_SIDE && H <= PM_MAX_SIDE && W <= PM_MAX_SIDE;
}

}  // namespace

extern "C" {

size_t hedit_pixel_metrics_workspace_bytes(int N, int H, int W) {
  if (!sizes_ok(N, H, W)) return 0;
  return (size_t)N * PM_NQ * tiles_x(W) * tiles_y(H) * sizeof(double);
}

int hedit_pixel_metrics(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask_pred, const uint8_t* mask_gt, int N, int H, int W, double* out,
                        void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(pred && gt && out && workspace, "pixel_metrics: null");
  ARG_CHECK(N >= 1 && N <= HEDIT_PIXEL_METRICS_MAX_BATCH, "pixel_metrics: 1 <= N <= 64");
  ARG_CHECK(H >= PM_MIN_SIDE && W >= PM_MIN_SIDE, "pixel_metrics: height and width must be at least 11 (one SSIM window)");
  ARG_CHECK(H <= PM_MAX_SIDE && W <= PM_MAX_SIDE, "pixel_metrics: height and width must be at most 16384");
  ARG_CHECK(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0, "pixel_metrics: out and workspace must be 8-byte aligned");
  const size_t need = hedit_pixel_metrics_workspace_bytes(N, H, W);
  if (workspace_bytes < need) {
    hedit_set_error("bad argument: pixel_metrics: workspace too small (need " + std::to_string(need) + " bytes, got " + std::to_string(workspace_bytes) +
                    ")");
    return HEDIT_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int ntx = tiles_x(W), ntiles = ntx * tiles_y(H);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(pixel_tile_kernel, dim3(ntiles, N), dim3(PM_THREADS), 0, st, pred, gt, mask_pred, mask_gt, N, H, W, ntx, ntiles, partial);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(pixel_finalise_kernel, dim3(N), dim3(PM_THREADS), 0, st, partial, ntiles, H, W, (mask_pred || mask_gt) ? 1 : 0, out);
  LAUNCH_CHECK();
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
