// The small fp32 kernels every pre-LN transformer encoder of the library runs around its GEMMs and its own attention kernel
// (vit.hip: the style Gram encoder; text.hip: the CLIP text encoder; clipimg.hip: the CLIP image tower; dino.hip: the DINO key
// extractor): patch extraction, token assembly, LayerNorm forward, out = res + raw + bias, and the row gather of the pooled
// outputs.  One definition each; what differs between the encoders is an argument (the LayerNorm eps, a null pointer for a
// term an encoder does not have).  An optional term is a branch on its pointer, never an added 0.f: -0.0f + 0.f is +0.0f.
// The host side (block struct, registration, packing, the block forward) is encoder.h.
#include "common.h"
#include "kernels.h"

namespace {

// img [B][3][R][R] -> X [B*P*P][3*p*p], column = (c, ky, kx): a conv with kernel = stride = p is a linear map.
// bwd: the inverse permutation X -> img (every pixel belongs to exactly one patch)
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, float* __restrict__ X, int B, int R, int p, int bwd) {
  const int P = R / p, K = 3 * p * p;
  const long total = (long)B * P * P * K;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int k = (int)(i % K);
    const long row = i / K;
    const int b = (int)(row / (P * P)), pr = (int)(row % (P * P));
    const int c = k / (p * p), ky = (k / p) % p, kx = k % p;
    const long src = (((long)b * 3 + c) * R + (pr / P) * p + ky) * R + (pr % P) * p + kx;
    if (bwd) const_cast<float*>(img)[src] = X[i];
    else X[i] = img[src];
  }
}
// T[b][0] = cls + pos[0]; T[b][1+l] = E[b][l] + pos[1+l], or (E[b][l] + conv bias) + pos[1+l] when the patch conv has a bias
__global__ __launch_bounds__(256) void tokens_kernel(const float* __restrict__ E, const float* __restrict__ cbias, const float* __restrict__ cls,
                                                     const float* __restrict__ pos, float* __restrict__ T, int B, int L, int W) {
  const long total = (long)B * L * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int w = (int)(i % W);
    const long row = i / W;
    const int b = (int)(row / L), l = (int)(row % L);
    if (cbias) T[i] = (l == 0 ? cls[w] : E[((long)b * (L - 1) + l - 1) * W + w] + cbias[w]) + pos[(long)l * W + w];
    else T[i] = (l == 0 ? cls[w] : E[((long)b * (L - 1) + l - 1) * W + w]) + pos[(long)l * W + w];
  }
}
// R[b] = T[b][idx ? clamp(idx[b]) : 0]: the pooled row of a prompt, or the class rows
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ T, const int32_t* __restrict__ idx, float* __restrict__ R,
                                                          int B, int L, int W) {
  const long total = (long)B * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int w = (int)(i % W), b = (int)(i / W);
    int l = idx ? idx[b] : 0;
    l = l < 0 ? 0 : (l >= L ? L - 1 : l);
    R[i] = T[((long)b * L + l) * W + w];
  }
}
// LayerNorm over W, one wave per row; stats (or null): [rows][2] = (mean, rstd), kept for a backward pass
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                 float* __restrict__ y, float* __restrict__ stats, long rows, int W, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * W;
  float s = 0.f;
  for (int i = lane; i < W; i += 64) s += xr[i];
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
  for (int i = lane; i < W; i += 64) { const float d = xr[i] - mean; q += d * d; }
  const float rstd = rsqrtf(wave_sum(q) / (float)W + eps);
  for (int i = lane; i < W; i += 64) y[row * W + i] = (xr[i] - mean) * rstd * g[i] + b[i];
  if (stats && lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
}
// out = res + raw + bias, or raw + bias without a residual
__global__ __launch_bounds__(256) void add_bias_res_kernel(const float* __restrict__ raw, const float* __restrict__ bias, const float* __restrict__ res,
                                                           float* __restrict__ out, long total, int W) {
  if (res) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) out[i] = res[i] + raw[i] + bias[i % W];
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) out[i] = raw[i] + bias[i % W];
  }
}

}  // namespace

int enc_patchify_launch(const float* img, float* X, int B, int R, int p, int bwd, hipStream_t st) {
  const int P = R / p;
  hipLaunchKernelGGL(patchify_kernel, dim3(ew_grid((long)B * P * P * 3 * p * p)), dim3(256), 0, st, img, X, B, R, p, bwd);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
int enc_tokens_launch(const float* E, const float* cbias, const float* cls, const float* pos, float* T, int B, int L, int W, hipStream_t st) {
  hipLaunchKernelGGL(tokens_kernel, dim3(ew_grid((long)B * L * W)), dim3(256), 0, st, E, cbias, cls, pos, T, B, L, W);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
int enc_gather_rows_launch(const float* T, const int32_t* idx, float* R, int B, int L, int W, hipStream_t st) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3(ew_grid((long)B * W)), dim3(256), 0, st, T, idx, R, B, L, W);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
int enc_ln_launch(const float* x, const float* g, const float* b, float* y, float* stats, long rows, int W, float eps, hipStream_t st) {
  hipLaunchKernelGGL(ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, g, b, y, stats, rows, W, eps);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
int enc_add_bias_res_launch(const float* raw, const float* bias, const float* res, float* out, long total, int W, hipStream_t st) {
  hipLaunchKernelGGL(add_bias_res_kernel, dim3(ew_grid(total)), dim3(256), 0, st, raw, bias, res, out, total, W);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
