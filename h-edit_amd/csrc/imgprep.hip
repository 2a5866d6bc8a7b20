// The image side of the evaluator's CLIP metrics on the device, and the head of its local_clip column.
//
// hedit_image_prep: what PIL's Image.resize + a crop + ToTensor / Normalize do to a uint8 image, bit for bit.  The resample is
// Pillow's Resample.c for 8-bit images: two separable passes, horizontal first, the intermediate ROUNDED AND CLAMPED TO UINT8
// between them; taps in 32-bit fixed point with 22 fractional bits, an int32 accumulator that starts at 1 << 21, the result
// clamp(acc >> 22, 0, 255).  The kernels know no filter: they take the [out][ksize] int32 taps and the (first, count) pair of
// every output index that the host built in float64 (hedit/image_prep.py: bilinear and bicubic), and a null table for an axis
// whose size does not change -- Pillow skips that pass, here it is a copy.  The normalisation is a [3][256] fp32 look-up table,
// also the host's, so the output bits are those of the host formula by construction.
//
//   launch 1  (rows)     source rows [row0, row0 + nrows) -- the rows the crop's vertical taps read -- at the crop's columns:
//                        uint8 workspace [B][nrows][cw][3]
//   launch 2  (columns)  the crop's rows from the workspace -> fp32 [B][3][ch][cw] through the table (+ the uint8 pixels
//                        [B][ch][cw][3] when asked for)
// Only pixels the crop needs are computed.  One thread per output value, integer arithmetic: no atomics, nothing synchronises,
// image b has the bits of the B = 1 call, and nothing reads the 16-bit storage type (both storage builds give the same bits).
// The (first, count) pairs live in device memory and cannot be checked by the entry; a pair that leaves the source is cut to it.
//
// hedit_clip_direction: cos(e^, D) of text-guided/evaluation/local_clip_evaluation.py (clip_directional_loss with the
// DirectionMetric), one workgroup per pair, everything after the fp32 loads in fp64:
//   s^_j = s_j / |s_j|, t^_j = t_j / |t_j| per template; d = sum_j (t^_j - s^_j) / T (j in index order); D = d / |d|
//   a^ = a / |a|, b^ = b / |b|; e = b^ - a^; e^ = e / (|e| + 1e-7); out = e^ . D / (max(|e^|, 1e-8) max(|D|, 1e-8))
// Reductions over E: lane / thread l takes e = l, l + n, l + 2n, ... in order, then a fixed butterfly (wave) or LDS tree
// (workgroup) -- functions of E alone, so out[p] has the bits of the P = 1 call.  Equal image features give e = 0 and exactly
// 0.0; equal prompt features give d = 0 and NaN, the reference's 0 / 0.
#include "../../include/hedit.h"
#include "common.h"

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_MAX_SIDE = 16384;
constexpr int IP_PREC = 22;

// clamp((1 << 21 + sum_k p[(first + k) stride] taps[k]) >> 22, 0, 255)
__device__ __forceinline__ int ip_resample(const uint8_t* __restrict__ p, size_t stride, const int32_t* __restrict__ taps, int first, int count) {
  int acc = 1 << (IP_PREC - 1);
  for (int k = 0; k < count; ++k) acc += (int)p[(size_t)(first + k) * stride] * taps[k];
  acc >>= IP_PREC;
  return min(max(acc, 0), 255);
}

__global__ __launch_bounds__(IP_THREADS) void ip_rows_kernel(const uint8_t* __restrict__ src, int H, int W, int row0, int nrows, int left, int cw,
                                                             const int32_t* __restrict__ taps, const int32_t* __restrict__ bounds, int ksize,
                                                             uint8_t* __restrict__ ws) {
  const int i = blockIdx.x * IP_THREADS + threadIdx.x;
  if (i >= cw * 3) return;
  const int x = i / 3, c = i - 3 * x, r = blockIdx.y, b = blockIdx.z;
  const int ox = left + x;
  const uint8_t* row = src + (((size_t)b * H + row0 + r) * W) * 3 + c;
  int v;
  if (taps == nullptr) {
    v = row[(size_t)ox * 3];
  } else {
    const int first = min(max(bounds[2 * ox], 0), W);
    const int count = min(min(bounds[2 * ox + 1], ksize), W - first);
    v = ip_resample(row, 3, taps + (size_t)ox * ksize, first, count);
  }
  ws[(((size_t)b * nrows + r) * cw + x) * 3 + c] = (uint8_t)v;
}

__global__ __launch_bounds__(IP_THREADS) void ip_cols_kernel(const uint8_t* __restrict__ ws, int row0, int nrows, int top, int ch, int cw,
                                                             const int32_t* __restrict__ taps, const int32_t* __restrict__ bounds, int ksize,
                                                             const float* __restrict__ lut, float* __restrict__ out, uint8_t* __restrict__ out_u8) {
  const int i = blockIdx.x * IP_THREADS + threadIdx.x;
  if (i >= cw * 3) return;
  const int c = i / cw, x = i - c * cw, y = blockIdx.y, b = blockIdx.z;   // channel-major: the fp32 stores of a wave are contiguous
  const uint8_t* col = ws + ((size_t)b * nrows * cw + x) * 3 + c;
  const size_t stride = (size_t)cw * 3;
  int v;
  if (taps == nullptr) {
    v = col[(size_t)y * stride];                       // row0 == top, nrows == ch
  } else {
    const int oy = top + y;
    const int first = min(max(bounds[2 * oy] - row0, 0), nrows);
    const int count = min(min(bounds[2 * oy + 1], ksize), nrows - first);
    v = ip_resample(col, stride, taps + (size_t)oy * ksize, first, count);
  }
  out[(((size_t)b * 3 + c) * ch + y) * cw + x] = lut[c * 256 + v];
  if (out_u8 != nullptr) out_u8[(((size_t)b * ch + y) * cw + x) * 3 + c] = (uint8_t)v;
}

bool side_ok(int v) { return v >= 1 && v <= IP_MAX_SIDE; }

// ---------------------------------------------------------------------------------------------------- the direction head
constexpr int CD_THREADS = 256;
constexpr int CD_WAVE = 64;
constexpr int CD_WAVES = CD_THREADS / CD_WAVE;

// |v|^2 of one fp32 vector by one wave: lane l takes e = l, l + 64, ... in order, then the xor butterfly (every lane ends with
// the same sum: each level adds the same two values in either order)
__device__ __forceinline__ double cd_wave_sumsq(const float* __restrict__ v, int E, int lane) {
  double s = 0.0;
  for (int e = lane; e < E; e += CD_WAVE) {
    const double x = (double)v[e];
    s += x * x;
  }
  for (int m = CD_WAVE / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, CD_WAVE);
  return s;
}

// the workgroup's sum of one value per thread: a fixed LDS tree; every thread returns the total
__device__ __forceinline__ double cd_block_sum(double v, double* s_red, int tid) {
  __syncthreads();                                     // the previous result has been read
  s_red[tid] = v;
  __syncthreads();
  for (int s = CD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  return s_red[0];
}

__global__ __launch_bounds__(CD_THREADS) void clip_direction_kernel(const float* __restrict__ txt, const float* __restrict__ img, int T, int E,
                                                                    double* __restrict__ out) {
  __shared__ double s_norm[2 * HEDIT_CLIP_DIRECTION_MAX_TEMPLATES];      // |s_j| then |t_j|
  __shared__ double s_d[HEDIT_CLIP_DIRECTION_MAX_DIM];
  __shared__ double s_red[CD_THREADS];
  const int tid = threadIdx.x, lane = tid % CD_WAVE, wave = tid / CD_WAVE, p = blockIdx.x;
  const float* tx = txt + (size_t)p * 2 * T * E;
  const float* im = img + (size_t)p * 2 * E;
  for (int v = wave; v < 2 * T; v += CD_WAVES) {
    const double n = sqrt(cd_wave_sumsq(tx + (size_t)v * E, E, lane));
    if (lane == 0) s_norm[v] = n;
  }
  const double na = sqrt(cd_wave_sumsq(im, E, lane)), nb = sqrt(cd_wave_sumsq(im + E, E, lane));       // every wave, the same bits
  __syncthreads();
  // d = mean_j (t^_j - s^_j), per component in index order; |d|^2
  double part = 0.0;
  for (int e = tid; e < E; e += CD_THREADS) {
    double s = 0.0;
    for (int j = 0; j < T; ++j) s += (double)tx[(size_t)(T + j) * E + e] / s_norm[T + j] - (double)tx[(size_t)j * E + e] / s_norm[j];
    s = s / (double)T;
    s_d[e] = s;
    part += s * s;
  }
  const double nd = sqrt(cd_block_sum(part, s_red, tid));
  // e = b^ - a^; |e|
  part = 0.0;
  for (int e = tid; e < E; e += CD_THREADS) {
    const double x = (double)im[E + e] / nb - (double)im[e] / na;
    part += x * x;
  }
  const double ne = sqrt(cd_block_sum(part, s_red, tid));
  // e^ = e / (|e| + 1e-7), D = d / |d|: their dot product and norms
  double dot = 0.0, n1 = 0.0, n2 = 0.0;
  for (int e = tid; e < E; e += CD_THREADS) {
    const double x = ((double)im[E + e] / nb - (double)im[e] / na) / (ne + 1e-7);
    const double y = s_d[e] / nd;
    dot += x * y;
    n1 += x * x;
    n2 += y * y;
  }
  dot = cd_block_sum(dot, s_red, tid);
  n1 = sqrt(cd_block_sum(n1, s_red, tid));
  n2 = sqrt(cd_block_sum(n2, s_red, tid));
  // fmax would drop a NaN norm; the reference's clamp keeps it
  const double m1 = n1 < 1e-8 ? 1e-8 : n1, m2 = n2 < 1e-8 ? 1e-8 : n2;
  if (tid == 0) out[p] = dot / (m1 * m2);
}

}  // namespace

extern "C" {

size_t hedit_image_prep_workspace_bytes(int B, int rows, int crop_width) {
  if (B < 1 || B > HEDIT_IMAGE_PREP_MAX_BATCH || !side_ok(rows) || !side_ok(crop_width)) return 0;
  return (size_t)B * rows * crop_width * 3;
}

int hedit_image_prep(const uint8_t* src, int B, int H, int W, int Hr, int Wr, int top, int left, int crop_height, int crop_width,
                     const int32_t* taps_x, const int32_t* bounds_x, int ksize_x, const int32_t* taps_y, const int32_t* bounds_y, int ksize_y,
                     int row0, int nrows, const float* lut, float* out, uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream) try {
  ARG_CHECK(src && lut && out && workspace, "image_prep: null");
  ARG_CHECK(B >= 1 && B <= HEDIT_IMAGE_PREP_MAX_BATCH, "image_prep: 1 <= B <= 64");
  ARG_CHECK(side_ok(H) && side_ok(W), "image_prep: height and width must be in [1, 16384]");
  ARG_CHECK(side_ok(Hr) && side_ok(Wr), "image_prep: the resized height and width must be in [1, 16384]");
  ARG_CHECK(crop_height >= 1 && crop_width >= 1 && top >= 0 && left >= 0 && top <= Hr - crop_height && left <= Wr - crop_width,
            "image_prep: the crop leaves the resized image");
  ARG_CHECK((taps_x == nullptr) == (bounds_x == nullptr) && (taps_y == nullptr) == (bounds_y == nullptr), "image_prep: taps and bounds go together");
  ARG_CHECK(taps_x != nullptr || Wr == W, "image_prep: a null horizontal table means an unchanged width");
  ARG_CHECK(taps_y != nullptr || Hr == H, "image_prep: a null vertical table means an unchanged height");
  ARG_CHECK((taps_x == nullptr || (ksize_x >= 1 && ksize_x <= HEDIT_IMAGE_PREP_MAX_TAPS)) &&
                (taps_y == nullptr || (ksize_y >= 1 && ksize_y <= HEDIT_IMAGE_PREP_MAX_TAPS)),
            "image_prep: taps per output index outside [1, 1024]");
  ARG_CHECK(row0 >= 0 && nrows >= 1 && row0 <= H - nrows, "image_prep: the source rows leave the image");
  ARG_CHECK(taps_y != nullptr || (row0 == top && nrows == crop_height), "image_prep: with an unchanged height the source rows are the crop's");
  const size_t need = hedit_image_prep_workspace_bytes(B, nrows, crop_width);
  if (workspace_bytes < need) {
    hedit_set_error("bad argument: image_prep: workspace too small (need " + std::to_string(need) + " bytes, got " + std::to_string(workspace_bytes) + ")");
    return HEDIT_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  const int gx = cdiv((long)crop_width * 3, IP_THREADS);
  hipLaunchKernelGGL(ip_rows_kernel, dim3(gx, nrows, B), dim3(IP_THREADS), 0, st, src, H, W, row0, nrows, left, crop_width, taps_x, bounds_x, ksize_x, ws);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(ip_cols_kernel, dim3(gx, crop_height, B), dim3(IP_THREADS), 0, st, ws, row0, nrows, top, crop_height, crop_width, taps_y, bounds_y,
                     ksize_y, lut, out, out_u8);
  LAUNCH_CHECK();
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

int hedit_clip_direction(const float* txt, const float* img, int P, int T, int E, double* out, void* stream) try {
  ARG_CHECK(txt && img && out, "clip_direction: null");
  ARG_CHECK(P >= 1 && P <= HEDIT_CLIP_DIRECTION_MAX_PAIRS, "clip_direction: 1 <= P <= 64");
  ARG_CHECK(T >= 1 && T <= HEDIT_CLIP_DIRECTION_MAX_TEMPLATES, "clip_direction: 1 <= T <= 256");
  ARG_CHECK(E >= 4 && E % 4 == 0 && E <= HEDIT_CLIP_DIRECTION_MAX_DIM, "clip_direction: E must be a multiple of 4, at most 4096");
  ARG_CHECK(reinterpret_cast<uintptr_t>(out) % 8 == 0, "clip_direction: out must be 8-byte aligned");
  hipLaunchKernelGGL(clip_direction_kernel, dim3(P), dim3(CD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), txt, img, T, E, out);
  LAUNCH_CHECK();
  return HEDIT_OK;
} catch (...) { return hedit_abi_catch(); }

}  // extern "C"
