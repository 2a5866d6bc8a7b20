// Input gradient of the stride-2 3x3 convolution with padding (0,1,0,1) (conv3x3 mode 2 with asym: the
// downsampling conv of the pixel UNet, face-swapping/diffusion/diffusion.py:56-71), and the skip concatenation's
// backward.  What `torch.autograd.grad(loss, xt)` pulls through `Downsample.conv` when Edit Friendly differentiates the
// rewards through the eps-network (face-swapping/inversion/ef.py:64-66,95,106).
//
//   forward   y[o,p]  = sum_{a,b in 0..2} W[a,b] x[2o+a, 2p+b]          (x zero at row Hin and column Win)
//   backward  dx[i,j] = sum W[a,b]^T dy[(i-a)/2, (j-b)/2]                over the taps with i-a, j-b even and in range
//
// By the parity (pi, pj) of the dx pixel that is four sub-convolutions over dy: even rows take a in {0, 2} (dy rows
// u, u-1 for i = 2u), odd rows take a = 1 (dy row u for i = 2u+1); columns alike -> 4 / 2 / 2 / 1 taps, 9 in all per dy
// pixel: the forward conv's FLOPs, a quarter of a 9-tap gather on the zero-stuffed dy.
//
// One launch, grid.z = the phase.  A block of 4 waves (2 x 2) owns 64 dx pixels of one phase x BN input channels; the K
// loop runs over (tap of the phase, 64-channel slab of Cout) with v_mfma_f32_16x16x32 (weights as the "A" operand,
// like gemm.hip: a lane ends up with 4 consecutive channels of one pixel).  Operands are staged global -> registers ->
// LDS (128-byte rows, 16-byte chunk c of row r in slot c ^ (r & 7): conflict-free ds_read_b128 fragments), the loads of
// the next K-tile in flight during the MFMAs of the current one.  Every output element is ONE fp32 chain over
// (slab, tap, channel) in a fixed order -- a function of the layer's shape only, never of the batch or of the tile the
// pixel fell into; no atomics, no split.
#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // (not HIP's uint4 struct: its aggregate copies defeat SROA)

// PAD1: the symmetric padding 1 of the SD UNet's Downsample2D instead: y[o,p] = sum W[a,b] x[2o+a-1, 2p+b-1], so a dx pixel
// takes the taps with i + 1 - a even -- the parities mirrored: even rows a = 1 (dy row u for i = 2u), odd rows a in {0, 2}
// (dy rows u + 1, u for i = 2u + 1; row Hq is outside) -> 1 / 2 / 2 / 4 taps.
template <int BN, bool PAD1 = false>
__global__ __launch_bounds__(256) void conv3x3_s2_dgrad_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wt,
                                                               bf16_t* __restrict__ dx, int B, int Hq, int Wq, int O, int I) {
  constexpr int BM = 64, BK = 64;
  constexpr int NI = BN / 32;          // 16-wide channel sub-tiles per wave
  constexpr int MI = 2;                // 16-wide pixel sub-tiles per wave
  constexpr int W_CH = BN / 32;        // 16-byte chunks of the weight tile per thread
  __shared__ __attribute__((aligned(16))) char smem[(BM + BN) * BK * 2];
  char* const sa = smem;
  char* const sw = smem + BM * BK * 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ph = blockIdx.z, pi = ph >> 1, pj = ph & 1;
  const int ny = (pi != 0) == PAD1 ? 2 : 1, nx = (pj != 0) == PAD1 ? 2 : 1, ntap = ny * nx;
  const long Mq = (long)B * Hq * Wq;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // staging roles: activation chunk (row, c) = (id >> 3, id & 7) for id = tid, tid + 256; weights alike
  int a_b[2], a_u[2], a_v[2];
  bool a_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = m0 + ((tid + i * 256) >> 3);
    a_ok[i] = m < Mq;
    const long mm = a_ok[i] ? m : 0;
    a_v[i] = (int)(mm % Wq);
    a_u[i] = (int)((mm / Wq) % Hq);
    a_b[i] = (int)(mm / ((long)Wq * Hq));
  }
  const int c8 = (tid & 7) * 8;
  const int nkt = ntap * (O / BK);

  u32x4 ra[2], rw[W_CH];
  auto load_tile = [&](int kt) __attribute__((always_inline)) {
    const int tap = kt % ntap, slab = kt / ntap;
    const int ty = tap / nx, tx = tap - ty * nx;
    int sy, sx, a9;
    if constexpr (PAD1) {
      sy = pi ? ty - 1 : 0, sx = pj ? tx - 1 : 0;               // dy rows u + 1 (a = 0), u (a = 2)
      a9 = (pi ? 2 * ty : 1) * 3 + (pj ? 2 * tx : 1);
    } else {
      sy = pi ? 0 : ty, sx = pj ? 0 : tx;                       // dy row / column shift (u - sy, v - sx)
      a9 = (pi ? 1 : 2 * ty) * 3 + (pj ? 1 : 2 * tx);           // the tap's index in the 3x3 filter
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = a_u[i] - sy, v = a_v[i] - sx;
      ra[i] = (u32x4){0u, 0u, 0u, 0u};
      if (a_ok[i] && u >= 0 && v >= 0 && (!PAD1 || (u < Hq && v < Wq)))
        ra[i] = *reinterpret_cast<const u32x4*>(dy + (((long)a_b[i] * Hq + u) * Wq + v) * O + slab * BK + c8);
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int n = n0 + ((tid + i * 256) >> 3);               // < I: I % BN == 0
      rw[i] = *reinterpret_cast<const u32x4*>(wt + ((long)n * 9 + a9) * O + slab * BK + c8);
    }
  };
  auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid + i * 256) >> 3;
      *reinterpret_cast<u32x4*>(sa + row * 128 + (((tid & 7) ^ (row & 7)) << 4)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int row = (tid + i * 256) >> 3;
      *reinterpret_cast<u32x4*>(sw + row * 128 + (((tid & 7) ^ (row & 7)) << 4)) = rw[i];
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int rd_x = (fq ^ (fr & 7)) << 4;
  const int a_rd = (wm * 32 + fr) * 128 + rd_x;
  const int w_rd = (wn * (BN / 2) + fr) * 128 + rd_x;

  load_tile(0);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();                      // the previous tile's fragments are in registers everywhere
    store_tile();
    __syncthreads();
    if (kt + 1 < nkt) load_tile(kt + 1);  // in flight during the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 xf[MI], wf[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(sa + ((a_rd ^ (ks << 6)) + i * 2048));
#pragma unroll
      for (int j = 0; j < NI; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sw + ((w_rd ^ (ks << 6)) + j * 2048));
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = MFMA_16x16x32_ST(wf[j], xf[i], acc[i][j], 0, 0, 0);
    }
  }

  // lane (fr, fq) of sub-tile (i, j): pixel row wm*32 + i*16 + fr, channels wn*BN/2 + j*16 + fq*4 .. +3
  const int Hin = 2 * Hq, Win = 2 * Wq;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const long m = m0 + wm * 32 + i * 16 + fr;
    if (m >= Mq) continue;
    const int v = (int)(m % Wq);
    const int u = (int)((m / Wq) % Hq);
    const long b = m / ((long)Wq * Hq);
    bf16_t* row = dx + ((b * Hin + 2 * u + pi) * Win + 2 * v + pj) * I + n0 + wn * (BN / 2) + fq * 4;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      uint2 o;
      o.x = pack_bf16x2(acc[i][j][0], acc[i][j][1]);
      o.y = pack_bf16x2(acc[i][j][2], acc[i][j][3]);
      *reinterpret_cast<uint2*>(row + j * 16) = o;
    }
  }
}

// conv3x3 OIHW fp32 -> bf16 [I][9][O], taps in place (tap = a * 3 + b of the forward filter)
__global__ __launch_bounds__(256) void pack_conv3x3_s2_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int O, int I) {
  const long total = (long)I * 9 * O;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int o = (int)(idx % O);
    const long t = idx / O;
    const int tap = (int)(t % 9);
    const int i = (int)(t / 9);
    out[idx] = f32_to_bf16(w[((long)o * I + i) * 9 + tap]);
  }
}

// dst [M][c] (+)= src [M][ld] columns [off, off + c), 8 channels per thread
__global__ __launch_bounds__(256) void slice_add_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, long total_v, int ld,
                                                        int off, int c, int accumulate) {
  const int CV = c / 8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_v; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const long m = i / CV;
    const uint4 s = *reinterpret_cast<const uint4*>(src + m * ld + off + cv * 8);
    uint4* d = reinterpret_cast<uint4*>(dst + i * 8);
    if (accumulate) {
      float a[8], f[8];
      unpack8(*d, a);
      unpack8(s, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += f[j];
      *d = pack8(a);
    } else {
      *d = s;
    }
  }
}

}  // namespace

namespace {
template <bool PAD1>
int s2_dgrad_launch(const bf16_t* dy, const bf16_t* wt, bf16_t* dx, int B, int Hin, int Win, int O, int I, hipStream_t st) {
  ARG_CHECK(B >= 1 && Hin >= 2 && Win >= 2 && Hin % 2 == 0 && Win % 2 == 0, "conv3x3_s2_dgrad: even input height and width");
  ARG_CHECK(O % 64 == 0 && I % 64 == 0, "conv3x3_s2_dgrad: channel counts must be multiples of 64");
  const int Hq = Hin / 2, Wq = Win / 2;
  const long Mq = (long)B * Hq * Wq;
  ARG_CHECK(Mq * 4 * (I > O ? I : O) < (1L << 40) && (Mq + 63) / 64 < (1L << 31), "conv3x3_s2_dgrad: tensor too large");
  // the 128-channel tile re-uses an activation fragment twice as often; the narrow one keeps small layers spread over the CUs
  if (I % 128 == 0 && Mq >= 4096) {
    hipLaunchKernelGGL((conv3x3_s2_dgrad_kernel<128, PAD1>), dim3((unsigned)((Mq + 63) / 64), I / 128, 4), dim3(256), 0, st, dy, wt, dx, B, Hq,
                       Wq, O, I);
  } else {
    hipLaunchKernelGGL((conv3x3_s2_dgrad_kernel<64, PAD1>), dim3((unsigned)((Mq + 63) / 64), I / 64, 4), dim3(256), 0, st, dy, wt, dx, B, Hq,
                       Wq, O, I);
  }
  LAUNCH_CHECK();
  return HEDIT_OK;
}
}  // namespace

int conv3x3_s2_dgrad_launch(const bf16_t* dy, const bf16_t* wt, bf16_t* dx, int B, int Hin, int Win, int O, int I, hipStream_t st) {
  return s2_dgrad_launch<false>(dy, wt, dx, B, Hin, Win, O, I, st);
}
int conv3x3_s2_dgrad_pad1_launch(const bf16_t* dy, const bf16_t* wt, bf16_t* dx, int B, int Hin, int Win, int O, int I, hipStream_t st) {
  return s2_dgrad_launch<true>(dy, wt, dx, B, Hin, Win, O, I, st);
}

int pack_conv3x3_s2_dgrad_launch(const float* w_oihw, bf16_t* out, int O, int I, hipStream_t st) {
  hipLaunchKernelGGL(pack_conv3x3_s2_dgrad_kernel, dim3(ew_grid((long)O * I * 9)), dim3(256), 0, st, w_oihw, out, O, I);
  LAUNCH_CHECK();
  return HEDIT_OK;
}

int slice_add_launch(const bf16_t* src, int ld, int off, int c, bf16_t* dst, long rows, int accumulate, hipStream_t st) {
  ARG_CHECK(c >= 8 && c % 8 == 0 && off % 8 == 0 && ld % 8 == 0 && off >= 0 && off + c <= ld, "slice_add: c, off, ld multiples of 8, off + c <= ld");
  const long total_v = rows * (c / 8);
  hipLaunchKernelGGL(slice_add_kernel, dim3(ew_grid(total_v)), dim3(256), 0, st, src, dst, total_v, ld, off, c, accumulate);
  LAUNCH_CHECK();
  return HEDIT_OK;
}
