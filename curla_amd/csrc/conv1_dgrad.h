// Gradient of the first (stride-2) convolution with respect to its float observation: the saliency / input-gradient
// path of the differentiable encoder (curla_amd/autograd.py; not part of update(), whose observations are uint8 and
// never receive a gradient).  Included by conv.hip.
//
//   dobs[n][c][y][x] = scale * sum_{o, ky, kx : y = 2 oy + ky, x = 2 ox + kx} g[n][oy][ox][o] * w[o][c][ky][kx]
//
// g is conv1's pre-activation output gradient (NHWC [B][Ho][Wo][F], already ReLU-masked by the layer above), w the
// layer's OIHW weight in place in the parameter buffer, dobs float NCHW [B][C][H][W] (the observation's own shape).
//
// Form: one thread per 2 x 2 block of input pixels (y = 2i + dy, x = 2j + dx).  Such a block is reached from exactly
// four output positions, (i, j), (i, j-1), (i-1, j), (i-1, j-1), through 4 + 2 + 2 + 1 = 9 (position, tap) pairs --
// each of the 9 taps once -- so every thread runs the same 9 F C multiply-adds with no parity divergence (a position
// outside the output reads a valid row and is multiplied by 0), and every weight a lane reads is the same for the
// whole wave: a scalar load and a scalar operand of the VALU FMA, never an LDS or vector load.  The filters are walked
// in trips of FC (4 for C <= 6, 2 above): a trip's 9 FC C weights must fit the scalar registers -- one trip over all
// 32 filters spilled ~2000 of them.  The g values are the trip's FC contiguous floats of each position's NHWC row;
// neighbouring threads share three of their four positions, which the caches absorb, so HBM sees g about once.
// Outputs: 4 C floats per thread, stored as rows of the NCHW tensor (adjacent threads, adjacent x).  Pixels no output
// touches (the last row / column of an even size) come out as zero.  Any filter count that is a multiple of 4.
#pragma once

namespace {

template <int C, int FC>
__global__ __launch_bounds__(256) void conv1_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                          float* __restrict__ dobs, int B, int H, int W, int Ho, int Wo,
                                                          int F, int H2, int W2, float scale) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)B * H2 * W2) return;
  const int j = (int)(t % W2);
  const long long r = t / W2;
  const int i = (int)(r % H2), n = (int)(r / H2);
  // the four output positions' g rows; a position outside the output reads a valid address and is multiplied by 0
  const float* gp[4];
  float keep[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int oy = i - (q >> 1), ox = j - (q & 1);
    const bool ok = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
    gp[q] = g + (((size_t)n * Ho + (ok ? oy : 0)) * Wo + (ok ? ox : 0)) * F;
    keep[q] = ok ? 1.f : 0.f;
  }
  float acc[2][2][C];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[dy][dx][c] = 0.f;
  // FC filters per trip (a float4 of each position's row per 4 filters); the trip's 9 FC C weights are uniform across
  // the wave -- scalar loads, few enough per trip to stay in scalar registers
#pragma unroll 1
  for (int f0 = 0; f0 < F; f0 += FC) {
    float gv[4][FC];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int v = 0; v < FC / 2; ++v) {
        const f32x2 x2 = reinterpret_cast<const f32x2*>(gp[q] + f0)[v];
        gv[q][2 * v] = x2[0] * keep[q], gv[q][2 * v + 1] = x2[1] * keep[q];
      }
#pragma unroll
    for (int o = 0; o < FC; ++o) {
      const float* wo = w + (size_t)(f0 + o) * C * 9;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* k = wo + c * 9;  // k[ky * 3 + kx]
        // q = 0 (oy = i, ox = j): taps (dy, dx); q = 1 (ox = j - 1): (dy, 2) -> dx = 0; q = 2 (oy = i - 1): (2, dx) -> dy = 0;
        // q = 3: (2, 2) -> (0, 0)
        acc[0][0][c] = fmaf(gv[0][o], k[0], acc[0][0][c]);
        acc[0][1][c] = fmaf(gv[0][o], k[1], acc[0][1][c]);
        acc[1][0][c] = fmaf(gv[0][o], k[3], acc[1][0][c]);
        acc[1][1][c] = fmaf(gv[0][o], k[4], acc[1][1][c]);
        acc[0][0][c] = fmaf(gv[1][o], k[2], acc[0][0][c]);
        acc[1][0][c] = fmaf(gv[1][o], k[5], acc[1][0][c]);
        acc[0][0][c] = fmaf(gv[2][o], k[6], acc[0][0][c]);
        acc[0][1][c] = fmaf(gv[2][o], k[7], acc[0][1][c]);
        acc[0][0][c] = fmaf(gv[3][o], k[8], acc[0][0][c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int y = 2 * i + dy;
      if (y >= H) continue;
      float* row = dobs + (((size_t)n * C + c) * H + y) * W;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int x = 2 * j + dx;
        if (x < W) row[x] = scale * acc[dy][dx][c];
      }
    }
}

template <int C>
int conv1_dgrad_launch(const float* g, const float* w, float* dobs, int B, int H, int W, int F, float scale,
                       hipStream_t st) {
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1, H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  const long long n = (long long)B * H2 * W2;
  const dim3 grid((unsigned)((n + 255) / 256));
  // (filters per trip: 9 FC C scalar weights must fit the scalar register file)
  hipLaunchKernelGGL((conv1_dgrad_kernel<C, (C <= 6 ? 4 : 2)>), grid, dim3(256), 0, st, g, w, dobs, B, H, W, Ho, Wo, F, H2,
                     W2, scale);
  return curla_launch_status();
}

}  // namespace

extern "C" int curla_conv1_dgrad(const float* g, const float* w, float* dobs, int B, int C, int H, int W, int channels,
                                 float scale, void* stream) {
  CURLA_REQUIRE(g && w && dobs && B > 0 && H >= 3 && W >= 3 && aligned16(g));
  if (!gen::channels_ok(channels)) return CURLA_ERR_UNSUPPORTED;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  switch (C) {
    case 3: return conv1_dgrad_launch<3>(g, w, dobs, B, H, W, channels, scale, st);
    case 6: return conv1_dgrad_launch<6>(g, w, dobs, B, H, W, channels, scale, st);
    case 9: return conv1_dgrad_launch<9>(g, w, dobs, B, H, W, channels, scale, st);
    case 12: return conv1_dgrad_launch<12>(g, w, dobs, B, H, W, channels, scale, st);
    default: return CURLA_ERR_UNSUPPORTED;  // 3 x frame_stack of 1..4, as conv1_fwd
  }
}
