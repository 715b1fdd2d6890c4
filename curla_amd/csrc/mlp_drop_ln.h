// DroQ's dropout in front of the critics' LayerNorms (CurlSacAgent(critic_layer_norm=True, critic_dropout=p)): each
// hidden layer is Linear - Dropout(p) - LayerNorm - ReLU, y = relu(LN(m * h * s)) with the keep mask m and
// s = 1 / (1 - p).  The kernels are mlp_ln.h's with the mask in front: the same one-wave-per-row, NF-register form, in
// place, the same twin and group strides, save_first and partial sums; mlp_ln.h's own kernels stay as they are and
// mlp_ln_param_grad_kernel finishes the parameter gradients of both.  The mask is never stored: forward and backward
// compute it from (seed, counter, tag) and the element's position (common.h: dropout_words), one Philox
// evaluation per four of a lane's registers.  Included by heads.hip inside its anonymous namespace, behind mlp_ln.h.
#pragma once

struct DropArgs {
  float p, scale;  // drop probability in [0, 1), 1.0f / (1.0f - p)
  unsigned long long seed, counter;
  // rng_dev != nullptr: (seed, counter) are read from device memory when the kernel RUNS (rng_dev[0], rng_dev[1]), as
  // the policy head reads its stream position (mlp_out.h) -- a captured graph is replayed with new masks
  const unsigned long long* rng_dev;
  int tag;  // 1..255; group o of a launch over groups of twins draws under tag + 2 o
};

// keep[j] <=> feature lane + 64 j of (twin z, row) survives; rows are numbered within the launch's group
template <int NF>
__device__ __forceinline__ void dropout_mask(const DropArgs& dr, int tag, int z, int row, int B, int H, int lane,
                                             bool (&keep)[NF]) {
  const unsigned long long seed = dr.rng_dev ? dr.rng_dev[0] : dr.seed;
  const unsigned long long counter = dr.rng_dev ? dr.rng_dev[1] : dr.counter;
  const unsigned long long rows_before = (unsigned long long)z * B + row;
  const int chunks = (H + 255) >> 8;
#pragma unroll
  for (int q = 0; q < (NF + 3) / 4; ++q) {
    unsigned w[4];
    dropout_words(seed, counter, (unsigned)tag, rows_before, chunks, q, lane, w);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * q + k < NF) keep[4 * q + k] = dropout_keep(w[k], dr.p);
  }
}

// mlp_ln_relu_fwd_kernel on m * h * s: the statistics, xhat and rstd are those of the dropped activation.
template <int NF>
__global__ void mlp_drop_ln_relu_fwd_kernel(float* h, long long sH, long long sH2, const float* gamma, const float* beta,
                                            long long sP, long long sP2, float* xhat, float* rstd, int save_first, int B,
                                            int H, int nb, float eps, DropArgs dr) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const int z = blockIdx.y % nb, o = blockIdx.y / nb;
  float* hr = h + z * sH + o * sH2 + (size_t)row * H;
  const float* g = gamma + z * sP + o * sP2;
  const float* bt = beta + z * sP + o * sP2;
  float v[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {  // (the row's loads do not wait for the mask: the Philox rounds run under them)
    const int f = lane + 64 * j;
    v[j] = f < H ? hr[f] : 0.f;
  }
  bool keep[NF];
  dropout_mask<NF>(dr, dr.tag + 2 * o, z, row, B, H, lane, keep);
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    v[j] = keep[j] ? v[j] * dr.scale : 0.f;
    tot += v[j];
  }
  const float mean = wave_sum(tot) / H;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    v[j] = lane + 64 * j < H ? v[j] - mean : 0.f;
    sq += v[j] * v[j];
  }
  const float rs = 1.0f / sqrtf(wave_sum(sq) / H + eps);
  const bool save = xhat && o >= save_first;
  const size_t srow = ((size_t)(o - save_first) * nb + z) * B + row;  // (only used when save)
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    if (f < H) {
      const float xh = v[j] * rs;
      hr[f] = fmaxf(xh * g[f] + bt[f], 0.f);
      if (save) xhat[srow * H + f] = xh;
    }
  }
  if (save && lane == 0) rstd[srow] = rs;
}

// mlp_ln_bwd_kernel with the mask regenerated (tag: the forward's for this group) and m * s applied to its result
// BEFORE that goes into the bias partials: dh leaves as the gradient of the Linear's output, `partial`'s third plane
// sums that; dgamma / dbeta as without dropout (xhat is that of the dropped activation).
template <int NF>
__global__ void mlp_drop_ln_bwd_kernel(float* dh, long long sDh, const float* xhat, const float* rstd, const float* gamma,
                                       long long sP, int B, int H, float* partial, DropArgs dr) {
  __shared__ float part[4][3][NF * 64];
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  const int lane = threadIdx.x & 63;
  const int z = blockIdx.y;
  const bool live = row < B;
  if (!live && !partial) return;
  float* drow = dh + z * sDh + (size_t)row * H;                     // (dereferenced for live rows only)
  const float* xr = xhat + ((size_t)z * B + row) * H;
  const float* gm = gamma + z * sP;
  float g[NF], xh[NF], d[NF], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    g[j] = 0.f, xh[j] = 0.f, d[j] = 0.f;
    if (live && f < H) {
      d[j] = drow[f];
      g[j] = d[j] * gm[f];
      xh[j] = xr[f];
    }
    s1 += g[j];
    s2 += g[j] * xh[j];
  }
  bool keep[NF];
  dropout_mask<NF>(dr, dr.tag, z, row, B, H, lane, keep);            // (under the loads; a dead row's mask selects zeros)
  const float m1 = wave_sum(s1) / H;
  const float m2 = wave_sum(s2) / H;
  const float rs = live ? rstd[(size_t)z * B + row] : 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    const float o = live && f < H && keep[j] ? rs * (g[j] - m1 - xh[j] * m2) * dr.scale : 0.f;
    if (live && f < H) drow[f] = o;
    if (partial) part[wave][0][f] = d[j] * xh[j], part[wave][1][f] = d[j], part[wave][2][f] = o;
  }
  if (partial) {
    __syncthreads();
    float* out = partial + ((size_t)z * gridDim.x + blockIdx.x) * 3 * H;
    for (int i = threadIdx.x; i < 3 * H; i += blockDim.x) {
      const int q = i / H, f = i - q * H;
      out[i] = ((part[0][q][f] + part[1][q][f]) + part[2][q][f]) + part[3][q][f];
    }
  }
}
