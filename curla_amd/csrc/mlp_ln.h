// LayerNorm behind the hidden layers of the twin Q functions (CurlSacAgent(critic_layer_norm=True): each trunk is
// Linear - LayerNorm - ReLU - Linear - LayerNorm - ReLU - Linear, curl_sac.py:129-139 with the normalisation of DroQ /
// RLPD in front of each ReLU).  The forward works in place on the activation the GEMM has just written
// (mlp_ln_relu_fwd_kernel), the backward in place on the ReLU-masked hidden gradient (mlp_ln_bwd_kernel), and the
// parameter gradients are finished by a small launch of their own (mlp_ln_param_grad_kernel).  One wave per row, a lane
// holds features lane, lane + 64, ...: NF as in layernorm.h, i.e. H <= 1024.  Unlike layernorm.h's kernels these address
// twins (blockIdx.y % nb, `s*` strides) and groups of twins (blockIdx.y / nb, `s*2` strides) like the GEMMs in front of
// them.  Included by heads.hip inside its anonymous namespace, behind reduce.h (wave_sum).
#pragma once

// h[o][z][row][:] <- relu(xhat * gamma[o][z] + beta[o][z]), xhat = (h - mean) * rstd over the row's H features.
// xhat / rstd (both or neither): saved for the groups o >= save_first, dense: xhat[o - save_first][z][B][H],
// rstd[o - save_first][z][B].  Rows past B do nothing.
template <int NF>
__global__ void mlp_ln_relu_fwd_kernel(float* h, long long sH, long long sH2, const float* gamma, const float* beta,
                                       long long sP, long long sP2, float* xhat, float* rstd, int save_first, int B,
                                       int H, int nb, float eps) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const int z = blockIdx.y % nb, o = blockIdx.y / nb;
  float* hr = h + z * sH + o * sH2 + (size_t)row * H;
  const float* g = gamma + z * sP + o * sP2;
  const float* bt = beta + z * sP + o * sP2;
  float v[NF];
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    v[j] = f < H ? hr[f] : 0.f;
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

// dh[z][row][:] <- rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dh * gamma[z]: the gradient of the pre-LayerNorm
// activation from the (ReLU-masked) gradient of the LayerNorm's output, in place.  xhat [nb][B][H], rstd [nb][B] dense.
// `partial` (NULL: no parameter gradients, rows past B return at once) [nb][gridDim.x][3][H]: the workgroup's four rows'
// contributions to dgamma (dh xhat), dbeta (dh) and the bias gradient of the Linear in front (the new dh), added in
// wave (= row) order.
template <int NF>
__global__ void mlp_ln_bwd_kernel(float* dh, long long sDh, const float* xhat, const float* rstd, const float* gamma,
                                  long long sP, int B, int H, float* partial) {
  __shared__ float part[4][3][NF * 64];
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  const int lane = threadIdx.x & 63;
  const int z = blockIdx.y;
  const bool live = row < B;
  if (!live && !partial) return;
  float* dr = dh + z * sDh + (size_t)row * H;                       // (dereferenced for live rows only)
  const float* xr = xhat + ((size_t)z * B + row) * H;
  const float* gm = gamma + z * sP;
  float g[NF], xh[NF], d[NF], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    g[j] = 0.f, xh[j] = 0.f, d[j] = 0.f;
    if (live && f < H) {
      d[j] = dr[f];
      g[j] = d[j] * gm[f];
      xh[j] = xr[f];
    }
    s1 += g[j];
    s2 += g[j] * xh[j];
  }
  const float m1 = wave_sum(s1) / H;
  const float m2 = wave_sum(s2) / H;
  const float rs = live ? rstd[(size_t)z * B + row] : 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    const float o = rs * (g[j] - m1 - xh[j] * m2);
    if (live && f < H) dr[f] = o;
    if (partial) part[wave][0][f] = d[j] * xh[j], part[wave][1][f] = d[j], part[wave][2][f] = live && f < H ? o : 0.f;
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

// dgamma[z][f], dbeta[z][f], dbias[z][f] = the sums over the nparts partials of mlp_ln_bwd_kernel, in part order (eight
// loads in flight, added in that order): one thread per (quantity, feature), blockIdx.y = twin.
__global__ void mlp_ln_param_grad_kernel(const float* partial, int nparts, int H, float* dgamma, float* dbeta,
                                         float* dbias, long long sG) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * H) return;
  const int z = blockIdx.y;
  const float* p = partial + (size_t)z * nparts * 3 * H + i;
  const size_t step = (size_t)3 * H;
  float a = 0.f;
  int s = 0;
  for (; s + 8 <= nparts; s += 8) {
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = p[(s + k) * step];
#pragma unroll
    for (int k = 0; k < 8; ++k) a += t[k];
  }
  for (; s < nparts; ++s) a += p[s * step];
  const int q = i / H, f = i - q * H;
  float* out = q == 0 ? dgamma : q == 1 ? dbeta : dbias;
  out[z * sG + f] = a;
}
