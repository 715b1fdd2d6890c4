// The deterministic second pass of every weight gradient: dW = the sum of the per-workgroup slabs the weight-gradient
// kernels leave (conv_rw_wgrad.h, conv_rw_wgrad2.h, conv1_rw.h, conv1_wgrad.h, conv_generic.h).  Included by conv.hip
// inside its anonymous namespace.
#pragma once

// second pass: dW = sum over workgroup slabs.  32 elements x 32 slab-groups per
// block; each group adds its slabs in slab order, the 32 group sums are added in
// group order (fixed order => bitwise reproducible).
__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* partial, int nslabs, int nw, int nb, float* dw,
                                                            float* db) {
  __shared__ float sm[32][33];
  const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + c;
  const int n = nw + nb;  // (nb bias sums behind the nw weight sums of a slab: 32, or the filter count of the generic path)
  float s = 0.f;
  if (i < n) {
    int k = part;
    for (; k + 7 * 32 < nslabs; k += 8 * 32) {  // 8 slabs in flight, added in slab order
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(size_t)(k + 32 * u) * n + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; k < nslabs; k += 32) s += partial[(size_t)k * n + i];
  }
  sm[part][c] = s;
  __syncthreads();
  if (part == 0 && i < n) {
    float t = sm[0][c];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += sm[k][c];
    if (i < nw)
      dw[i] = t;
    else
      db[i - nw] = t;
  }
}

// the same for up to kMaxReduceJobs weight gradients in ONE launch: the backward pass of an encoder leaves one slab set
// per conv layer and nothing reads dW before the pass is over, so the per-layer reductions need not be launches of
// their own (each would cost the 4.8 us launch floor for ~1 us of work)
constexpr int kMaxReduceJobs = 8;
struct ReduceJobs {
  const float* partial[kMaxReduceJobs];
  float* dw[kMaxReduceJobs];
  float* db[kMaxReduceJobs];
  int nslabs[kMaxReduceJobs], nw[kMaxReduceJobs], nb[kMaxReduceJobs], first_block[kMaxReduceJobs + 1];
  int njobs;
};

__global__ __launch_bounds__(1024) void wgrad_reduce_multi_kernel(ReduceJobs J) {
  __shared__ float sm[32][33];
  int j = 0;
  while (j + 1 < J.njobs && (int)blockIdx.x >= J.first_block[j + 1]) ++j;
  const float* partial = J.partial[j];
  const int nslabs = J.nslabs[j], nw = J.nw[j];
  const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int i = ((int)blockIdx.x - J.first_block[j]) * 32 + c;
  const int n = nw + J.nb[j];
  float s = 0.f;
  if (i < n) {
    int k = part;
    for (; k + 7 * 32 < nslabs; k += 8 * 32) {  // 8 slabs in flight, added in slab order
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(size_t)(k + 32 * u) * n + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; k < nslabs; k += 32) s += partial[(size_t)k * n + i];
  }
  sm[part][c] = s;
  __syncthreads();
  if (part == 0 && i < n) {
    float t = sm[0][c];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += sm[k][c];
    if (i < nw)
      J.dw[j][i] = t;
    else
      J.db[j][i - nw] = t;
  }
}
