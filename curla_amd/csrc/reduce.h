// Fixed-order reductions: the wave- and block-wide sums the other kernels of heads.hip are built on, and the column-sum,
// mean and gradient square-sum kernels (bias gradients, logged losses, the norm a clipped Adam step needs).  Included by
// heads.hip inside its anonymous namespace, first: every header behind it may use wave_sum / wave_max / block_sum_256.
#pragma once

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// block-wide fixed-order sum of one value per thread (256 threads); result valid in every thread
__device__ __forceinline__ float block_sum_256(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// the same in double (the gradient norm: grad_sqsum_kernel's partials and their sum inside the Adam kernels)
__device__ __forceinline__ double block_sum_256(double v, double* sm) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// partials[blockIdx.x] = sum of g[i]^2 over the block's grid-stride share of one flat run, in double: the product of two
// floats is exact in double and a sum of n <= 2^22 of them is good to n 2^-53 relative, far inside a float32 ulp of the
// norm.  A thread adds its elements in index order, the block sums its threads in a fixed order, no atomics: the
// partials depend only on the gradient's bytes, n, the grid and `vec` (16-byte loads when the run is 16-byte aligned --
// adam_step_kernel's rule).  The grid is the number of partials (<= 256: one Adam block sums them with one load per
// thread, optim.h clip_coef).
__global__ void __launch_bounds__(256) grad_sqsum_kernel(const float* __restrict__ g, size_t n, int vec,
                                                         double* __restrict__ partials) {
  __shared__ double sm[4];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  size_t done = 0;
  if (vec) {
    const size_t n4 = n >> 2;
#pragma unroll 4
    for (size_t i = tid; i < n4; i += stride) {
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)gg[e] * (double)gg[e];
    }
    done = n4 << 2;
  }
#pragma unroll 4
  for (size_t i = done + tid; i < n; i += stride) acc += (double)g[i] * (double)g[i];
  const double s = block_sum_256(acc, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[z][n] = sum_m X[z][m][n]  (bias gradients); 32 columns x 32 row-parts per block, fixed order
__global__ __launch_bounds__(1024) void colsum_kernel(const float* X, int M, int N, int ldx, long long sX, float* out,
                                                      long long sOut) {
  __shared__ float sm[32][33];
  const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + c;
  const float* x = X + blockIdx.y * sX;
  float a = 0.f;
  if (n < N) {
    int m = part;
    for (; m + 7 * 32 < M; m += 8 * 32) {  // 8 rows in flight, accumulated in row order
      float t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] = x[(size_t)(m + 32 * k) * ldx + n];
#pragma unroll
      for (int k = 0; k < 8; ++k) a += t[k];
    }
    for (; m < M; m += 32) a += x[(size_t)m * ldx + n];
  }
  sm[part][c] = a;
  __syncthreads();
  if (part == 0 && n < N) {
    float t = sm[0][c];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += sm[k][c];
    out[blockIdx.y * sOut + n] = t;
  }
}

// three column sums in one launch (the three bias gradients of an MLP backward): blockIdx.z picks the matrix
struct Colsum3Args {
  const float* X[3];
  float* out[3];
  int N[3];
  long long sX[3];
};
__global__ __launch_bounds__(1024) void colsum3_kernel(Colsum3Args a, int M, long long sOut) {
  __shared__ float sm[32][33];
  const int z = blockIdx.z;
  const int N = a.N[z];
  const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + c;
  if (blockIdx.x * 32 >= N) return;  // block-uniform
  const float* x = a.X[z] + blockIdx.y * a.sX[z];
  float acc = 0.f;
  if (n < N) {
    int m = part;
    for (; m + 7 * 32 < M; m += 8 * 32) {  // 8 rows in flight, accumulated in row order
      float t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] = x[(size_t)(m + 32 * k) * N + n];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += t[k];
    }
    for (; m < M; m += 32) acc += x[(size_t)m * N + n];
  }
  sm[part][c] = acc;
  __syncthreads();
  if (part == 0 && n < N) {
    float t = sm[0][c];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += sm[k][c];
    a.out[z][blockIdx.y * sOut + n] = t;
  }
}

__global__ void mean_kernel(const float* x, int n, float* out) {
  __shared__ float sm[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += x[i];
  const float s = block_sum_256(a, sm);
  if (threadIdx.x == 0) out[0] = s / n;
}
