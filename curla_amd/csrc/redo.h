// Dormant-neuron scores and ReDo recycling (Sokar et al., ICML 2023) for the hidden layers of the actor
// trunk and the twin Q functions: the column sums of |h| over a minibatch (dormant_colsum_kernel), the scores, masks and
// counts per layer (dormant_mask_kernel) and the recycling of the masked units' parameters and Adam moments in the flat
// buffers (redo_recycle_kernel).  Plain loads and stores, no atomics, every sum in a fixed order: a rerun writes the same
// bits.  Included by heads.hip inside its anonymous namespace.
#pragma once

typedef int redo_i32x4 __attribute__((ext_vector_type(4)));

// sums[n][j] = sum over b of |h[n][b][j]| in float32, b in index order.  One thread per column (coalesced along H),
// blockIdx.y = the network; the loads of a column are independent of the running sum, so the compiler keeps several in
// flight while the additions stay in order.
__global__ void __launch_bounds__(64) dormant_colsum_kernel(const float* __restrict__ h, long long sH, int B, int H,
                                                            float* __restrict__ sums, long long sS) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= H) return;
  const float* col = h + (size_t)blockIdx.y * sH + j;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < B; ++b) s += fabsf(col[(size_t)b * H]);
  sums[(size_t)blockIdx.y * sS + j] = s;
}

// One workgroup per layer l (row l of sums [L][H]):
//   total = sum_j (double) sums[j] -- thread t adds its columns t, t + 256, ... in index order, thread 0 then adds the
//           256 partial sums in index order
//   mean = total / H;  score[j] = (float)((double) sums[j] / mean);  mask[j] = mean == 0 or score[j] <= tau (float32
//   compare: false for a NaN);  count = the units masked;  fraction = (float)((double) count / H).
__global__ void __launch_bounds__(256) dormant_mask_kernel(const float* __restrict__ sums, int H, float tau,
                                                           float* __restrict__ score, int* __restrict__ mask,
                                                           int* __restrict__ count, float* __restrict__ fraction) {
  __shared__ double part[256];
  __shared__ int cnt[256];
  __shared__ double mean_s;
  const int t = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * H;
  double p = 0.;
  for (int j = t; j < H; j += 256) p += (double)sums[row + j];
  part[t] = p;
  __syncthreads();
  if (t == 0) {
    double total = 0.;
    for (int i = 0; i < 256; ++i) total += part[i];
    mean_s = total / (double)H;
  }
  __syncthreads();
  const double mean = mean_s;
  int c = 0;
  for (int j = t; j < H; j += 256) {
    const float sc = (float)((double)sums[row + j] / mean);
    const int dormant = (mean == 0.) || (sc <= tau);
    score[row + j] = sc;
    mask[row + j] = dormant;
    c += dormant;
  }
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {
    int n = 0;
    for (int i = 0; i < 256; ++i) n += cnt[i];
    count[blockIdx.x] = n;
    fraction[blockIdx.x] = (float)((double)n / (double)H);
  }
}

// The segments of one recycle launch: a [rows][cols] matrix (a vector: cols 1) `offset` floats into the flat block, with
// the mask rows of its output units (row_layer) and of its input units (col_layer), -1 where it has none.
constexpr int kMaxRedoSegs = CURLA_REDO_MAX_SEGS;

struct RedoSeg {
  long long offset;
  int rows, cols, row_layer, col_layer, vec;
};

struct RedoSegs {
  RedoSeg s[kMaxRedoSegs];
};

// element (i, j) of a segment: 0 where its input unit is masked, else the fresh value where its output unit is, else not
// written; the moments 0 wherever the parameter is written
__device__ __forceinline__ void redo_one(float* p, float* m, float* v, const float* f, size_t at, int r, int c) {
  if (!(r | c)) return;
  p[at] = c ? 0.f : f[at];
  m[at] = 0.f;
  v[at] = 0.f;
}

// grid (x, segment, network).  Network n works `stride` floats into the four arrays and takes the mask rows
// row_layer + n * mask_twin and col_layer + n * mask_twin of mask [.][H].  A segment with `vec` (decided per launch and
// per segment on the host: the four arrays and the mask 16-byte aligned, stride, offset and cols multiples of 4) moves
// whole float4s -- four elements of one row -- where the row is masked; a float4 of an unmasked row writes only its
// masked columns, element by element.  param, m and v are never read.
__global__ void __launch_bounds__(256) redo_recycle_kernel(float* __restrict__ param, float* __restrict__ m,
                                                           float* __restrict__ v, const float* __restrict__ fresh,
                                                           long long stride, RedoSegs segs, const int* __restrict__ mask,
                                                           int H, int mask_twin) {
  const RedoSeg sg = segs.s[blockIdx.y];
  const int n = blockIdx.z;
  const size_t base = (size_t)n * stride + sg.offset;
  float *P = param + base, *M = m + base, *V = v + base;
  const float* F = fresh + base;
  const int* rmask = sg.row_layer >= 0 ? mask + (size_t)(sg.row_layer + n * mask_twin) * H : nullptr;
  const int* cmask = sg.col_layer >= 0 ? mask + (size_t)(sg.col_layer + n * mask_twin) * H : nullptr;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t count = (size_t)sg.rows * sg.cols;
  if (sg.vec) {
    const int c4 = sg.cols >> 2;
    for (size_t q = tid; q < (count >> 2); q += step) {
      const int i = (int)(q / c4), j = (int)(q % c4) << 2;
      const int r = rmask ? rmask[i] : 0;
      redo_i32x4 c = {0, 0, 0, 0};
      if (cmask) c = *reinterpret_cast<const redo_i32x4*>(cmask + j);
      if (r) {
        f32x4 f = reinterpret_cast<const f32x4*>(F)[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = c[e] ? 0.f : f[e];
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f32x4*>(P)[q] = f;
        reinterpret_cast<f32x4*>(M)[q] = z;
        reinterpret_cast<f32x4*>(V)[q] = z;
      } else if (c[0] | c[1] | c[2] | c[3]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) redo_one(P, M, V, F, (q << 2) + e, 0, c[e]);
      }
    }
    return;
  }
  for (size_t q = tid; q < count; q += step) {
    const int i = (int)(q / sg.cols), j = (int)(q % sg.cols);
    redo_one(P, M, V, F, q, rmask ? rmask[i] : 0, cmask ? cmask[j] : 0);
  }
}
