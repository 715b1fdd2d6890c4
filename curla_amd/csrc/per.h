// Proportional prioritized replay (Schaul et al. 2016) on the HBM-resident ring: ReplayBuffer(prioritized=True).
// Included by heads.hip inside its anonymous namespace, behind reduce.h (wave_sum / block_sum_256).
//
// Storage: s float [capacity], the stored value p_i^alpha of every ring row (0: never written, never drawn) |
// sums double [ceil(capacity / kPerChunk)], sums[c] = the sum of chunk c's current values in the fixed order of
// per_chunk_sum | vmax float [1], the largest value ever given (new transitions get it).
//
// Every kernel here keeps a row index below `capacity` by construction: rows handed in are taken modulo nothing and
// must be in range (as for the gathers), rows drawn are picked among the rows whose value is > 0.
#pragma once

constexpr int kPerChunk = CURLA_PER_CHUNK;  // rows per chunk sum (curla_hip.h; ops.PER_CHUNK)
static_assert(kPerChunk == 256, "per_chunk_sum and per_sample_kernel are written for 256 rows: 4 per lane, 1 per thread");

__device__ __forceinline__ long long per_row(const int64_t* rows, long long first, long long capacity, int i) {
  return rows ? (long long)rows[i] : (first + i) % capacity;
}

// a stored value as the kernels keep it: finite and non-negative with the sign bit clear, so that floats order like
// their bit patterns and every sum stays finite (NaN, -0 and negatives -> +0, +inf -> FLT_MAX)
__device__ __forceinline__ float per_clean(float v) { return v > 0.f ? fminf(v, 3.402823466e+38f) : 0.f; }

// ---- curla_per_set: three stream-ordered phases (a launch each), so that no workgroup sums a chunk before every row
// of the call is written ----
// phase 1 (given values only): the rows of the call forget their old value -- duplicates all store the same 0
__global__ void per_clear_kernel(float* s, const int64_t* rows, long long first, long long capacity, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) s[per_row(rows, first, capacity, i)] = 0.f;
}

// phase 2: given values -- the maximum of a row's candidates (atomicMax on the word: the order of arrival does not
// matter), and the maximum scalar raised; no values -- every row takes the maximum scalar (duplicates store the same)
__global__ void per_write_kernel(float* s, float* vmax, const int64_t* rows, long long first, long long capacity,
                                 const float* values, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long r = per_row(rows, first, capacity, i);
  if (values) {
    const unsigned bits = __float_as_uint(per_clean(values[i]));
    atomicMax(reinterpret_cast<unsigned*>(s + r), bits);
    atomicMax(reinterpret_cast<unsigned*>(vmax), bits);
  } else {
    s[r] = *vmax;
  }
}

// The sum of chunk c in float64, by one wave, in a fixed order: lane l adds rows l, l + 64, l + 128, l + 192 of the
// chunk in this order, then the 64 partial sums go through the xor tree 32, 16, ... 1.  Valid in every lane.
__device__ __forceinline__ double per_chunk_sum(const float* s, long long capacity, long long c, int lane) {
  double a = 0.;
#pragma unroll
  for (int j = 0; j < kPerChunk / 64; ++j) {
    const long long r = c * kPerChunk + lane + 64 * j;
    a += r < capacity ? (double)s[r] : 0.;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
  return a;
}

// phase 3: one wave per row of the call re-sums that row's chunk (a row whose predecessor in the call lies in the same
// chunk leaves it to the predecessor; chunks summed twice get the same bits twice)
__global__ void per_resum_kernel(const float* s, double* sums, const int64_t* rows, long long first, long long capacity,
                                 int n) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const long long c = per_row(rows, first, capacity, i) / kPerChunk;
  if (i > 0 && per_row(rows, first, capacity, i - 1) / kPerChunk == c) return;
  const double t = per_chunk_sum(s, capacity, c, lane);
  if (lane == 0) sums[c] = t;
}

// ---- curla_per_sample: one workgroup of 256 threads per sample ----
// target = u_k * total, row = the smallest i with cumsum(s)[i] > target, found in three levels: 64 segments of chunk
// sums, the chunks of one segment, the rows of one chunk.  WITHIN a level the prefixes compared with the target are one
// sequential float64 sum of non-negative terms (hence non-decreasing, so "the first one above the target" is one
// position).  ACROSS levels the sums are associated differently -- a segment's sum is accumulated from 0 and then added
// to its base while the walk through its chunks accumulates from the base, and a chunk sum is tree-ordered
// (per_chunk_sum) while the walk over its rows is sequential -- so with sums that are not exact a level may round the
// other way than the level above it and its walk may run past its end (as it does when the target is not below the
// total).  The level then takes its LAST entry with a positive value: a row with s == 0 is never drawn.
// Reads nchunks * 8 + kPerChunk * 4 bytes; writes block int64 [k] = row, [B + k] = capacity + row, prob[k] = s / total.
__global__ void per_sample_kernel(const float* s, const double* sums, long long capacity,
                                  unsigned long long* block, int u_word, int prob_word, int B) {
  __shared__ double seg_sum[64];
  __shared__ float val[kPerChunk];
  __shared__ double sh_acc, sh_total, sh_target;
  __shared__ long long sh_chunk;
  __shared__ int sh_first, sh_last;
  const int k = blockIdx.x, t = threadIdx.x;
  const long long nchunks = (capacity + kPerChunk - 1) / kPerChunk;
  const long long seg = (nchunks + 63) / 64;  // chunks per segment
  if (t == 0) sh_first = kPerChunk, sh_last = -1;
  const long long c0 = min(nchunks, t * seg), c1 = min(nchunks, c0 + seg);  // (t < 64: this lane's segment)
  double local = 0.;
  if (t < 64) {
    for (long long c = c0; c < c1; ++c) local += sums[c];
    seg_sum[t] = local;
  }
  __syncthreads();
  if (t < 64) {  // wave 0: the two upper levels
    double base = 0.;  // every lane adds the segments in front of it in the same order: one sequential prefix
    for (int j = 0; j < t; ++j) base += seg_sum[j];
    const double next = base + local;
    const double total = __shfl(next, 63);
    const double target = reinterpret_cast<const double*>(block)[u_word + k] * total;
    const unsigned long long above = __ballot(next > target), mass = __ballot(local > 0.);
    int pick = -1;
    if (above)
      pick = __ffsll((long long)above) - 1;
    else if (mass)
      pick = 63 - __clzll((long long)mass);
    if (pick < 0 && t == 0) sh_chunk = -1, sh_total = 0., sh_target = 0., sh_acc = 0.;
    if (t == pick) {
      double acc = base, last_acc = base;
      long long found = -1, last = -1;
      for (long long c = c0; c < c1; ++c) {
        const double v = sums[c], nx = acc + v;
        if (v > 0.) last = c, last_acc = acc;
        if (nx > target) {
          found = c;
          break;
        }
        acc = nx;
      }
      if (found < 0) found = last, acc = last_acc;
      sh_chunk = found, sh_acc = acc, sh_total = total, sh_target = target;
    }
  }
  __syncthreads();
  const long long c = sh_chunk;
  if (c < 0) {  // nothing stored anywhere: row 0 with probability 0 (the caller refuses to sample an empty buffer)
    if (t == 0) {
      block[k] = 0ull, block[B + k] = (unsigned long long)capacity;
      reinterpret_cast<float*>(block)[prob_word + k] = 0.f;
    }
    return;
  }
  const long long r = c * kPerChunk + t;
  const float mine = r < capacity ? s[r] : 0.f;
  val[t] = mine;
  __syncthreads();
  double p = sh_acc;  // the sequential prefix up to and including this thread's row
  for (int j = 0; j <= t; ++j) p += (double)val[j];
  if (p > sh_target) atomicMin(&sh_first, t);
  if (mine > 0.f) atomicMax(&sh_last, t);
  __syncthreads();
  if (t == 0) {
    const int j = sh_first < kPerChunk ? sh_first : sh_last;  // (sh_last >= 0: the chunk's sum is positive)
    const long long row = c * kPerChunk + (j < 0 ? 0 : j);
    block[k] = (unsigned long long)row, block[B + k] = (unsigned long long)(capacity + row);
    reinterpret_cast<float*>(block)[prob_word + k] = (float)((double)val[j < 0 ? 0 : j] / sh_total);
  }
}

// ---- curla_per_td: importance weights, the weighted loss and its gradient, the new stored values (one workgroup) ----
//   w_k = (min_j P_j / P_k)^beta;  dq[k], dq[sTwin + k] *= w_k  (in place: dq is the unweighted loss's gradient);
//   loss = (1/B) sum_k w_k [(q1_k - t_k)^2 + (q2_k - t_k)^2];  value_k = (0.5 (|q1_k - t_k| + |q2_k - t_k|) + eps)^alpha
__global__ void per_td_kernel(const float* q, long long sTwin, const float* target_q, const float* prob, float beta,
                              float eps, float alpha, int B, float* dq, float* loss, float* w, float* value) {
  __shared__ float sm[4];
  float lo = INFINITY;
  for (int b = threadIdx.x; b < B; b += 256) lo = fminf(lo, prob[b]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = lo;
  __syncthreads();
  lo = fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3]));
  float a1 = 0.f, a2 = 0.f;
  const float inv = 1.f / B;
  for (int b = threadIdx.x; b < B; b += 256) {
    // (prob == 0: a sample of a draw that found no mass anywhere -- it gets no weight instead of 0/0)
    const float wk = prob[b] > 0.f ? powf(lo / prob[b], beta) : 0.f;
    const float d1 = q[b] - target_q[b], d2 = q[sTwin + b] - target_q[b];
    w[b] = wk;
    a1 += wk * d1 * d1;
    a2 += wk * d2 * d2;
    dq[b] *= wk;
    dq[sTwin + b] *= wk;
    value[b] = powf(0.5f * (fabsf(d1) + fabsf(d2)) + eps, alpha);
  }
  const float s1 = block_sum_256(a1, sm);
  const float s2 = block_sum_256(a2, sm);
  if (threadIdx.x == 0) loss[0] = s1 * inv + s2 * inv;
}
