// The categorical HL-Gauss critic (Imani & White 2018; Farebrother et al. 2024): each Q function outputs
// M logits over the bins of [v_min, v_max], Q = sum_j softmax(l)_j c_j, and the critic is trained by cross-entropy on a
// Gaussian-smoothed histogram of the scalar TD target.  Included by heads.hip inside its anonymous namespace, behind
// reduce.h (wave_sum / wave_max / block_sum_256) and sac_loss.h (td_target_pinned).
//   w = (v_max - v_min) / M,  e_j = v_min + j w (j = 0 .. M),  c_j = v_min + (j + 1/2) w,  Phi(x) = (1 + erf(x / sqrt 2)) / 2
// One wave per minibatch row, four rows per workgroup; lane l holds the bins l, l + 64, l + 128, l + 192 (M <= 256) in
// registers.  No atomics and fixed orders throughout: a rerun writes the same bits.
#pragma once

constexpr int kHlgMax = 256;            // the most bins: four per lane
constexpr int kHlgSlots = kHlgMax / 64;

// (contraction is off in the pieces a TD target is made of: both instantiations of the critic kernel, and either wave
// of a pair of views, then round every product and sum alike -- td_target_pinned's reason)
__device__ __forceinline__ float hlg_centre(int j, float v_min, float w) {
#pragma clang fp contract(off)
  return v_min + ((float)j + 0.5f) * w;
}

// softmax of one row of M logits: ex[k] = exp(l_j - max) for the lane's bins j = lane + 64 k (0 behind M); returns
// sum_j ex_j, the same in every lane, and leaves the row max in `mx`
__device__ __forceinline__ float hlg_softmax(const float* __restrict__ l, int M, int lane, float (&ex)[kHlgSlots],
                                             float (&lg)[kHlgSlots], float& mx) {
#pragma clang fp contract(off)
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kHlgSlots; ++k) {
    const int j = lane + 64 * k;
    lg[k] = j < M ? l[j] : -INFINITY;
    m = fmaxf(m, lg[k]);
  }
  mx = wave_max(m);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < kHlgSlots; ++k) {
    ex[k] = lane + 64 * k < M ? expf(lg[k] - mx) : 0.f;
    se += ex[k];
  }
  return wave_sum(se);
}

// sum_j ex_j c_j / se: the expectation of the bin centres, the same in every lane
__device__ __forceinline__ float hlg_expect(const float (&ex)[kHlgSlots], float se, int M, int lane, float v_min, float w) {
#pragma clang fp contract(off)
  float sc = 0.f;
#pragma unroll
  for (int k = 0; k < kHlgSlots; ++k) {
    const int j = lane + 64 * k;
    if (j < M) sc += ex[k] * hlg_centre(j, v_min, w);
  }
  return wave_sum(sc) / se;
}

// Q of one row of logits
__device__ __forceinline__ float hlg_row_q(const float* __restrict__ l, int M, int lane, float v_min, float w) {
  float ex[kHlgSlots], lg[kHlgSlots], mx;
  const float se = hlg_softmax(l, M, lane, ex, lg, mx);
  return hlg_expect(ex, se, M, lane, v_min, w);
}

// position b's TD target from the two target networks' logits, by td_target_pinned's arithmetic: whichever wave
// evaluates it gets the same bits
__device__ __forceinline__ float hlg_td_target(const float* __restrict__ tq, long long sT, int b, int M, int lane,
                                               float v_min, float w, float alpha, const float* __restrict__ log_pi,
                                               const float* __restrict__ reward, const float* __restrict__ not_done,
                                               float discount) {
  const float q0 = hlg_row_q(tq + (size_t)b * M, M, lane, v_min, w);
  const float q1 = hlg_row_q(tq + sT + (size_t)b * M, M, lane, v_min, w);
  return td_target_pinned(q0, q1, alpha, log_pi[b], reward[b], not_done[b], discount);
}

// The critic phase.  y = reward + not_done * discount * (min(Q'_0, Q'_1) - alpha * log_pi) from the target logits tq;
// VIEWS (B even, H = B / 2): positions p and p + H both take 0.5 (y_p + y_{p+H}), the lower position evaluated first by
// either wave; y is clamped to [v_min, v_max] and written to target_q[row];
//   t_j = (erf((e_{j+1} - y) s) - erf((e_j - y) s)) / (erf((e_M - y) s) - erf((e_0 - y) s)),  s = 1 / (sigma sqrt 2)
//   row_loss[row] = -sum_n sum_j t_j log_softmax(q[n][row])_j,  dq[n][row][j] = (softmax(q[n][row])_j - t_j) inv_n
// (inv_n = 1 / B, or 1 / H with views); the loss is hlg_row_sum_kernel's fixed-order sum of row_loss times inv_n.
template <bool VIEWS>
__global__ void __launch_bounds__(256) hlg_critic_loss_kernel(const float* __restrict__ q, long long sQ,
                                                              const float* __restrict__ tq, long long sT,
                                                              const float* __restrict__ log_pi,
                                                              const float* __restrict__ reward,
                                                              const float* __restrict__ not_done,
                                                              const double* __restrict__ log_alpha, float discount,
                                                              int B, int M, float v_min, float v_max, float sigma,
                                                              float* __restrict__ dq, long long sD,
                                                              float* __restrict__ target_q,
                                                              float* __restrict__ row_loss) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // wave-uniform; nothing below crosses waves
  const float w = (v_max - v_min) / (float)M;
  const float alpha = (float)exp(*log_alpha);
  float y;
  if (VIEWS) {
    const int H = B / 2, p = row < H ? row : row - H;
    const float y0 = hlg_td_target(tq, sT, p, M, lane, v_min, w, alpha, log_pi, reward, not_done, discount);
    const float y1 = hlg_td_target(tq, sT, p + H, M, lane, v_min, w, alpha, log_pi, reward, not_done, discount);
    y = 0.5f * (y0 + y1);
  } else {
    y = hlg_td_target(tq, sT, row, M, lane, v_min, w, alpha, log_pi, reward, not_done, discount);
  }
  y = fminf(fmaxf(y, v_min), v_max);
  if (lane == 0) target_q[row] = y;

  const float s = 0.70710678118654752f / sigma;
  const float z = erff((v_min + (float)M * w - y) * s) - erff((v_min - y) * s);  // (2 x) the mass inside the range
  float t[kHlgSlots];
#pragma unroll
  for (int k = 0; k < kHlgSlots; ++k) {
    const int j = lane + 64 * k;
    t[k] = 0.f;
    if (j < M) t[k] = (erff((v_min + (float)(j + 1) * w - y) * s) - erff((v_min + (float)j * w - y) * s)) / z;
  }
  const float inv_n = 1.f / (float)(VIEWS ? B / 2 : B);
  float loss = 0.f;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    float ex[kHlgSlots], lg[kHlgSlots], mx;
    const float se = hlg_softmax(q + n * sQ + (size_t)row * M, M, lane, ex, lg, mx);
    const float lse = logf(se), inv_se = 1.f / se;
#pragma unroll
    for (int k = 0; k < kHlgSlots; ++k) {
      const int j = lane + 64 * k;
      if (j < M) {
        loss -= t[k] * ((lg[k] - mx) - lse);
        dq[n * sD + (size_t)row * M + j] = (ex[k] * inv_se - t[k]) * inv_n;
      }
    }
  }
  loss = wave_sum(loss);
  if (lane == 0) row_loss[row] = loss;
}

// out[0] = (sum of x[0 .. n)) * scale, in the block's fixed order
__global__ void hlg_row_sum_kernel(const float* x, int n, float scale, float* out) {
  __shared__ float sm[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += x[i];
  const float s = block_sum_256(a, sm);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// The actor phase, per row: Q_n = sum_j p_{n,j} c_j, row_q[row] = min(Q_0, Q_1), and
// dq[n][row][j] = g_n p_{n,j} (c_j - Q_n) with actor_loss_kernel's g: -1 / B for the smaller network, -0.5 / B each on
// an exact tie, 0 for the larger.  The scalars are hlg_actor_scalars_kernel's.
__global__ void __launch_bounds__(256) hlg_actor_rows_kernel(const float* __restrict__ q, long long sQ, int B, int M,
                                                             float v_min, float v_max, float* __restrict__ row_q,
                                                             float* __restrict__ dq, long long sD) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // wave-uniform
  const float w = (v_max - v_min) / (float)M;
  float ex[2][kHlgSlots], lg[kHlgSlots], mx, se[2], qn[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    se[n] = hlg_softmax(q + n * sQ + (size_t)row * M, M, lane, ex[n], lg, mx);
    qn[n] = hlg_expect(ex[n], se[n], M, lane, v_min, w);
  }
  if (lane == 0) row_q[row] = fminf(qn[0], qn[1]);
  const float inv = 1.f / B;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const float g = qn[n] < qn[1 - n] ? -inv : (qn[0] == qn[1] ? -0.5f * inv : 0.f);
    const float inv_se = 1.f / se[n];
#pragma unroll
    for (int k = 0; k < kHlgSlots; ++k) {
      const int j = lane + 64 * k;
      if (j < M) dq[n * sD + (size_t)row * M + j] = g * (ex[n][k] * inv_se) * (hlg_centre(j, v_min, w) - qn[n]);
    }
  }
}

// actor_loss_kernel's scalars with the row's min(Q_0, Q_1) read from row_q: one block, its fixed-order sums over rows
// scalars: [0] actor_loss [1] alpha_loss [2] entropy mean [3] alpha
__global__ void hlg_actor_scalars_kernel(const float* row_q, const float* log_pi, const float* log_std, int A,
                                         const double* log_alpha, float target_entropy, int B, float* scalars,
                                         double* dlog_alpha) {
  __shared__ float sm[4];
  const float alpha = (float)exp(*log_alpha);
  const float inv = 1.f / B;
  float al = 0.f, hl = 0.f, en = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    al += alpha * log_pi[b] - row_q[b];
    hl += -log_pi[b] - target_entropy;
    float e = 0.f;
    for (int a = 0; a < A; ++a) e += log_std[(size_t)b * A + a];
    en += 0.5f * A * (1.0f + 1.8378770664093453f) + e;
  }
  const float s_al = block_sum_256(al, sm);
  const float s_hl = block_sum_256(hl, sm);
  const float s_en = block_sum_256(en, sm);
  if (threadIdx.x == 0) {
    scalars[0] = s_al * inv;
    scalars[1] = alpha * (s_hl * inv);
    scalars[2] = s_en * inv;
    scalars[3] = alpha;
    if (dlog_alpha) *dlog_alpha = (double)(alpha * (s_hl * inv));  // d/dlog_alpha exp(log_alpha)*c = alpha*c
  }
}
