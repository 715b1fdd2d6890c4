// Truncated quantile critics (Kuznetsov et al., ICML 2020): the critic loss over M quantile atoms per Q
// function -- pool and rank the two target networks' atoms, keep the K = 2 (M - d) smallest, regress every online atom
// on the kept ones with the quantile Huber loss -- and the actor loss over the mean of all atoms.  Included by heads.hip
// inside its anonymous namespace, behind reduce.h (wave_sum / block_sum_256).
#pragma once

// the value lane `j` (wave-uniform) holds, in every lane
__device__ __forceinline__ float lane_value(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// One wave per minibatch row, four rows per workgroup.  Lane l < 2M holds pooled target atom l = z'[l / M][row][l % M]
// and online atom l = theta[l / M][row][l % M]; the lanes behind hold nothing.
//   rank_l = #{ j : z_j < z_l or (z_j == z_l and j < l) }     (a permutation of 0 .. 2M-1: ties take index order)
//   kept_l = rank_l < K,  y_l = reward + not_done * discount * (z_l - alpha * log_pi)
//   lane l: sum over the kept j, in index order, of w * huber(u) and of w * clamp(u, -1, 1), u = y_j - theta_l,
//           w = |tau_i - [u < 0]|, tau_i = (2 i + 1) / (2 M), i = l % M
//   dq_l = -sum / (B 2 M K);  row_loss[row] = wave_sum(lanes' sums) / (2 M K): the mean over rows is the loss.
// No atomics and fixed orders throughout: a rerun writes the same bits.
__global__ void __launch_bounds__(256) tqc_critic_loss_kernel(const float* __restrict__ q, long long sQ,
                                                              const float* __restrict__ tq, long long sT,
                                                              const float* __restrict__ log_pi,
                                                              const float* __restrict__ reward,
                                                              const float* __restrict__ not_done,
                                                              const double* __restrict__ log_alpha, float discount,
                                                              int B, int M, int d, float* __restrict__ dq, long long sD,
                                                              float* __restrict__ row_loss) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // wave-uniform; nothing below crosses waves
  const int n2 = 2 * M, K = 2 * (M - d);
  const bool live = lane < n2;
  const int n = lane >= M ? 1 : 0, i = lane - n * M;
  const size_t at = (size_t)row * M + i;
  const float z = live ? tq[n * sT + at] : 0.f;
  const float theta = live ? q[n * sQ + at] : 0.f;
  int rank = 0;
  for (int j = 0; j < n2; ++j) {
    const float zj = lane_value(z, j);
    rank += (zj < z || (zj == z && j < lane)) ? 1 : 0;
  }
  const unsigned long long kept = __ballot(live && rank < K);
  const float alpha = (float)exp(*log_alpha);
  const float y = reward[row] + not_done[row] * discount * (z - alpha * log_pi[row]);
  const float tau = (2 * i + 1) / (float)n2;
  float loss = 0.f, grad = 0.f;
  for (int j = 0; j < n2; ++j) {
    if (!((kept >> j) & 1)) continue;  // wave-uniform
    const float u = lane_value(y, j) - theta;
    const float au = fabsf(u);
    const float w = u < 0.f ? 1.f - tau : tau;
    loss += w * (au <= 1.f ? 0.5f * u * u : au - 0.5f);
    grad += w * fminf(fmaxf(u, -1.f), 1.f);
  }
  const float inv_row = 1.f / ((float)n2 * (float)K);
  if (live) dq[n * sD + at] = -grad * (inv_row / (float)B);
  const float s = wave_sum(live ? loss : 0.f);
  if (lane == 0) row_loss[row] = s * inv_row;
}

// actor_loss_kernel (sac_loss.h) with the row's Q term the mean of its 2M atoms and no min: dq = -1 / (2 M B) everywhere.
// scalars: [0] actor_loss [1] alpha_loss [2] entropy mean [3] alpha
__global__ void tqc_actor_loss_kernel(const float* q, long long sQ, const float* log_pi, const float* log_std, int A,
                                      const double* log_alpha, float target_entropy, int B, int M, float* scalars,
                                      float* dq, long long sD, double* dlog_alpha) {
  __shared__ float sm[4];
  const float alpha = (float)exp(*log_alpha);
  const float inv = 1.f / B, inv_atoms = 1.f / (2 * M);
  float al = 0.f, hl = 0.f, en = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* q1 = q + (size_t)b * M;
    float qs = 0.f;
    for (int i = 0; i < M; ++i) qs += q1[i];
    for (int i = 0; i < M; ++i) qs += q1[sQ + i];
    al += alpha * log_pi[b] - qs * inv_atoms;
    hl += -log_pi[b] - target_entropy;
    float e = 0.f;
    for (int a = 0; a < A; ++a) e += log_std[(size_t)b * A + a];
    en += 0.5f * A * (1.0f + 1.8378770664093453f) + e;
  }
  const float g = -inv * inv_atoms;
  for (int k = threadIdx.x; k < B * M; k += 256) {
    dq[k] = g;
    dq[sD + k] = g;
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
