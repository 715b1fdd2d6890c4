// SAC targets and losses (curl_sac.py:353-359,378-399), the twin-Q input's concat / split, and the CURL cross-entropy
// (curl_sac.py:411-413) as launches of their own.  Included by heads.hip inside its anonymous namespace, behind reduce.h
// (wave_sum / wave_max / block_sum_256).
#pragma once

// xa[z] = [ zfeat | act ] for the twin-Q input
__global__ void concat_kernel(const float* zf, const float* act, int B, int F, int A, float* xa) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * (F + A)) return;
  const int b = i / (F + A), c = i - b * (F + A);
  xa[i] = c < F ? zf[(size_t)b * F + c] : act[(size_t)b * A + (c - F)];
}

// dxa[2][B][F+A] -> dz[B][F] (sum over the twin) and/or dact[B][A]
__global__ void split_sum_kernel(const float* dxa, long long sTwin, int B, int F, int A, float* dz, float* dact) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * (F + A)) return;
  const int b = i / (F + A), c = i - b * (F + A);
  const float v = dxa[i] + dxa[sTwin + i];
  if (c < F) {
    if (dz) dz[(size_t)b * F + c] = v;
  } else if (dact) {
    dact[(size_t)b * A + (c - F)] = v;
  }
}

// target_Q = r + not_done * gamma * (min(tq1,tq2) - alpha*log_pi)      (curl_sac.py:353-355)
__global__ void td_target_kernel(const float* tq, long long sTwin, const float* log_pi, const float* reward,
                                 const float* not_done, const double* log_alpha, float discount, int B,
                                 float* target_q) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float alpha = (float)exp(*log_alpha);
  const float v = fminf(tq[b], tq[sTwin + b]) - alpha * log_pi[b];
  target_q[b] = reward[b] + not_done[b] * discount * v;
}

// loss = mse(q1,tQ) + mse(q2,tQ); dq = 2(q - tQ)/B                    (curl_sac.py:359)
__global__ void critic_loss_kernel(const float* q, long long sTwin, const float* target_q, int B, float* loss,
                                   float* dq) {
  __shared__ float sm[4];
  float a1 = 0.f, a2 = 0.f;
  const float inv = 1.f / B;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float d1 = q[b] - target_q[b], d2 = q[sTwin + b] - target_q[b];
    a1 += d1 * d1;
    a2 += d2 * d2;
    dq[b] = 2.f * d1 * inv;
    dq[sTwin + b] = 2.f * d2 * inv;
  }
  const float s1 = block_sum_256(a1, sm);
  const float s2 = block_sum_256(a2, sm);
  if (threadIdx.x == 0) loss[0] = s1 * inv + s2 * inv;
}

// the two kernels above in one launch (the TD target only feeds the loss): target_q is still written out
__global__ void critic_td_loss_kernel(const float* q, const float* tq, long long sTwin, const float* log_pi,
                                      const float* reward, const float* not_done, const double* log_alpha,
                                      float discount, int B, float* target_q, float* loss, float* dq) {
  __shared__ float sm[4];
  float a1 = 0.f, a2 = 0.f;
  const float inv = 1.f / B;
  const float alpha = (float)exp(*log_alpha);
  for (int b = threadIdx.x; b < B; b += 256) {
    const float v = fminf(tq[b], tq[sTwin + b]) - alpha * log_pi[b];
    const float t = reward[b] + not_done[b] * discount * v;
    target_q[b] = t;
    const float d1 = q[b] - t, d2 = q[sTwin + b] - t;
    a1 += d1 * d1;
    a2 += d2 * d2;
    dq[b] = 2.f * d1 * inv;
    dq[sTwin + b] = 2.f * d2 * inv;
  }
  const float s1 = block_sum_256(a1, sm);
  const float s2 = block_sum_256(a2, sm);
  if (threadIdx.x == 0) loss[0] = s1 * inv + s2 * inv;
}

// One position's TD target by the operations the loop of critic_td_loss_kernel compiles to for gfx950 -- alpha * log_pi
// and not_done * discount rounded (one packed multiply), the subtraction from the min rounded, the last multiply-add
// fused -- stated explicitly: a loop with other surroundings is contracted otherwise (the subtraction fused as well), and
// two identical views must give that kernel's target bit for bit (tests/test_gpu_aug_views.py holds the two together).
__device__ __forceinline__ float td_target_pinned(float tq1, float tq2, float alpha, float log_pi, float reward,
                                                  float not_done, float discount) {
#pragma clang fp contract(off)
  const float v = fminf(tq1, tq2) - alpha * log_pi;
  return __builtin_fmaf(not_done * discount, v, reward);
}

// critic_td_loss_kernel over two augmented views of every transition (DrQ's K = 2, M = 2; B even): positions p and
// p + H, H = B / 2, are one transition seen twice.  Both get the mean of their two targets, tbar = 0.5 (t_p + t_{p+H}),
// each t by the arithmetic above; loss = (1 / H) sum over all B positions and both twins of (q - tbar)^2 -- the two
// views' MSEs over H transitions, summed --, dq = 2 (q - tbar) (1 / H).  One thread per pair, so target_q's two copies
// are one value; the block sums are the fixed-order ones.
__global__ void critic_td_loss_views_kernel(const float* q, const float* tq, long long sTwin, const float* log_pi,
                                            const float* reward, const float* not_done, const double* log_alpha,
                                            float discount, int B, float* target_q, float* loss, float* dq) {
  __shared__ float sm[4];
  float a1 = 0.f, a2 = 0.f;
  const int H = B / 2;
  const float inv = 1.f / H;
  const float alpha = (float)exp(*log_alpha);
  for (int p = threadIdx.x; p < H; p += 256) {
    float t2[2];
    for (int k = 0; k < 2; ++k) {
      const int b = p + k * H;
      t2[k] = td_target_pinned(tq[b], tq[sTwin + b], alpha, log_pi[b], reward[b], not_done[b], discount);
    }
    const float t = 0.5f * (t2[0] + t2[1]);
    for (int k = 0; k < 2; ++k) {
      const int b = p + k * H;
      target_q[b] = t;
      const float d1 = q[b] - t, d2 = q[sTwin + b] - t;
      a1 += d1 * d1;
      a2 += d2 * d2;
      dq[b] = 2.f * d1 * inv;
      dq[sTwin + b] = 2.f * d2 * inv;
    }
  }
  const float s1 = block_sum_256(a1, sm);
  const float s2 = block_sum_256(a2, sm);
  if (threadIdx.x == 0) loss[0] = s1 * inv + s2 * inv;
}

// actor/alpha losses and their seeds                                  (curl_sac.py:378-399)
// scalars: [0] actor_loss [1] alpha_loss [2] entropy mean [3] alpha
__global__ void actor_loss_kernel(const float* q, long long sTwin, const float* log_pi, const float* log_std, int A,
                                  const double* log_alpha, float target_entropy, int B, float* scalars, float* dq,
                                  double* dlog_alpha) {
  __shared__ float sm[4];
  const float alpha = (float)exp(*log_alpha);
  const float inv = 1.f / B;
  float al = 0.f, hl = 0.f, en = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float q1 = q[b], q2 = q[sTwin + b];
    al += alpha * log_pi[b] - fminf(q1, q2);
    hl += -log_pi[b] - target_entropy;
    float e = 0.f;
    for (int a = 0; a < A; ++a) e += log_std[(size_t)b * A + a];
    en += 0.5f * A * (1.0f + 1.8378770664093453f) + e;
    // d(-min)/dq: the smaller one takes -1/B; an exact tie splits it (torch.min backward)
    dq[b] = q1 < q2 ? -inv : (q1 == q2 ? -0.5f * inv : 0.f);
    dq[sTwin + b] = q2 < q1 ? -inv : (q1 == q2 ? -0.5f * inv : 0.f);
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

// CURL InfoNCE: loss = mean_a( logsumexp_b(l[a][:]) - l[a][a] ); dl = (softmax - I)/B
// VIEWS (two augmented views per transition, B even): row a's partner column (a + B/2) % B -- the other view of the
// anchor's own transition, no negative -- is left out of the max and of the sum, and its dl is exactly 0.
template <bool VIEWS>
__global__ void curl_ce_kernel(const float* logits, int B, int ld, float* row_loss, float* dlogits) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const float* l = logits + (size_t)row * ld;
  const int partner = VIEWS ? (row + B / 2) % B : -1;
  float mx = -INFINITY;
  for (int j = lane; j < B; j += 64)
    if (!VIEWS || j != partner) mx = fmaxf(mx, l[j]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int j = lane; j < B; j += 64)
    if (!VIEWS || j != partner) se += expf(l[j] - mx);
  se = wave_sum(se);
  const float lse = logf(se) + mx;
  if (lane == 0) row_loss[row] = lse - l[row];
  if (dlogits) {
    const float inv = 1.f / B;
    for (int j = lane; j < B; j += 64) {
      const float p = expf(l[j] - lse);
      dlogits[(size_t)row * ld + j] = VIEWS && j == partner ? 0.f : (p - (j == row ? 1.f : 0.f)) * inv;
    }
  }
}
