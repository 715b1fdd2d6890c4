// The self-predictive latent loss (SPR / BYOL's normalised regression, one step): pred_loss_kernel<NF>.  Included by
// heads.hip inside its anonymous namespace, behind reduce.h (wave_sum).
#pragma once

// Per row b of p (the predictor's output) and t (the target encoder's latent, a constant), both [B][F]:
//   ph = p / max(|p|, eps), th = t / max(|t|, eps)                      (F.normalize's default, eps = 1e-12)
//   row_loss[b] = sum_f (ph_f - th_f)^2                                  (= 2 - 2 cos(p, t) where neither is zero)
//   dp[b] = (2 / B) (I - ph ph^T)(ph - th) / |p|     for |p| >= eps      (d mean_b row_loss[b] / d p[b])
//         = (2 / B) (ph - th) / eps                  below it            (the clamp's branch, as autograd has it)
// The norms are float32 square roots of float32 sums of squares.  One wave per row, four rows per 256-thread block; lane
// l holds features l, l + 64, ... (NF of them, compile-time: the row is read once and stays in registers); a lane adds
// its features in index order, the wave its lanes by wave_sum's butterfly: a fixed order, no atomics, nothing shared
// between waves.  A NaN norm stays a NaN (the comparisons below are written so that it does), so a row with a
// non-finite input has non-finite outputs and no other row sees it.
constexpr float kPredEps = 1e-12f;

template <int NF>
__global__ __launch_bounds__(256) void pred_loss_kernel(const float* p, const float* t, int B, int F, float* row_loss,
                                                        float* dp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // (wave-uniform: rows past B do nothing)
  const float* pr = p + (size_t)row * F;
  const float* tr = t + (size_t)row * F;
  float pv[NF], tv[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int f = lane + 64 * i;
    pv[i] = f < F ? pr[f] : 0.f;
    tv[i] = f < F ? tr[f] : 0.f;
  }
  float sp = 0.f, st = 0.f;
#pragma unroll
  for (int i = 0; i < NF; ++i) sp += pv[i] * pv[i], st += tv[i] * tv[i];
  const float np = sqrtf(wave_sum(sp)), nt = sqrtf(wave_sum(st));
  const float cp = np < kPredEps ? kPredEps : np, ct = nt < kPredEps ? kPredEps : nt;
  float sl = 0.f, sd = 0.f;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const float ph = pv[i] / cp, d = ph - tv[i] / ct;  // (lanes past F: 0 - 0)
    pv[i] = ph, tv[i] = d;
    sl += d * d, sd += ph * d;
  }
  sl = wave_sum(sl), sd = wave_sum(sd);
  if (lane == 0) row_loss[row] = sl;
  const float scale = 2.f / (float)B;
  const bool live = np >= kPredEps;
  float* dr = dp + (size_t)row * F;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int f = lane + 64 * i;
    if (f < F) dr[f] = live ? scale * (tv[i] - pv[i] * sd) / np : scale * tv[i] / kPredEps;
  }
}
