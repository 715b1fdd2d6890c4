// LayerNorm behind the encoder fc layer (encoder.py:67,101): the forward that also adds up the fc's split-K partials
// (fc_ln_fwd_kernel), the backward (ln_bwd_kernel) and the parameter gradients as a launch of their own
// (ln_param_grad_kernel).  Included by heads.hip inside its anonymous namespace, behind reduce.h (wave_sum).
#pragma once

// ---- fc split-K reduce + bias + LayerNorm (one wave per row; a lane holds features lane, lane+64, ...:
// NF = ceil(F / 64) rounded up to 1, 2, 3, 4, 8 or 16, i.e. F <= 1024: the reference's --encoder_feature_dim is free,
// train.py:80; 50 is what every configuration uses) ----
// (blockIdx.y = job: up to kMaxLnJobs encoders' features in one launch -- the actor's, the target critic's and the
// critic's at the top of update_critic, curl_sac.py:350-358)
constexpr int kMaxLnJobs = 4;
struct FcLnJobs {
  CurlaFcLnJob j[kMaxLnJobs];
};

template <int NF>
__global__ void fc_ln_fwd_kernel(FcLnJobs jobs, int nsplit, long long sSplit, int ldp, int B, int F, float eps, int A) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;
  const CurlaFcLnJob& jb = jobs.j[blockIdx.y];
  const float *P = jb.partial, *bias = jb.bias, *gamma = jb.gamma, *beta = jb.beta, *act = jb.act;
  float *fc_out = jb.fc_out, *y = jb.y, *xhat = jb.xhat, *rstd = jb.rstd, *xa = jb.xa;
  const int tanh_out = jb.tanh_out;
  float v[NF];
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    v[j] = 0.f;
    if (f < F) {
      // same summation order as a plain loop, but 8 partials are fetched together (the loop is pure load latency)
      const float* p = P + (size_t)row * ldp + f;
      float a = 0.f;
      int s = 0;
      for (; s + 8 <= nsplit; s += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = p[(s + k) * sSplit];
#pragma unroll
        for (int k = 0; k < 8; ++k) a += t[k];
      }
      for (; s < nsplit; ++s) a += p[s * sSplit];
      v[j] = a + bias[f];
    }
    tot += v[j];
  }
  const float mean = wave_sum(tot) / F;
  float d[NF], sq = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    d[j] = lane + 64 * j < F ? v[j] - mean : 0.f;
    sq += d[j] * d[j];
  }
  const float var = wave_sum(sq) / F;
  const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    if (f < F) {
      const float xh = d[j] * rs;
      float o = xh * gamma[f] + beta[f];
      if (tanh_out) o = tanhf(o);
      if (fc_out) fc_out[(size_t)row * F + f] = v[j];
      y[(size_t)row * F + f] = o;
      if (xhat) xhat[(size_t)row * F + f] = xh;
      if (xa) xa[(size_t)row * (F + A) + f] = o;  // torch.cat([z, action], 1) written in place (curl_sac.py:138)
    }
  }
  if (xa && act && lane < A) xa[(size_t)row * (F + A) + F + lane] = act[(size_t)row * A + lane];
  if (lane == 0 && rstd) rstd[row] = rs;
}

// dx = rstd * (dy*gamma - mean(dy*gamma) - xhat * mean(dy*gamma*xhat)).  The incoming gradient is dy[b*ld + f]
// (+ dy2[b*ld + f] when dy2 is given: the two halves of the twin-Q input gradient, torch.cat's backward at
// curl_sac.py:138, summed here instead of in a pass of their own)
// `partial` (optional) [gridDim.x][3][F]: the workgroup's four rows' contributions to dgamma (dy xhat), dbeta (dy) and
// the fc bias gradient (dx), added in wave (= row) order -- the column sums over the whole batch are finished by one
// extra workgroup of the NEXT launch that walks these rows anyway, the fc backward (curla_fc_bwd_ln / curla_fc_dw_ln),
// instead of by a launch of their own (ln_param_grad_kernel).
template <int NF>
__global__ void ln_bwd_kernel(const float* dy, const float* dy2, int ld, const float* xhat, const float* rstd,
                              const float* gamma, int B, int F, float* dx, float* partial) {
  __shared__ float part[4][3][NF * 64];
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  const int lane = threadIdx.x & 63;
  const bool live = row < B;
  if (!live && !partial) return;
  float g[NF], xh[NF], d[NF], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    g[j] = 0.f, xh[j] = 0.f, d[j] = 0.f;
    if (live && f < F) {
      d[j] = dy[(size_t)row * ld + f];
      if (dy2) d[j] += dy2[(size_t)row * ld + f];
      g[j] = d[j] * gamma[f];
      xh[j] = xhat[(size_t)row * F + f];
    }
    s1 += g[j];
    s2 += g[j] * xh[j];
  }
  const float m1 = wave_sum(s1) / F;
  const float m2 = wave_sum(s2) / F;
  const float rs = live ? rstd[row] : 0.f;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = lane + 64 * j;
    const float o = rs * (g[j] - m1 - xh[j] * m2);
    if (live && f < F) dx[(size_t)row * F + f] = o;
    if (partial) part[wave][0][f] = d[j] * xh[j], part[wave][1][f] = d[j], part[wave][2][f] = live ? o : 0.f;
  }
  if (partial) {
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * F; i += blockDim.x) {
      const int q = i / F, f = i - q * F;
      partial[(size_t)blockIdx.x * 3 * F + i] = ((part[0][q][f] + part[1][q][f]) + part[2][q][f]) + part[3][q][f];
    }
  }
}

// dgamma[f] = sum_b dy*xhat ; dbeta[f] = sum_b dy ; optionally dbias[f] = sum_b dx (the gradient of the fc bias
// that feeds the LayerNorm: the same walk over the rows).  One block of 1024 per 16 features: 64 row parts, so a
// thread's rows (8 at B = 512) are all in flight at once and F = 50 is four workgroups instead of one -- the kernel
// is pure load latency.  The parts are added in a fixed order: the 4 of a wave by lane exchange, the 16 waves in
// wave order.
__global__ __launch_bounds__(1024) void ln_param_grad_kernel(const float* dy, const float* dy2, int ld, const float* xhat,
                                                             const float* dx, int B, int F, float* dgamma,
                                                             float* dbeta, float* dbias) {
  __shared__ float sg[16][16], sb[16][16], sx[16][16];
  const int fl = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int f = blockIdx.x * 16 + fl;
  float ag = 0.f, ab = 0.f, ax = 0.f;
  if (f < F) {
    int b = part;
    for (; b + 7 * 64 < B; b += 8 * 64) {  // 8 rows in flight, accumulated in row order
      float d[8], x[8], e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        d[k] = dy[(size_t)(b + 64 * k) * ld + f], x[k] = xhat[(size_t)(b + 64 * k) * F + f];
        if (dy2) d[k] += dy2[(size_t)(b + 64 * k) * ld + f];
        e[k] = dbias ? dx[(size_t)(b + 64 * k) * F + f] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) ag += d[k] * x[k], ab += d[k], ax += e[k];
    }
    for (; b < B; b += 64) {
      float d = dy[(size_t)b * ld + f];
      if (dy2) d += dy2[(size_t)b * ld + f];
      ag += d * xhat[(size_t)b * F + f];
      ab += d;
      if (dbias) ax += dx[(size_t)b * F + f];
    }
  }
  // lanes l, l^16, l^32, l^48 hold the same feature: (p0 + p1) + (p2 + p3) in every lane
  ag += __shfl_xor(ag, 16), ab += __shfl_xor(ab, 16), ax += __shfl_xor(ax, 16);
  ag += __shfl_xor(ag, 32), ab += __shfl_xor(ab, 32), ax += __shfl_xor(ax, 32);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 16) sg[wave][fl] = ag, sb[wave][fl] = ab, sx[wave][fl] = ax;
  __syncthreads();
  if (threadIdx.x < 16 && f < F) {
    float g = sg[0][fl], bsum = sb[0][fl], xs = sx[0][fl];
#pragma unroll
    for (int k = 1; k < 16; ++k) g += sg[k][fl], bsum += sb[k][fl], xs += sx[k][fl];
    dgamma[f] = g;
    dbeta[f] = bsum;
    if (dbias) dbias[f] = xs;
  }
}
