// The small last layers of the actor / Q trunks (mlp_out_fwd_kernel, mlp_out_bwd_kernel) and the squashed-Gaussian
// policy head, fused into the actor's last layer or as launches of its own (actor_head_fwd_kernel and the two backward
// kernels); beside it the deterministic DrQ-v2 head tanh(o) + clipped noise (det_head_fwd_kernel and its two backward
// kernels), fused the same way.  Included by heads.hip inside its anonymous namespace, behind reduce.h (wave_sum).
#pragma once

// ---- last layer of the actor / Q trunks: hidden -> N outputs with N tiny (Q: 1, actor: 2|A|) ----
// As GEMMs these are 16-32 workgroups walking K = 1024 behind two barriers per step (15-22 us each, pure latency);
// here the forward is one wave per row and the backward one pass over the activations that produces both the
// data gradient (ReLU mask of the layer below fused) and the weight gradient.
constexpr int kMaxOut = 16;

// ---- policy head (curl_sac.py:20-35, 87-108), one row: trunk output [mu | raw log_std] -> tanh(mu), pi, log_pi, ... ----
constexpr int kMaxA = 8;
constexpr float kHalfLog2Pi = 0.9189385332046727f;
struct HeadArgs {
  const float* noise;
  float *mu_t, *pi_t, *log_pi, *log_std, *tanh_ls, *pi_xa;  // pi_xa: pi also as the action columns of the Q input rows
  int A, xa_ld;
  float lo, hi;
  // noise_gen != nullptr (noise == nullptr then): the standard-normal draws of `torch.randn_like(mu)` (curl_sac.py:97)
  // are produced HERE -- element i from the Philox4x32-10 stream (rng_seed, counter rng_offset + i / 4, output i % 4),
  // Box-Muller -- and stored to noise_gen[i] for the backward pass, instead of by a launch of their own
  float* noise_gen;
  unsigned long long rng_seed, rng_offset;
  // rng_dev != nullptr: (seed, offset) are read from device memory when the kernel RUNS (rng_dev[0], rng_dev[1]) -- a
  // captured graph is replayed with new stream positions
  const unsigned long long* rng_dev;
  // the deterministic head (det_head_one) only: the standard deviation of its noise, read from device memory when the
  // kernel RUNS (a schedule is data, a captured graph never holds it), and the clip of the scaled noise (+inf: none)
  const float* std;
  float clip;
};

// (philox4x32_10 / philox_normal: common.h, shared with the noisy-cover kernel of augment.hip)
__device__ __forceinline__ void actor_head_one(float mu, float raw, int b, int a, const HeadArgs& hd, float& lp,
                                               float& corr) {
  const int A = hd.A;
  const float t = tanhf(raw);
  const float ls = hd.lo + 0.5f * (hd.hi - hd.lo) * (t + 1.f);
  if (hd.mu_t) hd.mu_t[(size_t)b * A + a] = tanhf(mu);
  if (hd.log_std) hd.log_std[(size_t)b * A + a] = ls;
  if (hd.tanh_ls) hd.tanh_ls[(size_t)b * A + a] = t;
  if (hd.noise || hd.noise_gen) {
    float n;
    if (hd.noise_gen) {
      const unsigned long long seed = hd.rng_dev ? hd.rng_dev[0] : hd.rng_seed;
      const unsigned long long offs = hd.rng_dev ? hd.rng_dev[1] : hd.rng_offset;
      n = philox_normal(seed, offs, (unsigned)(b * A + a));
      hd.noise_gen[(size_t)b * A + a] = n;
    } else {
      n = hd.noise[(size_t)b * A + a];
    }
    const float p = tanhf(mu + n * expf(ls));
    if (hd.pi_t) hd.pi_t[(size_t)b * A + a] = p;
    if (hd.pi_xa) hd.pi_xa[(size_t)b * hd.xa_ld + a] = p;
    lp += -0.5f * n * n - ls;
    corr += logf(fmaxf(1.f - p * p, 0.f) + 1e-6f);
  }
}

// one thread walks the row's actions
__device__ __forceinline__ void actor_head_row(const float* out2a_row, int b, const HeadArgs& hd) {
  float lp = 0.f, corr = 0.f;
  for (int a = 0; a < hd.A; ++a) actor_head_one(out2a_row[a], out2a_row[hd.A + a], b, a, hd, lp, corr);
  if ((hd.noise || hd.noise_gen) && hd.log_pi) hd.log_pi[b] = lp - kHalfLog2Pi * hd.A - corr;
}

// ---- deterministic policy head (DrQ-v2), one element: trunk output o [B][A] -> m = tanh(o), pi = clamp(m + e, -lim, lim)
// with e = clamp(s n, -c, c), lim = 1 - 1e-6 (DrQ-v2's TruncatedNormal.sample); log_std = log(s), a constant ----
constexpr int kHeadGauss = 1, kHeadDet = 2;  // the HEAD kinds of mlp_out_fwd_kernel (0: none)
__device__ __forceinline__ void det_head_one(float o, int b, int a, const HeadArgs& hd) {
  const size_t e = (size_t)b * hd.A + a;
  const float m = tanhf(o);
  const float s = *hd.std;
  if (hd.mu_t) hd.mu_t[e] = m;
  if (hd.log_std) hd.log_std[e] = (float)log((double)s);  // (in double: the float32 nearest to log(s), whatever s)
  if (hd.noise || hd.noise_gen) {
    float n;
    if (hd.noise_gen) {
      const unsigned long long seed = hd.rng_dev ? hd.rng_dev[0] : hd.rng_seed;
      const unsigned long long offs = hd.rng_dev ? hd.rng_dev[1] : hd.rng_offset;
      n = philox_normal(seed, offs, (unsigned)(b * hd.A + a));
      hd.noise_gen[e] = n;
    } else {
      n = hd.noise[e];
    }
    const float lim = 1.f - 1e-6f;
    const float ev = fminf(fmaxf(s * n, -hd.clip), hd.clip);
    const float p = fminf(fmaxf(m + ev, -lim), lim);
    if (hd.pi_t) hd.pi_t[e] = p;
    if (hd.pi_xa) hd.pi_xa[(size_t)b * hd.xa_ld + a] = p;
  }
}

// one thread walks the row's actions; log_pi is the constant 0 (no entropy term: the critic losses' alpha * 0)
__device__ __forceinline__ void det_head_row(const float* out_row, int b, const HeadArgs& hd) {
  for (int a = 0; a < hd.A; ++a) det_head_one(out_row[a], b, a, hd);
  if (hd.log_pi) hd.log_pi[b] = 0.f;
}

// out[z][m][n] = bias[z][n] + sum_k h[z][m][k] * W[z][n][k]        (curl_sac.py:73-74,132-133 forward)
// (two-level batch: blockIdx.y = outer * nb_inner + inner; the outer level's strides end in 2)
// HEAD: the outputs are the actor trunk's [mu | raw log_std] and the wave that produced a row also runs the policy
// head on it (a launch of its own otherwise: a few hundred cycles of work per row behind a 5 us launch); HEAD is the
// head's kind -- 0 none, kHeadGauss, kHeadDet (the outputs are then the A pre-squash means alone)
// R rows per wave: a weight float4 is loaded once for R rows; a row's sums do not depend on R (R = 1 is what runs).
// LDSW: the block first copies the N weight rows into LDS and its four waves read them from there -- with several
// rows (the actor's 8 x 1024) every wave otherwise pulls 32 KB through the L2 for itself, 16 MB per launch.
template <int HEAD, int R, bool LDSW>
__global__ __launch_bounds__(256) void mlp_out_fwd_kernel(const float* h, long long sH, long long sH2, const float* W,
                                                          long long sW, long long sW2, const float* bias, long long sB,
                                                          long long sB2, float* out, long long sOut, long long sOut2,
                                                          int M, int N, int K, int nb_inner, HeadArgs hd) {
  extern __shared__ __attribute__((aligned(16))) float wlds[];
  const int zo = blockIdx.y / nb_inner, zi = blockIdx.y - zo * nb_inner;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R, lane = threadIdx.x & 63;
  const float* hz = h + zi * sH + zo * sH2;
  const float* Wz = W + zi * sW + zo * sW2;
  if (LDSW) {
    const int n4 = (N * K) >> 2;
    for (int i = threadIdx.x; i < n4; i += 256)
      reinterpret_cast<f32x4*>(wlds)[i] = reinterpret_cast<const f32x4*>(Wz)[i];
    __syncthreads();
    Wz = wlds;
  }
  if (row0 >= M) return;
  float acc[R][kMaxOut];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int n = 0; n < kMaxOut; ++n) acc[r][n] = 0.f;
  for (int k = 4 * lane; k < K; k += 256) {  // (K % 4 == 0 checked by the host)
    f32x4 hv[R];
#pragma unroll
    for (int r = 0; r < R; ++r)  // (rows past the end re-read the last one; never stored)
      hv[r] = *reinterpret_cast<const f32x4*>(hz + (size_t)min(row0 + r, M - 1) * K + k);
#pragma unroll
    for (int n = 0; n < kMaxOut; ++n)
      if (n < N) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(Wz + (size_t)n * K + k);
#pragma unroll
        for (int r = 0; r < R; ++r)
          acc[r][n] += hv[r][0] * wv[0] + hv[r][1] * wv[1] + hv[r][2] * wv[2] + hv[r][3] * wv[3];
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = row0 + r;
    if (row >= M) break;  // wave-uniform
#pragma unroll
    for (int n = 0; n < kMaxOut; ++n)
      if (n < N) {
        const float s = wave_sum(acc[r][n]);
        acc[r][n] = s;
        if (lane == 0)
          out[zi * sOut + zo * sOut2 + (size_t)row * N + n] = s + (bias ? bias[zi * sB + zo * sB2 + n] : 0.f);
      }
    if (HEAD == kHeadDet) {
      float o = 0.f;
#pragma unroll
      for (int n = 0; n < kMaxOut; ++n) {
        const float v = n < N ? acc[r][n] + (bias ? bias[n] : 0.f) : 0.f;
        if (n == lane) o = v;
      }
      if (lane < hd.A) det_head_one(o, row, lane, hd);
      if (lane == 0 && hd.log_pi) hd.log_pi[row] = 0.f;
    }
    if (HEAD == kHeadGauss) {
      // every lane holds the row's outputs: lane a < A takes action a, the two sums over the actions are then added
      // in action order by lane 0 (the same order as the one-thread walk)
      float mu = 0.f, raw = 0.f;
#pragma unroll
      for (int n = 0; n < kMaxOut; ++n) {
        const float v = n < N ? acc[r][n] + (bias ? bias[n] : 0.f) : 0.f;
        if (n == lane) mu = v;
        if (n == lane + hd.A) raw = v;
      }
      float lp = 0.f, corr = 0.f;
      if (lane < hd.A) actor_head_one(mu, raw, row, lane, hd, lp, corr);
      float lps = 0.f, cs = 0.f;
      for (int a = 0; a < hd.A; ++a) lps += __shfl(lp, a), cs += __shfl(corr, a);
      if (lane == 0 && (hd.noise || hd.noise_gen) && hd.log_pi) hd.log_pi[row] = lps - kHalfLog2Pi * hd.A - cs;
    }
  }
}

// dh[z][m][k] = (h[z][m][k] > 0) * sum_n dy[z][m][n] * W[z][n][k];   dW[z][n][k] = sum_m dy[z][m][n] * h[z][m][k]
// One block = 16 k-columns x 64 row parts (K/16 x nbatch blocks: 128 for the twin Q functions); a thread's rows are
// all in flight at once; the 64 partial dW sums are added in part order (fixed order).
constexpr int kOutRows = 8;  // rows per thread per pass (64 parts x 8 = 512 rows per pass)
// db_out[z][n] = sum_m dy[z][m][n] and db_h[z][k] = sum_m dh[z][m][k] (optional): the bias gradients of this layer and
// of the one below -- the block already walks every row of its 16 columns.
// GEN: where dy comes from.  0: memory.  1 / 2: the twin Q functions' output gradient is a per-row formula of a few
// scalars -- the TD error of update_critic (curl_sac.py:350-362) or d(-min(Q1, Q2))/dQ of the actor loss
// (curl_sac.py:378-383) -- so every block evaluates it for its rows instead of waiting for a loss kernel's launch,
// and block (0, 0) also adds up that kernel's scalars (loss values, d(alpha loss)/d(log_alpha)).  N == 1, z = twin.
struct LossGen {
  const float *q, *tq, *log_pi, *reward, *not_done, *log_std;
  const double* log_alpha;
  double* dlog_alpha;
  float *target_q, *scalars, *dq;
  long long sTwin;
  float discount, target_entropy;
  int A;
};

// block-wide fixed-order sum of one value per thread (1024 threads); result valid in every thread
__device__ __forceinline__ float block_sum_1024(float v, float* sm16) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm16[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = sm16[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) t += sm16[w];
  return t;
}

template <int GEN>
__global__ __launch_bounds__(1024) void mlp_out_bwd_kernel(const float* dy, long long sDy, const float* h,
                                                           long long sH, const float* W, long long sW, float* dh,
                                                           long long sDh, float* dW, long long sDW, int M, int N,
                                                           int K, float* db_out, float* db_h, long long sDb, LossGen lg) {
  __shared__ float sm[64][17];
  const int z = blockIdx.y;
  const float alpha = GEN ? (float)exp(*lg.log_alpha) : 0.f;
  const float inv = GEN ? 1.f / M : 0.f;
  auto gen = [&](int m, float& target) -> float {  // dy[z][m] (and, GEN 1, the TD target of row m)
    if (GEN == 1) {
      const float v = fminf(lg.tq[m], lg.tq[lg.sTwin + m]) - alpha * lg.log_pi[m];
      target = lg.reward[m] + lg.not_done[m] * lg.discount * v;
      return 2.f * (lg.q[z * lg.sTwin + m] - target) * inv;
    }
    const float q1 = lg.q[m], q2 = lg.q[lg.sTwin + m];
    target = 0.f;
    // d(-min)/dq: the smaller one takes -1/B; an exact tie splits it (torch.min backward)
    if (z == 0) return q1 < q2 ? -inv : (q1 == q2 ? -0.5f * inv : 0.f);
    return q2 < q1 ? -inv : (q1 == q2 ? -0.5f * inv : 0.f);
  };
  const int kl = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + kl;
  const bool kv = k < K;
  const float* dyz = dy + z * sDy;
  const float* hz = h + z * sH;
  float* dhz = dh + z * sDh;
  float wreg[kMaxOut], acc[kMaxOut];
#pragma unroll
  for (int n = 0; n < kMaxOut; ++n) {
    wreg[n] = (n < N && kv) ? W[z * sW + (size_t)n * K + k] : 0.f;
    acc[n] = 0.f;
  }
  float bh = 0.f, bo = 0.f;  // column sums of dh (column k) and, in block 0, of dy (column kl)
  const bool do_bo = db_out && blockIdx.x == 0 && kl < N;
  for (int m0 = part; m0 < M; m0 += 64 * kOutRows) {
    float hv[kOutRows];
#pragma unroll
    for (int u = 0; u < kOutRows; ++u) {
      const int m = m0 + 64 * u;
      hv[u] = (m < M && kv) ? hz[(size_t)m * K + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kOutRows; ++u) {
      const int m = m0 + 64 * u;
      if (m < M) {
        float s = 0.f;
        if (GEN) {
          float target;
          const float d = gen(m, target);
          s = d * wreg[0];
          acc[0] += d * hv[u];
          if (do_bo) bo += d;
          if (blockIdx.x == 0 && kl == 0) {  // one block per twin also leaves dy (and the target) in memory
            lg.dq[z * lg.sTwin + m] = d;
            if (GEN == 1 && z == 0) lg.target_q[m] = target;
          }
        } else {
#pragma unroll
          for (int n = 0; n < kMaxOut; ++n)
            if (n < N) {
              const float d = dyz[(size_t)m * N + n];
              s += d * wreg[n];
              acc[n] += d * hv[u];
            }
          if (do_bo) bo += dyz[(size_t)m * N + kl];
        }
        const float dv = hv[u] > 0.f ? s : 0.f;
        if (kv) dhz[(size_t)m * K + k] = dv;
        bh += dv;
      }
    }
  }
  // fixed-order sums over the 64 row parts: dW's first row and the two bias sums share one barrier pair (three thread
  // rows add one array each), dW's remaining rows follow one by one
  __shared__ float sm_h[64][17], sm_o[64][17];
  const bool want_o = db_out && blockIdx.x == 0;  // block-uniform
  __syncthreads();
  if (dW) sm[part][kl] = acc[0];
  if (db_h) sm_h[part][kl] = bh;
  if (want_o) sm_o[part][kl] = bo;
  __syncthreads();
  if (part < 3) {
    const float(*src)[17] = part == 0 ? sm : (part == 1 ? sm_h : sm_o);
    const bool on = part == 0 ? (dW != nullptr && kv) : (part == 1 ? (db_h != nullptr && kv) : (want_o && kl < N));
    if (on) {
      float t = src[0][kl];
#pragma unroll 8
      for (int p = 1; p < 64; ++p) t += src[p][kl];
      if (part == 0)
        dW[z * sDW + k] = t;
      else if (part == 1)
        db_h[z * sDb + k] = t;
      else
        db_out[z * sDb + kl] = t;
    }
  }
  if (GEN && blockIdx.x == 0 && z == 0) {  // the loss kernel's scalars (block-uniform branch)
    __shared__ float sm16[16];
    if (GEN == 1) {
      float a1 = 0.f, a2 = 0.f;
      for (int b = threadIdx.x; b < M; b += 1024) {
        const float v = fminf(lg.tq[b], lg.tq[lg.sTwin + b]) - alpha * lg.log_pi[b];
        const float t = lg.reward[b] + lg.not_done[b] * lg.discount * v;
        const float d1 = lg.q[b] - t, d2 = lg.q[lg.sTwin + b] - t;
        a1 += d1 * d1, a2 += d2 * d2;
      }
      const float s1 = block_sum_1024(a1, sm16);
      const float s2 = block_sum_1024(a2, sm16);
      if (threadIdx.x == 0) lg.scalars[0] = s1 * inv + s2 * inv;
    } else {
      float al = 0.f, hl = 0.f, en = 0.f;
      for (int b = threadIdx.x; b < M; b += 1024) {
        al += alpha * lg.log_pi[b] - fminf(lg.q[b], lg.q[lg.sTwin + b]);
        hl += -lg.log_pi[b] - lg.target_entropy;
        float e = 0.f;
        for (int a = 0; a < lg.A; ++a) e += lg.log_std[(size_t)b * lg.A + a];
        en += 0.5f * lg.A * (1.0f + 1.8378770664093453f) + e;
      }
      const float s_al = block_sum_1024(al, sm16);
      const float s_hl = block_sum_1024(hl, sm16);
      const float s_en = block_sum_1024(en, sm16);
      if (threadIdx.x == 0) {
        lg.scalars[0] = s_al * inv;
        lg.scalars[1] = alpha * (s_hl * inv);
        lg.scalars[2] = s_en * inv;
        lg.scalars[3] = alpha;
        if (lg.dlog_alpha) *lg.dlog_alpha = (double)(alpha * (s_hl * inv));  // d/dlog_alpha exp(log_alpha)*c = alpha*c
      }
    }
  }
  if (dW == nullptr) return;  // block-uniform
#pragma unroll
  for (int n = 1; n < kMaxOut; ++n)
    if (n < N) {  // block-uniform
      __syncthreads();
      sm[part][kl] = acc[n];
      __syncthreads();
      if (part == 0 && kv) {
        float t = sm[0][kl];
#pragma unroll 8
        for (int p = 1; p < 64; ++p) t += sm[p][kl];
        dW[z * sDW + (size_t)n * K + k] = t;
      }
    }
}

// ---- policy head, a launch of its own (acting path; training fuses it into mlp_out_fwd_kernel<true>) ----
__global__ void actor_head_fwd_kernel(const float* out2a, int B, HeadArgs hd) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  actor_head_row(out2a + (size_t)b * 2 * hd.A, b, hd);
}

// gradient of (sum_a gpi[a]*pi[a] + glp*log_pi) wrt the trunk output [mu | raw_log_std]
// gpi[b][a] = gpi[b*gpi_ld + a] (+ gpi2[b*gpi_ld + a]): the action columns of the twin-Q input gradient can be read in
// place, summed over the twin (curl_sac.py:138), instead of through a `split_sum` pass
__global__ void actor_head_bwd_kernel(const float* gpi, const float* gpi2, int gpi_ld, const float* glp_scalar,
                                      const double* log_alpha, float glp_scale, const float* noise, const float* pi_t,
                                      const float* log_std, const float* tanh_ls, int B, int A, float lo, float hi,
                                      float* dout2a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  // d loss / d log_pi is the same for every row: alpha/B (actor loss) unless given explicitly
  const float glp = glp_scalar ? glp_scalar[b] : glp_scale * (float)exp(*log_alpha);
  for (int a = 0; a < A; ++a) {
    const float p = pi_t[(size_t)b * A + a];
    const float om = 1.f - p * p;
    float gp = gpi[(size_t)b * gpi_ld + a];
    if (gpi2) gp += gpi2[(size_t)b * gpi_ld + a];
    if (om > 0.f) gp += glp * (2.f * p / (om + 1e-6f));
    const float gu = gp * om;
    const float ls = log_std[(size_t)b * A + a];
    const float t = tanh_ls[(size_t)b * A + a];
    const float gls = gu * noise[(size_t)b * A + a] * expf(ls) - glp;
    dout2a[(size_t)b * 2 * A + a] = gu;
    dout2a[(size_t)b * 2 * A + A + a] = gls * 0.5f * (hi - lo) * (1.f - t * t);
  }
}

// general backward of the squashed-Gaussian head (curl_sac.py:20-35,87-108) for any upstream gradients of its four
// outputs (NULL = zero): mu_out = tanh(mu), log_std = lo + (hi - lo)(tanh(raw) + 1) / 2, pi = tanh(mu + noise exp(log_std)),
// log_pi = sum(-noise^2 / 2 - log_std) - A log(2 pi) / 2 - sum log(relu(1 - pi^2) + 1e-6); noise is a constant.
// dmu / dpi / dlog_std are [B][A], dlog_pi [B] (the [B, 1] column); writes d[mu | raw] = dout2a [B][2A].
__global__ void policy_head_bwd_kernel(const float* dmu, const float* dpi, const float* dlog_pi, const float* dlog_std,
                                       const float* noise, const float* mu_t, const float* pi_t, const float* log_std,
                                       const float* tanh_ls, int B, int A, float lo, float hi, float* dout2a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float glp = dlog_pi ? dlog_pi[b] : 0.f;
  const bool sampled = dpi || dlog_pi;
  for (int a = 0; a < A; ++a) {
    const size_t e = (size_t)b * A + a;
    float gmu = 0.f, gls = dlog_std ? dlog_std[e] : 0.f;
    if (dmu) {
      const float m = mu_t[e];
      gmu = dmu[e] * (1.f - m * m);
    }
    if (sampled) {
      const float p = pi_t[e];
      const float om = 1.f - p * p;
      float gp = dpi ? dpi[e] : 0.f;
      if (om > 0.f) gp += glp * (2.f * p / (om + 1e-6f));  // d/dpi of -log(relu(1 - pi^2) + 1e-6)
      const float gu = gp * om;                               // through tanh
      gmu += gu;
      gls += gu * noise[e] * expf(log_std[e]) - glp;          // pi's std, and gaussian_logprob's -log_std
    }
    const float t = tanh_ls[e];
    dout2a[(size_t)b * 2 * A + a] = gmu;
    dout2a[(size_t)b * 2 * A + A + a] = gls * 0.5f * (hi - lo) * (1.f - t * t);
  }
}

// ---- deterministic policy head, a launch of its own (acting path; training fuses it into mlp_out_fwd_kernel<kHeadDet>) ----
__global__ void det_head_fwd_kernel(const float* out, int B, HeadArgs hd) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  det_head_row(out + (size_t)b * hd.A, b, hd);
}

// gradient of sum_a gpi[a] * pi[a] wrt the trunk output o [B][A]: d pi / d o = 1 - m^2 (straight through the outer clamp;
// the noise depends on no parameter).  gpi is addressed as actor_head_bwd_kernel's: gpi[b*gpi_ld + a] (+ gpi2[...]), the
// action columns of the twin-Q input gradient read in place and summed over the twin
__global__ void det_head_bwd_kernel(const float* gpi, const float* gpi2, int gpi_ld, const float* mu_t, int B, int A,
                                    float* dout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int a = 0; a < A; ++a) {
    const float m = mu_t[(size_t)b * A + a];
    float gp = gpi[(size_t)b * gpi_ld + a];
    if (gpi2) gp += gpi2[(size_t)b * gpi_ld + a];
    dout[(size_t)b * A + a] = gp * (1.f - m * m);
  }
}

// general backward of the deterministic head for upstream gradients of mu and pi (NULL = zero), [B][A] each:
// d o = (dmu + dpi)(1 - m^2); log_pi and log_std are constants
__global__ void det_policy_head_bwd_kernel(const float* dmu, const float* dpi, const float* mu_t, int B, int A,
                                           float* dout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int a = 0; a < A; ++a) {
    const size_t e = (size_t)b * A + a;
    const float m = mu_t[e];
    const float g = (dmu ? dmu[e] : 0.f) + (dpi ? dpi[e] : 0.f);
    dout[e] = g * (1.f - m * m);
  }
}
