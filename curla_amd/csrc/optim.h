// The optimiser step over the flat parameter buffers: the target networks' soft update (soft_update_kernel,
// soft_update2_kernel), the shrink-and-perturb of a network reset (shrink_perturb2_kernel) and Adam, one step or two back to back, with the float64 scalar and the target lerp that can
// ride along (adam_step_kernel, adam_step2_kernel), clipping by the global gradient norm (AdamClip) and decoupled weight
// decay (decay_one: AdamW) included.
// Included by heads.hip inside its anonymous namespace.
#pragma once

// target <- tau*p + (1-tau)*target                                     (utils.py:37-41)
__global__ void soft_update_kernel(const float* p, float* tgt, size_t n, float tau, float omt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // two roundings of the products and one of the sum, as `tau * p + (1 - tau) * t` evaluates in torch (no fused
  // multiply-add), so the targets match the reference's bit for bit given the same inputs
  for (; i < n; i += stride) {
#pragma clang fp contract(off)
    tgt[i] = tau * p[i] + omt * tgt[i];
  }
}

// the same over one flat block whose first `split` elements take (tau_a, 1-tau_a) and the rest (tau_b, 1-tau_b):
// the encoder and the Q functions of the critic are adjacent in the flat layout and have their own rates
__global__ void soft_update2_kernel(const float* p, float* tgt, size_t n, size_t split, float tau_a, float omt_a,
                                    float tau_b, float omt_b) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
#pragma clang fp contract(off)
    const bool a = i < split;
    tgt[i] = (a ? tau_a : tau_b) * p[i] + (a ? omt_a : omt_b) * tgt[i];
  }
}

// Shrink and perturb (network resets): p <- keep * p + new * fresh over one flat block whose first `split`
// elements take (keep_a, new_a) and the rest (keep_b, new_b), soft_update2_kernel's range convention; the target copy
// (tgt != nullptr) takes the same formula on its own old value with the same fresh value.
//   0 < keep < 1 : two products and a sum, each rounding once (no fused multiply-add), as soft_update_kernel
//   keep == 0    : p = fresh by SELECTION -- the old value is not read, so a NaN or Inf in it does not survive
//   keep == 1    : the element is neither read nor written (a stored -0.0 stays -0.0), in either array
// `keep` is uniform over a wave except in the one wave that straddles `split`.
__device__ __forceinline__ void shrink_perturb_one(float* p, float* t, const float* f, float keep, float nw) {
#pragma clang fp contract(off)
  if (keep == 1.0f) return;
  const float fr = *f;
  if (keep == 0.0f) {
    *p = fr;
    if (t) *t = fr;
    return;
  }
  *p = keep * *p + nw * fr;
  if (t) *t = keep * *t + nw * fr;
}

// vec: p, tgt (when given) and fresh are 16-byte aligned -- 16-byte accesses over the whole float4s that lie on one side
// of `split`, element by element in the one that straddles it and in the tail; else element by element throughout.
__global__ void __launch_bounds__(256) shrink_perturb2_kernel(float* p, float* tgt, const float* fresh, size_t n,
                                                              size_t split, int vec, float keep_a, float new_a,
                                                              float keep_b, float new_b) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (vec) {
    const size_t n4 = n >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      const size_t base = i << 2;
      if (base < split && base + 4 > split) {  // the one float4 with elements on both sides
        for (int e = 0; e < 4; ++e) {
          const bool a = base + e < split;
          shrink_perturb_one(p + base + e, tgt ? tgt + base + e : nullptr, fresh + base + e, a ? keep_a : keep_b,
                             a ? new_a : new_b);
        }
        continue;
      }
      const bool a = base < split;
      const float keep = a ? keep_a : keep_b, nw = a ? new_a : new_b;
      if (keep == 1.0f) continue;
      const f32x4 ff = reinterpret_cast<const f32x4*>(fresh)[i];
      if (keep == 0.0f) {
        reinterpret_cast<f32x4*>(p)[i] = ff;
        if (tgt) reinterpret_cast<f32x4*>(tgt)[i] = ff;
        continue;
      }
      {
#pragma clang fp contract(off)
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = keep * pp[e] + nw * ff[e];
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if (tgt) {
          f32x4 tt = reinterpret_cast<f32x4*>(tgt)[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) tt[e] = keep * tt[e] + nw * ff[e];
          reinterpret_cast<f32x4*>(tgt)[i] = tt;
        }
      }
    }
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    const bool a = i < split;
    shrink_perturb_one(p + i, tgt ? tgt + i : nullptr, fresh + i, a ? keep_a : keep_b, a ? new_a : new_b);
  }
}

// One Adam step over a flat run of parameters (torch.optim.Adam, weight_decay 0, no amsgrad; curl_sac.py:299-313):
//   m += (1-b1)(g-m);  v = b2 v + (1-b2) g g;  p -= step_size * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// with step_size = lr/(1-b1^t) and the two bias corrections evaluated on the host in double, as torch's
// single-tensor Adam does.  Seven fp32 streams (4 read, 3 written), 16-byte accesses when the run is 16-byte
// aligned: HBM-bound (28 B per parameter).
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float w1, float b2, float w2,
                                         float step_size, float bc2_sqrt, float eps) {
  // (no fused multiply-adds: every product and sum rounds on its own, as torch's element-wise Adam does, and the
  // one-step and two-step kernels then agree bit for bit whatever the compiler would have contracted in each)
#pragma clang fp contract(off)
  m = (w1 < 0.5f) ? m + w1 * (g - m) : g - (g - m) * (1.0f - w1);
  v = v * b2 + (w2 * g) * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - (step_size * m) / denom;
}

// Decoupled weight decay (torch.optim.AdamW; Adam with decoupled_weight_decay=True): p <- p * d in front of the Adam
// update, d = (float)(1 - lr * weight_decay) formed on the host in double as torch forms it.  ONE multiply with one
// rounding; the update then runs on the decayed parameter.  The gradient, the clip coefficient and the moments do not
// see d.  (Contraction off here as in adam_one: the product must round before the update's subtraction consumes it.)
__device__ __forceinline__ float decay_one(float p, float d) {
#pragma clang fp contract(off)
  return p * d;
}

// A float64 scalar parameter stepped by the same launch (log_alpha beside the actor's parameters: the reference steps
// actor_optimizer and log_alpha_optimizer back to back, curl_sac.py:393-404); p == nullptr: none.
struct AdamScalar64 {
  double *p, *m, *v;
  const double* g;
  double w1, b2, w2, step_size, bc2_sqrt, eps;
  const double* dyn;  // != nullptr: step_size = dyn[0], bc2_sqrt = dyn[1], read when the kernel runs
};

// The target network's soft update in the same pass: target <- tau p + (1 - tau) target with the parameter this launch
// has just stepped (utils.py:37-41 right after critic_optimizer.step(), curl_sac.py:367,442-445); elements [0, split)
// take (tau_a, omt_a), the rest (tau_b, omt_b).  tgt == nullptr: none.
struct AdamLerp {
  float* tgt;
  size_t split;
  float tau_a, omt_a, tau_b, omt_b;
};
__device__ __forceinline__ float lerp_one(float p, float t, float tau, float omt) {
#pragma clang fp contract(off)
  return tau * p + omt * t;  // two roundings of the products and one of the sum, as soft_update_kernel
}

// Clipping by the global gradient norm inside the step (torch.nn.utils.clip_grad_norm_, norm_type 2, right in front of
// the optimizer's step).  `partials` are the `count` (1 .. 256) double sums of squares grad_sqsum_kernel left for ALL the
// runs of this step; every block adds them up in the same fixed order, so every block of every launch of the step holds
// the same norm = sqrt(sum) and coef = min(1, max_norm / (norm + 1e-6)), formed in double and rounded to float once.
// coef != 1: the gradient is scaled (one rounding per element), written back -- .grad afterwards is what Adam consumed,
// as with torch -- and stepped on; coef == 1: nothing is written and the step is the unclipped one.  A NaN norm gives a
// NaN coefficient (torch's clamp(max=1) lets it through too).  Block 0 leaves (norm, coef) in stats[0 .. 1].
// The kernels are templates on whether they clip: without (partials == nullptr) they are the ones they were.
struct AdamClip {
  const double* partials;
  int count;
  double max_norm;
  float* stats;
};
__device__ __forceinline__ float clip_coef(const AdamClip& c) {
  __shared__ double sm[4];
  const double total = block_sum_256((int)threadIdx.x < c.count ? c.partials[threadIdx.x] : 0.0, sm);
  const double norm = sqrt(total);
  double cd = c.max_norm / (norm + 1e-6);
  if (cd > 1.0) cd = 1.0;  // (a NaN stays)
  const float coef = (float)cd;
  if (blockIdx.x == 0 && threadIdx.x == 0) c.stats[0] = (float)norm, c.stats[1] = coef;
  return coef;
}
__device__ __forceinline__ float clip_one(float g, float coef) {
#pragma clang fp contract(off)
  return coef * g;
}

// CLIP false is the kernel without clipping, instruction for instruction what it was (the gradient const, no LDS);
// CLIP true writes the gradient, and only where the coefficient is not 1: each element by the thread that read it.
// DECAY false is the kernel without weight decay, likewise what it was (`d` is not read); DECAY true multiplies every
// parameter by d before its update, in the vector path and the scalar tail alike.  The float64 rider is never decayed
// (its optimizer is its own); the lerp rider reads the stepped, decayed parameter.
template <bool CLIP>
using AdamGrad = std::conditional_t<CLIP, float, const float>;

template <bool CLIP, bool DECAY>
__global__ void __launch_bounds__(256) adam_step_kernel(float* __restrict__ p, AdamGrad<CLIP>* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, size_t n,
                                                        int vec, float w1, float b2, float w2, float step_size,
                                                        float bc2_sqrt, float eps, AdamScalar64 sc, AdamLerp lp,
                                                        const float* __restrict__ dyn, AdamClip clip, float d) {
  float coef = 1.0f;
  if constexpr (CLIP) coef = clip_coef(clip);
  const bool scale = CLIP && coef != 1.0f;
  // dyn != nullptr: the two step-dependent factors lr / (1 - b1^t) and sqrt(1 - b2^t) come from device memory, written
  // there (by the host, through the update's pinned control block) before the kernel runs: a captured graph is
  // replayed with new step counts.  The same two floats the host would have passed by value.
  if (dyn) step_size = dyn[0], bc2_sqrt = dyn[1];
  if (sc.p && blockIdx.x == 0 && threadIdx.x == 0) {  // torch's single-tensor Adam, in double
#pragma clang fp contract(off)
    if (sc.dyn) sc.step_size = sc.dyn[0], sc.bc2_sqrt = sc.dyn[1];
    const double gs = *sc.g;
    double ms = *sc.m, vs = *sc.v;
    ms = (sc.w1 < 0.5) ? ms + sc.w1 * (gs - ms) : gs - (gs - ms) * (1.0 - sc.w1);
    vs = vs * sc.b2 + (sc.w2 * gs) * gs;
    *sc.m = ms, *sc.v = vs;
    *sc.p = *sc.p - sc.step_size * (ms / (sqrt(vs) / sc.bc2_sqrt + sc.eps));
  }
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (vec) {
    const size_t n4 = n >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
      f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
      if constexpr (CLIP) {
        if (scale) {
#pragma unroll
          for (int e = 0; e < 4; ++e) gg[e] = clip_one(gg[e], coef);
          reinterpret_cast<f32x4*>(g)[i] = gg;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        if constexpr (DECAY) pe = decay_one(pe, d);
        adam_one(pe, gg[e], me, ve, w1, b2, w2, step_size, bc2_sqrt, eps);
        pp[e] = pe, mm[e] = me, vv[e] = ve;
      }
      reinterpret_cast<f32x4*>(p)[i] = pp;
      reinterpret_cast<f32x4*>(m)[i] = mm;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if (lp.tgt) {  // (vec implies target and split are 16-byte granular too: a float4 lies on one side of split)
        f32x4 tt = reinterpret_cast<f32x4*>(lp.tgt)[i];
        const bool a = 4 * i < lp.split;
#pragma unroll
        for (int e = 0; e < 4; ++e) tt[e] = lerp_one(pp[e], tt[e], a ? lp.tau_a : lp.tau_b, a ? lp.omt_a : lp.omt_b);
        reinterpret_cast<f32x4*>(lp.tgt)[i] = tt;
      }
    }
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    float gi = g[i];
    if constexpr (CLIP) {
      if (scale) g[i] = gi = clip_one(gi, coef);
    }
    if constexpr (DECAY) p[i] = decay_one(p[i], d);
    adam_one(p[i], gi, m[i], v[i], w1, b2, w2, step_size, bc2_sqrt, eps);
    if (lp.tgt) lp.tgt[i] = lerp_one(p[i], lp.tgt[i], i < lp.split ? lp.tau_a : lp.tau_b, i < lp.split ? lp.omt_a : lp.omt_b);
  }
}

// Two Adam steps of two optimizers on the SAME parameters with the same gradient, back to back, in one pass (the
// reference steps the encoder with encoder_optimizer and then again with cpc_optimizer, curl_sac.py:418-423): elements
// [0, n_pre) belong to the second optimizer only (CURL.W in front of the encoder in the flat buffer), the rest take
// step 1 then step 2 exactly as the two launches would (the same per-element operation order).  With DECAY each
// optimizer's factor goes in front of its own step, as first.step(); second.step() of two AdamWs: behind n_pre
// p *= d1, Adam 1, p *= d2, Adam 2; the first n_pre elements p *= d2, Adam 2.
struct AdamHyper {
  float w1, b2, w2, step_size, bc2_sqrt, eps;
};
// ... with the optimizer's decay factor (decay_one): what the DECAY kernels take, so that the kernels without weight
// decay keep the arguments -- and with them the code -- they had
struct AdamHyperDecay : AdamHyper {
  float d;
};
template <bool DECAY>
using AdamHyperOf = std::conditional_t<DECAY, AdamHyperDecay, AdamHyper>;

template <bool CLIP, bool DECAY>
__global__ void __launch_bounds__(256) adam_step2_kernel(float* __restrict__ p, AdamGrad<CLIP>* __restrict__ g,
                                                         float* __restrict__ m1, float* __restrict__ v1,
                                                         float* __restrict__ m2, float* __restrict__ v2, size_t n,
                                                         size_t n_pre, int vec, AdamHyperOf<DECAY> h1,
                                                         AdamHyperOf<DECAY> h2,
                                                         const float* __restrict__ dyn, AdamClip clip) {
  // (adam_step_kernel: the gradient is clipped ONCE, over the whole run, and both steps consume the clipped value)
  float coef = 1.0f;
  if constexpr (CLIP) coef = clip_coef(clip);
  const bool scale = CLIP && coef != 1.0f;
  if (dyn) h1.step_size = dyn[0], h1.bc2_sqrt = dyn[1], h2.step_size = dyn[2], h2.bc2_sqrt = dyn[3];  // (adam_step_kernel)
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (vec) {  // everything 16-byte aligned and n_pre a multiple of 4: a float4 lies on one side of n_pre
    const size_t n4 = n >> 2, pre4 = n_pre >> 2;
    for (size_t i = tid; i < n4; i += stride) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
      f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
      if constexpr (CLIP) {
        if (scale) {
#pragma unroll
          for (int e = 0; e < 4; ++e) gg[e] = clip_one(gg[e], coef);
          reinterpret_cast<f32x4*>(g)[i] = gg;
        }
      }
      if (i >= pre4) {
        f32x4 mm = reinterpret_cast<f32x4*>(m1)[i - pre4], vv = reinterpret_cast<f32x4*>(v1)[i - pre4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], me = mm[e], ve = vv[e];
          if constexpr (DECAY) pe = decay_one(pe, h1.d);
          adam_one(pe, gg[e], me, ve, h1.w1, h1.b2, h1.w2, h1.step_size, h1.bc2_sqrt, h1.eps);
          pp[e] = pe, mm[e] = me, vv[e] = ve;
        }
        reinterpret_cast<f32x4*>(m1)[i - pre4] = mm;
        reinterpret_cast<f32x4*>(v1)[i - pre4] = vv;
      }
      f32x4 mm = reinterpret_cast<f32x4*>(m2)[i], vv = reinterpret_cast<f32x4*>(v2)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], me = mm[e], ve = vv[e];
        if constexpr (DECAY) pe = decay_one(pe, h2.d);
        adam_one(pe, gg[e], me, ve, h2.w1, h2.b2, h2.w2, h2.step_size, h2.bc2_sqrt, h2.eps);
        pp[e] = pe, mm[e] = me, vv[e] = ve;
      }
      reinterpret_cast<f32x4*>(m2)[i] = mm;
      reinterpret_cast<f32x4*>(v2)[i] = vv;
      reinterpret_cast<f32x4*>(p)[i] = pp;
    }
    done = n4 << 2;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    float pi = p[i];
    float gi = g[i];
    if constexpr (CLIP) {
      if (scale) g[i] = gi = clip_one(gi, coef);
    }
    if (i >= n_pre) {
      float m = m1[i - n_pre], v = v1[i - n_pre];
      if constexpr (DECAY) pi = decay_one(pi, h1.d);
      adam_one(pi, gi, m, v, h1.w1, h1.b2, h1.w2, h1.step_size, h1.bc2_sqrt, h1.eps);
      m1[i - n_pre] = m, v1[i - n_pre] = v;
    }
    float m = m2[i], v = v2[i];
    if constexpr (DECAY) pi = decay_one(pi, h2.d);
    adam_one(pi, gi, m, v, h2.w1, h2.b2, h2.w2, h2.step_size, h2.bc2_sqrt, h2.eps);
    m2[i] = m, v2[i] = v;
    p[i] = pi;
  }
}
