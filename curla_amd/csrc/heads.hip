// Small fused kernels around the GEMMs: LayerNorm (encoder.py:67,101),
// squashed-Gaussian policy head (curl_sac.py:20-35,87-108), SAC targets and
// losses (curl_sac.py:353-359,378-399), CURL cross-entropy (curl_sac.py:411-413),
// target soft update (utils.py:37-41), the optimiser step, and the replay
// ring's movers: minibatch staging, prioritized replay, frame stores, and the
// crop materialiser for callers that want the reference's float NCHW minibatch
// tensors (utils.py:151-166).
// All reductions are fixed-order (bitwise reproducible run to run).
//
// This file: the host side -- the launch helper, the run-time -> template dispatch that names every instantiation, the
// builders of the kernels' argument blocks, the C ABI (include/curla_hip.h).  The kernels live in the headers included
// in place below, one subject each.
#include "common.h"

#include "f64_rider.h"  // f64_pack_kernel, f64_unpack_kernel: C names, so outside the namespace

namespace {

#include "reduce.h"        // wave_sum, wave_max, block_sum_256; colsum, colsum3, mean and grad_sqsum kernels
#include "layernorm.h"     // fc_ln_fwd_kernel<NF>, ln_bwd_kernel<NF>, ln_param_grad_kernel
#include "mlp_ln.h"        // mlp_ln_relu_fwd_kernel<NF>, mlp_ln_bwd_kernel<NF>, mlp_ln_param_grad_kernel (the critics' LayerNorm)
#include "mlp_drop_ln.h"   // mlp_drop_ln_relu_fwd_kernel<NF>, mlp_drop_ln_bwd_kernel<NF> (DroQ's dropout in front of that LayerNorm)
#include "mlp_out.h"       // mlp_out_fwd_kernel<HEAD, R, LDSW>, mlp_out_bwd_kernel<GEN>, the policy head's three kernels
#include "sac_loss.h"      // concat / split_sum, td_target, critic_loss, critic_td_loss(_views), actor_loss, curl_ce<VIEWS>
#include "tqc.h"           // tqc_critic_loss_kernel, tqc_actor_loss_kernel (truncated quantile critics)
#include "hlgauss.h"       // hlg_critic_loss_kernel<VIEWS>, hlg_actor_rows_kernel, hlg_actor_scalars_kernel (the HL-Gauss critic)
#include "curl_head.h"     // curl_head_kernel<NTILE>
#include "pred_loss.h"     // pred_loss_kernel<NF> (the self-predictive latent loss)
#include "redo.h"          // dormant_colsum_kernel, dormant_mask_kernel, redo_recycle_kernel (dormant-neuron scores, ReDo)
#include "optim.h"         // soft_update_kernel, soft_update2_kernel, shrink_perturb2_kernel, adam_step_kernel<CLIP, DECAY>, adam_step2_kernel<CLIP, DECAY>
#include "sample_stage.h"  // a minibatch's index block and scalars: sample_stage_kernel<HOST, NSTEP, POS>, pos_walk_kernel
#include "ring.h"          // crop_nchw_kernel, store_frame_kernel, gather_stacks_kernel<FAST>, nhwc_to_nchw_kernel
#include "per.h"           // prioritized replay: per_set's three phases, per_sample_kernel, per_td_kernel
#include "stage.h"         // stage_frames_kernel<C>: N planar frames into N ring slots, crop fused (batched acting)
#include "add_vec.h"       // add_vec_kernel<C>: a vector step of N environments into the ring (ReplayBuffer.add_vec)

// ------------------------------ host side ------------------------------
// Every launch of this file: launch, report the launch status.  A kernel's dynamic-LDS limit is NOT touched here: the
// one kernel that needs more than the default 48 KB (curl_head_kernel) raises it in front of its launch, and the LDS
// form of mlp_out_fwd_kernel is chosen only where the weights fit the default.
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), dim3 grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, args...);
  return curla_launch_status();
}

inline int nblocks(size_t n, int bs, int cap = 4096) {
  size_t b = (n + bs - 1) / bs;
  return (int)(b < (size_t)cap ? b : cap);
}

// LayerNorm width F (1 .. 1024, checked by the callers) -> the features a lane holds, NF = ceil(F / 64) rounded up to
// one of the compiled 1, 2, 3, 4, 8, 16; f(std::integral_constant<int, NF>)
template <typename Fn>
int dispatch_ln_width(int F, Fn&& f) {
  const int n = (F + 63) / 64;
  return dispatch_int<1, 2, 3, 4, 8, 16>(n <= 4 ? n : n <= 8 ? 8 : 16, f);
}

// curla_ln_bwd_twin (partial == nullptr) and curla_ln_bwd_partial
int ln_bwd_launch(const float* dy, const float* dy2, int ld_dy, const float* xhat, const float* rstd, const float* gamma,
                  int B, int F, float* dx, float* partial, hipStream_t st) {
  return dispatch_ln_width(F, [&](auto nf) {
    return launch(ln_bwd_kernel<nf()>, dim3((B + 3) / 4), 256, 0, st, dy, dy2, ld_dy, xhat, rstd, gamma, B, F, dx, partial);
  });
}

// The last layer's forward, plain (HEAD false) or with the policy head run by the same launch.  The block stages the N
// weight rows in LDS when there are at least two (one row: a wave reads 4 KB once, nothing to share; the head's 2A
// always are) and they fit the 48 KB a kernel may use without asking.
// (R = 4 rows per wave to share the weight loads was measured for the actor's 8 outputs: 25 us against 14 -- the
// layer is load latency, and 128 waves hide less of it than 512)
template <int HEAD>
int mlp_out_fwd_launch(const float* h, long long sH, long long sH2, const float* W, long long sW, long long sW2,
                       const float* bias, long long sB, long long sB2, float* out, long long sOut, long long sOut2, int M,
                       int N, int K, int nb, int nb2, const HeadArgs& hd, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((M + 3) / 4, nb * nb2);
  const size_t wbytes = (size_t)N * K * sizeof(float);
  if (N >= 2 && wbytes <= 48 * 1024)
    return launch(mlp_out_fwd_kernel<HEAD, 1, true>, grid, 256, wbytes, st, h, sH, sH2, W, sW, sW2, bias, sB, sB2, out, sOut,
                  sOut2, M, N, K, nb, hd);
  return launch(mlp_out_fwd_kernel<HEAD, 1, false>, grid, 256, 0, st, h, sH, sH2, W, sW, sW2, bias, sB, sB2, out, sOut,
                sOut2, M, N, K, nb, hd);
}

int head_args(const float* noise, int B, int A, float log_std_min, float log_std_max, float* mu, float* pi, float* log_pi,
              float* log_std, float* tanh_ls, float* pi_xa, int xa_ld, HeadArgs* hd) {
  CURLA_REQUIRE(B > 0 && A > 0 && A <= kMaxA);
  CURLA_REQUIRE(!noise || pi || pi_xa);
  CURLA_REQUIRE(!pi_xa || (noise && xa_ld >= A));
  hd->noise = noise, hd->mu_t = mu, hd->pi_t = pi, hd->log_pi = log_pi, hd->log_std = log_std, hd->tanh_ls = tanh_ls;
  hd->pi_xa = pi_xa, hd->A = A, hd->xa_ld = xa_ld, hd->lo = log_std_min, hd->hi = log_std_max;
  hd->noise_gen = nullptr, hd->rng_seed = 0, hd->rng_offset = 0, hd->rng_dev = nullptr, hd->std = nullptr, hd->clip = 0.f;
  return CURLA_OK;
}

// the same with the noise drawn inside the kernel (written to noise_out [B][A])
int head_args_rng(float* noise_out, unsigned long long seed, unsigned long long offset, const unsigned long long* rng_dev,
                  int B, int A, float log_std_min, float log_std_max, float* mu, float* pi, float* log_pi, float* log_std,
                  float* tanh_ls, float* pi_xa, int xa_ld, HeadArgs* hd) {
  CURLA_REQUIRE(noise_out && (reinterpret_cast<uintptr_t>(rng_dev) & 7) == 0);
  const int rc = head_args(noise_out, B, A, log_std_min, log_std_max, mu, pi, log_pi, log_std, tanh_ls, pi_xa, xa_ld, hd);
  if (rc != CURLA_OK) return rc;
  hd->noise = nullptr, hd->noise_gen = noise_out, hd->rng_seed = seed, hd->rng_offset = offset, hd->rng_dev = rng_dev;
  return CURLA_OK;
}

// the policy head as a launch of its own (curla_actor_head_fwd, curla_actor_head_fwd_rng)
int actor_head_launch(const float* trunk_out, int B, const HeadArgs& hd, void* stream) {
  return launch(actor_head_fwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), trunk_out, B, hd);
}

// ... and inside the actor trunk's last layer (curla_mlp_out_head_fwd, curla_mlp_out_head_fwd_rng)
int mlp_out_head_launch(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                        const HeadArgs& hd, void* stream) {
  if (2 * A > kMaxOut || K % 4 != 0) return CURLA_ERR_UNSUPPORTED;
  CURLA_REQUIRE(aligned16(h) && aligned16(W));
  return mlp_out_fwd_launch<kHeadGauss>(h, 0LL, 0LL, W, 0LL, 0LL, bias, 0LL, 0LL, trunk_out, 0LL, 0LL, B, 2 * A, K, 1, 1, hd,
                                        stream);
}

// The deterministic head's argument block (curla_det_head_fwd and its three relatives): the Gaussian head's checks, then
// its own -- the device scalar `std` is required, the clip is >= 0 (+inf: none; false for a NaN).  `noise_out` != NULL:
// the draws are made inside the launch (head_args_rng).
int det_head_args(const float* noise, float* noise_out, unsigned long long seed, unsigned long long offset,
                  const unsigned long long* rng_dev, const float* std, float clip, int B, int A, float* mu, float* pi,
                  float* log_pi, float* log_std, float* pi_xa, int xa_ld, HeadArgs* hd) {
  CURLA_REQUIRE(std && (reinterpret_cast<uintptr_t>(std) & 3) == 0 && clip >= 0.f);
  const int rc = noise_out ? head_args_rng(noise_out, seed, offset, rng_dev, B, A, 0.f, 0.f, mu, pi, log_pi, log_std, nullptr,
                                           pi_xa, xa_ld, hd)
                           : head_args(noise, B, A, 0.f, 0.f, mu, pi, log_pi, log_std, nullptr, pi_xa, xa_ld, hd);
  if (rc != CURLA_OK) return rc;
  hd->std = std, hd->clip = clip;
  return CURLA_OK;
}

int det_head_launch(const float* trunk_out, int B, const HeadArgs& hd, void* stream) {
  return launch(det_head_fwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), trunk_out, B, hd);
}

int mlp_out_det_head_launch(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                            const HeadArgs& hd, void* stream) {
  if (K % 4 != 0) return CURLA_ERR_UNSUPPORTED;  // (A <= kMaxA <= kMaxOut has been checked)
  CURLA_REQUIRE(aligned16(h) && aligned16(W));
  return mlp_out_fwd_launch<kHeadDet>(h, 0LL, 0LL, W, 0LL, 0LL, bias, 0LL, 0LL, trunk_out, 0LL, 0LL, B, A, K, 1, 1, hd, stream);
}

// the step-dependent factors evaluated in double, as torch's single-tensor Adam does
AdamHyper adam_hyper(double lr, double beta1, double beta2, double eps, long long step) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  AdamHyper h;
  h.w1 = (float)(1.0 - beta1), h.b2 = (float)beta2, h.w2 = (float)(1.0 - beta2);
  h.step_size = (float)(lr / bc1), h.bc2_sqrt = (float)sqrt(bc2), h.eps = (float)eps;
  return h;
}

// The decay factor of the curla_adamw_* entry points (optim.h decay_one): 1 - lr * weight_decay formed in double and
// rounded to float once, as torch's AdamW forms it (param.mul_(1 - lr * weight_decay)).
float decay_factor(double lr, double weight_decay) { return (float)(1.0 - lr * weight_decay); }
bool weight_decay_ok(double weight_decay) { return weight_decay >= 0. && weight_decay < HUGE_VAL; }  // (false for a NaN)

template <typename... P>
bool float_pointers(const P*... p) {  // none NULL, none off 4 bytes
  return (... && (p != nullptr && (reinterpret_cast<uintptr_t>(p) & 3) == 0));
}

// The clip argument of the curla_adam_step*_clip entry points (optim.h AdamClip), checked: the partials of
// curla_grad_sqsum (doubles, 1 .. CURLA_CLIP_MAX_PARTIALS of them), a positive max_norm (inf allowed), the stats slot.
int clip_args(const double* partials, int n_partials, double max_norm, float* stats, AdamClip* clip) {
  CURLA_REQUIRE(partials && stats && (reinterpret_cast<uintptr_t>(partials) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(stats) & 3) == 0 && n_partials >= 1 && n_partials <= CURLA_CLIP_MAX_PARTIALS &&
                max_norm > 0.);  // (false for a NaN)
  clip->partials = partials, clip->count = n_partials, clip->max_norm = max_norm, clip->stats = stats;
  return CURLA_OK;
}

// The clip argument of the curla_adamw_* entry points: partials == NULL is the unclipped launch (n_partials must then be
// 0; max_norm and stats are not looked at, `grad` is not written), anything else is clip_args'.
int clip_args_or_none(const double* partials, int n_partials, double max_norm, float* stats, AdamClip* clip) {
  if (partials) return clip_args(partials, n_partials, max_norm, stats, clip);
  CURLA_REQUIRE(n_partials == 0);
  *clip = AdamClip{};
  return CURLA_OK;
}

// `grad` is written only by a clipping launch (clip.partials != nullptr): the plain entry points hand in their const
// gradient and an empty clip.  `decay` != nullptr (the curla_adamw_* entry points): the kernels that multiply the
// parameter by *decay first; nullptr: the kernels without weight decay, as they were.
int adam_step_launch(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                     double beta2, double eps, long long step, const float* dyn, const AdamScalar64& sc, void* stream,
                     const AdamLerp& lp = AdamLerp{}, const AdamClip& clip = AdamClip{}, const float* decay = nullptr) {
  CURLA_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1 && beta1 >= 0. && beta1 < 1. &&
                beta2 >= 0. && beta2 < 1. && (reinterpret_cast<uintptr_t>(dyn) & 3) == 0);
  const AdamHyper hy = adam_hyper(lr, beta1, beta2, eps, step);
  const int vec = aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) &&
                  (!lp.tgt || (aligned16(lp.tgt) && lp.split % 4 == 0));
  const dim3 grid(nblocks((n + 3) / 4, 256, 8192));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* cgrad = grad;
  if (decay && clip.partials)
    return launch(adam_step_kernel<true, true>, grid, 256, 0, st, param, grad, exp_avg, exp_avg_sq, n, vec, hy.w1, hy.b2,
                  hy.w2, hy.step_size, hy.bc2_sqrt, hy.eps, sc, lp, dyn, clip, *decay);
  if (decay)
    return launch(adam_step_kernel<false, true>, grid, 256, 0, st, param, cgrad, exp_avg, exp_avg_sq, n, vec, hy.w1, hy.b2,
                  hy.w2, hy.step_size, hy.bc2_sqrt, hy.eps, sc, lp, dyn, clip, *decay);
  if (clip.partials)
    return launch(adam_step_kernel<true, false>, grid, 256, 0, st, param, grad, exp_avg, exp_avg_sq, n, vec, hy.w1, hy.b2,
                  hy.w2, hy.step_size, hy.bc2_sqrt, hy.eps, sc, lp, dyn, clip, 1.0f);
  return launch(adam_step_kernel<false, false>, grid, 256, 0, st, param, cgrad, exp_avg, exp_avg_sq, n, vec, hy.w1, hy.b2,
                hy.w2, hy.step_size, hy.bc2_sqrt, hy.eps, sc, lp, dyn, clip, 1.0f);
}

// curla_adam_step2, curla_adam_step2_clip and (decay != nullptr: the two optimizers' factors, for the kernels that apply
// them) curla_adamw_step2
int adam_step2_launch(float* param, float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2, float* exp_avg_sq2,
                      size_t n, size_t n_pre, const AdamHyper& h1, const AdamHyper& h2, const float* dyn, void* stream,
                      const AdamClip& clip = AdamClip{}, const float* decay = nullptr) {
  const int vec = (n_pre % 4 == 0) && aligned16(param) && aligned16(grad) && aligned16(exp_avg1) &&
                  aligned16(exp_avg_sq1) && aligned16(exp_avg2) && aligned16(exp_avg_sq2);
  const dim3 grid(nblocks((n + 3) / 4, 256, 8192));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* cgrad = grad;
  if (decay) {
    const AdamHyperDecay d1{h1, decay[0]}, d2{h2, decay[1]};
    if (clip.partials)
      return launch(adam_step2_kernel<true, true>, grid, 256, 0, st, param, grad, exp_avg1, exp_avg_sq1, exp_avg2,
                    exp_avg_sq2, n, n_pre, vec, d1, d2, dyn, clip);
    return launch(adam_step2_kernel<false, true>, grid, 256, 0, st, param, cgrad, exp_avg1, exp_avg_sq1, exp_avg2,
                  exp_avg_sq2, n, n_pre, vec, d1, d2, dyn, clip);
  }
  if (clip.partials)
    return launch(adam_step2_kernel<true, false>, grid, 256, 0, st, param, grad, exp_avg1, exp_avg_sq1, exp_avg2,
                  exp_avg_sq2, n, n_pre, vec, h1, h2, dyn, clip);
  return launch(adam_step2_kernel<false, false>, grid, 256, 0, st, param, cgrad, exp_avg1, exp_avg_sq1, exp_avg2,
                exp_avg_sq2, n, n_pre, vec, h1, h2, dyn, clip);
}

// [a, a + na) and [b, b + nb) share no byte
inline bool curla_disjoint(long long a, long long na, long long b, long long nb) { return a + na <= b || b + nb <= a; }

// The geometry of a minibatch's block of `limit` bytes at `host` (NULL: it is on the device already, and `limit` bounds
// its regions) and `dev`: 8-byte aligned, a pinned block shorter than 1 GiB, and the regions a walk writes -- next_row
// (B words), pos_row (2B), pos_run (3B); -1: the block has none -- 8-byte aligned, behind the 2B index words, inside the
// block, none overlapping another (sample_stage.h: walk_owns_word).
bool sample_block_ok(const void* host, const void* dev, long long limit, int B, long long next_row_offset,
                     long long pos_offset, long long run_offset) {
  if (((uintptr_t)host | (uintptr_t)dev) % 8 != 0) return false;
  if (limit % 8 != 0 || limit < 8LL * B || (host && limit >= (1LL << 30))) return false;
  const long long off[3] = {next_row_offset, pos_offset, run_offset}, len[3] = {8LL * B, 16LL * B, 24LL * B};
  for (int i = 0; i < 3; ++i) {
    if (off[i] == -1) continue;
    if (off[i] % 8 != 0 || off[i] < 16LL * B || off[i] + len[i] > limit) return false;
    for (int j = 0; j < i; ++j)
      if (off[j] != -1 && !curla_disjoint(off[i], len[i], off[j], len[j])) return false;
  }
  return true;
}

// One thread per word of the pinned block and per scalar of the minibatch, whichever are more.
int sample_stage_launch(void (*kernel)(SampleStageArgs), const SampleStageArgs& a, void* stream) {
  const int nthreads = a.nwords > a.B * (a.A + 2) ? a.nwords : a.B * (a.A + 2);
  return launch(kernel, dim3((nthreads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), a);
}

// A block offset in bytes as the kernels take it, in words (-1, the block has no such region, stays)
inline int block_word(long long offset) { return offset == -1 ? -1 : (int)(offset / 8); }

// A chain walk's step (the _strided entry points): at least 1, and the lanes tile the ring
inline bool stride_ok(long long capacity, long long stride) {
  return stride >= 1 && capacity >= 1 && capacity % stride == 0;
}

// The arguments every instantiation takes; a block that is on the device already (host_block NULL) has no pinned words
// to copy.  The entry points with a walk add theirs.
SampleStageArgs sample_stage_args(const void* host_block, void* device_block, long long nbytes, const float* scalars,
                                  int B, int A, float* action, float* reward, float* not_done) {
  SampleStageArgs a = {};
  a.host = static_cast<const unsigned long long*>(host_block), a.dev = static_cast<unsigned long long*>(device_block);
  a.nwords = host_block ? (int)(nbytes / 8) : 0;
  a.sc = scalars, a.B = B, a.A = A, a.act = action, a.rew = reward, a.nd = not_done;
  return a;
}

// 4 output pixels per thread, C of 3, 6, 9, 12 (curla_stage_frames_u8 with dword-aligned pointers)
template <int C>
int stage_frames_launch(const uint8_t* nchw, size_t src_bytes, uint8_t* out, uint32_t npix, int Hs, int Ws, int top,
                        int left, int Hd, int Wd, hipStream_t st) {
  const uint32_t groups = (npix + 3) / 4;
  const uint32_t blocks = (groups + 255) / 256;
  return launch(stage_frames_kernel<C>, dim3(blocks < 8192u ? blocks : 8192u), 256, 0, st, nchw, src_bytes, out, npix, Hs,
                Ws, top, left, Hd, Wd);
}

// the dropout arguments of curla_mlp_drop_ln_relu_fwd / _bwd, checked: p in [0, 1), the tags of all `groups` in 1..255
int drop_args(float p, unsigned long long seed, unsigned long long counter, const unsigned long long* rng_dev, int tag,
              int groups, DropArgs* dr) {
  CURLA_REQUIRE(p >= 0.f && p < 1.f && tag >= 1 && tag <= 255 && groups >= 1 && tag + 2LL * (groups - 1) <= 255 &&
                (reinterpret_cast<uintptr_t>(rng_dev) & 7) == 0);  // (p: false for a NaN)
  dr->p = p, dr->scale = 1.0f / (1.0f - p), dr->seed = seed, dr->counter = counter, dr->rng_dev = rng_dev, dr->tag = tag;
  return CURLA_OK;
}

}  // namespace

extern "C" {

int curla_fc_ln_fwd_multi(int njobs, const CurlaFcLnJob* jobs, int nsplit, long long split_stride, int ldp, int B,
                          int F, float eps, int A, void* stream) {
  CURLA_REQUIRE(jobs && njobs > 0 && njobs <= kMaxLnJobs && B > 0 && F > 0 && nsplit > 0 && A >= 0 && A <= 64);
  FcLnJobs js = {};
  for (int i = 0; i < njobs; ++i) {
    const CurlaFcLnJob& j = jobs[i];
    CURLA_REQUIRE(j.partial && j.bias && j.gamma && j.beta && j.y);
    CURLA_REQUIRE(!j.xa || A > 0);
    js.j[i] = j;
  }
  if (F > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_ln_width(F, [&](auto nf) {
    return launch(fc_ln_fwd_kernel<nf()>, dim3((B + 3) / 4, njobs), 256, 0, st, js, nsplit, split_stride, ldp, B, F, eps, A);
  });
}

int curla_fc_ln_fwd(const float* partial, int nsplit, long long split_stride, int ldp, const float* bias,
                    const float* gamma, const float* beta, int B, int F, float eps, float* fc_out, float* y,
                    float* xhat, float* rstd, int tanh_out, float* xa, const float* act, int A, void* stream) {
  CURLA_REQUIRE(!xa || (act && A > 0 && A <= 64));
  CurlaFcLnJob j;
  j.partial = partial, j.bias = bias, j.gamma = gamma, j.beta = beta, j.fc_out = fc_out, j.y = y, j.xhat = xhat;
  j.rstd = rstd, j.xa = xa, j.act = act, j.tanh_out = tanh_out;
  return curla_fc_ln_fwd_multi(1, &j, nsplit, split_stride, ldp, B, F, eps, xa ? A : 0, stream);
}

int curla_ln_bwd_twin(const float* dy, const float* dy2, int ld_dy, const float* xhat, const float* rstd,
                      const float* gamma, int B, int F, float* dx, float* dgamma, float* dbeta, float* dbias_in,
                      void* stream) {
  CURLA_REQUIRE(dy && xhat && rstd && gamma && dx && B > 0 && F > 0 && ld_dy >= F);
  if (F > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CURLA_REQUIRE(!dbias_in || (dgamma && dbeta));
  const int rc = ln_bwd_launch(dy, dy2, ld_dy, xhat, rstd, gamma, B, F, dx, nullptr, st);
  if (rc != CURLA_OK || !(dgamma && dbeta)) return rc;
  return launch(ln_param_grad_kernel, dim3((F + 15) / 16), 1024, 0, st, dy, dy2, ld_dy, xhat, dx, B, F, dgamma, dbeta,
                dbias_in);
}

int curla_ln_bwd_partial(const float* dy, const float* dy2, int ld_dy, const float* xhat, const float* rstd,
                         const float* gamma, int B, int F, float* dx, float* partial, int* nparts, void* stream) {
  CURLA_REQUIRE(dy && xhat && rstd && gamma && dx && partial && nparts && B > 0 && F > 0 && ld_dy >= F);
  if (F > 1024) return CURLA_ERR_UNSUPPORTED;
  const int rc = ln_bwd_launch(dy, dy2, ld_dy, xhat, rstd, gamma, B, F, dx, partial, static_cast<hipStream_t>(stream));
  *nparts = (B + 3) / 4;
  return rc;
}

int curla_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int B, int F, float* dx,
                 float* dgamma, float* dbeta, float* dbias_in, void* stream) {
  return curla_ln_bwd_twin(dy, nullptr, F, xhat, rstd, gamma, B, F, dx, dgamma, dbeta, dbias_in, stream);
}

int curla_mlp_ln_relu_fwd(float* h, long long strideH, long long strideH2, const float* gamma, const float* beta,
                          long long strideP, long long strideP2, float* xhat, float* rstd, int save_first, int B, int H,
                          int nbatch, int nbatch2, float eps, void* stream) {
  CURLA_REQUIRE(h && gamma && beta && B > 0 && H > 0 && nbatch > 0 && nbatch2 > 0);
  CURLA_REQUIRE(!xhat == !rstd && (!xhat || (save_first >= 0 && save_first < nbatch2)));
  if (H > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_ln_width(H, [&](auto nf) {
    return launch(mlp_ln_relu_fwd_kernel<nf()>, dim3((B + 3) / 4, nbatch * nbatch2), 256, 0, st, h, strideH, strideH2, gamma,
                  beta, strideP, strideP2, xhat, rstd, save_first, B, H, nbatch, eps);
  });
}

int curla_mlp_ln_bwd(float* dh, long long strideDh, const float* xhat, const float* rstd, const float* gamma,
                     long long strideP, int B, int H, int nbatch, float* partial, float* dgamma, float* dbeta,
                     float* dbias, long long strideG, void* stream) {
  CURLA_REQUIRE(dh && xhat && rstd && gamma && B > 0 && H > 0 && nbatch > 0);
  const bool params = partial || dgamma || dbeta || dbias;
  CURLA_REQUIRE(!params || (partial && dgamma && dbeta && dbias));
  if (H > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nparts = (B + 3) / 4;
  const int rc = dispatch_ln_width(H, [&](auto nf) {
    return launch(mlp_ln_bwd_kernel<nf()>, dim3(nparts, nbatch), 256, 0, st, dh, strideDh, xhat, rstd, gamma, strideP, B, H,
                  partial);
  });
  if (rc != CURLA_OK || !params) return rc;
  return launch(mlp_ln_param_grad_kernel, dim3((3 * H + 255) / 256, nbatch), 256, 0, st,
                static_cast<const float*>(partial), nparts, H, dgamma, dbeta, dbias, strideG);
}

int curla_mlp_drop_ln_relu_fwd(float* h, long long strideH, long long strideH2, const float* gamma, const float* beta,
                               long long strideP, long long strideP2, float* xhat, float* rstd, int save_first, int B,
                               int H, int nbatch, int nbatch2, float eps, float p, unsigned long long seed,
                               unsigned long long counter, const unsigned long long* rng_dev, int tag, void* stream) {
  CURLA_REQUIRE(h && gamma && beta && B > 0 && H > 0 && nbatch > 0 && nbatch2 > 0);
  CURLA_REQUIRE(!xhat == !rstd && (!xhat || (save_first >= 0 && save_first < nbatch2)));
  DropArgs dr;
  const int rc = drop_args(p, seed, counter, rng_dev, tag, nbatch2, &dr);
  if (rc != CURLA_OK) return rc;
  if (H > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch_ln_width(H, [&](auto nf) {
    return launch(mlp_drop_ln_relu_fwd_kernel<nf()>, dim3((B + 3) / 4, nbatch * nbatch2), 256, 0, st, h, strideH, strideH2,
                  gamma, beta, strideP, strideP2, xhat, rstd, save_first, B, H, nbatch, eps, dr);
  });
}

int curla_mlp_drop_ln_bwd(float* dh, long long strideDh, const float* xhat, const float* rstd, const float* gamma,
                          long long strideP, int B, int H, int nbatch, float* partial, float* dgamma, float* dbeta,
                          float* dbias, long long strideG, float p, unsigned long long seed, unsigned long long counter,
                          const unsigned long long* rng_dev, int tag, void* stream) {
  CURLA_REQUIRE(dh && xhat && rstd && gamma && B > 0 && H > 0 && nbatch > 0);
  const bool params = partial || dgamma || dbeta || dbias;
  CURLA_REQUIRE(!params || (partial && dgamma && dbeta && dbias));
  DropArgs dr;
  int rc = drop_args(p, seed, counter, rng_dev, tag, 1, &dr);
  if (rc != CURLA_OK) return rc;
  if (H > 1024) return CURLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nparts = (B + 3) / 4;
  rc = dispatch_ln_width(H, [&](auto nf) {
    return launch(mlp_drop_ln_bwd_kernel<nf()>, dim3(nparts, nbatch), 256, 0, st, dh, strideDh, xhat, rstd, gamma, strideP,
                  B, H, partial, dr);
  });
  if (rc != CURLA_OK || !params) return rc;
  return launch(mlp_ln_param_grad_kernel, dim3((3 * H + 255) / 256, nbatch), 256, 0, st,
                static_cast<const float*>(partial), nparts, H, dgamma, dbeta, dbias, strideG);
}

int curla_colsum(const float* X, int M, int N, int ldx, long long strideX, float* out, long long strideOut, int nbatch,
                 void* stream) {
  CURLA_REQUIRE(X && out && M > 0 && N > 0 && nbatch > 0);
  return launch(colsum_kernel, dim3((N + 31) / 32, nbatch), 1024, 0, static_cast<hipStream_t>(stream), X, M, N, ldx,
                strideX, out, strideOut);
}

int curla_colsum3(const float* X0, int N0, const float* X1, int N1, const float* X2, int N2, int M, float* out0,
                  float* out1, float* out2, long long strideOut, int nbatch, void* stream) {
  CURLA_REQUIRE(X0 && X1 && X2 && out0 && out1 && out2 && M > 0 && N0 > 0 && N1 > 0 && N2 > 0 && nbatch > 0);
  Colsum3Args a = {};
  a.X[0] = X0, a.X[1] = X1, a.X[2] = X2, a.out[0] = out0, a.out[1] = out1, a.out[2] = out2;
  a.N[0] = N0, a.N[1] = N1, a.N[2] = N2;
  a.sX[0] = (long long)M * N0, a.sX[1] = (long long)M * N1, a.sX[2] = (long long)M * N2;
  const int nmax = N0 > N1 ? (N0 > N2 ? N0 : N2) : (N1 > N2 ? N1 : N2);
  return launch(colsum3_kernel, dim3((nmax + 31) / 32, nbatch, 3), 1024, 0, static_cast<hipStream_t>(stream), a, M,
                strideOut);
}

int curla_mlp_out_fwd(const float* h, long long strideH, const float* W, long long strideW, const float* bias,
                      long long strideBias, float* out, long long strideOut, int M, int N, int K, int nbatch,
                      void* stream) {
  CURLA_REQUIRE(h && W && out && M > 0 && N > 0 && K > 0 && nbatch > 0);
  if (N > kMaxOut || K % 4 != 0 || strideH % 4 != 0 || strideW % 4 != 0) return CURLA_ERR_UNSUPPORTED;
  CURLA_REQUIRE(aligned16(h) && aligned16(W));
  return mlp_out_fwd_launch<0>(h, strideH, 0LL, W, strideW, 0LL, bias, strideBias, 0LL, out, strideOut, 0LL, M, N, K,
                                   nbatch, 1, HeadArgs{}, stream);
}

int curla_mlp_out_fwd_nested(const float* h, long long strideH, long long strideH2, const float* W, long long strideW,
                             long long strideW2, const float* bias, long long strideBias, long long strideBias2,
                             float* out, long long strideOut, long long strideOut2, int M, int N, int K, int nbatch,
                             int nbatch2, void* stream) {
  CURLA_REQUIRE(h && W && out && M > 0 && N > 0 && K > 0 && nbatch > 0 && nbatch2 > 0);
  if (N > kMaxOut || K % 4 != 0 || strideH % 4 != 0 || strideW % 4 != 0 || strideH2 % 4 != 0 || strideW2 % 4 != 0)
    return CURLA_ERR_UNSUPPORTED;
  CURLA_REQUIRE(aligned16(h) && aligned16(W));
  return mlp_out_fwd_launch<0>(h, strideH, strideH2, W, strideW, strideW2, bias, strideBias, strideBias2, out,
                                   strideOut, strideOut2, M, N, K, nbatch, nbatch2, HeadArgs{}, stream);
}

int curla_mlp_out_bwd_bias(const float* dy, long long strideDy, const float* h, long long strideH, const float* W,
                           long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int M, int N,
                           int K, int nbatch, float* db_out, float* db_hidden, long long strideDb, void* stream) {
  CURLA_REQUIRE(dy && h && W && dh && M > 0 && N > 0 && K > 0 && nbatch > 0);
  if (N > kMaxOut) return CURLA_ERR_UNSUPPORTED;
  return launch(mlp_out_bwd_kernel<0>, dim3((K + 15) / 16, nbatch), 1024, 0, static_cast<hipStream_t>(stream), dy, strideDy,
                h, strideH, W, strideW, dh, strideDh, dW, strideDW, M, N, K, db_out, db_hidden, strideDb, LossGen{});
}

int curla_mlp_out_bwd_loss(const CurlaLossArgs* loss, const float* h, long long strideH, const float* W,
                           long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int B, int K,
                           float* db_out, float* db_hidden, long long strideDb, void* stream) {
  CURLA_REQUIRE(loss && h && W && dh && B > 0 && K > 0);
  CURLA_REQUIRE(loss->q && loss->log_pi && loss->log_alpha && loss->scalars && loss->dq && loss->twin_stride >= B);
  LossGen lg = {};
  lg.q = loss->q, lg.tq = loss->target_q_twin, lg.log_pi = loss->log_pi, lg.reward = loss->reward;
  lg.not_done = loss->not_done, lg.log_std = loss->log_std, lg.log_alpha = loss->log_alpha;
  lg.dlog_alpha = loss->dlog_alpha, lg.target_q = loss->target_q, lg.scalars = loss->scalars, lg.dq = loss->dq;
  lg.sTwin = loss->twin_stride, lg.discount = loss->discount, lg.target_entropy = loss->target_entropy, lg.A = loss->A;
  const dim3 grid((K + 15) / 16, 2);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* const no_dy = nullptr;  // (the kernel makes dy from the loss inputs)
  if (loss->kind == 1) {
    CURLA_REQUIRE(loss->target_q_twin && loss->reward && loss->not_done && loss->target_q);
    return launch(mlp_out_bwd_kernel<1>, grid, 1024, 0, st, no_dy, 0LL, h, strideH, W, strideW, dh, strideDh, dW, strideDW,
                  B, 1, K, db_out, db_hidden, strideDb, lg);
  }
  if (loss->kind == 2) {
    CURLA_REQUIRE(loss->log_std && loss->A > 0);
    return launch(mlp_out_bwd_kernel<2>, grid, 1024, 0, st, no_dy, 0LL, h, strideH, W, strideW, dh, strideDh, dW, strideDW,
                  B, 1, K, db_out, db_hidden, strideDb, lg);
  }
  return CURLA_ERR_ARG;
}

int curla_mlp_out_bwd(const float* dy, long long strideDy, const float* h, long long strideH, const float* W,
                      long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int M, int N,
                      int K, int nbatch, void* stream) {
  return curla_mlp_out_bwd_bias(dy, strideDy, h, strideH, W, strideW, dh, strideDh, dW, strideDW, M, N, K, nbatch,
                                nullptr, nullptr, 0, stream);
}

int curla_actor_head_fwd(const float* trunk_out, const float* noise, int B, int A, float log_std_min,
                         float log_std_max, float* mu, float* pi, float* log_pi, float* log_std, float* tanh_ls,
                         float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(trunk_out);
  HeadArgs hd;
  const int rc = head_args(noise, B, A, log_std_min, log_std_max, mu, pi, log_pi, log_std, tanh_ls, pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : actor_head_launch(trunk_out, B, hd, stream);
}

int curla_actor_head_fwd_rng(const float* trunk_out, float* noise_out, unsigned long long seed,
                             unsigned long long offset, const unsigned long long* rng_dev, int B, int A,
                             float log_std_min, float log_std_max, float* mu, float* pi, float* log_pi, float* log_std,
                             float* tanh_ls, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(trunk_out);
  HeadArgs hd;
  const int rc = head_args_rng(noise_out, seed, offset, rng_dev, B, A, log_std_min, log_std_max, mu, pi, log_pi, log_std, tanh_ls,
                               pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : actor_head_launch(trunk_out, B, hd, stream);
}

int curla_mlp_out_head_fwd_rng(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                               float* noise_out, unsigned long long seed, unsigned long long offset,
                               const unsigned long long* rng_dev, float log_std_min, float log_std_max, float* mu,
                               float* pi, float* log_pi, float* log_std, float* tanh_ls, float* pi_xa, int xa_ld,
                               void* stream) {
  CURLA_REQUIRE(h && W && trunk_out && K > 0);
  HeadArgs hd;
  const int rc = head_args_rng(noise_out, seed, offset, rng_dev, B, A, log_std_min, log_std_max, mu, pi, log_pi, log_std, tanh_ls,
                               pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : mlp_out_head_launch(h, W, bias, trunk_out, B, A, K, hd, stream);
}

int curla_mlp_out_head_fwd(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                           const float* noise, float log_std_min, float log_std_max, float* mu, float* pi,
                           float* log_pi, float* log_std, float* tanh_ls, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(h && W && trunk_out && K > 0);
  HeadArgs hd;
  const int rc = head_args(noise, B, A, log_std_min, log_std_max, mu, pi, log_pi, log_std, tanh_ls, pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : mlp_out_head_launch(h, W, bias, trunk_out, B, A, K, hd, stream);
}

int curla_actor_head_bwd(const float* gpi, const float* gpi2, int gpi_ld, const float* glp_rows, const double* log_alpha,
                         float glp_scale, const float* noise, const float* pi, const float* log_std,
                         const float* tanh_ls, int B, int A, float log_std_min, float log_std_max, float* dtrunk_out,
                         void* stream) {
  CURLA_REQUIRE(gpi && noise && pi && log_std && tanh_ls && dtrunk_out && B > 0 && A > 0 && A <= kMaxA && gpi_ld >= A);
  CURLA_REQUIRE(glp_rows || log_alpha);
  return launch(actor_head_bwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), gpi, gpi2, gpi_ld,
                glp_rows, log_alpha, glp_scale, noise, pi, log_std, tanh_ls, B, A, log_std_min, log_std_max, dtrunk_out);
}

int curla_policy_head_bwd(const float* dmu, const float* dpi, const float* dlog_pi, const float* dlog_std,
                          const float* noise, const float* mu, const float* pi, const float* log_std,
                          const float* tanh_ls, int B, int A, float log_std_min, float log_std_max, float* dtrunk_out,
                          void* stream) {
  CURLA_REQUIRE(tanh_ls && dtrunk_out && B > 0 && A > 0 && A <= kMaxA);
  CURLA_REQUIRE(!dmu || mu);
  CURLA_REQUIRE(!(dpi || dlog_pi) || (noise && pi && log_std));
  return launch(policy_head_bwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), dmu, dpi, dlog_pi,
                dlog_std, noise, mu, pi, log_std, tanh_ls, B, A, log_std_min, log_std_max, dtrunk_out);
}

int curla_det_head_fwd(const float* trunk_out, const float* noise, const float* std, float clip, int B, int A, float* mu,
                       float* pi, float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(trunk_out);
  HeadArgs hd;
  const int rc = det_head_args(noise, nullptr, 0, 0, nullptr, std, clip, B, A, mu, pi, log_pi, log_std, pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : det_head_launch(trunk_out, B, hd, stream);
}

int curla_det_head_fwd_rng(const float* trunk_out, float* noise_out, unsigned long long seed, unsigned long long offset,
                           const unsigned long long* rng_dev, const float* std, float clip, int B, int A, float* mu,
                           float* pi, float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(trunk_out && noise_out);
  HeadArgs hd;
  const int rc = det_head_args(nullptr, noise_out, seed, offset, rng_dev, std, clip, B, A, mu, pi, log_pi, log_std, pi_xa,
                               xa_ld, &hd);
  return rc != CURLA_OK ? rc : det_head_launch(trunk_out, B, hd, stream);
}

int curla_mlp_out_det_head_fwd(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                               const float* noise, const float* std, float clip, float* mu, float* pi, float* log_pi,
                               float* log_std, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(h && W && trunk_out && K > 0);
  HeadArgs hd;
  const int rc = det_head_args(noise, nullptr, 0, 0, nullptr, std, clip, B, A, mu, pi, log_pi, log_std, pi_xa, xa_ld, &hd);
  return rc != CURLA_OK ? rc : mlp_out_det_head_launch(h, W, bias, trunk_out, B, A, K, hd, stream);
}

int curla_mlp_out_det_head_fwd_rng(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                                   float* noise_out, unsigned long long seed, unsigned long long offset,
                                   const unsigned long long* rng_dev, const float* std, float clip, float* mu, float* pi,
                                   float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream) {
  CURLA_REQUIRE(h && W && trunk_out && K > 0 && noise_out);
  HeadArgs hd;
  const int rc = det_head_args(nullptr, noise_out, seed, offset, rng_dev, std, clip, B, A, mu, pi, log_pi, log_std, pi_xa,
                               xa_ld, &hd);
  return rc != CURLA_OK ? rc : mlp_out_det_head_launch(h, W, bias, trunk_out, B, A, K, hd, stream);
}

int curla_det_head_bwd(const float* gpi, const float* gpi2, int gpi_ld, const float* mu, int B, int A, float* dtrunk_out,
                       void* stream) {
  CURLA_REQUIRE(gpi && mu && dtrunk_out && B > 0 && A > 0 && A <= kMaxA && gpi_ld >= A);
  return launch(det_head_bwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), gpi, gpi2, gpi_ld, mu,
                B, A, dtrunk_out);
}

int curla_det_policy_head_bwd(const float* dmu, const float* dpi, const float* mu, int B, int A, float* dtrunk_out,
                              void* stream) {
  CURLA_REQUIRE(mu && dtrunk_out && B > 0 && A > 0 && A <= kMaxA);
  return launch(det_policy_head_bwd_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), dmu, dpi, mu, B,
                A, dtrunk_out);
}

int curla_concat(const float* z, const float* act, int B, int F, int A, float* xa, void* stream) {
  CURLA_REQUIRE(z && act && xa && B > 0 && F > 0 && A > 0);
  return launch(concat_kernel, dim3((B * (F + A) + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), z, act, B, F, A,
                xa);
}

int curla_split_sum(const float* dxa, long long twin_stride, int B, int F, int A, float* dz, float* dact,
                    void* stream) {
  CURLA_REQUIRE(dxa && B > 0 && F > 0 && A > 0 && (dz || dact) && twin_stride >= (long long)B * (F + A));
  return launch(split_sum_kernel, dim3((B * (F + A) + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), dxa,
                twin_stride, B, F, A, dz, dact);
}

int curla_td_target(const float* tq, long long twin_stride, const float* log_pi, const float* reward,
                    const float* not_done, const double* log_alpha, float discount, int B, float* target_q,
                    void* stream) {
  CURLA_REQUIRE(tq && log_pi && reward && not_done && log_alpha && target_q && B > 0 && twin_stride >= B);
  return launch(td_target_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), tq, twin_stride, log_pi,
                reward, not_done, log_alpha, discount, B, target_q);
}

int curla_critic_loss(const float* q, long long twin_stride, const float* target_q, int B, float* loss, float* dq,
                      void* stream) {
  CURLA_REQUIRE(q && target_q && loss && dq && B > 0 && twin_stride >= B);
  return launch(critic_loss_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, twin_stride, target_q, B, loss,
                dq);
}

int curla_critic_td_loss(const float* q, const float* tq, long long twin_stride, const float* log_pi,
                         const float* reward, const float* not_done, const double* log_alpha, float discount, int B,
                         float* target_q, float* loss, float* dq, void* stream) {
  CURLA_REQUIRE(q && tq && log_pi && reward && not_done && log_alpha && target_q && loss && dq && B > 0 &&
                twin_stride >= B);
  return launch(critic_td_loss_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, tq, twin_stride, log_pi,
                reward, not_done, log_alpha, discount, B, target_q, loss, dq);
}

int curla_critic_td_loss_views(const float* q, const float* tq, long long twin_stride, const float* log_pi,
                               const float* reward, const float* not_done, const double* log_alpha, float discount,
                               int B, float* target_q, float* loss, float* dq, void* stream) {
  CURLA_REQUIRE(q && tq && log_pi && reward && not_done && log_alpha && target_q && loss && dq && B > 0 && B % 2 == 0 &&
                twin_stride >= B);
  return launch(critic_td_loss_views_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, tq, twin_stride, log_pi,
                reward, not_done, log_alpha, discount, B, target_q, loss, dq);
}

int curla_actor_loss(const float* q, long long twin_stride, const float* log_pi, const float* log_std, int A,
                     const double* log_alpha, float target_entropy, int B, float* scalars4, float* dq,
                     double* dlog_alpha, void* stream) {
  CURLA_REQUIRE(q && log_pi && log_std && log_alpha && scalars4 && dq && B > 0 && A > 0 && twin_stride >= B);
  return launch(actor_loss_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, twin_stride, log_pi, log_std, A,
                log_alpha, target_entropy, B, scalars4, dq, dlog_alpha);
}

int curla_tqc_critic_loss(const float* q, long long q_twin_stride, const float* tq, long long tq_twin_stride,
                          const float* log_pi, const float* reward, const float* not_done, const double* log_alpha,
                          float discount, int B, int M, int d, float* dq, long long dq_twin_stride, float* row_loss,
                          float* loss, void* stream) {
  CURLA_REQUIRE(q && tq && log_pi && reward && not_done && log_alpha && dq && row_loss && B > 0);
  CURLA_REQUIRE(M >= 1 && M <= 32 && d >= 0 && d < M);
  const long long dense = (long long)B * M;
  CURLA_REQUIRE(q_twin_stride >= dense && tq_twin_stride >= dense && dq_twin_stride >= dense);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch(tqc_critic_loss_kernel, dim3((B + 3) / 4), 256, 0, st, q, q_twin_stride, tq, tq_twin_stride,
                        log_pi, reward, not_done, log_alpha, discount, B, M, d, dq, dq_twin_stride, row_loss);
  if (rc != CURLA_OK || !loss) return rc;
  return launch(mean_kernel, dim3(1), 256, 0, st, row_loss, B, loss);  // the fixed-order mean over rows
}

int curla_tqc_actor_loss(const float* q, long long q_twin_stride, const float* log_pi, const float* log_std, int A,
                         const double* log_alpha, float target_entropy, int B, int M, float* scalars4, float* dq,
                         long long dq_twin_stride, double* dlog_alpha, void* stream) {
  CURLA_REQUIRE(q && log_pi && log_std && log_alpha && scalars4 && dq && B > 0 && A > 0 && M >= 1 && M <= 32);
  CURLA_REQUIRE(q_twin_stride >= (long long)B * M && dq_twin_stride >= (long long)B * M);
  return launch(tqc_actor_loss_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, q_twin_stride, log_pi,
                log_std, A, log_alpha, target_entropy, B, M, scalars4, dq, dq_twin_stride, dlog_alpha);
}

int curla_hlg_critic_loss(const float* q, long long q_twin_stride, const float* tq, long long tq_twin_stride,
                          const float* log_pi, const float* reward, const float* not_done, const double* log_alpha,
                          float discount, int B, int M, float v_min, float v_max, float sigma, int views, float* dq,
                          long long dq_twin_stride, float* target_q, float* row_loss, float* loss, void* stream) {
  CURLA_REQUIRE(q && tq && log_pi && reward && not_done && log_alpha && dq && target_q && row_loss && B > 0);
  CURLA_REQUIRE(M >= 2 && M <= kHlgMax && std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max);
  CURLA_REQUIRE(std::isfinite(sigma) && sigma > 0.f && (views == 0 || (views == 1 && B % 2 == 0)));
  const long long dense = (long long)B * M;
  CURLA_REQUIRE(q_twin_stride >= dense && tq_twin_stride >= dense && dq_twin_stride >= dense);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto kernel = views ? hlg_critic_loss_kernel<true> : hlg_critic_loss_kernel<false>;
  const int rc = launch(kernel, dim3((B + 3) / 4), 256, 0, st, q, q_twin_stride, tq, tq_twin_stride, log_pi, reward,
                        not_done, log_alpha, discount, B, M, v_min, v_max, sigma, dq, dq_twin_stride, target_q, row_loss);
  if (rc != CURLA_OK || !loss) return rc;
  // the fixed-order sum over rows, over N = B transitions (B / 2 with views)
  return launch(hlg_row_sum_kernel, dim3(1), 256, 0, st, row_loss, B, 1.f / (float)(views ? B / 2 : B), loss);
}

int curla_hlg_actor_loss(const float* q, long long q_twin_stride, const float* log_pi, const float* log_std, int A,
                         const double* log_alpha, float target_entropy, int B, int M, float v_min, float v_max,
                         float* row_q, float* scalars4, float* dq, long long dq_twin_stride, double* dlog_alpha,
                         void* stream) {
  CURLA_REQUIRE(q && log_pi && log_std && log_alpha && row_q && scalars4 && dq && B > 0 && A > 0);
  CURLA_REQUIRE(M >= 2 && M <= kHlgMax && std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max);
  CURLA_REQUIRE(q_twin_stride >= (long long)B * M && dq_twin_stride >= (long long)B * M);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch(hlg_actor_rows_kernel, dim3((B + 3) / 4), 256, 0, st, q, q_twin_stride, B, M, v_min, v_max, row_q,
                        dq, dq_twin_stride);
  if (rc != CURLA_OK) return rc;
  return launch(hlg_actor_scalars_kernel, dim3(1), 256, 0, st, row_q, log_pi, log_std, A, log_alpha, target_entropy, B,
                scalars4, dlog_alpha);
}

int curla_curl_ce(const float* logits, int B, int ld, float* row_loss, float* loss, float* dlogits, void* stream) {
  CURLA_REQUIRE(logits && row_loss && B > 0 && ld >= B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch(curl_ce_kernel<false>, dim3((B + 3) / 4), 256, 0, st, logits, B, ld, row_loss, dlogits);
  if (rc != CURLA_OK || !loss) return rc;
  return launch(mean_kernel, dim3(1), 256, 0, st, row_loss, B, loss);  // only when it is logged
}

int curla_curl_ce_views(const float* logits, int B, int ld, float* row_loss, float* loss, float* dlogits, void* stream) {
  CURLA_REQUIRE(logits && row_loss && B > 0 && B % 2 == 0 && ld >= B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch(curl_ce_kernel<true>, dim3((B + 3) / 4), 256, 0, st, logits, B, ld, row_loss, dlogits);
  if (rc != CURLA_OK || !loss) return rc;
  return launch(mean_kernel, dim3(1), 256, 0, st, row_loss, B, loss);  // only when it is logged
}

int curla_curl_head(const float* z_a, const float* z_pos, const float* wz, const float* xhat, const float* rstd,
                    const float* gamma, int B, int F, float* row_loss, float* loss, float* dfc, float* ln_partial,
                    int* nparts, float* w_partial, float* logits, float* dlogits, float* dz, void* stream) {
  CURLA_REQUIRE(z_a && z_pos && wz && xhat && rstd && gamma && row_loss && dfc && ln_partial && nparts && w_partial);
  // 128-row multiples (every wave of a block takes whole column tiles), at most 1024 rows (accumulator tiles per wave),
  // 49..52 features (phase A's k per lane group is compiled in: 13)
  if (B <= 0 || B % 128 != 0 || B > 1024 || F <= 4 * kCurlMaxKQ - 4 || F > 4 * kCurlMaxKQ) return CURLA_ERR_UNSUPPORTED;
  CurlHeadArgs a = {};
  a.za = z_a, a.zp = z_pos, a.wz = wz, a.xhat = xhat, a.rstd = rstd, a.gamma = gamma, a.row_loss = row_loss, a.dfc = dfc;
  a.ln_partial = ln_partial, a.w_partial = w_partial, a.logits = logits, a.dlogits = dlogits, a.dz = dz, a.B = B, a.F = F;
  const size_t lds = (size_t)(16 * (B + 4) + 16 * 64 + 2 * 16 * 64 + 2 * 8 * 16 + 16 + 8 * 3 * 64 + 2 * 4 * 16 * 64) * sizeof(float);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // NTILE = B / 128 (1 .. 8 by the check above); 59 .. 115 KB of dynamic LDS: the one kernel of this file whose limit is raised
  int rc = dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(B / 128, [&](auto ntile) {
    if (curla_set_dyn_lds(reinterpret_cast<const void*>(curl_head_kernel<ntile()>), lds) != CURLA_OK) return CURLA_ERR_LAUNCH;
    return launch(curl_head_kernel<ntile()>, dim3(2 * (B / 16)), 512, lds, st, a);
  });
  if (rc != CURLA_OK) return rc;
  if (loss) rc = launch(mean_kernel, dim3(1), 256, 0, st, row_loss, B, loss);  // only when it is logged
  *nparts = B / 16;
  return rc;
}

int curla_pred_loss(const float* p, const float* t, int B, int F, float* row_loss, float* loss, float* dp, void* stream) {
  CURLA_REQUIRE(p && t && row_loss && dp && B > 0 && F >= 1 && F <= 1024);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = dispatch_ln_width(F, [&](auto nf) {
    return launch(pred_loss_kernel<nf()>, dim3((B + 3) / 4), 256, 0, st, p, t, B, F, row_loss, dp);
  });
  if (rc != CURLA_OK || !loss) return rc;
  return launch(mean_kernel, dim3(1), 256, 0, st, row_loss, B, loss);  // the fixed-order mean over rows, where asked for
}

int curla_f64_pack(const double* value, float* words, void* stream) {
  CURLA_REQUIRE(value && words && (reinterpret_cast<uintptr_t>(value) & 7) == 0 && (reinterpret_cast<uintptr_t>(words) & 3) == 0);
  return launch(f64_pack_kernel, dim3(1), 64, 0, static_cast<hipStream_t>(stream), value, words);
}

int curla_f64_unpack(const float* words, double n_mul, double n_div, double* value, void* stream) {
  CURLA_REQUIRE(value && words && n_mul >= 1. && n_div >= 1. && (reinterpret_cast<uintptr_t>(value) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(words) & 3) == 0);
  return launch(f64_unpack_kernel, dim3(1), 64, 0, static_cast<hipStream_t>(stream), words, n_mul, n_div, value);
}

int curla_mean(const float* x, int n, float* out, void* stream) {
  CURLA_REQUIRE(x && out && n > 0);
  return launch(mean_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), x, n, out);
}

int curla_soft_update(const float* param, float* target, size_t n, float tau, float one_minus_tau, void* stream) {
  CURLA_REQUIRE(param && target && n > 0);
  return launch(soft_update_kernel, dim3(nblocks(n, 256)), 256, 0, static_cast<hipStream_t>(stream), param, target, n, tau,
                one_minus_tau);
}

int curla_soft_update2(const float* param, float* target, size_t n, size_t split, float tau_a, float one_minus_tau_a,
                       float tau_b, float one_minus_tau_b, void* stream) {
  CURLA_REQUIRE(param && target && n > 0 && split <= n);
  return launch(soft_update2_kernel, dim3(nblocks(n, 256)), 256, 0, static_cast<hipStream_t>(stream), param, target, n,
                split, tau_a, one_minus_tau_a, tau_b, one_minus_tau_b);
}

int curla_shrink_perturb2(float* param, float* target, const float* fresh, size_t n, size_t split, float keep_a,
                          float new_a, float keep_b, float new_b, void* stream) {
  // (a NaN keep fails both comparisons; the pointers' low bits: floats)
  CURLA_REQUIRE(float_pointers(param, fresh) && (reinterpret_cast<uintptr_t>(target) & 3) == 0 && n > 0 && split <= n &&
                keep_a >= 0.f && keep_a <= 1.f && keep_b >= 0.f && keep_b <= 1.f);
  const int vec = aligned16(param) && aligned16(fresh) && aligned16(target);  // (NULL counts as aligned: not accessed)
  return launch(shrink_perturb2_kernel, dim3(nblocks(vec ? (n + 3) / 4 : n, 256, 8192)), 256, 0,
                static_cast<hipStream_t>(stream), param, target, fresh, n, split, vec, keep_a, new_a, keep_b, new_b);
}

int curla_dormant_colsum(const float* h, long long h_stride, int nb, int B, int H, float* sums, long long sums_stride,
                         void* stream) {
  CURLA_REQUIRE(float_pointers(h, sums) && B >= 1 && H >= 1 && nb >= 1 && h_stride >= (long long)B * H &&
                sums_stride >= H);
  return launch(dormant_colsum_kernel, dim3((H + 63) / 64, nb), 64, 0, static_cast<hipStream_t>(stream), h, h_stride, B, H,
                sums, sums_stride);
}

int curla_dormant_mask(const float* sums, int L, int H, float tau, float* score, int* mask, int* count, float* fraction,
                       void* stream) {
  CURLA_REQUIRE(float_pointers(sums, score, fraction) && float_pointers(mask, count) && L >= 1 && H >= 1 &&
                tau >= 0.f);  // (false for a NaN)
  return launch(dormant_mask_kernel, dim3(L), 256, 0, static_cast<hipStream_t>(stream), sums, H, tau, score, mask, count,
                fraction);
}

int curla_redo_recycle(float* param, float* m, float* v, const float* fresh, long long stride, int nb,
                       const CurlaRedoSeg* segs, int nsegs, const int* mask, int L, int H, int mask_twin, void* stream) {
  CURLA_REQUIRE(float_pointers(param, m, v, fresh) && float_pointers(mask) && segs && nb >= 1 && H >= 1 && L >= 1 &&
                nsegs >= 1 && nsegs <= kMaxRedoSegs && mask_twin >= 0 && (long long)(nb - 1) * mask_twin < L);
  const int top = L - 1 - (nb - 1) * mask_twin;  // the last mask row network 0 may name
  const bool vec = aligned16(param) && aligned16(m) && aligned16(v) && aligned16(fresh) && aligned16(mask) &&
                   (nb == 1 || stride % 4 == 0);
  RedoSegs a = {};
  long long most = 0;
  for (int i = 0; i < nsegs; ++i) {
    const CurlaRedoSeg& s = segs[i];
    CURLA_REQUIRE(s.rows >= 1 && s.cols >= 1 && s.offset >= 0 && s.row_layer >= -1 && s.row_layer <= top &&
                  s.col_layer >= -1 && s.col_layer <= top);
    CURLA_REQUIRE((s.row_layer < 0 || s.rows == H) && (s.col_layer < 0 || s.cols == H));
    const long long count = (long long)s.rows * s.cols;
    CURLA_REQUIRE(nb == 1 || s.offset + count <= stride);
    a.s[i] = RedoSeg{s.offset, s.rows, s.cols, s.row_layer, s.col_layer, vec && s.offset % 4 == 0 && s.cols % 4 == 0};
    const long long work = a.s[i].vec ? count / 4 : count;
    most = work > most ? work : most;
  }
  return launch(redo_recycle_kernel, dim3(nblocks((size_t)most, 256, 1024), nsegs, nb), 256, 0,
                static_cast<hipStream_t>(stream), param, m, v, fresh, stride, a, mask, H, mask_twin);
}

int curla_adam_step_lerp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                         double beta1, double beta2, double eps, long long step, const float* dyn, float* target,
                         size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                         void* stream) {
  CURLA_REQUIRE(target && split <= n);
  AdamScalar64 none = {};
  AdamLerp lp{target, split, tau_a, one_minus_tau_a, tau_b, one_minus_tau_b};
  return adam_step_launch(param, const_cast<float*>(grad), exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none,
                          stream, lp);
}

int curla_adam_step_lerp_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                              double beta1, double beta2, double eps, long long step, const float* dyn, float* target,
                              size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                              const double* partials, int n_partials, double max_norm, float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(float_pointers(param, grad, exp_avg, exp_avg_sq, target) && split <= n);
  AdamScalar64 none = {};
  AdamLerp lp{target, split, tau_a, one_minus_tau_a, tau_b, one_minus_tau_b};
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none, stream, lp, clip);
}

int curla_grad_sqsum(const float* grad, size_t n, double* partials, int n_partials, void* stream) {
  CURLA_REQUIRE(float_pointers(grad) && partials && (reinterpret_cast<uintptr_t>(partials) & 7) == 0 && n > 0 &&
                n_partials >= 1 && n_partials <= CURLA_CLIP_MAX_PARTIALS);
  return launch(grad_sqsum_kernel, dim3(n_partials), 256, 0, static_cast<hipStream_t>(stream), grad, n,
                (int)aligned16(grad), partials);
}

int curla_adam_step_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                         double beta2, double eps, long long step, const float* dyn, const double* partials,
                         int n_partials, double max_norm, float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(float_pointers(param, grad, exp_avg, exp_avg_sq));
  AdamScalar64 none = {};
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none, stream, AdamLerp{},
                          clip);
}

int curla_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                    double beta1, double beta2, double eps, long long step, const float* dyn, void* stream) {
  AdamScalar64 none = {};
  return adam_step_launch(param, const_cast<float*>(grad), exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none,
                          stream);
}

// the float64 rider of curla_adam_step_scalar64 and curla_adam_step_scalar64_clip, checked
int scalar64_args(double* param64, const double* grad64, double* exp_avg64, double* exp_avg_sq64, double lr64,
                  double beta1_64, double beta2_64, double eps64, long long step64, const double* dyn64, AdamScalar64* sc) {
  CURLA_REQUIRE(param64 && grad64 && exp_avg64 && exp_avg_sq64 && step64 >= 1 && beta1_64 >= 0. && beta1_64 < 1. &&
                beta2_64 >= 0. && beta2_64 < 1. && (reinterpret_cast<uintptr_t>(dyn64) & 7) == 0);
  sc->p = param64, sc->g = grad64, sc->m = exp_avg64, sc->v = exp_avg_sq64;
  sc->w1 = 1.0 - beta1_64, sc->b2 = beta2_64, sc->w2 = 1.0 - beta2_64;
  sc->step_size = lr64 / (1.0 - pow(beta1_64, (double)step64));
  sc->bc2_sqrt = sqrt(1.0 - pow(beta2_64, (double)step64)), sc->eps = eps64, sc->dyn = dyn64;
  return CURLA_OK;
}

int curla_adam_step_scalar64(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                             double beta1, double beta2, double eps, long long step, const float* dyn, double* param64,
                             const double* grad64, double* exp_avg64, double* exp_avg_sq64, double lr64, double beta1_64,
                             double beta2_64, double eps64, long long step64, const double* dyn64, void* stream) {
  AdamScalar64 sc;
  const int rc =
      scalar64_args(param64, grad64, exp_avg64, exp_avg_sq64, lr64, beta1_64, beta2_64, eps64, step64, dyn64, &sc);
  if (rc != CURLA_OK) return rc;
  return adam_step_launch(param, const_cast<float*>(grad), exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, sc,
                          stream);
}

int curla_adam_step_scalar64_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                  double beta1, double beta2, double eps, long long step, const float* dyn,
                                  double* param64, const double* grad64, double* exp_avg64, double* exp_avg_sq64,
                                  double lr64, double beta1_64, double beta2_64, double eps64, long long step64,
                                  const double* dyn64, const double* partials, int n_partials, double max_norm,
                                  float* stats, void* stream) {
  AdamClip clip;
  int rc = clip_args(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(float_pointers(param, grad, exp_avg, exp_avg_sq) &&
                ((reinterpret_cast<uintptr_t>(param64) | reinterpret_cast<uintptr_t>(grad64) |
                  reinterpret_cast<uintptr_t>(exp_avg64) | reinterpret_cast<uintptr_t>(exp_avg_sq64)) & 7) == 0);
  AdamScalar64 sc;
  rc = scalar64_args(param64, grad64, exp_avg64, exp_avg_sq64, lr64, beta1_64, beta2_64, eps64, step64, dyn64, &sc);
  if (rc != CURLA_OK) return rc;
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, sc, stream, AdamLerp{},
                          clip);
}

int curla_adam_step2(float* param, const float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2,
                     float* exp_avg_sq2, size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1, double eps1,
                     long long step1, double lr2, double beta1_2, double beta2_2, double eps2, long long step2,
                     const float* dyn, void* stream) {
  CURLA_REQUIRE(param && grad && exp_avg1 && exp_avg_sq1 && exp_avg2 && exp_avg_sq2 && n > 0 && n_pre <= n &&
                step1 >= 1 && step2 >= 1 && (reinterpret_cast<uintptr_t>(dyn) & 3) == 0);
  CURLA_REQUIRE(beta1_1 >= 0. && beta1_1 < 1. && beta2_1 >= 0. && beta2_1 < 1. && beta1_2 >= 0. && beta1_2 < 1. &&
                beta2_2 >= 0. && beta2_2 < 1.);
  return adam_step2_launch(param, const_cast<float*>(grad), exp_avg1, exp_avg_sq1, exp_avg2, exp_avg_sq2, n, n_pre,
                           adam_hyper(lr1, beta1_1, beta2_1, eps1, step1), adam_hyper(lr2, beta1_2, beta2_2, eps2, step2),
                           dyn, stream);
}

int curla_adam_step2_clip(float* param, float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2,
                          float* exp_avg_sq2, size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1,
                          double eps1, long long step1, double lr2, double beta1_2, double beta2_2, double eps2,
                          long long step2, const float* dyn, const double* partials, int n_partials, double max_norm,
                          float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(float_pointers(param, grad, exp_avg1, exp_avg_sq1, exp_avg2, exp_avg_sq2) && n > 0 && n_pre <= n &&
                step1 >= 1 && step2 >= 1 && (reinterpret_cast<uintptr_t>(dyn) & 3) == 0);
  CURLA_REQUIRE(beta1_1 >= 0. && beta1_1 < 1. && beta2_1 >= 0. && beta2_1 < 1. && beta1_2 >= 0. && beta1_2 < 1. &&
                beta2_2 >= 0. && beta2_2 < 1.);
  return adam_step2_launch(param, grad, exp_avg1, exp_avg_sq1, exp_avg2, exp_avg_sq2, n, n_pre,
                           adam_hyper(lr1, beta1_1, beta2_1, eps1, step1), adam_hyper(lr2, beta1_2, beta2_2, eps2, step2),
                           dyn, stream, clip);
}

// Decoupled weight decay (AdamW): the _clip namesakes with a `weight_decay` behind each `eps` of the flat run; partials
// == NULL is the unclipped launch.
int curla_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                     double beta2, double eps, double weight_decay, long long step, const float* dyn,
                     const double* partials, int n_partials, double max_norm, float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args_or_none(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(weight_decay_ok(weight_decay) && float_pointers(param, grad, exp_avg, exp_avg_sq));
  AdamScalar64 none = {};
  const float d = decay_factor(lr, weight_decay);
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none, stream, AdamLerp{},
                          clip, &d);
}

int curla_adamw_step_lerp(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                          double beta2, double eps, double weight_decay, long long step, const float* dyn, float* target,
                          size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                          const double* partials, int n_partials, double max_norm, float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args_or_none(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(weight_decay_ok(weight_decay) && float_pointers(param, grad, exp_avg, exp_avg_sq, target) && split <= n);
  AdamScalar64 none = {};
  AdamLerp lp{target, split, tau_a, one_minus_tau_a, tau_b, one_minus_tau_b};
  const float d = decay_factor(lr, weight_decay);
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, none, stream, lp, clip, &d);
}

int curla_adamw_step_scalar64(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                              double beta1, double beta2, double eps, double weight_decay, long long step,
                              const float* dyn, double* param64, const double* grad64, double* exp_avg64,
                              double* exp_avg_sq64, double lr64, double beta1_64, double beta2_64, double eps64,
                              long long step64, const double* dyn64, const double* partials, int n_partials,
                              double max_norm, float* stats, void* stream) {
  AdamClip clip;
  int rc = clip_args_or_none(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(weight_decay_ok(weight_decay) && float_pointers(param, grad, exp_avg, exp_avg_sq) &&
                ((reinterpret_cast<uintptr_t>(param64) | reinterpret_cast<uintptr_t>(grad64) |
                  reinterpret_cast<uintptr_t>(exp_avg64) | reinterpret_cast<uintptr_t>(exp_avg_sq64)) & 7) == 0);
  AdamScalar64 sc;
  rc = scalar64_args(param64, grad64, exp_avg64, exp_avg_sq64, lr64, beta1_64, beta2_64, eps64, step64, dyn64, &sc);
  if (rc != CURLA_OK) return rc;
  const float d = decay_factor(lr, weight_decay);  // (the flat run's: the scalar is never decayed)
  return adam_step_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, dyn, sc, stream, AdamLerp{},
                          clip, &d);
}

int curla_adamw_step2(float* param, float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2, float* exp_avg_sq2,
                      size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1, double eps1,
                      double weight_decay1, long long step1, double lr2, double beta1_2, double beta2_2, double eps2,
                      double weight_decay2, long long step2, const float* dyn, const double* partials, int n_partials,
                      double max_norm, float* stats, void* stream) {
  AdamClip clip;
  const int rc = clip_args_or_none(partials, n_partials, max_norm, stats, &clip);
  if (rc != CURLA_OK) return rc;
  CURLA_REQUIRE(weight_decay_ok(weight_decay1) && weight_decay_ok(weight_decay2) &&
                float_pointers(param, grad, exp_avg1, exp_avg_sq1, exp_avg2, exp_avg_sq2) && n > 0 && n_pre <= n &&
                step1 >= 1 && step2 >= 1 && (reinterpret_cast<uintptr_t>(dyn) & 3) == 0);
  CURLA_REQUIRE(beta1_1 >= 0. && beta1_1 < 1. && beta2_1 >= 0. && beta2_1 < 1. && beta1_2 >= 0. && beta1_2 < 1. &&
                beta2_2 >= 0. && beta2_2 < 1.);
  const float d[2] = {decay_factor(lr1, weight_decay1), decay_factor(lr2, weight_decay2)};
  return adam_step2_launch(param, grad, exp_avg1, exp_avg_sq1, exp_avg2, exp_avg_sq2, n, n_pre,
                           adam_hyper(lr1, beta1_1, beta2_1, eps1, step1), adam_hyper(lr2, beta1_2, beta2_2, eps2, step2),
                           dyn, stream, clip, d);
}

int curla_host_device_pointer(void* host, void** device) {
  CURLA_REQUIRE(host && device);
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess || !d) {
    (void)hipGetLastError();
    return CURLA_ERR_ARG;
  }
  *device = d;
  return CURLA_OK;
}

// `idx` need not be the start of a block (nor 8-byte aligned): it is the device block's word 0, which is all this
// instantiation reads, so there is no geometry to check.
int curla_gather_transition_scalars(const float* scalars, const int64_t* idx, int B, int A, float* action, float* reward,
                                    float* not_done, void* stream) {
  CURLA_REQUIRE(scalars && idx && action && reward && not_done && B > 0 && A > 0);
  return sample_stage_launch(
      sample_stage_kernel<false, false, false>,
      sample_stage_args(nullptr, const_cast<int64_t*>(idx), 0, scalars, B, A, action, reward, not_done), stream);
}

int curla_sample_stage(const void* host_block, void* device_block, long long nbytes, const float* scalars, int B, int A,
                       float* action, float* reward, float* not_done, void* stream) {
  CURLA_REQUIRE(host_block && device_block && scalars && action && reward && not_done && B > 0 && A > 0);
  CURLA_REQUIRE(sample_block_ok(host_block, device_block, nbytes, B, -1, -1, -1));
  return sample_stage_launch(
      sample_stage_kernel<true, false, false>,
      sample_stage_args(host_block, device_block, nbytes, scalars, B, A, action, reward, not_done), stream);
}

int curla_nstep_compose_strided(void* device_block, long long next_row_offset, const float* scalars, const uint8_t* cont,
                                long long capacity, long long stride, int n, float discount, int B, int A, float* action,
                                float* reward, float* not_done, void* stream) {
  CURLA_REQUIRE(device_block && scalars && cont && action && reward && not_done && B > 0 && A > 0);
  CURLA_REQUIRE(n >= 1 && stride_ok(capacity, stride) && next_row_offset != -1);
  // this entry point holds the START of next_row below 1 GiB, the others the end of every region
  CURLA_REQUIRE(sample_block_ok(nullptr, device_block, (1LL << 30) - 8 + 8LL * B, B, next_row_offset, -1, -1));
  SampleStageArgs a = sample_stage_args(nullptr, device_block, 0, scalars, B, A, action, reward, not_done);
  a.nr_word = block_word(next_row_offset), a.cont = cont, a.capacity = capacity, a.stride = stride, a.n = n;
  a.gamma = discount;
  return sample_stage_launch(sample_stage_kernel<false, true, false>, a, stream);
}

int curla_nstep_compose(void* device_block, long long next_row_offset, const float* scalars, const uint8_t* cont,
                        long long capacity, int n, float discount, int B, int A, float* action, float* reward,
                        float* not_done, void* stream) {
  return curla_nstep_compose_strided(device_block, next_row_offset, scalars, cont, capacity, 1, n, discount, B, A, action,
                                     reward, not_done, stream);
}

int curla_sample_stage_nstep_strided(const void* host_block, void* device_block, long long nbytes,
                                     long long next_row_offset, const float* scalars, const uint8_t* cont,
                                     long long capacity, long long stride, int n, float discount, int B, int A,
                                     float* action, float* reward, float* not_done, void* stream) {
  CURLA_REQUIRE(host_block && device_block && scalars && cont && action && reward && not_done && B > 0 && A > 0);
  CURLA_REQUIRE(n >= 1 && stride_ok(capacity, stride) && next_row_offset != -1);
  CURLA_REQUIRE(sample_block_ok(host_block, device_block, nbytes, B, next_row_offset, -1, -1));
  SampleStageArgs a = sample_stage_args(host_block, device_block, nbytes, scalars, B, A, action, reward, not_done);
  a.nr_word = block_word(next_row_offset), a.cont = cont, a.capacity = capacity, a.stride = stride, a.n = n;
  a.gamma = discount;
  return sample_stage_launch(sample_stage_kernel<true, true, false>, a, stream);
}

int curla_sample_stage_nstep(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                             const float* scalars, const uint8_t* cont, long long capacity, int n, float discount, int B,
                             int A, float* action, float* reward, float* not_done, void* stream) {
  return curla_sample_stage_nstep_strided(host_block, device_block, nbytes, next_row_offset, scalars, cont, capacity, 1, n,
                                          discount, B, A, action, reward, not_done, stream);
}

int curla_pos_walk_strided(void* device_block, long long pos_offset, long long run_offset, long long next_row_offset,
                           const uint8_t* cont, long long capacity, long long stride, int k, int n, int B, void* stream) {
  CURLA_REQUIRE(device_block && B > 0 && k >= 1 && n >= 1 && stride_ok(capacity, stride) && pos_offset != -1);
  CURLA_REQUIRE(cont || (k == 1 && (n == 1 || run_offset == -1)));
  CURLA_REQUIRE(sample_block_ok(nullptr, device_block, 1LL << 30, B, next_row_offset, pos_offset, run_offset));
  return launch(pos_walk_kernel, dim3((B + 255) / 256), 256, 0, static_cast<hipStream_t>(stream),
                static_cast<unsigned long long*>(device_block), block_word(pos_offset), block_word(run_offset), cont,
                capacity, stride, k, n, B);
}

int curla_pos_walk(void* device_block, long long pos_offset, long long run_offset, long long next_row_offset,
                   const uint8_t* cont, long long capacity, int k, int n, int B, void* stream) {
  return curla_pos_walk_strided(device_block, pos_offset, run_offset, next_row_offset, cont, capacity, 1, k, n, B, stream);
}

int curla_sample_stage_pos_strided(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                                   long long pos_offset, long long run_offset, const float* scalars, const uint8_t* cont,
                                   long long capacity, long long stride, int n, float discount, int k, int B, int A,
                                   float* action, float* reward, float* not_done, void* stream) {
  CURLA_REQUIRE(host_block && device_block && scalars && action && reward && not_done && B > 0 && A > 0);
  CURLA_REQUIRE(k >= 1 && n >= 1 && stride_ok(capacity, stride) && pos_offset != -1);
  CURLA_REQUIRE(next_row_offset != -1 || n == 1);  // without a next_row region there is no composition
  CURLA_REQUIRE(cont || (k == 1 && n == 1));
  CURLA_REQUIRE(sample_block_ok(host_block, device_block, nbytes, B, next_row_offset, pos_offset, run_offset));
  SampleStageArgs a = sample_stage_args(host_block, device_block, nbytes, scalars, B, A, action, reward, not_done);
  a.nr_word = block_word(next_row_offset), a.pos_word = block_word(pos_offset), a.run_word = block_word(run_offset);
  a.cont = cont, a.capacity = capacity, a.stride = stride, a.n = n, a.gamma = discount, a.k = k;
  return sample_stage_launch(
      next_row_offset == -1 ? sample_stage_kernel<true, false, true> : sample_stage_kernel<true, true, true>, a, stream);
}

int curla_sample_stage_pos(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                           long long pos_offset, long long run_offset, const float* scalars, const uint8_t* cont,
                           long long capacity, int n, float discount, int k, int B, int A, float* action, float* reward,
                           float* not_done, void* stream) {
  return curla_sample_stage_pos_strided(host_block, device_block, nbytes, next_row_offset, pos_offset, run_offset, scalars,
                                        cont, capacity, 1, n, discount, k, B, A, action, reward, not_done, stream);
}

int curla_per_set(float* s, double* sums, float* vmax, long long capacity, const int64_t* rows, long long first_row,
                  const float* values, int n, void* stream) {
  CURLA_REQUIRE(s && sums && vmax && n >= 1 && capacity >= 1);
  CURLA_REQUIRE((((uintptr_t)s | (uintptr_t)vmax | (uintptr_t)values) & 3) == 0 && (((uintptr_t)sums | (uintptr_t)rows) & 7) == 0);
  CURLA_REQUIRE(rows || (first_row >= 0 && first_row < capacity));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((n + 255) / 256);
  int rc = CURLA_OK;
  if (values && (rc = launch(per_clear_kernel, grid, 256, 0, st, s, rows, first_row, capacity, n)) != CURLA_OK) return rc;
  if ((rc = launch(per_write_kernel, grid, 256, 0, st, s, vmax, rows, first_row, capacity, values, n)) != CURLA_OK) return rc;
  return launch(per_resum_kernel, dim3((n + 3) / 4), 256, 0, st, s, sums, rows, first_row, capacity, n);
}

int curla_per_sample(const float* s, const double* sums, long long capacity, void* device_block, long long u_offset,
                     long long prob_offset, int B, void* stream) {
  CURLA_REQUIRE(s && sums && device_block && B >= 1 && capacity >= 1);
  CURLA_REQUIRE(((uintptr_t)s & 3) == 0 && (((uintptr_t)sums | (uintptr_t)device_block) & 7) == 0);
  CURLA_REQUIRE(u_offset % 8 == 0 && prob_offset % 4 == 0 && u_offset >= 16LL * B && prob_offset >= 16LL * B);
  CURLA_REQUIRE(u_offset < (1LL << 30) && prob_offset < (1LL << 30));
  CURLA_REQUIRE(u_offset + 8LL * B <= prob_offset || prob_offset + 4LL * B <= u_offset);
  return launch(per_sample_kernel, dim3(B), 256, 0, static_cast<hipStream_t>(stream), s, sums, capacity,
                static_cast<unsigned long long*>(device_block), (int)(u_offset / 8), (int)(prob_offset / 4), B);
}

int curla_per_td(const float* q, long long twin_stride, const float* target_q, const float* prob, float beta, float eps,
                 float alpha, int B, float* dq, float* loss, float* w, float* value, void* stream) {
  CURLA_REQUIRE(q && target_q && prob && dq && loss && w && value && B >= 1 && twin_stride >= B);
  CURLA_REQUIRE((((uintptr_t)q | (uintptr_t)target_q | (uintptr_t)prob | (uintptr_t)dq | (uintptr_t)loss | (uintptr_t)w |
                  (uintptr_t)value) & 3) == 0);
  CURLA_REQUIRE(beta >= 0.f && beta <= 1.f && eps > 0.f && alpha >= 0.f);
  return launch(per_td_kernel, dim3(1), 256, 0, static_cast<hipStream_t>(stream), q, twin_stride, target_q, prob, beta, eps,
                alpha, B, dq, loss, w, value);
}

int curla_crop_nchw(const uint8_t* frames, const int64_t* idx, const int32_t* h1, const int32_t* w1, int B, int C,
                    int Hs, int Ws, int Hc, int Wc, float* out_f32, uint8_t* out_u8, void* stream) {
  CURLA_REQUIRE(frames && (out_f32 || out_u8) && B > 0 && C > 0 && Hc > 0 && Wc > 0 && Hs >= Hc && Ws >= Wc);
  return launch(crop_nchw_kernel, dim3(nblocks((size_t)B * C * Hc * Wc, 256)), 256, 0, static_cast<hipStream_t>(stream),
                frames, idx, h1, w1, B, C, Hs, Ws, Hc, Wc, out_f32, out_u8);
}

int curla_store_frame(const uint8_t* chw, uint8_t* frames, long long slot, int C, int H, int W, void* stream) {
  CURLA_REQUIRE(chw && frames && slot >= 0 && C > 0 && H > 0 && W > 0);
  return launch(store_frame_kernel, dim3(nblocks((size_t)C * H * W, 256, 256)), 256, 0, static_cast<hipStream_t>(stream),
                chw, frames, (int64_t)slot, C, H, W);
}

int curla_stage_frames_u8(const uint8_t* nchw, uint8_t* frames, long long first_slot, int N, int C, int Hs, int Ws,
                          int top, int left, int Hd, int Wd, void* stream) {
  CURLA_REQUIRE(nchw && frames && first_slot >= 0 && N >= 1 && C >= 1 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0);
  CURLA_REQUIRE(top >= 0 && left >= 0 && (long long)top + Hd <= Hs && (long long)left + Wd <= Ws);
  const size_t npix = (size_t)N * Hd * Wd, slot = (size_t)Hd * Wd * C;
  CURLA_REQUIRE(npix < (1ull << 31));  // (the kernels number the output pixels in 32 bits)
  const size_t src_bytes = (size_t)N * C * Hs * Ws;
  uint8_t* out = frames + (size_t)first_slot * slot;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool words = ((reinterpret_cast<uintptr_t>(nchw) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
  const uint32_t np = (uint32_t)npix;
  if (words && C == 3) return stage_frames_launch<3>(nchw, src_bytes, out, np, Hs, Ws, top, left, Hd, Wd, st);
  if (words && C == 6) return stage_frames_launch<6>(nchw, src_bytes, out, np, Hs, Ws, top, left, Hd, Wd, st);
  if (words && C == 9) return stage_frames_launch<9>(nchw, src_bytes, out, np, Hs, Ws, top, left, Hd, Wd, st);
  if (words && C == 12) return stage_frames_launch<12>(nchw, src_bytes, out, np, Hs, Ws, top, left, Hd, Wd, st);
  // other channel counts, pointers off a dword boundary: the same bytes one by one
  return launch(stage_frames_bytes_kernel, dim3(nblocks(npix * C, 256, 8192)), 256, 0, st, nchw, out, npix * C, C, Hs, Ws,
                top, left, Hd, Wd);
}

int curla_add_vec(const uint8_t* block, uint8_t* obs_ring, uint8_t* next_ring, float* scalars, uint8_t* cont,
                  long long capacity, long long first, int has_prev, int N, int C, int H, int W, int A, void* stream) {
  CURLA_REQUIRE(block && obs_ring && next_ring && scalars && N >= 1 && C >= 1 && H > 0 && W > 0 && A > 0);
  CURLA_REQUIRE(capacity >= 1 && capacity % N == 0 && first >= 0 && first % N == 0 && first + N <= capacity);
  CURLA_REQUIRE(!has_prev || (cont && capacity > N));  // (capacity == N: the previous run IS the new one)
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(block) | reinterpret_cast<uintptr_t>(scalars)) & 3) == 0);
  const size_t HW = (size_t)H * W;
  CURLA_REQUIRE(2 * (size_t)N * HW < (1ull << 31));  // (the groups number the staged pixels in 32 bits)
  AddVecArgs a = {};
  a.block = block, a.obs = obs_ring, a.next = next_ring, a.sc = scalars, a.cont = cont, a.first = first;
  a.prev = !has_prev ? -1 : first >= N ? first - N : capacity - N;
  a.N = N, a.C = C, a.H = H, a.W = W, a.A = A;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t tail = (size_t)N * (A + 2) + 2 * (size_t)N;
  // whole 4-pixel groups per frame and dword-aligned rows on both rings: the transpose in registers
  const bool words = HW % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(obs_ring) | reinterpret_cast<uintptr_t>(next_ring)) & 3) == 0;
  const dim3 grid(nblocks((words ? 2 * N * HW / 4 : 2 * N * HW * C) + tail, 256, 8192));
  if (words && C == 3) return launch(add_vec_kernel<3>, grid, 256, 0, st, a);
  if (words && C == 6) return launch(add_vec_kernel<6>, grid, 256, 0, st, a);
  if (words && C == 9) return launch(add_vec_kernel<9>, grid, 256, 0, st, a);
  if (words && C == 12) return launch(add_vec_kernel<12>, grid, 256, 0, st, a);
  // other channel counts, frames that are no whole number of groups, rings off a dword boundary: byte by byte
  return launch(add_vec_kernel<ADD_VEC_BYTES>, grid, 256, 0, st, a);
}

int curla_gather_stacks(const uint8_t* store, const int32_t* fid, int fid_stride, const int64_t* idx, int B, int K,
                        int H, int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(store && fid && out && B > 0 && K > 0 && H > 0 && W > 0 && fid_stride >= K);
  const int HW = H * W;
  const size_t n = (size_t)B * ((HW + 3) / 4);
  const bool fast = K <= 4 && HW % 4 == 0 && (reinterpret_cast<uintptr_t>(store) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  return launch(fast ? gather_stacks_kernel<true> : gather_stacks_kernel<false>, dim3(nblocks(n, 256, 8192)), 256, 0,
                static_cast<hipStream_t>(stream), store, fid, fid_stride, idx, B, K, HW, out);
}

int curla_nhwc_to_nchw(const float* in, float* out, int B, int H, int W, int C, void* stream) {
  CURLA_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && C > 0);
  return launch(nhwc_to_nchw_kernel, dim3(nblocks((size_t)B * H * W * C, 256)), 256, 0, static_cast<hipStream_t>(stream),
                in, out, B, H, W, C);
}

const char* curla_version(void) { return "curla_hip 0.8 (gfx950, abi 8)"; }

int curla_abi_version(void) { return CURLA_ABI_VERSION; }

}  // extern "C"
