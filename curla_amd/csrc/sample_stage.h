// Staging a minibatch: its index block to the device and the sampled transitions' scalars out of the ring, with the
// n-step composition and the temporal positive's walk beside them.  Included by heads.hip inside its anonymous
// namespace, in front of the other replay / ring kernels (ring.h, per.h, stage.h).
//
// One kernel template, sample_stage_kernel<HOST, NSTEP, POS>, behind six entry points (curla_hip.h):
//   <0,0,0> curla_gather_transition_scalars     <1,0,0> curla_sample_stage
//   <0,1,0> curla_nstep_compose                 <1,1,0> curla_sample_stage_nstep
//   <1,0,1>, <1,1,1> curla_sample_stage_pos (without / with a next_row region)
// The four that walk also have a _strided form (the walks step by `stride` rows: ReplayBuffer(n_envs=N) keeps each
// environment in a lane of stride N); the namesakes are those with stride 1.
// HOST: the block (indices, crop offsets; ~20 KB) is read from pinned host memory over PCIe with system-scope loads and
// written to its device slot by the same launch -- no copy-engine transfer (and its queue hand-over, ~15 us of idle
// stream) in front of every update; otherwise the block is on the device already.  NSTEP: the reward is the n-step
// return.  POS: the positive's rows are walked.  curla_pos_walk, the walk alone on a device block, keeps a kernel of its
// own (pos_walk_kernel: one thread per sample, no scalars).
#pragma once

// The row `stride` behind ring row r, modulo capacity (0 <= r < capacity, 1 <= stride <= capacity): the next row of r's
// lane.  stride 1 is the single-environment ring; a buffer of N environments keeps lane e in rows e, e + N, ...
__device__ __forceinline__ long long next_in_lane(long long r, long long stride, long long capacity) {
  r += stride;
  return r >= capacity ? r - capacity : r;
}

// n-step return of sample b, which starts at ring row r0 (beyond the reference; DrQ-v2's multi-step TD target): walk
// forward while the continuity flag of the current row is set, at most n - 1 times,
//   R = reward[r0]; g = 1;  per step: r = (r + stride) % capacity; g = g * gamma; R = R + g * reward[r]
// in fp32 with every product and sum rounded on its own (contraction is switched off for this function -- hipcc's
// default would fuse g * reward into the sum, and HIP's __fmul_rn / __fadd_rn are plain operators that fuse as well:
// the NumPy restatement of the tests gives the same bits).  Hands the TD kernels reward = R and
// not_done = not_done[r_last] * g, and the bootstrap row r_last twice: as capacity + r_last in word B + b of the block
// (the double ring's next_obs half) and as r_last in next_row[b].
__device__ __forceinline__ void nstep_compose_one(const float* sc, const uint8_t* cont, long long capacity,
                                                  long long stride, int n, float gamma, int A, long long r0, int b, int B,
                                                  unsigned long long* dev, unsigned long long* next_row, float* rew,
                                                  float* nd) {
#pragma clang fp contract(off)
  const size_t ld = (size_t)A + 2;
  float R = sc[(size_t)r0 * ld + A], g = 1.f;
  long long r = r0;
  for (int m = 1; m < n && cont[r]; ++m) {
    r = next_in_lane(r, stride, capacity);
    g = g * gamma;
    const float term = g * sc[(size_t)r * ld + A];
    R = R + term;
  }
  rew[b] = R;
  nd[b] = sc[(size_t)r * ld + A + 1] * g;
  dev[B + b] = (unsigned long long)(capacity + r);
  next_row[b] = (unsigned long long)r;
}

// Ring row r0 advanced along the continuity flags at most `steps` times (steps == 0 reads no flag): the row walk of
// nstep_compose_one without its arithmetic.
__device__ __forceinline__ long long chain_walk(const uint8_t* cont, long long capacity, long long stride, long long r0,
                                                int steps) {
  long long r = r0;
  for (int m = 0; m < steps && cont[r]; ++m) r = next_in_lane(r, stride, capacity);
  return r;
}

// Temporal positive of sample b, which starts at ring row r0 (beyond the reference; the positive selection of ATC,
// Stooke et al. 2021): the positive is next_obs of row r = r0 walked k - 1 links, i.e. the observation min(k, steps the
// chain still has) steps after obs[r0].  Written twice into pos[0 .. 2B): r in word b, capacity + r (the double ring's
// next_obs half) in word B + b.  `run` (or NULL): int64 [3B] = obs | next_obs | pos rows of the double ring for ONE
// launch of a scratch augmentation -- r0, capacity + (r0 walked n - 1 links: the n-step bootstrap row, walked again
// here so that no word of the block is read that another thread of the launch writes), capacity + r.
__device__ __forceinline__ void temporal_pos_one(const uint8_t* cont, long long capacity, long long stride, int k, int n,
                                                 long long r0, int b, int B, unsigned long long* pos,
                                                 unsigned long long* run) {
  const long long r = chain_walk(cont, capacity, stride, r0, k - 1);
  pos[b] = (unsigned long long)r;
  pos[B + b] = (unsigned long long)(capacity + r);
  if (run) {
    run[b] = (unsigned long long)r0;
    run[B + b] = (unsigned long long)(capacity + chain_walk(cont, capacity, stride, r0, n - 1));
    run[2 * B + b] = (unsigned long long)(capacity + r);
  }
}

// The walk on a block that is already on the device (idx = its first B words): one thread per sample.
__global__ void pos_walk_kernel(unsigned long long* dev, int pos_word, int run_word, const uint8_t* cont,
                                long long capacity, long long stride, int k, int n, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  temporal_pos_one(cont, capacity, stride, k, n, (long long)dev[b], b, B, dev + pos_word,
                   run_word >= 0 ? dev + run_word : nullptr);
}

// The block as 8-byte words; idx = its first B words, of which the start rows are read.  What an instantiation does not
// use keeps its default.
struct SampleStageArgs {
  const unsigned long long* host = nullptr;        // HOST: the pinned block, nwords words
  unsigned long long* dev;                         // the device block (without HOST, NSTEP and POS it is only read)
  int nwords = 0;
  int nr_word = -1, pos_word = -1, run_word = -1;  // first word of next_row (NSTEP), pos_row (POS), pos_run (POS; -1: none)
  const float* sc;                                 // the ring's [capacity][A + 2] scalar rows: action | reward | not_done
  const uint8_t* cont = nullptr;                   // the ring's continuity flags, read by the walks
  long long capacity = 0;
  long long stride = 1;                            // rows between a row and the next one of its lane (the walks' step)
  int n = 1, k = 1;                                // links + 1 of the n-step return (NSTEP) and of the positive (POS)
  float gamma = 1.f;
  int B, A;
  float *act, *rew, *nd;                           // out: [B][A], [B], [B]
};

__device__ __forceinline__ unsigned long long load_pinned(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Does a walk of this instantiation write word i of the block?  The single-writer rule of the staging launch: the copy
// leaves these words out, so each of them has exactly one writer -- sample b's reward thread for the composition's
// (B .. 2B - 1 and the B words of next_row), its not_done thread for the positive's (the 2B words of pos_row and, where
// present, the 3B of pos_run) --, and a walking thread reads its start row from the pinned block with the same
// system-scope load as the copy: nothing in the launch reads a word that another thread of it writes.  The two walks
// are independent (k and n are unrelated), and the entry points hold the regions disjoint (sample_block_ok).
template <bool NSTEP, bool POS>
__device__ __forceinline__ bool walk_owns_word(const SampleStageArgs& a, int i) {
  bool owned = false;
  if constexpr (NSTEP) owned = (i >= a.B && i < 2 * a.B) || (i >= a.nr_word && i < a.nr_word + a.B);
  if constexpr (POS)
    owned = owned || (i >= a.pos_word && i < a.pos_word + 2 * a.B) ||
            (a.run_word >= 0 && i >= a.run_word && i < a.run_word + 3 * a.B);
  return owned;
}

// act[b][:] = sc[r0][0:A], rew[b] = sc[r0][A], nd[b] = sc[r0][A+1] for r0 = idx[b]: the action / reward / not_done of
// the sampled transitions (utils.py:159-166), one thread per scalar; NSTEP: reward and not_done composed along the
// chain by the reward's thread; POS: the positive walked by the not_done's thread; HOST: thread i also copies word i.
template <bool HOST, bool NSTEP, bool POS>
__global__ void sample_stage_kernel(const SampleStageArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (HOST)
    if (i < a.nwords && !walk_owns_word<NSTEP, POS>(a, i)) a.dev[i] = load_pinned(a.host + i);
  if (i >= a.B * (a.A + 2)) return;
  const int b = i / (a.A + 2), c = i - b * (a.A + 2);
  if constexpr (NSTEP && !POS)
    if (c > a.A) return;  // the reward's thread writes not_done too
  const long long r0 = (long long)(HOST ? load_pinned(a.host + b) : a.dev[b]);
  const float v = a.sc[(size_t)r0 * (a.A + 2) + c];
  if (c < a.A) {
    a.act[(size_t)b * a.A + c] = v;
  } else if (c == a.A) {
    if constexpr (NSTEP)
      nstep_compose_one(a.sc, a.cont, a.capacity, a.stride, a.n, a.gamma, a.A, r0, b, a.B, a.dev, a.dev + a.nr_word, a.rew,
                        a.nd);
    else
      a.rew[b] = v;
  } else {
    if constexpr (!NSTEP) a.nd[b] = v;
    if constexpr (POS)
      temporal_pos_one(a.cont, a.capacity, a.stride, a.k, a.n, r0, b, a.B, a.dev + a.pos_word,
                       a.run_word >= 0 ? a.dev + a.run_word : nullptr);
  }
}
