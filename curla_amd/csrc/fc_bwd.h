// The streaming kernels of the encoder fc layer's backward pass (fc_dx_kernel, fc_dw_kernel, the one-pass fc_bwd_kernel)
// and the deferred LayerNorm sums that ride along (LnReduce, ln_reduce_block).  Included by gemm.hip inside its anonymous
// namespace.
#pragma once

// ---------------------------------------------------------------------------
// Backward of the encoder fc layer (encoder.py:98, z = fc(h), h = the NHWC-flattened conv output, K = 30752 columns at
// 84x84): both products have ONE tiny dimension (F <= 64 features) and stream a [B][K] matrix of tens of MB once.
// The generic kernel cuts them into 64 x 64 tiles of 2 k-tiles each -- thousands of short workgroups whose time is
// prologue and epilogue.  Here a workgroup owns 64 columns for its whole life and nothing is staged in LDS: the big
// operand is read with one float4 per lane whose four components are the column operands of four MFMA tiles
// (column j of tile c is n0 + 4j + c), so that the four accumulators of a lane hold 4 CONSECUTIVE columns and every
// wave store / mask load is 256 contiguous bytes per matrix row.
//   fc_dx:  G[b][n] = (mask[b][n] > 0) * sum_f dz[b][f] W[f][n]     (ReLU mask of the last conv layer fused)
//   fc_dw:  dW[f][n] = sum_b dz[b][f] x[b][n]
// ---------------------------------------------------------------------------
__device__ float g_zero16[16];  // where lanes past a reduction range point their operand load (see conv.hip g_zero_px)

// (kFcMaxSteps, F <= 64: fc_plan.h)
struct FcBwdArgs {
  const float* dz;    // [B][F]
  const float* W;     // fc_dx: weight [F][K];  fc_dw: x [B][K]
  const float* mask;  // fc_dx: [B][K] (may be NULL)
  float* out;         // fc_dx: G [B][K];  fc_dw: dW [F][K]
  int B, F, K;
};

template <int KS>  // KS = ceil(F / 4) k-steps
__device__ __forceinline__ void fc_dx_body(const FcBwdArgs& g, const int bid) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int n0 = bid * 64;
  const int ncol = n0 + 4 * li;            // this lane's 4 columns (float4)
  const bool cvalid = ncol + 3 < g.K;      // K % 4 == 0: a float4 is inside or outside as a whole
  const int nc = cvalid ? ncol : n0;       // (columns past the edge re-read the first ones; their results are not stored)
  // column operand: W[f = 4s + kq][nc .. nc+3] for every k-step, kept for the workgroup's whole life
  f32x4 wv[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int f = 4 * s + kq;
    wv[s] = *reinterpret_cast<const f32x4*>(g.W + (size_t)min(f, g.F - 1) * g.K + nc);
  }
  const int ntiles = (g.B + 15) >> 4;
  // row operand of b-tile t: dz[16t + li][4s + kq]; features past F multiply a zero (loaded from the zero page)
  auto load_dz = [&](int t, float (&dv)[KS]) {
    const int b = min(16 * t + li, g.B - 1);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int f = 4 * s + kq;
      dv[s] = *(f < g.F ? g.dz + (size_t)b * g.F + f : g_zero16);
    }
  };
  auto load_mask = [&](int t, f32x4 (&mk)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = min(16 * t + 4 * kq + r, g.B - 1);
      mk[r] = g.mask ? *reinterpret_cast<const f32x4*>(g.mask + (size_t)b * g.K + nc) : f32x4{1.f, 1.f, 1.f, 1.f};
    }
  };
  auto compute = [&](int t, const float (&dv)[KS], const f32x4 (&mk)[4]) {
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = mfma16(dv[s], wv[s][c], acc[c]);
    // lane (li, kq): rows b = 16t + 4kq + r, columns nc + c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * t + 4 * kq + r;
      f32x4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = mk[r][c] > 0.f ? v[c] : 0.f;
      if (cvalid && b < g.B) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(g.out + (size_t)b * g.K + ncol));
    }
  };
  // this wave's b-tiles: wave, wave + 4, ...; operands (and the mask) of the next tile are requested before the current
  // one's MFMAs (a third register set in flight measured no faster: 39.4 against 37.5 us at B = 512, K = 30752)
  float dA[KS], dB[KS];
  f32x4 mA[4], mB[4];
  int t = wave;
  if (t < ntiles) {
    load_dz(t, dA);
    load_mask(t, mA);
  }
  for (; t < ntiles; t += 8) {
    const int t1 = min(t + 4, ntiles - 1), t2 = min(t + 8, ntiles - 1);  // (past the end: re-read the last tile)
    load_dz(t1, dB);
    load_mask(t1, mB);
    __builtin_amdgcn_sched_barrier(0);
    compute(t, dA, mA);
    __builtin_amdgcn_sched_barrier(0);
    load_dz(t2, dA);
    load_mask(t2, mA);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 4 < ntiles) compute(t + 4, dB, mB);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int KS>
__global__ __launch_bounds__(256, 2) void fc_dx_kernel(FcBwdArgs g) {
  fc_dx_body<KS>(g, blockIdx.x);
}

template <int NT>  // NT = ceil(F / 16) feature tiles
__device__ __forceinline__ void fc_dw_body(const FcBwdArgs& g, const int bid) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves][NT][4][64 lanes] float4
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int n0 = bid * 64;
  const int ncol = n0 + 4 * li;
  const bool cvalid = ncol + 3 < g.K;
  const int nc = cvalid ? ncol : n0;
  const int nsteps = (g.B + 3) >> 2;  // k-steps of 4 rows b
  const int s0 = (int)((long long)wave * nsteps / 4), s1 = (int)((long long)(wave + 1) * nsteps / 4);
  f32x4 acc[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0, 0, 0, 0};
  // step s: rows b = 4s + kq.  Column operand: x[b][nc..nc+3]; row operand of feature tile t: dz[b][16t + li]
  // (features past F: re-read feature F-1, those output rows are not stored; rows past B: zeros from the zero page)
  auto fetch = [&](int s, f32x4& xv, float (&dv)[NT]) {
    const int b = 4 * min(s, s1 - 1) + kq;
    const bool bv = b < g.B;
    xv = *reinterpret_cast<const f32x4*>(g.W + (size_t)min(b, g.B - 1) * g.K + nc);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      dv[t] = *(bv ? g.dz + (size_t)b * g.F + min(16 * t + li, g.F - 1) : g_zero16);
  };
  auto multiply = [&](const f32x4& xv, const float (&dv)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] = mfma16(dv[t], xv[c], acc[t][c]);
  };
  if (s1 > s0) {
    // eight register sets: a k-step is 16 MFMAs (~0.4 us with the SIMD shared), an HBM round trip several times that
    constexpr int D = 8;
    f32x4 xr[D];
    float dr[D][NT];
#pragma unroll
    for (int d = 0; d < D - 1; ++d) fetch(s0 + d, xr[d], dr[d]);
    for (int s = s0; s < s1; s += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        fetch(s + d + D - 1, xr[(d + D - 1) % D], dr[(d + D - 1) % D]);
        __builtin_amdgcn_sched_barrier(0);
        if (s + d < s1) multiply(xr[d], dr[d]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // sum over the four waves (b ranges) in wave order, then wave w writes feature tile(s) w, w+4, ...
  f32x4* r4 = reinterpret_cast<f32x4*>(red);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) r4[((wave * NT + t) * 4 + c) * 64 + lane] = acc[t][c];
  __syncthreads();
  for (int t = wave; t < NT; t += 4) {
    f32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = r4[((0 * NT + t) * 4 + c) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) v[c] += r4[((w * NT + t) * 4 + c) * 64 + lane];
    }
    // lane (li, kq): rows f = 16t + 4kq + r, columns nc + c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * t + 4 * kq + r;
      const f32x4 o = {v[0][r], v[1][r], v[2][r], v[3][r]};
      if (cvalid && f < g.F) *reinterpret_cast<f32x4*>(g.out + (size_t)f * g.K + ncol) = o;
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void fc_dw_kernel(FcBwdArgs g) {
  fc_dw_body<NT>(g, blockIdx.x);
}

// Both products of the fc backward in ONE pass over the activations: the ReLU mask of the data gradient and the
// column operand of the weight gradient are the SAME matrix x (the last conv layer's output), and both bodies above
// read it in the same lane layout -- lane (li, kq) holds x[16t + 4kq + r][nc .. nc+3], r = 0..3, of b-tile t: for the
// data gradient that is the mask of its four accumulator rows, for the weight gradient the column operand of k-step r
// (a step multiplies rows 16t + 4kq + r: any order of the batch rows is a valid k order as long as the dz operand
// follows it).  One workgroup per 64 columns does both, x is read from HBM once instead of twice (63 of 206 MB per
// launch at B = 512, K = 30752).
// (B % 16 == 0, 4 (KS - 1) < F <= 4 KS and matrices below 2 GB, checked by the host.)  Every operand goes through
// buffer loads -- descriptor in SGPRs, a 32-bit lane offset that never changes, the tile / row / k-step part of the
// address in the scalar offset: with flat addresses the ~45 loads of a tile kept 64-bit lane addresses alive (35 spilled
// registers, each reload a full wait in front of its load).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float buf_f32(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 buf_f32x4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// NT feature tiles of 16 go through the matrix pipe; NTAIL further features (F = 16 NT + NTAIL: 50 = 3 x 16 + 2) are
// accumulated by VALU FMAs on the x values the lane holds anyway -- a fourth tile for two features would be an eighth
// of the kernel's MFMAs.
// DX = false: the weight gradient alone (the actor's fc layer: its conv stack is detached, curl_sac.py:375-376) -- the
// same walk without the data-gradient half.
// The LayerNorm parameter gradients that curla_ln_bwd_partial left as per-workgroup partial sums [nparts][3][F] (dgamma,
// dbeta, fc bias gradient): summed in partial order by ONE extra workgroup of this launch (the last), eight loads in
// flight -- a launch less per LayerNorm backward.  partial == nullptr: nothing to do, no extra workgroup.
struct LnReduce {
  const float* partial;
  int nparts, F;
  float *dgamma, *dbeta, *dbias;
  // a second set of partial sums for the same workgroup (the CURL head's dW partials, curla_curl_head):
  // xout[i] = sum over xparts partials of xpartial[p * xlen + i]; xpartial == nullptr: none
  const float* xpartial;
  int xparts, xlen;
  float* xout;
};
__device__ __forceinline__ void ln_reduce_block(const LnReduce& r) {
  if (r.xpartial) {
    for (int i = threadIdx.x; i < r.xlen; i += blockDim.x) {
      const float* p = r.xpartial + i;
      float a = 0.f;
      int k = 0;
      for (; k + 8 <= r.xparts; k += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(size_t)(k + u) * r.xlen];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += t[u];
      }
      for (; k < r.xparts; ++k) a += p[(size_t)k * r.xlen];
      r.xout[i] = a;
    }
  }
  for (int i = threadIdx.x; i < 3 * r.F; i += blockDim.x) {
    const int q = i / r.F, f = i - q * r.F;
    float* out = q == 0 ? r.dgamma : q == 1 ? r.dbeta : r.dbias;
    if (!out) continue;
    const float* p = r.partial + i;
    const size_t st = (size_t)3 * r.F;
    float a = 0.f;
    int k = 0;
    for (; k + 8 <= r.nparts; k += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = p[(k + u) * st];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += t[u];
    }
    for (; k < r.nparts; ++k) a += p[k * st];
    out[f] = a;
  }
}

template <int KS, int NT, int NTAIL, bool DX>
__global__ __launch_bounds__(256, 2) void fc_bwd_kernel(FcBwdArgs g, float* dW, LnReduce lnr) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves][NT][4][64 lanes] float4
  if (lnr.partial && blockIdx.x == gridDim.x - 1) {  // (the grid has one workgroup more than column blocks)
    ln_reduce_block(lnr);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 64;
  const int ncol = n0 + 4 * li;
  const bool cvalid = ncol + 3 < g.K;
  const int nc = cvalid ? ncol : n0;
  f32x4 wv[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int f = 4 * s + kq;
    wv[s] = DX ? *reinterpret_cast<const f32x4*>(g.W + (size_t)min(f, g.F - 1) * g.K + nc) : f32x4{0, 0, 0, 0};
  }
  f32x4 accw[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) accw[t][c] = f32x4{0, 0, 0, 0};
  f32x4 atail[NTAIL > 0 ? NTAIL : 1];  // [feature 16 NT + j] x this lane's 4 columns, summed over its rows
#pragma unroll
  for (int j = 0; j < (NTAIL > 0 ? NTAIL : 1); ++j) atail[j] = f32x4{0, 0, 0, 0};
  const unsigned tl_off = (unsigned)(4 * kq * g.F + 16 * NT) * 4u;  // dz[16t + 4kq + r][16 NT + j]: + 4 r F + 4 j
  const int ntiles = g.B >> 4;
  const unsigned dz_bytes = (unsigned)g.B * g.F * 4u, x_bytes = (unsigned)g.B * (unsigned)g.K * 4u;
  const __amdgpu_buffer_rsrc_t rdz = __builtin_amdgcn_make_buffer_rsrc((void*)g.dz, (short)0, (int)dz_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)g.mask, (short)0, (int)x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)g.out, (short)0, (int)x_bytes, 0x00020000);
  // lane offsets (bytes) inside a b-tile's 16 rows of dz / x; everything else of an address is wave-uniform
  const unsigned dv_off = (unsigned)(li * g.F + kq) * 4u;  // dz[16t + li][4s + kq]: + 16 s
  // last k-step: features past F multiply a zero -- their lanes point past the buffer (an out-of-range load returns 0)
  const unsigned dv_last = 4 * (KS - 1) + kq < g.F ? dv_off : 0x80000000u;
  unsigned dt_off[NT];                                    // dz[16t + 4kq + r][16ft + li]: + 4 r F
#pragma unroll
  for (int ft = 0; ft < NT; ++ft) dt_off[ft] = (unsigned)(4 * kq * g.F + min(16 * ft + li, g.F - 1)) * 4u;
  const unsigned x_off = ((unsigned)(4 * kq) * (unsigned)g.K + (unsigned)nc) * 4u;  // x[16t + 4kq + r][nc]: + 4 r K
  const unsigned rowF = 4u * g.F, rowK = 4u * (unsigned)g.K;
  auto load_dv = [&](int t, float (&dv)[KS]) {
    const unsigned base = (unsigned)t * 16u * rowF;
#pragma unroll
    for (int s = 0; s < KS - 1; ++s) dv[s] = buf_f32(rdz, dv_off, base + 16u * s);
    dv[KS - 1] = buf_f32(rdz, dv_last, base + 16u * (KS - 1));
  };
  auto load_dt = [&](int t, float (&dt)[4][NT]) {
    const unsigned base = (unsigned)t * 16u * rowF;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ft = 0; ft < NT; ++ft) dt[r][ft] = buf_f32(rdz, dt_off[ft], base + r * rowF);  // (features past F: F-1 again, never stored)
  };
  auto load_mk = [&](int t, f32x4 (&mk)[4]) {
    const unsigned base = (unsigned)t * 16u * rowK;
#pragma unroll
    for (int r = 0; r < 4; ++r) mk[r] = buf_f32x4(rx, x_off, base + r * rowK);
  };
  auto load_tl = [&](int t, float (&tl)[4][NTAIL > 0 ? NTAIL : 1]) {
    const unsigned base = (unsigned)t * 16u * rowF;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < NTAIL; ++j) tl[r][j] = buf_f32(rdz, tl_off, base + r * rowF + 4u * j);
  };
  float dv[KS], dt[4][NT], tl[4][NTAIL > 0 ? NTAIL : 1];
  // x comes from HBM and is requested a whole tile ahead (two register sets); the dz operands are L2 hits and each has
  // the other product's MFMAs to arrive under
  auto tile = [&](int t, int tnext, const f32x4 (&mk)[4], f32x4 (&mk_next)[4]) {
    load_mk(tnext, mk_next);
    load_dt(t, dt);
    if (NTAIL > 0) load_tl(t, tl);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0, 0, 0, 0};
    if (DX) {
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = mfma16(dv[s], wv[s][c], acc[c]);
      __builtin_amdgcn_sched_barrier(0);
      load_dv(tnext, dv);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ft = 0; ft < NT; ++ft)
#pragma unroll
        for (int c = 0; c < 4; ++c) accw[ft][c] = mfma16(dt[r][ft], mk[r][c], accw[ft][c]);
#pragma unroll
    for (int j = 0; j < NTAIL; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) atail[j] += tl[r][j] * mk[r];
    if (DX) {
      const unsigned obase = (unsigned)t * 16u * rowK;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = mk[r][c] > 0.f ? v[c] : 0.f;
        if (cvalid) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro, x_off, obase + r * rowK, 2);  // nt
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  f32x4 mA[4], mB[4];
  int t = wave;  // this wave's b-tiles: wave, wave + 4, ...
  if (t < ntiles) {
    load_mk(t, mA);
    if (DX) load_dv(t, dv);
  }
  for (; t < ntiles; t += 8) {
    tile(t, min(t + 4, ntiles - 1), mA, mB);  // (past the end: the last tile again, unused)
    if (t + 4 < ntiles) tile(t + 4, min(t + 8, ntiles - 1), mB, mA);
  }
  // weight gradient: sum over the four waves (b-tiles) in wave order, then wave w writes feature tile(s) w, w+4, ...
  f32x4* r4 = reinterpret_cast<f32x4*>(red);
  f32x4* t4 = r4 + 4 * NT * 4 * 64;  // tail features: [4 waves][NTAIL][16 column groups]
  if (NTAIL > 0) {
#pragma unroll
    for (int j = 0; j < NTAIL; ++j) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // the four row quarters (kq) of a column group sit in lanes li, li+16, li+32, li+48
        atail[j][c] += __shfl_xor(atail[j][c], 16);
        atail[j][c] += __shfl_xor(atail[j][c], 32);
      }
      if (kq == 0) t4[(wave * NTAIL + j) * 16 + li] = atail[j];
    }
  }
#pragma unroll
  for (int ft = 0; ft < NT; ++ft)
#pragma unroll
    for (int c = 0; c < 4; ++c) r4[((wave * NT + ft) * 4 + c) * 64 + lane] = accw[ft][c];
  __syncthreads();
  for (int ft = wave; ft < NT; ft += 4) {
    f32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = r4[((0 * NT + ft) * 4 + c) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) v[c] += r4[((w * NT + ft) * 4 + c) * 64 + lane];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * ft + 4 * kq + r;
      const f32x4 o = {v[0][r], v[1][r], v[2][r], v[3][r]};
      if (cvalid && f < g.F) *reinterpret_cast<f32x4*>(dW + (size_t)f * g.K + ncol) = o;
    }
  }
  if (NTAIL > 0 && tid < 16 * NTAIL) {  // (after the barrier above)
    const int j = tid >> 4, cg = tid & 15;
    f32x4 v = t4[(0 * NTAIL + j) * 16 + cg];
#pragma unroll
    for (int w = 1; w < 4; ++w) v += t4[(w * NTAIL + j) * 16 + cg];
    const int col = n0 + 4 * cg;
    if (col + 3 < g.K) *reinterpret_cast<f32x4*>(dW + (size_t)(16 * NT + j) * g.K + col) = v;
  }
}
