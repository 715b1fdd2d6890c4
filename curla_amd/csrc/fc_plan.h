// Which kernel an encoder-fc product takes, as host-only code: the plan of the split-K forward (fc_fwd_plan), of the two
// streaming backward products (fc_dx_plan, fc_dw_plan), of the one-pass backward (fc_one_pass_plan) and of the entry
// point that chooses between them (fc_bwd_plan) -- kernel and template arguments, grid, dynamic LDS bytes, refusal or
// fallback -- and the walk numbers the kernels of fc_fwd.h / fc_bwd.h derive from a shape (fc_*_walk).  Nothing here
// includes a device header or asks the options anything: the value of gemm_mfma arrives as an argument, so the
// decisions run (and are tested, tests/test_fc_plan_host.py) without a GPU.  Pointer checks (null, alignment) stay with
// the entry points in gemm.hip.  Included by gemm.hip in front of its kernel headers.
#pragma once

#include "../../include/curla_hip.h"
#include "options.h"

namespace {

constexpr int kFcMaxSteps = 16;              // backward: F <= 64 (k-steps of 4 features)
constexpr int kFcChunk = 4;                  // forward: k-slices per W chunk in LDS
constexpr int kFcPitch = 32 * kFcChunk + 4;  // floats per feature row of a chunk (16-byte aligned, off the bank stride)
constexpr long long kFcVec4Bytes = 16;       // one float4 of a kernel's LDS sums

// ------------------------------------------------------------------------------------------------------- forward
// fc_fwd_kernel<nt, ntail, b3>: 50 features = three tiles on the matrix pipe + two features on FMAs, 52..64 even = four
// tiles; one workgroup per (problem, 128-row group, split)
struct FcFwdPlan {
  int nt, ntail;
  bool b3;
  int nrg, grid;
  long long lds;
};

// the instantiated shapes: 50..64 even features, whole 128-row groups, 32-wide k-slices, at least one slice per split,
// 32-bit byte offsets, partial sums 8-byte aligned split by split; everything else: CURLA_ERR_UNSUPPORTED (the caller
// takes curla_gemm_multi)
inline int fc_fwd_plan(int nprob, int B, int F, int K, int nsplit, long long split_stride, int mfma, FcFwdPlan& p) {
  if (F < 50 || F > 64 || F % 2 != 0 || B % 128 != 0 || K % 32 != 0 || nsplit > K / 32 ||
      (long long)B * K * 4 >= (1LL << 31) || (long long)F * K * 4 >= (1LL << 31) || split_stride % 2 != 0)
    return CURLA_ERR_UNSUPPORTED;
  p.nt = F == 50 ? 3 : 4, p.ntail = F == 50 ? 2 : 0;
  p.b3 = mfma != kGemmMfmaF32;  // option gemm_mfma: f32 keeps the f32-input MFMA
  p.nrg = B / 128;
  p.grid = nprob * p.nrg * nsplit;
  p.lds = (long long)2 * 64 * kFcPitch * (long long)sizeof(float);
  return CURLA_OK;
}

// what the splits of a forward walk: slices per split (least, most), which (s1 - s0) mod 4 occur (bit m of mod4: the
// skip pattern of a split's last chunk), W chunks per split (least, most), whether any split starts off a multiple of 4
struct FcFwdWalk {
  int slices_min, slices_max, mod4, chunks_min, chunks_max;
  bool odd_start;
};
inline FcFwdWalk fc_fwd_walk(int K, int nsplit) {
  FcFwdWalk w = {1 << 30, 0, 0, 1 << 30, 0, false};
  const int nslices = K >> 5;
  for (int split = 0; split < nsplit; ++split) {
    const int s0 = (int)((long long)nslices * split / nsplit), s1 = (int)((long long)nslices * (split + 1) / nsplit);
    const int n = s1 - s0, c = (n + kFcChunk - 1) / kFcChunk;
    w.slices_min = n < w.slices_min ? n : w.slices_min, w.slices_max = n > w.slices_max ? n : w.slices_max;
    w.chunks_min = c < w.chunks_min ? c : w.chunks_min, w.chunks_max = c > w.chunks_max ? c : w.chunks_max;
    w.mod4 |= 1 << (n % 4);
    w.odd_start = w.odd_start || s0 % 4 != 0;
  }
  return w;
}

// ------------------------------------------------------------------------------------------------------ backward
// every backward entry point: at most 64 features, whole float4s along K
inline int fc_bwd_shape(int F, int K) { return F > 4 * kFcMaxSteps || (K % 4) != 0 ? CURLA_ERR_UNSUPPORTED : CURLA_OK; }

// the last 64-column block of a backward kernel: all 16 float4s, some of them, or a single one
enum FcLastBlock { kFcLastFull, kFcLastPart, kFcLastOne };
inline int fc_last_block(int K) { return K % 64 == 0 ? kFcLastFull : K % 64 == 4 ? kFcLastOne : kFcLastPart; }

// b-tiles (16 rows) per wave of fc_dx_kernel / fc_bwd_kernel: wave w takes tiles w, w + 4, ... of `ntiles`
inline void fc_btile_walk(int ntiles, int& tmin, int& tmax) {
  tmin = 1 << 30, tmax = 0;
  for (int wave = 0; wave < 4; ++wave) {
    const int n = wave < ntiles ? (ntiles - wave + 3) / 4 : 0;
    tmin = n < tmin ? n : tmin, tmax = n > tmax ? n : tmax;
  }
}

// k-steps (4 rows) per wave of fc_dw_kernel: the steps are cut into four consecutive ranges
inline void fc_dw_walk(int B, int& smin, int& smax) {
  smin = 1 << 30, smax = 0;
  const int nsteps = (B + 3) >> 2;
  for (int wave = 0; wave < 4; ++wave) {
    const int n = (int)((long long)(wave + 1) * nsteps / 4) - (int)((long long)wave * nsteps / 4);
    smin = n < smin ? n : smin, smax = n > smax ? n : smax;
  }
}

// fc_dx_kernel<ks>: ceil(F / 4) k-steps rounded up to an instantiated count; one workgroup per 64 columns, no LDS
struct FcDxPlan {
  int ks, grid;
};
inline int fc_dx_plan(int F, int K, FcDxPlan& p) {
  const int rc = fc_bwd_shape(F, K);
  if (rc != CURLA_OK) return rc;
  const int ks = (F + 3) / 4;
  p.ks = ks <= 4 ? 4 : ks <= 8 ? 8 : ks <= 13 ? 13 : 16;
  p.grid = (K + 63) / 64;
  return CURLA_OK;
}

// The one-pass kernel fc_bwd_kernel<13, nt, ntail, dx>: dx = true, both products (F = 50: 3 tiles on the matrix pipe +
// 2 features on VALU FMAs; F = 49, 51, 52: 4 tiles); dx = false, its weight-gradient half alone (F = 50).  One workgroup
// per 64 columns and one more for the deferred LayerNorm sums where there are any (ln).
struct FcOnePassPlan {
  int ks, nt, ntail;
  bool dx;
  int grid;
  long long lds;
};
inline FcOnePassPlan fc_one_pass_plan(bool dx, int F, int K, bool ln) {
  FcOnePassPlan p;
  p.ks = 13, p.dx = dx;
  p.nt = !dx || F == 50 ? 3 : 4, p.ntail = !dx || F == 50 ? 2 : 0;
  p.grid = (K + 63) / 64 + (ln ? 1 : 0);
  p.lds = (long long)4 * 4 * 4 * 64 * kFcVec4Bytes;  // (the 3 + 2 form needs less: 48 KB + 2 KB)
  return p;
}

// the weight gradient alone: the one-pass kernel's half (F = 50, whole 16-row tiles, x below 2 GB) or fc_dw_kernel<nt>,
// nt = ceil(F / 16) feature tiles, 16 KB of LDS each; there the deferred LayerNorm sums take a launch of their own
// (ln_launch: ln_reduce_kernel, one workgroup, in front)
struct FcDwPlan {
  bool one_pass;
  FcOnePassPlan op;
  int nt, grid;
  long long lds;
  bool ln_launch;
};
inline int fc_dw_plan(int B, int F, int K, bool ln, FcDwPlan& p) {
  const int rc = fc_bwd_shape(F, K);
  if (rc != CURLA_OK) return rc;
  p.one_pass = F == 50 && B % 16 == 0 && (long long)B * K * 4 < (1LL << 31);
  p.op = FcOnePassPlan{}, p.nt = p.grid = 0, p.lds = 0, p.ln_launch = false;
  if (p.one_pass) {
    p.op = fc_one_pass_plan(false, F, K, ln);
    return CURLA_OK;
  }
  p.ln_launch = ln;
  p.grid = (K + 63) / 64;
  p.nt = (F + 15) / 16;
  p.lds = (long long)4 * p.nt * 4 * 64 * kFcVec4Bytes;
  return CURLA_OK;
}

// both products: the one-pass kernel is instantiated for 49..52 features, whole 16-row tiles and matrices below 2 GB
// (32-bit buffer offsets); anything else takes the two streaming kernels (two_launches: fc_dx_plan + fc_dw_plan)
struct FcBwdPlan {
  bool two_launches;
  FcOnePassPlan op;
};
inline int fc_bwd_plan(int B, int F, int K, bool ln, FcBwdPlan& p) {
  const int rc = fc_bwd_shape(F, K);
  if (rc != CURLA_OK) return rc;
  const int ks = (F + 3) / 4, nt = (F + 15) / 16;
  p.two_launches = ks != 13 || nt != 4 || B % 16 != 0 || (long long)B * K * 4 >= (1LL << 31);  // (i.e. not F = 49..52)
  p.op = p.two_launches ? FcOnePassPlan{} : fc_one_pass_plan(true, F, K, ln);
  return CURLA_OK;
}

}  // namespace
