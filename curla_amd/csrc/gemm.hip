// Batched fp32 GEMM on the exact-f32 matrix pipe (v_mfma_f32_16x16x4_f32) with
// fused epilogues.  Serves every dense layer of the path: encoder fc
// (encoder.py:66,98) forward/backward, the actor trunk and twin-Q MLPs
// (curl_sac.py:70-74,129-133) and the CURL bilinear logits
// z_a (W z_pos^T) (curl_sac.py:219-220) with their backward products.
//
//   C[z][m][n] = epilogue( alpha * sum_k opA(A)[m][k] * opB(B)[n][k] )
//   opA: row-major A[m*lda + k]   or k-major A[k*lda + m]   (transposed operand)
//   opB: row-major B[n*ldb + k]   or k-major B[k*ldb + n]
//   epilogue: + bias[n], ReLU, zero where mask[m][n] <= 0 (ReLU backward).
// grid.z enumerates batch x split-K; a split writes its partial product to
// C + split * split_stride and the caller reduces (deterministic order).
//
// This file: the host side -- the builder of the kernels' argument block, the launch helper, the run-time -> template
// dispatch that names every instantiation, the C ABI (include/curla_hip.h).  The kernels live in the headers included
// in place below; which of them a product takes is decided in gemm_plan.h and fc_plan.h, host-only code.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "options.h"
#include "gemm_plan.h"
#include "fc_plan.h"

namespace {

#include "gemm_tile.h"
#include "fc_bwd.h"
#include "fc_fwd.h"
#include "gemm_small.h"

// ------------------------------ host side ------------------------------
// Every launch of this file: raise the kernel's dynamic-LDS limit to the launch's own byte count if (and only if) it
// uses dynamic LDS, launch, report the launch status.
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), dim3 grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
  // (once per kernel and device, thread-safe: curla_set_dyn_lds)
  if (lds && curla_set_dyn_lds(reinterpret_cast<const void*>(kernel), lds) != CURLA_OK) return CURLA_ERR_LAUNCH;
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, args...);
  return curla_launch_status();
}

// the one place that asks the device and the options what the plans depend on
GemmEnv gemm_env() { return GemmEnv{curla_cu_count(), curla_opt(kOptGemmTile), curla_opt(kOptGemmMfma), curla_opt(kOptLinearBwd)}; }

// The plain single-level product C[z] = A[z] B[z]^T by strides, every field set: no epilogue, alpha = 1, no k split, no
// second batch level, no column sums, no pointer table.  The entry points override what is theirs.
GemmArgs gemm_args(const float* A, int lda, long long sA, const float* B, int ldb, long long sB, float* C, int ldc,
                   long long sC, int M, int N, int K, int nbatch) {
  GemmArgs g = {};
  g.A = A, g.B = B, g.C = C;
  g.M = M, g.N = N, g.K = K, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.sA = sA, g.sB = sB, g.sC = sC;
  g.nbatch = g.nb_inner = nbatch, g.ksplit = 1;
  g.alpha = 1.f;
  g.vecA = (lda % 4 == 0) && (sA % 4 == 0) && aligned16(A);
  g.vecB = (ldb % 4 == 0) && (sB % 4 == 0) && aligned16(B);
  return g;
}

// a 256-thread tile in its three forms: bf16x3, interior + aligned, bounds-checked
template <bool AK, bool BKM, int TM, int TN>
int launch_tiled(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  const int grid = ((g.N + TN - 1) / TN) * ((g.M + TM - 1) / TM) * g.nbatch * g.ksplit;
  if (p.b3) return launch(gemm_kernel<AK, BKM, TM, TN, true, true>, grid, 256, 0, st, g);
  if (p.fast) return launch(gemm_kernel<AK, BKM, TM, TN, true, false>, grid, 256, 0, st, g);
  return launch(gemm_kernel<AK, BKM, TM, TN, false, false>, grid, 256, 0, st, g);
}

// the plan's kernel for one operand layout
template <bool AK, bool BKM>
int launch_planned(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  if (p.small) {
    const dim3 grid((g.N + 15) / 16, (g.M + 15) / 16, g.nbatch);
    if (p.wide) return launch(gemm_small_kernel<AK, BKM, 16, 2>, grid, 1024, 0, st, g);
    return launch(gemm_small_kernel<AK, BKM, 4, 8>, grid, 256, 0, st, g);
  }
  if (p.tbm == 128)
    return launch(gemm_kernel<AK, BKM, 128, 64, true, true, 512>, (g.N / 64) * (g.M / 128) * g.nbatch, 512, 0, st, g);
  if (p.tbm == 32) return launch_tiled<AK, BKM, 32, 32>(p, g, st);
  if (p.tbn == 32) return launch_tiled<AK, BKM, 64, 32>(p, g, st);
  return launch_tiled<AK, BKM, 64, 64>(p, g, st);
}

int gemm_launch(GemmArgs& g, int a_kmajor, int b_kmajor, hipStream_t st) {
  GemmPlan p;
  const int prc = gemm_plan(g, a_kmajor, b_kmajor, gemm_env(), p);
  if (prc != CURLA_OK) return prc;
  if (a_kmajor && b_kmajor) return launch_planned<true, true>(p, g, st);
  if (a_kmajor) return launch_planned<true, false>(p, g, st);
  if (b_kmajor) return launch_planned<false, true>(p, g, st);
  return launch_planned<false, false>(p, g, st);
}

// the tiled pairs of gemm_plan.h's kPairTiles, [row][b3]
using PairKernel = void (*)(GemmArgs, GemmArgs, int, int, int, int, int, int);
template <int I, bool B3>
constexpr PairKernel kPairKernel = gemm_pair_kernel<kPairTiles[I][0], kPairTiles[I][1], kPairTiles[I][2], kPairTiles[I][3], B3>;
constexpr PairKernel kTiledPairs[4][2] = {{kPairKernel<0, false>, kPairKernel<0, true>},
                                          {kPairKernel<1, false>, kPairKernel<1, true>},
                                          {kPairKernel<2, false>, kPairKernel<2, true>},
                                          {kPairKernel<3, false>, kPairKernel<3, true>}};

int launch_pair(PairKernel kernel, int threads, const LinearBwdPlan& q, const GemmArgs& g1, const GemmArgs& g2, hipStream_t st) {
  return launch(kernel, (unsigned)(q.n1 + q.n2), threads, 0, st, g1, g2, (int)q.n1, q.gx1, q.gy1, q.gx2, q.gy2, (int)q.n2);
}

// the one-pass kernel of the encoder fc backward as fc_plan.h planned it (fc_one_pass_plan)
int launch_fc_bwd(const FcOnePassPlan& p, const FcBwdArgs& gx, float* dW, const LnReduce& lnr, hipStream_t st) {
  const size_t lds = (size_t)p.lds;
  if (!p.dx) return launch(fc_bwd_kernel<13, 3, 2, false>, p.grid, 256, lds, st, gx, dW, lnr);
  if (p.nt == 3) return launch(fc_bwd_kernel<13, 3, 2, true>, p.grid, 256, lds, st, gx, dW, lnr);
  return launch(fc_bwd_kernel<13, 4, 0, true>, p.grid, 256, lds, st, gx, dW, lnr);
}

}  // namespace

extern "C" {

int curla_gemm(const float* A, int a_kmajor, int lda, long long strideA, const float* B, int b_kmajor, int ldb,
               long long strideB, float* C, int ldc, long long strideC, int M, int N, int K, int nbatch, int ksplit,
               long long split_stride, float alpha, const float* bias, long long strideBias, int relu,
               const float* mask, int ldmask, long long strideMask, void* stream) {
  CURLA_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0 && nbatch > 0 && ksplit > 0);
  CURLA_REQUIRE(ksplit == 1 || (!bias && !mask && !relu));
  GemmArgs g = gemm_args(A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, nbatch);
  g.ksplit = ksplit, g.sSplit = split_stride;
  g.alpha = alpha, g.relu = relu;
  g.bias = bias, g.sBias = strideBias;
  g.mask = mask, g.ldmask = ldmask, g.sMask = strideMask;
  return gemm_launch(g, a_kmajor, b_kmajor, static_cast<hipStream_t>(stream));
}

int curla_gemm_small_shape(int M, int N, int K, int nbatch) { return small_shape(M, N, K, nbatch) ? 1 : 0; }

int curla_gemm_colsum(const float* A, int a_kmajor, int lda, long long strideA, const float* B, int b_kmajor, int ldb,
                      long long strideB, float* C, int ldc, long long strideC, int M, int N, int K, int nbatch,
                      float* colsum, long long strideColsum, void* stream) {
  CURLA_REQUIRE(A && B && C && colsum && M > 0 && N > 0 && K > 0 && nbatch > 0);
  GemmArgs g = gemm_args(A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, nbatch);
  g.colsum = colsum, g.sColsum = strideColsum;
  return gemm_launch(g, a_kmajor, b_kmajor, static_cast<hipStream_t>(stream));
}

int curla_linear_bwd(const float* dy, long long stride_dy, const float* x, long long stride_x, const float* W,
                     long long stride_W, const float* mask, long long stride_mask, float* dW, long long stride_dW,
                     float* db, long long stride_db, float* dx, long long stride_dx, int B, int N, int K, int nbatch,
                     void* stream) {
  CURLA_REQUIRE(dy && x && W && dW && dx && B > 0 && N > 0 && K > 0 && nbatch > 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // dW[n][k] = sum_b dy[b][n] x[b][k]: both operands k-major (k = batch row)
  GemmArgs g1 = gemm_args(dy, N, stride_dy, x, K, stride_x, dW, K, stride_dW, N, K, B, nbatch);
  g1.colsum = db, g1.sColsum = stride_db;
  // dx[b][k] = sum_n dy[b][n] W[n][k], zero where mask <= 0: W k-major
  GemmArgs g2 = gemm_args(dy, N, stride_dy, W, K, stride_W, dx, K, stride_dx, B, K, N, nbatch);
  g2.mask = mask, g2.ldmask = K, g2.sMask = stride_mask;
  LinearBwdPlan q;
  int rc = linear_bwd_plan(g1, g2, gemm_env(), q);
  if (rc != CURLA_OK) return rc;
  switch (q.kind) {
    case kBwdSmallPair:
      return launch(gemm_small_pair_kernel<4, 8>, (unsigned)(q.n1 + q.n2), 256, 0, st, g1, g2, (int)q.n1, q.gx1, q.gy1, q.gx2,
                    q.gy2);
    case kBwdBigPair:
      if (q.second_first) return launch_pair(gemm_pair_kernel<128, 64, 128, 64, true, true, 512>, 512, q, g1, g2, st);
      return launch_pair(gemm_pair_kernel<128, 64, 128, 64, true, false, 512>, 512, q, g1, g2, st);
    case kBwdTiledPair: return launch_pair(kTiledPairs[q.pair][q.b3], 256, q, g1, g2, st);
    default: break;
  }
  rc = gemm_launch(g1, 1, 1, st);
  if (rc != CURLA_OK) return rc;
  return gemm_launch(g2, 0, 1, st);
}

int curla_gemm_nested(const float* A, int a_kmajor, int lda, long long strideA, long long strideA2, const float* B,
                      int b_kmajor, int ldb, long long strideB, long long strideB2, float* C, int ldc, long long strideC,
                      long long strideC2, int M, int N, int K, int nbatch, int nbatch2, float alpha, const float* bias,
                      long long strideBias, long long strideBias2, int relu, const float* mask, int ldmask,
                      long long strideMask, long long strideMask2, void* stream) {
  CURLA_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0 && nbatch > 0 && nbatch2 > 0);
  GemmArgs g = gemm_args(A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, nbatch * nbatch2);
  g.alpha = alpha, g.relu = relu;
  g.bias = bias, g.sBias = strideBias;
  g.mask = mask, g.ldmask = ldmask, g.sMask = strideMask;
  g.nb_inner = nbatch, g.sA2 = strideA2, g.sB2 = strideB2, g.sC2 = strideC2, g.sBias2 = strideBias2, g.sMask2 = strideMask2;
  g.vecA = g.vecA && (strideA2 % 4 == 0);
  g.vecB = g.vecB && (strideB2 % 4 == 0);
  return gemm_launch(g, a_kmajor, b_kmajor, static_cast<hipStream_t>(stream));
}

int curla_gemm_multi(int nprob, const float* const* A, const float* const* B, float* const* C, int lda, int ldb, int ldc,
                     int M, int N, int K, int ksplit, long long split_stride, void* stream) {
  CURLA_REQUIRE(nprob > 0 && nprob <= 4 && A && B && C && M > 0 && N > 0 && K > 0 && ksplit > 0);
  GemmArgs g = gemm_args(nullptr, lda, 0, nullptr, ldb, 0, nullptr, ldc, 0, M, N, K, nprob);
  g.ksplit = ksplit, g.sSplit = split_stride;
  g.nptr = nprob;
  for (int i = 0; i < nprob; ++i) {
    CURLA_REQUIRE(A[i] && B[i] && C[i]);
    g.Ap[i] = A[i], g.Bp[i] = B[i], g.Cp[i] = C[i];
    g.vecA = g.vecA && aligned16(A[i]);
    g.vecB = g.vecB && aligned16(B[i]);
  }
  return gemm_launch(g, 0, 0, static_cast<hipStream_t>(stream));
}

int curla_fc_fwd_multi(int nprob, const float* const* x, const float* const* W, float* const* partial, int B, int F, int K,
                       int nsplit, long long split_stride, int x_blocked, void* stream) {
  CURLA_REQUIRE(nprob > 0 && nprob <= 4 && x && W && partial && B > 0 && F > 0 && K > 0 && nsplit > 0);
  // the instantiated shapes (fc_plan.h); everything else: CURLA_ERR_UNSUPPORTED (the caller takes curla_gemm_multi)
  FcFwdPlan p;
  const int prc = fc_fwd_plan(nprob, B, F, K, nsplit, split_stride, curla_opt(kOptGemmMfma), p);
  if (prc != CURLA_OK) return prc;
  FcFwdArgs g;
  for (int i = 0; i < 4; ++i) {
    g.x[i] = i < nprob ? x[i] : nullptr, g.W[i] = i < nprob ? W[i] : nullptr, g.out[i] = i < nprob ? partial[i] : nullptr;
    if (i < nprob) {
      CURLA_REQUIRE(x[i] && W[i] && partial[i]);
      if (!aligned16(x[i]) || !aligned16(W[i]) || (reinterpret_cast<uintptr_t>(partial[i]) & 7)) return CURLA_ERR_UNSUPPORTED;
    }
  }
  g.nprob = nprob, g.B = B, g.F = F, g.K = K, g.nsplit = nsplit, g.nrg = p.nrg, g.split_stride = split_stride;
  g.blocked = x_blocked ? 1 : 0;
  const size_t lds = (size_t)p.lds;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.nt == 3) {
    if (p.b3) return launch(fc_fwd_kernel<3, 2, true>, p.grid, 256, lds, st, g);
    return launch(fc_fwd_kernel<3, 2, false>, p.grid, 256, lds, st, g);
  }
  if (p.b3) return launch(fc_fwd_kernel<4, 0, true>, p.grid, 256, lds, st, g);
  return launch(fc_fwd_kernel<4, 0, false>, p.grid, 256, lds, st, g);
}

static int fc_bwd_check(const float* dz, const float* big, const float* out, int B, int F, int K) {
  CURLA_REQUIRE(dz && big && out && B > 0 && F > 0 && K > 0);
  if (fc_bwd_shape(F, K) != CURLA_OK || !aligned16(big) || !aligned16(out)) return CURLA_ERR_UNSUPPORTED;
  return CURLA_OK;
}

int curla_fc_dx(const float* dz, const float* W, const float* mask, float* dx, int B, int F, int K, void* stream) {
  int rc = fc_bwd_check(dz, W, dx, B, F, K);
  if (rc != CURLA_OK) return rc;
  if (mask && !aligned16(mask)) return CURLA_ERR_UNSUPPORTED;
  FcBwdArgs g;
  g.dz = dz, g.W = W, g.mask = mask, g.out = dx, g.B = B, g.F = F, g.K = K;
  hipStream_t st = static_cast<hipStream_t>(stream);
  FcDxPlan p;
  if ((rc = fc_dx_plan(F, K, p)) != CURLA_OK) return rc;
  if (p.ks == 4) return launch(fc_dx_kernel<4>, p.grid, 256, 0, st, g);
  if (p.ks == 8) return launch(fc_dx_kernel<8>, p.grid, 256, 0, st, g);
  if (p.ks == 13) return launch(fc_dx_kernel<13>, p.grid, 256, 0, st, g);
  return launch(fc_dx_kernel<16>, p.grid, 256, 0, st, g);
}

// a separate launch for the deferred LayerNorm sums, for the shapes whose fc backward does not take the one-pass kernel
__global__ void ln_reduce_kernel(LnReduce r) { ln_reduce_block(r); }

static int ln_reduce_args(LnReduce& r, const float* partial, int nparts, int F, float* dgamma, float* dbeta,
                          float* dbias) {
  r.partial = partial, r.nparts = nparts, r.F = F, r.dgamma = dgamma, r.dbeta = dbeta, r.dbias = dbias;
  r.xpartial = nullptr, r.xparts = r.xlen = 0, r.xout = nullptr;
  if (!partial) return CURLA_OK;
  CURLA_REQUIRE(nparts > 0 && dgamma && dbeta);
  return CURLA_OK;
}

static int fc_dw_impl(const float* dz, const float* x, float* dW, int B, int F, int K, void* stream, const LnReduce& lnr) {
  int rc = fc_bwd_check(dz, x, dW, B, F, K);
  if (rc != CURLA_OK) return rc;
  FcBwdArgs g;
  g.dz = dz, g.W = x, g.mask = nullptr, g.out = dW, g.B = B, g.F = F, g.K = K;
  hipStream_t st = static_cast<hipStream_t>(stream);
  FcDwPlan p;
  if ((rc = fc_dw_plan(B, F, K, lnr.partial != nullptr, p)) != CURLA_OK) return rc;
  if (p.one_pass) {  // the one-pass kernel's weight-gradient half
    FcBwdArgs gx;
    gx.dz = dz, gx.W = nullptr, gx.mask = x, gx.out = nullptr, gx.B = B, gx.F = F, gx.K = K;
    return launch_fc_bwd(p.op, gx, dW, lnr, st);
  }
  if (p.ln_launch && (rc = launch(ln_reduce_kernel, 1, 256, 0, st, lnr)) != CURLA_OK) return rc;
  const size_t lds = (size_t)p.lds;  // 16 KB per feature tile
  if (p.nt == 1) return launch(fc_dw_kernel<1>, p.grid, 256, lds, st, g);
  if (p.nt == 2) return launch(fc_dw_kernel<2>, p.grid, 256, lds, st, g);
  if (p.nt == 3) return launch(fc_dw_kernel<3>, p.grid, 256, lds, st, g);
  return launch(fc_dw_kernel<4>, p.grid, 256, lds, st, g);
}

int curla_fc_dw(const float* dz, const float* x, float* dW, int B, int F, int K, void* stream) {
  return fc_dw_impl(dz, x, dW, B, F, K, stream, LnReduce{});
}

int curla_fc_dw_ln(const float* dz, const float* x, float* dW, int B, int F, int K, const float* ln_partial, int nparts,
                   float* dgamma, float* dbeta, float* dbias_in, void* stream) {
  LnReduce r;
  int rc = ln_reduce_args(r, ln_partial, nparts, F, dgamma, dbeta, dbias_in);
  if (rc != CURLA_OK) return rc;
  return fc_dw_impl(dz, x, dW, B, F, K, stream, r);
}

static int fc_bwd_impl(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                       void* stream, const LnReduce& lnr) {
  int rc = fc_bwd_check(dz, W, dx, B, F, K);
  if (rc != CURLA_OK) return rc;
  if ((rc = fc_bwd_check(dz, x, dW, B, F, K)) != CURLA_OK) return rc;
  // the one-pass kernel where it is instantiated (fc_plan.h); anything else takes the two streaming kernels
  FcBwdPlan p;
  if ((rc = fc_bwd_plan(B, F, K, lnr.partial != nullptr, p)) != CURLA_OK) return rc;
  if (p.two_launches) {
    if ((rc = curla_fc_dx(dz, W, x, dx, B, F, K, stream)) != CURLA_OK) return rc;
    return fc_dw_impl(dz, x, dW, B, F, K, stream, lnr);
  }
  FcBwdArgs gx;
  gx.dz = dz, gx.W = W, gx.mask = x, gx.out = dx, gx.B = B, gx.F = F, gx.K = K;
  return launch_fc_bwd(p.op, gx, dW, lnr, static_cast<hipStream_t>(stream));
}

int curla_fc_bwd(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                 void* stream) {
  return fc_bwd_impl(dz, W, x, dx, dW, B, F, K, stream, LnReduce{});
}

int curla_fc_bwd_ln(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                    const float* ln_partial, int nparts, float* dgamma, float* dbeta, float* dbias_in, void* stream) {
  LnReduce r;
  int rc = ln_reduce_args(r, ln_partial, nparts, F, dgamma, dbeta, dbias_in);
  if (rc != CURLA_OK) return rc;
  return fc_bwd_impl(dz, W, x, dx, dW, B, F, K, stream, r);
}

int curla_fc_bwd_ln2(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                     const float* ln_partial, int nparts, float* dgamma, float* dbeta, float* dbias_in,
                     const float* extra_partial, int extra_parts, int extra_len, float* extra_out, void* stream) {
  CURLA_REQUIRE(ln_partial && extra_partial && extra_out && extra_parts > 0 && extra_len > 0);
  LnReduce r;
  int rc = ln_reduce_args(r, ln_partial, nparts, F, dgamma, dbeta, dbias_in);
  if (rc != CURLA_OK) return rc;
  r.xpartial = extra_partial, r.xparts = extra_parts, r.xlen = extra_len, r.xout = extra_out;
  return fc_bwd_impl(dz, W, x, dx, dW, B, F, K, stream, r);
}

int curla_splitk_reduce(const float* partial, int nsplit, long long split_stride, int M, int N, int ldp, float* C,
                        int ldc, const float* bias, int relu, void* stream) {
  CURLA_REQUIRE(partial && C && nsplit > 0 && M > 0 && N > 0);
  return launch(splitk_reduce_kernel, (M * N + 255) / 256, 256, 0, static_cast<hipStream_t>(stream), partial, nsplit,
                split_stride, M, N, ldp, C, ldc, bias, relu);
}

}  // extern "C"
