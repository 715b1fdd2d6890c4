// Which kernel a GEMM takes, as host-only code: the kernels' argument block (GemmArgs), the plan of one product
// (gemm_plan) and of the two products of a linear layer's backward pass (linear_bwd_plan).  Nothing here includes a HIP
// header or asks the device or the options anything: the compute-unit count and the option values arrive in a GemmEnv,
// so the decisions run (and are tested, tests/test_gemm_plan_host.py) without a GPU.  Included by gemm.hip in front of
// its kernel headers.
#pragma once

#include "../../include/curla_hip.h"
#include "options.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32;

struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* mask;
  int M, N, K, lda, ldb, ldc, ldmask;
  long long sA, sB, sC, sBias, sMask, sSplit;
  int nbatch, ksplit, kchunk;
  float alpha;
  int relu, vecA, vecB;
  int stream_c;  // output far larger than the L2s (fc data gradient): streaming stores
  // two-level batch: item = outer * nb_inner + inner at base + inner * s + outer * s2 (e.g. the twin Q functions of
  // the target critic and of the critic: twins a block apart inside a flat buffer, the two flat buffers wherever
  // the allocator put them -- one launch for all four)
  int nb_inner;
  long long sA2, sB2, sC2, sBias2, sMask2;
  // colsum (small-output kernel only): also colsum[z][m] = alpha * sum_k opA[m][k] (a weight gradient dy^T x with the
  // bias gradient, the column sums of dy, from the operands it loads anyway)
  float* colsum;
  long long sColsum, sColsum2;
  // nptr > 0: the batch items are unrelated problems of one shape, given by pointer (A = Ap[batch] ...) instead of by
  // stride -- e.g. the fc products of three encoders on three activation tensors in one launch
  int nptr;
  const float* Ap[4];
  const float* Bp[4];
  float* Cp[4];
};

// what the decisions depend on besides the product itself: the compute units of the device and the values of the
// options gemm_tile, gemm_mfma and linear_bwd (options.h)
struct GemmEnv {
  int cu, tile, mfma, linear_bwd;
};

// small output, long k: one workgroup per 16 x 16 tile, k split over its waves (gemm_small_kernel)
inline bool small_shape(int M, int N, int K, int nbatch) {
  const long long t32 = (long long)((M + 31) / 32) * ((N + 31) / 32) * nbatch;
  return K >= 256 && K % 64 == 0 && t32 <= 128 && nbatch <= 65535;
}

// which kernel a product takes: the small-output kernel (16 or 4 waves per tile) or the tiled one with its tile shape
struct GemmPlan {
  bool small, wide, fast, b3;
  int tbm, tbn;
};

// the tiled kernel's arithmetic (option gemm_mfma): f32 = the f32-input MFMA everywhere; b3 = bf16x3 on the bf16 matrix
// cores for every interior, aligned tile; auto = bf16x3 where the 128 x 64 tile applies, f32 elsewhere.  History
// (profiles/r05_checks/r05_gemm_b3_vs_f32.txt): with the f32 form's own 64 x 64 / 64 x 32 / 32 x 32 tiles bf16x3 bought
// nothing (37.9 against 43.2 us, 45.1 / 45.2, 19.4 / 17.7) -- three bf16 images are 1.5 x the LDS bytes of the f32 tile
// and the matrix instructions take a sixth of the time, so those tiles are bound by LDS stores and fragment reads, not by
// the matrix pipe.  A 128 x 64 tile (a wave: 64 x 32, six fragment reads per 48 matrix instructions) halves the LDS
// traffic per product.

// whether the 128 x 64 bf16x3 tile can take this product at all (whole tiles, aligned operands, no k split)
inline bool big_tile_ok(const GemmArgs& g, const GemmEnv& env) {
  return env.mfma != kGemmMfmaF32 && g.ksplit == 1 && g.vecA && g.vecB && g.K % BK == 0 && g.K >= 4 * BK && g.M % 128 == 0 &&
         g.N % 64 == 0 && !g.colsum;
}
inline long long big_tile_count(const GemmArgs& g) { return (long long)(g.M / 128) * (g.N / 64) * g.nbatch; }

// (sets g.kchunk and g.stream_c of a product that takes the tiled kernel)
inline int gemm_plan(GemmArgs& g, int a_kmajor, int b_kmajor, const GemmEnv& env, GemmPlan& p, bool force_big = false) {
  const int M = g.M, N = g.N, K = g.K, nbatch = g.nbatch, ksplit = g.ksplit;
  p.small = ksplit == 1 && !g.bias && !g.mask && !g.relu && g.nptr == 0 && small_shape(M, N, K, nbatch);
  p.wide = false, p.fast = false, p.b3 = false, p.tbm = p.tbn = 16;
  if (g.colsum && !p.small) return CURLA_ERR_UNSUPPORTED;
  if (p.small) {
    const long long t16 = (long long)((M + 15) / 16) * ((N + 15) / 16) * nbatch;
    p.wide = t16 < 64 && K % 256 == 0;  // a handful of tiles: 16 waves each
    return CURLA_OK;
  }
  int kc = (K + ksplit - 1) / ksplit;
  kc = (kc + BK - 1) / BK * BK;  // chunk boundaries stay float4-aligned
  g.kchunk = kc;
  g.stream_c = (long long)M * N * nbatch * (long long)sizeof(float) >= (32LL << 20);
  // tile shape: 64x64 when that already fills the chip twice, else 64x32, else 32x32 (more, smaller
  // workgroups: at one workgroup per CU nothing hides the L2 latency of the single-buffered k loop)
  const long long cu2 = 2LL * env.cu;
  const long long zb = (long long)nbatch * ksplit;
  const long long wgs64 = (long long)((N + 63) / 64) * ((M + 63) / 64) * zb;
  const long long wgs6432 = (long long)((N + 31) / 32) * ((M + 63) / 64) * zb;
  int tbm = 64, tbn = 64;
  // (the encoder fc forward, [512 x 30752] x [30752 x 50] split 32 ways along K, lands here with 32-wide tiles and
  // so streams its 63 MB activation operand twice, 117 MB of HBM traffic per launch; the single-pass alternative,
  // one 64-wide N tile with a 64-way split, was measured: 26.9 us against 25.5 us -- the product is bound by the
  // padded MFMA work (N = 50 -> 64) and load latency, not by HBM bytes, and more, smaller workgroups hide those better)
  if (wgs64 < cu2 && N > 32) tbn = 32;
  // a single row of tiles streaming a k-major B (the fc weight gradient, M = 50): the wider tile reads 256-B
  // instead of 128-B pieces of each HBM row and is faster even at one workgroup per CU
  if (tbn == 32 && M <= 64 && a_kmajor && b_kmajor && 2 * wgs64 >= cu2) tbn = 64;
  if (tbn == 32 && wgs6432 < cu2 && M > 32) tbm = 32;
  // the 128 x 64 bf16x3 tile where it gives every CU a workgroup (or the caller has counted a pair's tiles together)
  bool big = big_tile_ok(g, env) && (force_big || big_tile_count(g) >= env.cu);
  switch (env.tile) {  // option gemm_tile (options.h; tools/gemm_shapes.py): a forced tile shape
    case kGemmTile6464: tbm = 64, tbn = 64, big = false; break;
    case kGemmTile6432: tbm = 64, tbn = 32, big = false; break;
    case kGemmTile3232: tbm = 32, tbn = 32, big = false; break;
    case kGemmTile12864: big = big_tile_ok(g, env); break;
    default: break;
  }
  if (big) {
    p.tbm = 128, p.tbn = 64, p.fast = true, p.b3 = true;
    g.kchunk = g.K;
    return CURLA_OK;
  }
  p.tbm = tbm, p.tbn = tbn;
  // interior + aligned everywhere: the k loop runs without bounds / alignment tests
  // (a k-major operand still needs whole tiles: its float4 runs along the rows)
  p.fast = g.vecA && g.vecB && (K % BK == 0) && (g.kchunk % BK == 0) && (!a_kmajor || M % tbm == 0) &&
           (!b_kmajor || N % tbn == 0);
  p.b3 = p.fast && env.mfma == kGemmMfmaB3;
  return CURLA_OK;
}

// Backward of a linear layer, g1 = the weight gradient dW = dy^T x (both operands k-major), g2 = the data gradient
// dx = (dy W) masked (W k-major): one launch for both where one kernel has their two tile shapes, else two launches.
enum LinearBwdKind {
  kBwdTwoLaunches,  // neither pair kernel fits both (or option linear_bwd = split): gemm_launch of each
  kBwdSmallPair,    // both take the small-output kernel with 4 waves: gemm_small_pair_kernel
  kBwdBigPair,      // both on the 128 x 64 bf16x3 tile: gemm_pair_kernel<128, 64, 128, 64, true, second_first, 512>
  kBwdTiledPair     // gemm_pair_kernel<row `pair` of kPairTiles, b3>
};
// (TM1, TN1, TM2, TN2) of the tiled pairs that exist: the shapes the twin-Q and the actor MLPs produce at batch 512
// and 1024, hidden 1024
constexpr int kPairTiles[4][4] = {{64, 64, 64, 32}, {64, 32, 32, 32}, {64, 64, 64, 64}, {64, 32, 64, 32}};

struct LinearBwdPlan {
  int kind;
  bool second_first;  // kBwdBigPair: the data gradient's workgroups first
  int pair;           // kBwdTiledPair: the row of kPairTiles
  bool b3;            // kBwdTiledPair: both products on bf16x3
  // tile columns and rows of each product and its workgroups gx * gy * nbatch (the first n1 workgroups of a pair
  // launch take the weight gradient)
  int gx1, gy1, gx2, gy2;
  long long n1, n2;
};

inline int linear_bwd_plan(GemmArgs& g1, GemmArgs& g2, const GemmEnv& env, LinearBwdPlan& q) {
  const bool split = env.linear_bwd == kLinearBwdSplit;  // (option linear_bwd, options.h)
  // the two products' 128 x 64 tiles are counted together: one launch holds both
  const bool both_big =
      !split && big_tile_ok(g1, env) && big_tile_ok(g2, env) && big_tile_count(g1) + big_tile_count(g2) >= env.cu;
  GemmPlan p1, p2;
  int rc = gemm_plan(g1, 1, 1, env, p1, both_big);
  if (rc != CURLA_OK) return rc;
  rc = gemm_plan(g2, 0, 1, env, p2, both_big);
  if (rc != CURLA_OK) return rc;
  q.gx1 = (g1.N + p1.tbn - 1) / p1.tbn, q.gy1 = (g1.M + p1.tbm - 1) / p1.tbm;  // (the small kernel's plan says 16 x 16)
  q.gx2 = (g2.N + p2.tbn - 1) / p2.tbn, q.gy2 = (g2.M + p2.tbm - 1) / p2.tbm;
  q.n1 = (long long)q.gx1 * q.gy1 * g1.nbatch, q.n2 = (long long)q.gx2 * q.gy2 * g2.nbatch;
  q.kind = kBwdTwoLaunches, q.second_first = false, q.pair = -1, q.b3 = false;
  if (split || q.n1 + q.n2 >= (1LL << 30)) return CURLA_OK;
  if (p1.small && p2.small && !p1.wide && !p2.wide) {
    q.kind = kBwdSmallPair;
  } else if (!p1.small && !p2.small && p1.fast && p2.fast && p1.tbm == 128 && p2.tbm == 128) {
    // (the data gradient's tiles run over k = N, the weight gradient's over k = the batch rows: the longer ones first)
    q.kind = kBwdBigPair, q.second_first = g2.K >= g1.K;
  } else if (!p1.small && !p2.small && p1.fast && p2.fast && p1.b3 == p2.b3) {
    for (int i = 0; i < 4 && q.kind == kBwdTwoLaunches; ++i)
      if (p1.tbm == kPairTiles[i][0] && p1.tbn == kPairTiles[i][1] && p2.tbm == kPairTiles[i][2] && p2.tbn == kPairTiles[i][3])
        q.kind = kBwdTiledPair, q.pair = i, q.b3 = p1.b3;
  }
  return CURLA_OK;
}

}  // namespace
