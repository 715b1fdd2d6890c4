// Prints the plan of csrc/gemm_plan.h for every product on its standard input (tests/test_gemm_plan_host.py): host code
// only, nothing from ROCm.  One product per line, 20 fields:
//   kind M N K nbatch ksplit a_kmajor b_kmajor vecA vecB bias mask relu colsum nptr cu gemm_tile gemm_mfma linear_bwd force_big
// kind "gemm": one product as curla_gemm / _colsum / _nested / _multi hand it to gemm_plan.
// kind "bwd":  curla_linear_bwd of a layer with M = batch rows, N = out features, K = in features (vecA: dy aligned,
//              vecB: x and W aligned, mask / colsum: the ReLU mask / the bias gradient are asked for; ksplit, the layout,
//              bias, relu, nptr and force_big are not read).
#include <stdio.h>
#include <string.h>

#include "gemm_plan.h"

static float dummy[4];

static void print_plan(const char* name, const GemmArgs& g, const GemmPlan& p, int rc) {
  printf("%s rc=%d small=%d wide=%d tbm=%d tbn=%d fast=%d b3=%d kchunk=%d stream_c=%d", name, rc, p.small, p.wide, p.tbm,
         p.tbn, p.fast, p.b3, g.kchunk, g.stream_c);
}

static GemmArgs product(int M, int N, int K, int nbatch, int vecA, int vecB) {
  GemmArgs g = {};
  g.M = M, g.N = N, g.K = K, g.nbatch = g.nb_inner = nbatch, g.ksplit = 1, g.alpha = 1.f, g.vecA = vecA, g.vecB = vecB;
  return g;
}

int main() {
  char kind[16];
  int M, N, K, nbatch, ksplit, ak, bk, vecA, vecB, bias, mask, relu, colsum, nptr, force_big;
  GemmEnv env;
  while (scanf("%15s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", kind, &M, &N, &K, &nbatch, &ksplit, &ak, &bk,
               &vecA, &vecB, &bias, &mask, &relu, &colsum, &nptr, &env.cu, &env.tile, &env.mfma, &env.linear_bwd,
               &force_big) == 20) {
    if (!strcmp(kind, "gemm")) {
      GemmArgs g = product(M, N, K, nbatch, vecA, vecB);
      g.ksplit = ksplit, g.relu = relu, g.nptr = nptr;
      g.bias = bias ? dummy : nullptr, g.mask = mask ? dummy : nullptr, g.colsum = colsum ? dummy : nullptr;
      GemmPlan p;
      const int rc = gemm_plan(g, ak, bk, env, p, force_big != 0);
      print_plan("gemm", g, p, rc);
      printf("\n");
    } else if (!strcmp(kind, "bwd")) {
      GemmArgs g1 = product(N, K, M, nbatch, vecA, vecB), g2 = product(M, K, N, nbatch, vecA, vecB);
      g1.colsum = colsum ? dummy : nullptr, g2.mask = mask ? dummy : nullptr;
      LinearBwdPlan q;
      const int rc = linear_bwd_plan(g1, g2, env, q);
      static const char* const names[] = {"two", "small_pair", "big_pair", "tiled_pair"};
      int t[4] = {0, 0, 0, 0};
      if (rc == CURLA_OK && q.kind == kBwdSmallPair) t[0] = t[1] = t[2] = t[3] = 16;
      if (rc == CURLA_OK && q.kind == kBwdBigPair) t[0] = t[2] = 128, t[1] = t[3] = 64;
      if (rc == CURLA_OK && q.kind == kBwdTiledPair) memcpy(t, kPairTiles[q.pair], sizeof t);
      if (rc != CURLA_OK) {
        printf("bwd rc=%d\n", rc);
      } else if (q.kind != kBwdTwoLaunches) {
        printf("bwd rc=0 %s second_first=%d tiles=%d,%d,%d,%d b3=%d grid=%d,%d,%d,%d n1=%lld n2=%lld kchunk=%d,%d stream_c=%d,%d\n",
               names[q.kind], q.second_first, t[0], t[1], t[2], t[3], q.kind == kBwdBigPair || q.b3, q.gx1, q.gy1, q.gx2,
               q.gy2, q.n1, q.n2, g1.kchunk, g2.kchunk, g1.stream_c, g2.stream_c);
      } else {  // two launches: each product planned on its own, as gemm_launch does
        GemmPlan p1, p2;
        const int rc1 = gemm_plan(g1, 1, 1, env, p1), rc2 = gemm_plan(g2, 0, 1, env, p2);
        printf("bwd rc=0 two ");
        print_plan("dW", g1, p1, rc1);
        print_plan(" dx", g2, p2, rc2);
        printf("\n");
      }
    } else {
      return 2;
    }
  }
  return feof(stdin) ? 0 : 2;
}
