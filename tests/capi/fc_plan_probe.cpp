// Prints the plan of csrc/fc_plan.h and the kernels' walk numbers for every shape on its standard input
// (tests/test_fc_plan_host.py): host code only, nothing from ROCm.  One shape per line, 9 fields:
//   entry B F K nprob nsplit split_stride gemm_mfma ln
// entry "fwd": curla_fc_fwd_multi (ln is not read); "dx": curla_fc_dx; "dw": curla_fc_dw / _dw_ln; "bwd": curla_fc_bwd /
// _bwd_ln / _bwd_ln2 (ln: deferred LayerNorm sums ride along; nprob, nsplit, split_stride and gemm_mfma are not read).
#include <stdio.h>
#include <string.h>

#include "fc_plan.h"

static const char* const kLast[] = {"full", "part", "one"};

static void print_dx(const char* name, int B, int F, int K) {
  FcDxPlan p;
  const int rc = fc_dx_plan(F, K, p);
  if (rc != CURLA_OK) {
    printf("%s rc=%d", name, rc);
    return;
  }
  int tmin, tmax;
  fc_btile_walk((B + 15) >> 4, tmin, tmax);
  printf("%s rc=0 fc_dx_kernel<%d> grid=%d lds=0 btiles=%d..%d last=%s", name, p.ks, p.grid, tmin, tmax,
         kLast[fc_last_block(K)]);
}

static void print_one_pass(const char* name, const FcOnePassPlan& p, int B, int K) {
  int tmin, tmax;
  fc_btile_walk(B >> 4, tmin, tmax);
  printf("%s rc=0 fc_bwd_kernel<%d,%d,%d,%s> grid=%d lds=%lld btiles=%d..%d last=%s", name, p.ks, p.nt, p.ntail,
         p.dx ? "true" : "false", p.grid, p.lds, tmin, tmax, kLast[fc_last_block(K)]);
}

static void print_dw(const char* name, int B, int F, int K, bool ln) {
  FcDwPlan p;
  const int rc = fc_dw_plan(B, F, K, ln, p);
  if (rc != CURLA_OK) {
    printf("%s rc=%d", name, rc);
    return;
  }
  if (p.one_pass) {
    print_one_pass(name, p.op, B, K);
    return;
  }
  int smin, smax;
  fc_dw_walk(B, smin, smax);
  printf("%s rc=0 fc_dw_kernel<%d> grid=%d lds=%lld ln_launch=%d ksteps=%d..%d last=%s", name, p.nt, p.grid, p.lds,
         p.ln_launch, smin, smax, kLast[fc_last_block(K)]);
}

int main() {
  char entry[16];
  int B, F, K, nprob, nsplit, mfma, ln;
  long long split_stride;
  while (scanf("%15s %d %d %d %d %d %lld %d %d", entry, &B, &F, &K, &nprob, &nsplit, &split_stride, &mfma, &ln) == 9) {
    if (B <= 0 || F <= 0 || K <= 0) return 2;
    if (!strcmp(entry, "fwd")) {
      if (nprob <= 0 || nprob > 4 || nsplit <= 0) return 2;
      FcFwdPlan p;
      const int rc = fc_fwd_plan(nprob, B, F, K, nsplit, split_stride, mfma, p);
      if (rc != CURLA_OK) {
        printf("fwd rc=%d\n", rc);
        continue;
      }
      const FcFwdWalk w = fc_fwd_walk(K, nsplit);
      printf("fwd rc=0 fc_fwd_kernel<%d,%d,%s> grid=%d lds=%lld nrg=%d slices=%d..%d mod4=%d%d%d%d chunks=%d..%d odd_start=%d\n",
             p.nt, p.ntail, p.b3 ? "true" : "false", p.grid, p.lds, p.nrg, w.slices_min, w.slices_max, w.mod4 & 1,
             (w.mod4 >> 1) & 1, (w.mod4 >> 2) & 1, (w.mod4 >> 3) & 1, w.chunks_min, w.chunks_max, w.odd_start);
    } else if (!strcmp(entry, "dx")) {
      print_dx("dx", B, F, K);
      printf("\n");
    } else if (!strcmp(entry, "dw")) {
      print_dw("dw", B, F, K, ln != 0);
      printf("\n");
    } else if (!strcmp(entry, "bwd")) {
      FcBwdPlan p;
      const int rc = fc_bwd_plan(B, F, K, ln != 0, p);
      if (rc != CURLA_OK) {
        printf("bwd rc=%d\n", rc);
      } else if (p.two_launches) {  // each product planned on its own, as the entry point runs them
        printf("bwd rc=0 two ");
        print_dx("dx", B, F, K);
        print_dw(" dw", B, F, K, ln != 0);
        printf("\n");
      } else {
        print_one_pass("bwd", p.op, B, K);
        printf("\n");
      }
    } else {
      return 2;
    }
  }
  return feof(stdin) ? 0 : 2;
}
