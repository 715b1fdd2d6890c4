// Prints the plans of csrc/conv_plan.h and csrc/conv1_plan.h for every line of its standard input
// (tests/test_conv_plan_host.py, tests/test_conv1_plan_host.py): host code only, nothing from ROCm.  One plan per line.
//
// Stride-1 strip plans, three fields:  form Ho Wo
// form "s1":       rw::plan (and rwb::plan, checked to be the same), the forward / data gradient on pixel pairs
// form "f43":      rw43::plan, the forward / data gradient on pixel quads
// form "wgrad_x":  rw::plan4, the weight gradient with Winograd along x
// form "wgrad_xy": rw::plan4p, the weight gradient with Winograd in both directions (rows are row pairs)
// Ho Wo are the planned output extents: the forward's output, the data gradient's Hi + 2, Wi + 2, the weight gradient's
// gradient extents.  Prints "nfull brem nr nseg ntr steps".
//
// First layer (3x3, stride 2):  c1 C Hc Wc  (crop Hc x Wc of C channels; the ring's frames are taken to be the crop,
// two samples) prints, in this order,
//   Ho Wo RSb RSf                       output extents, u8_row_bytes, f32_row_floats
//   th nbands lds                       the uint8 forward's bands (plan_u8_bands at its budget) and conv1_u8_band_lds
//   f_auto f_hybrid f_band f_rw f_rwb   select_conv1_u8_form under every value of option conv1_u8 (0 Rwb 1 Rw 2 Hybrid 3 Band)
//   w_auto w_f32 w_b16                  select_wgrad1_u8_form under every value of option wgrad1_u8 (0 B16 1 F32)
//   wth wnbands wlds_f32 wlds_b16       the uint8 weight gradient's bands and wgrad1_u8_lds of its two forms
//   fth flds gth glds                   plan_band_conv1 + f32_band_lds of the float forward / float weight gradient
//   s_nhwc_rw s_nhwc_band s_nchw_rw     select_conv1_f32_form (0 Rw 1 Band) by source and option conv1_f32
//   6 ints, 6 ints                      plan_units over Wo with 16 lane groups (forward walks) and 4 (wgrad1_rw)
// and  grid b16 pool cus  prints conv1_u8_rw_grid of the uint8 row walk (b16 = 1: the bf16 form's workgroup shape) and
// the waves per workgroup.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "conv1_plan.h"
#include "conv_plan.h"

static void print_geom(const rw::Geom& g, const char* end) {
  printf("%d %d %d %d %d %d%s", g.nfull, g.brem, g.nr, g.nseg, g.ntr, g.steps, end);
}

static int first_layer(int C, int Hc, int Wc) {
  using namespace conv1;
  if ((C != 3 && C != 6 && C != 9 && C != 12) || Hc < 3 || Wc < 3 || Hc > 4096 || Wc > 4096) return 2;
  const int Ho = (Hc - 3) / 2 + 1, Wo = (Wc - 3) / 2 + 1, RSb = u8_row_bytes(Wc, C);
  printf("%d %d %d %d ", Ho, Wo, RSb, f32_row_floats(Wc, C));
  const Bands fb = plan_u8_bands(Ho, RSb, kConv1U8BandBudget);
  printf("%d %d %zu ", fb.th, fb.nbands, conv1_u8_band_lds(fb.th, Wc, C));
  for (int opt = 0; opt < kConv1U8Values; ++opt) printf("%d ", (int)select_conv1_u8_form(opt, C, Hc, Wc, Wc, 2, Ho, Wo));
  for (int opt = 0; opt < kWgrad1U8Values; ++opt) printf("%d ", (int)select_wgrad1_u8_form(opt, false, C, Wc, Wo));
  const Bands wb = plan_u8_bands(Ho, RSb, kWgrad1U8BandBudget);
  printf("%d %d %zu %zu ", wb.th, wb.nbands, wgrad1_u8_lds(wb.th, Wc, C, 8, false), wgrad1_u8_lds(wb.th, Wc, C, 8, true));
  const int fth = plan_band_conv1(Ho, Wo, Wc, C, 0, kConv1F32BandBudget, 36);
  const int gth = plan_band_conv1(Ho, Wo, Wc, C, 0, kWgrad1F32BandBudget, 36);
  printf("%d %zu %d %zu ", fth, f32_band_lds(fth, Wc, C, conv1_weight_image_bytes(C)), gth,
         f32_band_lds(gth, Wc, C, wgrad1_slab_bytes(C)));
  printf("%d %d %d ", (int)select_conv1_f32_form(kConv1F32Rw, true, C, Hc, Wc),
         (int)select_conv1_f32_form(kConv1F32Band, true, C, Hc, Wc), (int)select_conv1_f32_form(kConv1F32Rw, false, C, Hc, Wc));
  rw::Geom g;
  g.Hi = Hc, g.Wi = Wc, g.Ho = Ho, g.Wo = Wo;
  rw::plan_units(g, Ho, Wo, 16);
  print_geom(g, " ");
  rw::plan_units(g, Ho, Wo, 4);
  print_geom(g, "\n");
  return 0;
}

int main() {
  char form[16];
  while (scanf("%15s", form) == 1) {
    if (!strcmp(form, "c1")) {
      int C, Hc, Wc;
      if (scanf("%d %d %d", &C, &Hc, &Wc) != 3) return 2;
      if (const int rc = first_layer(C, Hc, Wc)) return rc;
      continue;
    }
    if (!strcmp(form, "grid")) {
      int b16, cus;
      long long pool;
      if (scanf("%d %lld %d", &b16, &pool, &cus) != 3 || pool < 0 || pool > INT_MAX || cus < 1 || cus > 4096) return 2;
      const int threads = b16 ? conv1::kC1U8bThreads : conv1::kC1U8Threads;
      printf("%d %d\n", conv1::conv1_u8_rw_grid(pool, threads, b16 ? conv1::kC1U8bPerCU : conv1::kC1U8PerCU, cus), threads / 64);
      continue;
    }
    int Ho, Wo;
    if (scanf("%d %d", &Ho, &Wo) != 2) return 2;
    if (Ho < 1 || Wo < 1) return 2;
    rw::Geom g;
    if (!strcmp(form, "s1")) {
      g = rw::plan(Ho + 2, Wo + 2, Ho, Wo);
      const rw::Geom b = rwb::plan(Ho + 2, Wo + 2, Ho, Wo);
      if (b.nfull != g.nfull || b.brem != g.brem || b.nr != g.nr || b.nseg != g.nseg || b.ntr != g.ntr || b.steps != g.steps)
        return 3;
    } else if (!strcmp(form, "f43")) {
      g = rw43::plan(Ho + 2, Wo + 2, Ho, Wo);
    } else if (!strcmp(form, "wgrad_x")) {
      g = rw::plan4(Ho + 2, Wo + 2, Ho, Wo);
    } else if (!strcmp(form, "wgrad_xy")) {
      g = rw::plan4p(Ho + 2, Wo + 2, Ho, Wo);
    } else {
      return 2;
    }
    print_geom(g, "\n");
  }
  return feof(stdin) ? 0 : 2;
}
