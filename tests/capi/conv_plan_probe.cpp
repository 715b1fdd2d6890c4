// Prints the strip plan of csrc/conv_plan.h for every line of its standard input (tests/test_conv_plan_host.py): host
// code only, nothing from ROCm.  One plan per line, three fields:
//   form Ho Wo
// form "s1":       rw::plan (and rwb::plan, checked to be the same), the forward / data gradient on pixel pairs
// form "f43":      rw43::plan, the forward / data gradient on pixel quads
// form "wgrad_x":  rw::plan4, the weight gradient with Winograd along x
// form "wgrad_xy": rw::plan4p, the weight gradient with Winograd in both directions (rows are row pairs)
// Ho Wo are the planned output extents: the forward's output, the data gradient's Hi + 2, Wi + 2, the weight gradient's
// gradient extents.  Prints "nfull brem nr nseg ntr steps".
#include <stdio.h>
#include <string.h>

#include "conv_plan.h"

int main() {
  char form[16];
  int Ho, Wo;
  while (scanf("%15s %d %d", form, &Ho, &Wo) == 3) {
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
    printf("%d %d %d %d %d %d\n", g.nfull, g.brem, g.nr, g.nseg, g.ntr, g.steps);
  }
  return feof(stdin) ? 0 : 2;
}
