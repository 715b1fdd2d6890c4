// The strip plans of the stride-1 row-walk convolutions, as host-only code: the geometry block the kernels walk
// (rw::Geom), the planner (rw::plan_units) and the plan of every form -- forward / data gradient with Winograd F(2,3)
// (rw::plan; rwb::plan: the bf16x3 form walks the same strips) and F(4,3) (rw43::plan), weight gradient with Winograd
// along x (rw::plan4) and in both directions (rw::plan4p).  Nothing here uses a device builtin or asks the device
// anything, so the plans run (and are tested, tests/test_conv_plan_host.py) without a GPU.  Included by conv_rw.h, in
// front of the kernels that walk the plans (conv_rw.h, conv_rw43.h, conv_rwb.h, conv_rw_wgrad.h, conv_rw_wgrad2.h).
//
// Strips.  An image row has PW = ceil(Wo / 2) pairs.  Columns 16k .. 16k+15 form full strip k (Ho steps).  The b =
// PW mod 16 remaining columns are cut into vertical segments of nr rows so that 16 lanes are (column, segment)
// units: a remainder strip takes nr steps and its lanes start at different rows.  (Ho, Wo) = (35, 35): one full
// strip (35 steps) + 2 columns x 7 segments of 5 rows (5 steps) = 40 steps against 39.4 ideal.
#pragma once

namespace rw {

struct Geom {
  int Hi, Wi;    // input rows / columns
  int Ho, Wo;    // output rows / columns (forward: Hi-2, Wi-2; data gradient: Hi+2, Wi+2)
  int nfull;     // full strips
  int brem;      // remaining pair columns (0..15)
  int nr;        // rows per segment of the remainder strips
  int nseg;      // segments per remaining column = ceil(Ho / nr)
  int ntr;       // remainder strips = ceil(brem * nseg / 16)
  int steps;     // steps per sample = nfull * Ho + ntr * nr
};

// host: strips of `per` columns over `cols` column units and Ho rows (see "Strips" above): full strips of Ho steps,
// and the remaining columns cut into vertical segments of nr rows so that `per` lane groups are (column, segment) units
inline void plan_units(Geom& g, int Ho, int cols, int per) {
  g.nfull = cols / per, g.brem = cols % per;
  g.nr = g.nseg = g.ntr = 0;
  if (g.brem) {
    // segments of nr rows: brem * ceil(Ho / nr) units on `per` lane groups per strip; cost = strips x nr steps
    long best = -1;
    for (int nr = 1; nr <= Ho; ++nr) {
      const int nseg = (Ho + nr - 1) / nr;
      const int ntr = (g.brem * nseg + per - 1) / per;
      // a step costs the same whatever it computes; short segments also spend 2 of their nr + 2 row loads on halo
      const long cost = (long)ntr * nr * 64 + (long)ntr * 2 * 8;
      if (best < 0 || cost <= best) best = cost, g.nr = nr, g.nseg = nseg, g.ntr = ntr;
    }
  }
  g.steps = g.nfull * Ho + g.ntr * g.nr;
}

// strip plan of the stride-1 forward / data gradient: 16 pixel-pair columns per wave
inline Geom plan(int Hi, int Wi, int Ho, int Wo) {
  Geom g;
  g.Hi = Hi, g.Wi = Wi, g.Ho = Ho, g.Wo = Wo;
  plan_units(g, Ho, (Wo + 1) / 2, 16);
  return g;
}

// (weight gradient, conv_rw_wgrad.h) strips of 4 pair columns (one per lane group)
inline Geom plan4(int Hi, int Wi, int Ho, int Wo) {
  Geom g;
  g.Hi = Hi, g.Wi = Wi, g.Ho = Ho, g.Wo = Wo;
  plan_units(g, Ho, (Wo + 1) / 2, 4);
  return g;
}

// (weight gradient, conv_rw_wgrad2.h) strips of 4 pair columns over the gradient image in units of ROW PAIRS
// (Geom::Ho = pair rows)
inline Geom plan4p(int Hi, int Wi, int Ho, int Wo) {
  Geom g;
  g.Hi = Hi, g.Wi = Wi, g.Wo = Wo;
  g.Ho = (Ho + 1) / 2;
  plan_units(g, g.Ho, (Wo + 1) / 2, 4);
  return g;
}

}  // namespace rw

namespace rw43 {

// (conv_rw43.h) strip plan: 16 pixel-QUAD columns per wave
inline rw::Geom plan(int Hi, int Wi, int Ho, int Wo) {
  rw::Geom g;
  g.Hi = Hi, g.Wi = Wi, g.Ho = Ho, g.Wo = Wo;
  rw::plan_units(g, Ho, (Wo + 3) / 4, 16);
  return g;
}

}  // namespace rw43

namespace rwb {

// (conv_rwb.h) strip plan: 16 pixel-pair columns per wave (conv_rw.h's)
inline rw::Geom plan(int Hi, int Wi, int Ho, int Wo) { return rw::plan(Hi, Wi, Ho, Wo); }

}  // namespace rwb
