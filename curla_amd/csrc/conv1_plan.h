// The plans of the first conv layer (3x3, stride 2, C -> 32) as host-only code: row sizes of a crop kept in LDS, the
// bands of the banded kernels and their LDS bytes, the grid of the uint8 row walk, and which form runs.  Like
// conv_plan.h and gemm_plan.h nothing here uses a device builtin or asks the device anything: option values, the CU
// count and ablation switches are arguments, so the plans run (and are tested, tests/test_conv1_plan_host.py, through
// tests/capi/conv_plan_probe.cpp) without a GPU.  conv.hip keeps thin wrappers that read curla_opt / curla_cu_count.
#pragma once

#include <stddef.h>

#include "conv_plan.h"
#include "options.h"

namespace conv1 {

// bytes of a crop row kept as bytes in LDS (conv1_row_bytes of conv1_band.h) / floats of one kept as floats
// (conv1_row_stride), and the tallest band of 2 th + 1 byte rows within `budget` bytes
inline int u8_row_bytes(int Wc, int C) { return ((Wc * C + 15) & ~15) + 16; }
inline int f32_row_floats(int Wc, int C) { return ((Wc * C + 3) & ~3) + 4; }
inline int u8_band_rows(int Ho, int RSb, size_t budget) {
  int th = Ho;
  while (th > 1 && (size_t)(2 * th + 1) * RSb > budget) --th;
  return th;
}

// LDS budgets of the banded uint8 kernels: two 512-thread workgroups per CU (the four-wave weight gradient: four of 256)
constexpr size_t kConv1U8BandBudget = 76 * 1024;
constexpr size_t kWgrad1U8BandBudget = 76 * 1024, kWgrad1U8BandBudget4 = 38 * 1024;
// ... and of the float bands: the forward (two workgroups per CU) and the weight gradient (one)
constexpr size_t kConv1F32BandBudget = 76 * 1024, kWgrad1F32BandBudget = 150 * 1024;

// band height of the float banded kernels: the th within `lds_budget` that wastes the fewest tile slots of 8 waves and
// halo rows (g_px_per_row output-gradient pixels per band row of lds_pix floats ride along where a kernel stages them)
inline int plan_band_conv1(int Ho, int Wo, int Wc, int C, int g_px_per_row, size_t lds_budget, int lds_pix) {
  const int RS = f32_row_floats(Wc, C);
  int best = 1;
  double best_eff = -1.0;
  for (int th = 1; th <= Ho; ++th) {
    const size_t bytes = ((size_t)(2 * th + 1) * RS + (size_t)g_px_per_row * th * lds_pix) * sizeof(float);
    if (bytes > lds_budget) break;
    const int nb = (Ho + th - 1) / th;
    double work = 0, slots = 0;
    for (int bnd = 0; bnd < nb; ++bnd) {
      const int tha = (bnd == nb - 1) ? Ho - bnd * th : th;
      const int tiles = (tha * Wo + 15) / 16;
      work += tha * Wo / 16.0;
      slots += ((tiles + 7) / 8) * 8;
    }
    const double eff = work / slots * (2.0 * th) / (2.0 * th + 1 + 2);
    if (eff > best_eff) best_eff = eff, best = th;
  }
  return best;
}

// LDS bytes of a float band launch: 2 th + 1 rows of floats, or the other thing the same bytes hold (the forward's
// weight image, the weight gradient's slab)
inline size_t f32_band_lds(int th, int Wc, int C, size_t other_bytes) {
  const size_t band = ((size_t)(2 * th + 1) * f32_row_floats(Wc, C) + 8) * sizeof(float);
  return band > other_bytes ? band : other_bytes;
}
inline size_t conv1_weight_image_bytes(int C) { return (size_t)32 * C * 9 * sizeof(float); }
inline size_t wgrad1_slab_bytes(int C) { return (size_t)(32 * C * 9 + 32) * sizeof(float); }

// near-equal bands of 2 th + 1 byte rows within `budget`: th and nbands of a banded uint8 kernel
struct Bands {
  int th, nbands;
};
inline Bands plan_u8_bands(int Ho, int RSb, size_t budget) {
  const int th = u8_band_rows(Ho, RSb, budget);
  Bands b;
  b.nbands = (Ho + th - 1) / th;
  b.th = (Ho + b.nbands - 1) / b.nbands;
  return b;
}

// Conv1U8Form::Hybrid / Band: the band stays bytes in LDS, the tallest that leaves room for two workgroups per CU; the
// same bytes first hold the kernels' k-major weight image.  The LDS bytes of the launch.
inline size_t conv1_u8_band_lds(int th, int Wc, int C) {
  const size_t band = (size_t)(2 * th + 1) * u8_row_bytes(Wc, C) + 32;
  const size_t weights = (size_t)3 * ((3 * C + 3) & ~3) * 32 * sizeof(float);
  return band > weights ? band : weights;
}

// The uint8 weight gradient's LDS (nwaves = 8: two 512-thread workgroups per CU of <= 76 KB each; 4: four 256-thread
// ones of <= 38 KB): the band, the slab and the final cross-wave sum.
inline size_t wgrad1_u8_lds(int th, int Wc, int C, int nwaves, bool b16) {
  const int RSb = u8_row_bytes(Wc, C);
  size_t lds = (((size_t)(2 * th + 1) * RSb + 15) & ~(size_t)15) + 32;
  const size_t slab = wgrad1_slab_bytes(C);
  if (slab > lds) lds = slab;
  if ((size_t)nwaves * 1024 > lds) lds = (size_t)nwaves * 1024;  // the final cross-wave sum: one tile of every wave
  // ... and all of a wave's tiles at once (ONE pass of the sum: 48.3 -> 44.8 us at 84x84x9) where two workgroups of that
  // size still share a CU
  if (nwaves == 8) {
    const int k9 = 9 * C, ntiles = 2 * ((k9 % 16 == 1) ? k9 / 16 : (k9 + 15) / 16);
    const size_t one_pass = (size_t)ntiles * nwaves * 1024;
    if (one_pass <= 80 * 1024 && one_pass > lds) lds = one_pass;
  }
  if (b16) {
    const int ntd = (3 * C + 15) / 16;
    const size_t one_pass = (size_t)(2 * 3 * ntd) * nwaves * 1024;
    if (one_pass <= 80 * 1024 && one_pass > lds) lds = one_pass;
  }
  return lds;
}

// grid of the uint8 row walk (conv1_u8_rw.h): `per_cu` workgroups of `threads` per CU; fewer when a workgroup's share of
// the pool of steps (both minibatches) would drop below 8 steps per wave
inline int conv1_u8_rw_grid(long long pool, int threads, int per_cu, int cus) {
  const int cap = per_cu * cus;
  const int share = 8 * (threads / 64);
  const long long want = (pool + share - 1) / share;
  return want < cap ? (want < 1 ? 1 : (int)want) : cap;
}

// workgroup shapes of the uint8 row walk: f32-input MFMA (two 512-thread workgroups per CU) / bf16 matrix cores (three of 256)
constexpr int kC1U8Threads = 512, kC1U8PerCU = 2;
constexpr int kC1U8bThreads = 256, kC1U8bPerCU = 3;

// First-layer forward from the uint8 ring (`opt` = the value of option conv1_u8; the measurements behind it: conv.hip).
//   auto, rwb: Rwb where 3 C <= 32, else Rw;  rw: Rw;  hybrid, band: never a row walk.
//   A shape beyond the row walk's index limits, and hybrid / band, take Hybrid where the whole crop is one band of LDS
//   that leaves room for two workgroups per CU and a row is at most 64 16-byte runs (its staging gives a lane one run of
//   a row) -- unless the option says band; else Band.
enum class Conv1U8Form { Rwb, Rw, Hybrid, Band };
inline Conv1U8Form select_conv1_u8_form(int opt, int C, int Hs, int Ws, int Wc, int Btotal, int Ho, int Wo) {
  const bool walk_asked = opt == kConv1U8Auto || opt == kConv1U8Rw || opt == kConv1U8Rwb;
  const bool walk_fits =
      (long long)Hs * Ws * C < (1LL << 30) && (long long)Btotal * Ho * ((Wo + 15) / 16 + 1) < (1LL << 28);
  if (walk_asked && walk_fits) return opt != kConv1U8Rw && 3 * C <= 32 ? Conv1U8Form::Rwb : Conv1U8Form::Rw;
  const bool one_band = u8_band_rows(Ho, u8_row_bytes(Wc, C), kConv1U8BandBudget) == Ho;
  return one_band && Wc * C <= 64 * 16 && opt != kConv1U8Band ? Conv1U8Form::Hybrid : Conv1U8Form::Band;
}

// First layer and its weight gradient from a float tensor (`opt` = option conv1_f32): the row walk with nothing staged
// (conv1_rw.h) for NHWC minibatches within its 30-bit byte offsets, else the banded kernels.
enum class Conv1F32Form { Rw, Band };
inline Conv1F32Form select_conv1_f32_form(int opt, bool nhwc, int C, int Hc, int Wc) {
  const bool rw = nhwc && opt == kConv1F32Rw && (long long)Hc * Wc * C * 4 < (1LL << 30);
  return rw ? Conv1F32Form::Rw : Conv1F32Form::Band;
}

// First-layer weight gradient from the uint8 ring (`opt` = option wgrad1_u8; four_wave: the ablation build asks for the
// four-wave form, taken where a band of four rows fits its budget).
enum class Wgrad1U8Form { B16, F32, F32FourWave };
inline Wgrad1U8Form select_wgrad1_u8_form(int opt, bool four_wave, int C, int Wc, int Wo) {
  if (four_wave && (size_t)(2 * 4 + 1) * u8_row_bytes(Wc, C) <= kWgrad1U8BandBudget4) return Wgrad1U8Form::F32FourWave;
  return opt != kWgrad1U8F32 && Wo >= 8 && 3 * C <= 32 ? Wgrad1U8Form::B16 : Wgrad1U8Form::F32;
}

}  // namespace conv1
