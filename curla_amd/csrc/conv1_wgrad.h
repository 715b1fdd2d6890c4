// Weight gradient of the first conv layer in its forms that stage the input band in LDS, gfx950: from a float tensor
// (wgrad1_kernel) and from the uint8 ring with the band kept as bytes, on the f32-input MFMA (wgrad1_u8_kernel) or on the
// bf16 matrix cores (wgrad1_u8b_kernel).  Included by conv.hip inside its anonymous namespace, after conv1_band.h
// (whose staging helpers it shares) and the stride-1 weight-gradient headers.
#pragma once

// ---------------------------------------------------------------------------
// weight gradient of the first layer (stride 2, Cin = C, input re-read from
// the uint8 frames / float tensor exactly as the forward does).
// D[co][k'] with k' = dy*KR + dx*C + c (the forward's K index), K = pixels.
// ---------------------------------------------------------------------------
struct Wgrad1Args {
  const void* src;
  const int64_t* idx;
  const int32_t* h1;
  const int32_t* w1;
  const float* g;  // [B][Ho][Wo][32]
  float* partial;  // [grid][32*C*9 + 32]
  int B, C, Hs, Ws, Hc, Wc, Ho, Wo, th, nbands;
  float scale;
  unsigned lds_bytes;  // dynamic LDS of the launch (the uint8 kernel sizes its final cross-wave sum by it)
  int dbg;
};

template <int SRC, int C>
__global__ __launch_bounds__(512) void wgrad1_kernel(Wgrad1Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KR = (3 * C + 3) & ~3;
  constexpr int NT = (3 * KR + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int RS = conv1_row_stride(a.Wc, C);
  f32x4 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0, 0, 0, 0};
  float bsum[2] = {0.f, 0.f};
  int koff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = t * 16 + li;
    const int dy = k / KR, rr = k - dy * KR;
    koff[t] = (dy < 3) ? dy * RS + rr : 0;
  }

  const int nitems = a.B * a.nbands;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int band = item / a.B, b = item - band * a.B;  // band-major: every workgroup sees every band size
    const int y0 = band * a.th;
    const int tha = min(a.th, a.Ho - y0);
    conv1_stage<SRC>(lds, a.src, a.idx, a.h1, a.w1, b, C, a.Hs, a.Ws, a.Hc, a.Wc, 2 * y0, 2 * tha + 1, RS, a.scale,
                     tid, 512);
    __syncthreads();
    // (the gradient operand is loaded from HBM/L2 straight into MFMA registers, as in wgrad1_u8_kernel: every pixel
    // is needed by exactly one wave, and lanes with nothing to multiply read a zero page)
    const float* const gband = a.g + ((size_t)(b * a.Ho + y0) * a.Wo) * 32 + li;
    const int npix = tha * a.Wo;
    const int nunits = ((npix + 15) >> 4) << 2;
    // unit u's pixel of lane group kq is p = (u >> 2) * 16 + (u & 3) + 4 kq; this wave's units are u = wave, wave + 8,
    // ...: p advances by 32 per unit -- walked incrementally as (row, column), no division per unit
    int p = (wave >> 2) * 16 + (wave & 3) + 4 * kq;
    int ty = p / a.Wo, x = p - ty * a.Wo;
    const int qstep = 32 / a.Wo, rstep = 32 - qstep * a.Wo;
    for (int u = wave; u < nunits; u += 8) {
      const bool pv = p < npix;
      const float* gp = pv ? gband + p * 32 : g_zero_px;
      const float a0 = gp[0], a1 = gp[16];
      bsum[0] += a0;
      bsum[1] += a1;
      const float* ip = lds + (pv ? __mul24(2 * ty, RS) + __mul24(2 * x, C) : 0);
      float bv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) bv[t] = ip[koff[t]];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[0][t] = mfma16(a0, bv[t], acc[0][t]);
        acc[1][t] = mfma16(a1, bv[t], acc[1][t]);
      }
      p += 32, x += rstep, ty += qstep;  // at most one more wrap
      const bool wrap = x >= a.Wo;
      x = wrap ? x - a.Wo : x;
      ty = wrap ? ty + 1 : ty;
    }
    __syncthreads();
  }

  bsum[0] += __shfl_xor(bsum[0], 16);
  bsum[0] += __shfl_xor(bsum[0], 32);
  bsum[1] += __shfl_xor(bsum[1], 16);
  bsum[1] += __shfl_xor(bsum[1], 32);
  const int nw = 32 * C * 9;
  for (int w = 0; w < 8; ++w) {
    if (wave == w) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int k = t * 16 + li;
          const int dy = k / KR, rr = k - dy * KR;
          if (dy < 3 && rr < 3 * C) {
            const int dx = rr / C, c = rr - dx * C;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int co = mt * 16 + 4 * kq + r;
              float* d = lds + (co * C + c) * 9 + dy * 3 + dx;
              *d = (w == 0) ? acc[mt][t][r] : *d + acc[mt][t][r];
            }
          }
        }
      if (kq == 0) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          float* d = lds + nw + mt * 16 + li;
          *d = (w == 0) ? bsum[mt] : *d + bsum[mt];
        }
      }
    }
    __syncthreads();
  }
  float* slab = a.partial + (size_t)blockIdx.x * (nw + 32);
  for (int i = tid; i < nw + 32; i += 512) slab[i] = lds[i];
}

// first-layer weight gradient from the uint8 ring with the input band kept as bytes in LDS (see
// conv1_fwd_u8_kernel).  The gradient operand never enters LDS: lane (li, kq) of a k-step needs channels li and
// 16 + li of ONE pixel, every pixel is needed by exactly one wave, and the 16 lanes of a group read 64 contiguous
// bytes -- so each wave loads its own operand values from HBM/L2 one k-step ahead (the other three waves of the SIMD
// cover the latency).  That removes three quarters of the staging volume (53 KB of gradients per 16 KB of bytes at
// 84x84x9) and lets a workgroup take a whole crop as bytes.
// NW waves per workgroup: 8 (two workgroups per CU) or 4 (four smaller ones: the stage -> barrier -> multiply ->
// barrier phases of a workgroup do not overlap each other, so what covers a workgroup's staging is the number of
// OTHER workgroups on its CU that are multiplying at that moment)
template <int C, int NW>
__global__ __launch_bounds__(64 * NW) void wgrad1_u8_kernel(Wgrad1Args a) {
  constexpr int NTHR = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // k' = dy * 3C + dx * C + c, unpadded (9C values): NT tiles of 16.  At C = 9 that is 81 = 5 tiles + ONE column; a
  // sixth tile for it would be a sixth of all MFMAs, so that column (dy = 2, dx = 2, c = C-1) is accumulated by two
  // VALU FMAs per k-step instead (lane (li, kq) holds the gradient of channels li / 16+li at its pixel anyway).
  constexpr int K9 = 9 * C;
  constexpr bool TAIL = (K9 % 16 == 1);
  constexpr int NT = TAIL ? K9 / 16 : (K9 + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (uniform: the piece bookkeeping below stays scalar)
  const int li = lane & 15, kq = lane >> 4;
  const int RSb = conv1_row_bytes(a.Wc, C);
  f32x4 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0, 0, 0, 0};
  f32x2 bsum = {0.f, 0.f};   // (pairs: one packed add / fma for both halves of the output channels)
  f32x2 atail = {0.f, 0.f};
  int koff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = t * 16 + li;
    const int dy = k / (3 * C), rr = k - dy * (3 * C);
    koff[t] = (dy < 3) ? dy * RSb + rr : 0;
  }
  const int koff_tail = 2 * RSb + 3 * C - 1;
  const int nitems = a.B * a.nbands;
  uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int band = item / a.B, b = item - band * a.B;
    const int y0 = band * a.th;
    const int tha = min(a.th, a.Ho - y0);
    if (!ABL(1)) {
      const int64_t fi = a.idx ? rw::const_load(a.idx, b) : (int64_t)b;  // (scalar loads: b is wave-uniform)
      const int oh = a.h1 ? rw::const_load(a.h1, b) : 0, ow = a.w1 ? rw::const_load(a.w1, b) : 0;
      const uint8_t* crop = static_cast<const uint8_t*>(a.src) + ((size_t)fi * a.Hs + oh + 2 * y0) * a.Ws * C + (size_t)ow * C;
      if (a.Wc * C <= 64 * 16)  // a lane per 16-byte run of a row
        conv1_stage_rows<10>(ldsb, crop, a.Ws * C, a.Wc * C, 2 * tha + 1, RSb, 0, wave, NW, lane);
      else
        conv1_stage_u8(ldsb, static_cast<const uint8_t*>(a.src), a.idx, a.h1, a.w1, b, C, a.Hs, a.Ws, a.Wc, 2 * y0,
                       2 * tha + 1, RSb, tid, NTHR);
    }
    __syncthreads();
    const float* const gband = a.g + ((size_t)(b * a.Ho + y0) * a.Wo) * 32 + li;  // the band's pixels are contiguous
    // The walk.  A k-step ("unit") is 4 pixels, lane group kq takes one of them; units come in PIECES of UNR, and the
    // band's pieces are dealt to the waves round-robin (piece w, w + NW, ...).  Two kinds of piece:
    //   row piece:    UNR consecutive units of one output row (pixels 4u + kq): only the floor(Wo / 4) WHOLE units of
    //                 a row, so that no unit multiplies fewer than 4 pixels;
    //   column piece: the Wo % 4 columns a row's whole units leave over, walked DOWN -- a unit is rows 4u + kq of one
    //                 such column (at Wo = 37: 10 units for column 36 instead of a quarter-filled tenth unit in each
    //                 of the 37 rows: 343 units per crop, not 370).
    // In a row piece everything a unit needs sits at a COMPILE-TIME offset from per-piece bases: the byte operands at
    // (piece base + koff[t]) + 8 C jj, the two gradient values at piece base + 128 jj floats -- no per-unit address
    // arithmetic (the pixel-order walk spent ~45 VALU instructions per 12 MFMAs on it: matrix pipe busy 46 %).  Pieces
    // of 3 (not whole rows) so that the waves' shares differ by at most one piece: 115 pieces over 8 waves = 15 each
    // at most, 45 units, where whole rows gave 5 rows x 10 units.  The bytes are multiplied unscaled, `scale` is
    // applied once to the accumulated sums.
    constexpr int UNR = 3;
    const int fullu = a.Wo >> 2, remc = a.Wo & 3;
    const int cpr = (fullu + UNR - 1) / UNR;  // row pieces per row
    const int cpc = (((tha + 3) >> 2) + UNR - 1) / UNR;  // column pieces per left-over column
    const int nrow = tha * cpr, npieces = nrow + remc * cpc;
    const int kdiv = NW / max(cpr, 1), kmod = NW - kdiv * cpr;
    struct Piece {  // (wave-uniform)
      int q, ty, c;  // row piece: row ty, piece c of the row;  column piece (q >= nrow): left-over column ty, piece c
    };
    auto column_of = [&](Piece& p) {
      const int qq = p.q - nrow;
      p.ty = qq / cpc, p.c = qq - p.ty * cpc;
    };
    auto next_piece = [&](Piece& p) {
      p.q += NW;
      if (p.q < nrow) {
        p.c += kmod, p.ty += kdiv;
        if (p.c >= cpr) p.c -= cpr, ++p.ty;
      } else {
        column_of(p);
      }
    };
    // gradient values of a piece (from HBM/L2, one piece ahead of their use; pixels past the band: zero page)
    auto gload = [&](const Piece& p, f32x2 (&av)[UNR]) {
      if (p.q < nrow) {
        const float* gp = gband + (p.ty * a.Wo + 4 * UNR * p.c + kq) * 32;
        if (UNR * (p.c + 1) <= fullu) {
#pragma unroll
          for (int jj = 0; jj < UNR; ++jj) av[jj] = f32x2{gp[128 * jj], gp[128 * jj + 16]};
        } else {
#pragma unroll
          for (int jj = 0; jj < UNR; ++jj) {
            const float* g1 = UNR * p.c + jj < fullu ? gp + 128 * jj : g_zero_px;
            av[jj] = f32x2{g1[0], g1[16]};
          }
        }
      } else {
        const int x = 4 * fullu + p.ty;
#pragma unroll
        for (int jj = 0; jj < UNR; ++jj) {
          const int y = 4 * (UNR * p.c + jj) + kq;
          const float* g1 = (p.ty < remc && y < tha) ? gband + (y * a.Wo + x) * 32 : g_zero_px;
          av[jj] = f32x2{g1[0], g1[16]};
        }
      }
    };
    // operand bytes of a piece, LDS -> registers (also one piece ahead: the multiply below never waits for LDS).
    // Units past the row / the band get an address inside the band: their gradient is the zero page's.
    constexpr int NB = NT + (TAIL ? 1 : 0);
    struct Raw {
      uint32_t b[UNR][NB];
    };
    auto bload_unit = [&](const uint8_t* ub, uint32_t (&b)[NB]) {
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = ub[koff[t]];
      if (TAIL) b[NT] = ub[koff_tail];
    };
    auto bload = [&](const Piece& p, Raw& R) {
      if (p.q < nrow) {
        const uint8_t* rowb = ldsb + __mul24(2 * p.ty, RSb) + 2 * (4 * UNR * p.c + kq) * C;
        if (UNR * (p.c + 1) <= fullu) {  // the usual piece: compile-time offsets
#pragma unroll
          for (int jj = 0; jj < UNR; ++jj) bload_unit(rowb + 8 * C * jj, R.b[jj]);
        } else {
#pragma unroll
          for (int jj = 0; jj < UNR; ++jj) bload_unit(UNR * p.c + jj < fullu ? rowb + 8 * C * jj : rowb, R.b[jj]);
        }
      } else {
        const uint8_t* colb = ldsb + 2 * min(4 * fullu + p.ty, a.Wo - 1) * C;
#pragma unroll
        for (int jj = 0; jj < UNR; ++jj)
          bload_unit(colb + __mul24(2 * min(4 * (UNR * p.c + jj) + kq, tha - 1), RSb), R.b[jj]);
      }
    };
    auto mma = [&](const Raw& R, const f32x2 (&av)[UNR]) {
#pragma unroll
      for (int jj = 0; jj < UNR; ++jj) {
        float bv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bv[t] = (float)R.b[jj][t];
        bsum += av[jj];
        if (TAIL) {
          const float bt = (float)R.b[jj][NB - 1];
          atail += av[jj] * f32x2{bt, bt};
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          acc[0][t] = mfma16(av[jj][0], bv[t], acc[0][t]);
          acc[1][t] = mfma16(av[jj][1], bv[t], acc[1][t]);
        }
#ifndef CURLA_WG1_NOGROUP
        // a unit's conversions ahead of its MFMAs (a conversion right in front of the MFMA that reads it costs wait states)
        __builtin_amdgcn_sched_group_barrier(0x002, NB + 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2 * NT, 0);
#endif
      }
    };
    f32x2 avA[UNR], avB[UNR];
    Raw RA, RB;
    Piece cur;
    cur.q = ABL(2) ? npieces : wave;
    if (cur.q < nrow) cur.ty = cur.q / cpr, cur.c = cur.q - cur.ty * cpr;
    else column_of(cur);
    gload(cur, avA), bload(cur, RA);
    while (cur.q < npieces) {  // (wave-uniform)
      Piece nxt = cur;
      next_piece(nxt);
      gload(nxt, avB), bload(nxt, RB);  // (past the last piece: a column piece outside the band -- zero page, clamped bytes)
      __builtin_amdgcn_sched_barrier(0);
      mma(RA, avA);
      __builtin_amdgcn_sched_barrier(0);
      cur = nxt;
      if (cur.q >= npieces) break;
      next_piece(nxt);
      gload(nxt, avA), bload(nxt, RA);
      __builtin_amdgcn_sched_barrier(0);
      mma(RB, avB);
      __builtin_amdgcn_sched_barrier(0);
      cur = nxt;
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] *= a.scale;

  bsum[0] += __shfl_xor(bsum[0], 16);
  bsum[0] += __shfl_xor(bsum[0], 32);
  bsum[1] += __shfl_xor(bsum[1], 16);
  bsum[1] += __shfl_xor(bsum[1], 32);
  if (TAIL) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      atail[i] *= a.scale;
      atail[i] += __shfl_xor(atail[i], 16);
      atail[i] += __shfl_xor(atail[i], 32);
    }
  }
  // Cross-wave sum (waves in order: fixed order, reproducible) and the slab.  Every wave deposits its accumulator
  // tiles lane-contiguously (one ds_write_b128 per tile, no index arithmetic), as many tiles per pass as the LDS
  // holds for NW waves; after one barrier the threads add the NW copies of their slot and scatter the four sums
  // straight into the slab -- instead of NW serialised read-modify-write rounds over the output layout.
  const int nw = 32 * C * 9;
  float* slab = a.partial + (size_t)blockIdx.x * (nw + 32);
  if (ABL(4)) {  // timing only: no cross-wave sum, no slab
    float t = bsum[0] + bsum[1] + atail[0] + atail[1];
#pragma unroll
    for (int q = 0; q < 2 * NT; ++q) t += acc[q / NT][q % NT][0] + acc[q / NT][q % NT][3];
    if (t == 12345.678f) slab[tid] = t;
    return;
  }
  f32x4* l4 = reinterpret_cast<f32x4*>(lds);
  const int TC = max(1, min(2 * NT, (int)(a.lds_bytes / (NW * 1024))));  // tiles per pass (1 KB per tile and wave)
  __syncthreads();
  for (int t0 = 0; t0 < 2 * NT; t0 += TC) {
    const int nt = min(TC, 2 * NT - t0);
#pragma unroll
    for (int q = 0; q < 2 * NT; ++q)  // (tile q = mt * NT + t; compile-time register index, runtime range test)
      if (q >= t0 && q < t0 + nt) l4[(wave * TC + (q - t0)) * 64 + lane] = acc[q / NT][q % NT];
    __syncthreads();
    for (int sl = tid; sl < nt * 64; sl += NTHR) {
      const int q = t0 + sl / 64, ln = sl & 63;
      f32x4 v = l4[(0 * TC + (q - t0)) * 64 + ln];
      for (int w = 1; w < NW; ++w) v += l4[(w * TC + (q - t0)) * 64 + ln];
      const int mt = q / NT, t = q - mt * NT;
      const int k = t * 16 + (ln & 15);
      const int dy = k / (3 * C), rr = k - dy * (3 * C);
      if (dy < 3) {
        const int dx = rr / C, c = rr - dx * C;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = mt * 16 + 4 * (ln >> 4) + r;
          slab[(co * C + c) * 9 + dy * 3 + dx] = v[r];
        }
      }
    }
    __syncthreads();
  }
  if (kq == 0) {
    lds[(wave * 2 + 0) * 16 + li] = bsum[0], lds[(wave * 2 + 1) * 16 + li] = bsum[1];
    if (TAIL) lds[NW * 32 + (wave * 2 + 0) * 16 + li] = atail[0], lds[NW * 32 + (wave * 2 + 1) * 16 + li] = atail[1];
  }
  __syncthreads();
  if (tid < 32) {
    float v = lds[tid];  // wave 0: [mt][li] = tid
    for (int w = 1; w < NW; ++w) v += lds[w * 32 + tid];
    slab[nw + tid] = v;
    if (TAIL) {  // the column the tiles leave out: (dy, dx, c) = (2, 2, C-1) of output channel tid
      float t = lds[NW * 32 + tid];
      for (int w = 1; w < NW; ++w) t += lds[NW * 32 + w * 32 + tid];
      slab[(tid * C + (C - 1)) * 9 + 8] = t;
    }
  }
}


// The same weight gradient on the BF16 matrix cores (round 6; option wgrad1_u8 = auto / b16).  A uint8 pixel is EXACT in
// one bf16 (8 significand bits), the gradient is the exact sum of three (conv_rwb.h: split8) -- so a float32 product
// g x is three exact bf16 x bf16 products accumulated in fp32, nothing dropped.  One v_mfma_f32_16x16x32_bf16 takes a
// k-step of 32 PIXELS (lane group kq: pixels 8 kq .. 8 kq + 7) where the f32-input instruction takes 4: per 32 pixels
// 2 x NT x 3 matrix instructions of 16 cycles instead of 8 x 2 x NT of 32 -- 5.3 x fewer matrix cycles, which moves the
// loop from the matrix pipe (busy 0.53, 1.1 VALU per instruction) to the vector ALU: per unit and wave ~90 instructions
// split the 16 gradient values, ~70 turn the 8 x NT operand bytes into bf16 (v_cvt_f32_ubyte + one v_perm per pair: the
// float of an integer below 256 has an empty low half), ~60 walk the pixels.
// Columns: k' = (dy, rr = dx C + c) with every tap row dy padded to NTD = ceil(3 C / 16) tiles of 16 (96 columns for
// C = 9, where the unpadded 81 need six tiles as well): tile t = dy NTD + h reads byte (pixel base) + dy RSb + 16 h + li,
// i.e. ONE per-lane base per (pixel, dy) and compile-time offsets -- the padding columns multiply bytes of the
// neighbouring pixel (finite) and are dropped by the epilogue.
// Pixels: the band's pixels in row-major order, 32 per unit, units dealt round-robin to the waves (the gradient of a
// unit is 32 x 128 contiguous bytes); pixels past the band read zeros through the buffer range check and a clamped
// (valid) byte address.  What the loop waits for is the gradient (90 MB per 512 crops against 27 MB of bytes: timing-only
// builds without the byte reads, the split AND the products still take half the loop's time), so: four waves per SIMD
// (two 512-thread workgroups per CU, 128 registers) rather than three with deeper software pipelining (38 against 32 us),
// whole 128-byte lines per load instruction, and a tap row's bytes requested one tap row ahead.
template <int C, int NW>
__global__ __launch_bounds__(64 * NW, NW / 2) void wgrad1_u8b_kernel(Wgrad1Args a) {
  constexpr int NTHR = 64 * NW;
  constexpr int NTD = (3 * C + 15) / 16, NT = 3 * NTD;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using rwb::u32x4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int RSb = conv1_row_bytes(a.Wc, C);
  f32x4 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0, 0, 0, 0};
  f32x2 bsum = {0.f, 0.f};
  uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
  const int nitems = a.B * a.nbands;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int band = item / a.B, b = item - band * a.B;
    const int y0 = band * a.th;
    const int tha = min(a.th, a.Ho - y0);
    const int npix = tha * a.Wo;
    const int nunits = (npix + 31) >> 5;
    // the band's gradient, [pixel][32]: lane (li, kq) takes output channels 2 li and 2 li + 1 (rows li of the two channel
    // tiles: tile mt holds the channels of parity mt) of its 8 pixels -- ONE 8-byte load per pixel, a lane group reads a
    // pixel's whole 128-byte line (channel li and 16 + li as two 4-byte loads: twice the load instructions, each touching
    // half a line -- the loop waits for these loads, not for arithmetic); past the band: zeros
    const __amdgpu_buffer_rsrc_t rg = rw::uniform_rsrc(a.g + ((size_t)(b * a.Ho + y0) * a.Wo) * 32, npix * 128);
    float graw[2][8];
    auto gload = [&](int u) {
      const unsigned v0 = (unsigned)((32 * u + 8 * kq) * 128 + li * 8);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rg, v0 + 128u * jj, 0, 0));
        graw[0][jj] = v[0], graw[1][jj] = v[1];
      }
    };
    if (wave < nunits) gload(wave);  // (independent of the crop: in flight while the bytes are staged)
    if (!ABL(1)) {
      const int64_t fi = a.idx ? rw::const_load(a.idx, b) : (int64_t)b;  // (scalar loads: b is wave-uniform)
      const int oh = a.h1 ? rw::const_load(a.h1, b) : 0, ow = a.w1 ? rw::const_load(a.w1, b) : 0;
      const uint8_t* crop = static_cast<const uint8_t*>(a.src) + ((size_t)fi * a.Hs + oh + 2 * y0) * a.Ws * C + (size_t)ow * C;
      if (a.Wc * C <= 64 * 16)  // a lane per 16-byte run of a row
        conv1_stage_rows<10>(ldsb, crop, a.Ws * C, a.Wc * C, 2 * tha + 1, RSb, 0, wave, NW, lane);
      else
        conv1_stage_u8(ldsb, static_cast<const uint8_t*>(a.src), a.idx, a.h1, a.w1, b, C, a.Hs, a.Ws, a.Wc, 2 * y0,
                       2 * tha + 1, RSb, tid, NTHR);
    }
    __syncthreads();
    // first pixel of this lane in unit u = wave: (row, column) -> byte offset of its patch; a unit step is 32 NW pixels
    int p0 = 32 * wave + 8 * kq;
    int ty = p0 / a.Wo, x = p0 - ty * a.Wo;
    const int qstep = (32 * NW) / a.Wo, rstep = 32 * NW - qstep * a.Wo;
    const int px = 2 * C, wrap_add = 2 * RSb - 2 * (a.Wo - 1) * C;  // next pixel of a row / first pixel of the next row
    const int pb_last = 2 * (tha - 1) * RSb + 2 * (a.Wo - 1) * C + li;  // (pixels past the band: clamped, zero gradient)
    for (int u = ABL(2) ? nunits : wave; u < nunits; u += NW) {  // (wave-uniform)
      // ---- byte address of each of the 8 pixels' patch and the first tap row's bytes, in flight during the split
      int pb[8];
      {
        int xx = x, cur = __mul24(2 * ty, RSb) + 2 * x * C + li;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          pb[jj] = min(cur, pb_last);
          ++xx;
          const bool wrap = xx >= a.Wo;
          cur += wrap ? wrap_add : px;
          xx = wrap ? 0 : xx;
        }
      }
      uint32_t raw[8 * NTD];
      auto bread = [&](const int dy) {
        const uint8_t* rowb = ldsb + dy * RSb;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
#pragma unroll
          for (int h = 0; h < NTD; ++h) raw[jj * NTD + h] = rowb[pb[jj] + 16 * h];
      };
      if (!ABL(8)) bread(0);
      __builtin_amdgcn_sched_barrier(0);
      // ---- this unit's gradient values -> three bf16 operands per channel half; the next unit's are requested
      rwb::B3 G[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        float v[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) v[jj] = graw[mt][jj];
        bsum[mt] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        if (ABL(16)) {  // timing only: no split arithmetic
#pragma unroll
          for (int q = 0; q < 4; ++q)
            G[mt].h[q] = __builtin_bit_cast(unsigned, v[q]), G[mt].m[q] = __builtin_bit_cast(unsigned, v[q + 4]), G[mt].l[q] = G[mt].h[q];
        } else
          G[mt] = rwb::split8(v);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- tap row by tap row: 8 NTD bytes -> NTD B operands of 8 bf16 (the float of an integer below 256 has an empty
      // low half: its high half IS the bf16), the next tap row's bytes requested, then the six products of each tile
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        u32x4 X[NTD];
#pragma unroll
        for (int h = 0; h < NTD; ++h)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float f0 = (float)raw[(2 * q) * NTD + h], f1 = (float)raw[(2 * q + 1) * NTD + h];
            X[h][q] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, f1), __builtin_bit_cast(unsigned, f0), 0x07060302u);
          }
        __builtin_amdgcn_sched_barrier(0);
        if (dy < 2 && !ABL(8)) bread(dy + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (ABL(32)) {  // timing only: no matrix instructions
#pragma unroll
          for (int h = 0; h < NTD; ++h) acc[0][dy * NTD + h][0] += __builtin_bit_cast(float, X[h][0] ^ X[h][1] ^ X[h][2] ^ X[h][3] ^ G[0].l[0] ^ G[1].m[1] ^ G[0].h[2] ^ G[1].h[3] ^ G[0].m[0] ^ G[1].l[1]);
        } else
#pragma unroll
        for (int h = 0; h < NTD; ++h) {
          const int t = dy * NTD + h;
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[mt][t] = rwb::mfma_bf16(G[mt].l, X[h], acc[mt][t]);  // smallest part first
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[mt][t] = rwb::mfma_bf16(G[mt].m, X[h], acc[mt][t]);
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[mt][t] = rwb::mfma_bf16(G[mt].h, X[h], acc[mt][t]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the next unit's gradient values: requested here, behind the unit's arithmetic (their 16 registers are free
      // again; the SIMD's other three waves cover the latency -- requested before the products they cost 33 spills)
      if (u + NW < nunits) gload(u + NW);
      x += rstep, ty += qstep;  // at most one more wrap
      const bool wrap = x >= a.Wo;
      x = wrap ? x - a.Wo : x;
      ty = wrap ? ty + 1 : ty;
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] *= a.scale;
  bsum[0] += __shfl_xor(bsum[0], 16);
  bsum[0] += __shfl_xor(bsum[0], 32);
  bsum[1] += __shfl_xor(bsum[1], 16);
  bsum[1] += __shfl_xor(bsum[1], 32);
  // cross-wave sum in wave order and the slab, as wgrad1_u8_kernel (tile t: tap row t / NTD, columns 16 (t % NTD) + li)
  const int nw = 32 * C * 9;
  float* slab = a.partial + (size_t)blockIdx.x * (nw + 32);
  if (ABL(4)) {  // timing only: no cross-wave sum, no slab
    float t = bsum[0] + bsum[1];
#pragma unroll
    for (int q = 0; q < 2 * NT; ++q) t += acc[q / NT][q % NT][0] + acc[q / NT][q % NT][3];
    if (t == 12345.678f) slab[tid] = t;
    return;
  }
  f32x4* l4 = reinterpret_cast<f32x4*>(lds);
  const int TC = max(1, min(2 * NT, (int)(a.lds_bytes / (NW * 1024))));  // tiles per pass (1 KB per tile and wave)
  __syncthreads();
  for (int t0 = 0; t0 < 2 * NT; t0 += TC) {
    const int nt = min(TC, 2 * NT - t0);
#pragma unroll
    for (int q = 0; q < 2 * NT; ++q)
      if (q >= t0 && q < t0 + nt) l4[(wave * TC + (q - t0)) * 64 + lane] = acc[q / NT][q % NT];
    __syncthreads();
    for (int sl = tid; sl < nt * 64; sl += NTHR) {
      const int q = t0 + sl / 64, ln = sl & 63;
      f32x4 v = l4[(0 * TC + (q - t0)) * 64 + ln];
      for (int w = 1; w < NW; ++w) v += l4[(w * TC + (q - t0)) * 64 + ln];
      const int mt = q / NT, t = q - mt * NT;
      const int dy = t / NTD, rr = 16 * (t - dy * NTD) + (ln & 15);
      if (rr < 3 * C) {
        const int dx = rr / C, c = rr - dx * C;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = 2 * (4 * (ln >> 4) + r) + mt;  // (tile mt: the output channels of parity mt)
          slab[(co * C + c) * 9 + dy * 3 + dx] = v[r];
        }
      }
    }
    __syncthreads();
  }
  if (kq == 0) lds[(wave * 2 + 0) * 16 + li] = bsum[0], lds[(wave * 2 + 1) * 16 + li] = bsum[1];
  __syncthreads();
  if (tid < 32) {  // tid = mt * 16 + li: output channel 2 li + mt
    float v = lds[tid];
    for (int w = 1; w < NW; ++w) v += lds[w * 32 + tid];
    slab[nw + 2 * (tid & 15) + (tid >> 4)] = v;
  }
}
