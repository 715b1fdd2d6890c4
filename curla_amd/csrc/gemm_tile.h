// The tiled GEMM: one TBM x TBN output tile per workgroup out of LDS-staged operand tiles, on the f32-input MFMA or, as
// three bf16 parts per fp32 operand, on the bf16 matrix cores (gemm_tile), alone (gemm_kernel) and as the two products
// of a linear layer's backward pass in one launch (gemm_pair_kernel).  Included by gemm.hip inside its anonymous
// namespace, behind gemm_plan.h (GemmArgs, BM / BN / BK).
#pragma once

constexpr int RSTR = BK + 8;   // LDS stride, row-major tile [64][BK]: 40 floats -> 16-B aligned rows, ds_read_b128 of 16 rows x 4 k-quarters conflict-free
#ifndef CURLA_GEMM_KSTR
#define CURLA_GEMM_KSTR (BM + 4)
#endif
// LDS stride, k-major tile [BK][64].  A fragment read is k = 16j + 4kq + e of row li: bank = (k * KSTR + li) mod 32, and
// with KSTR = 68 (= 4 mod 32) that is (16 kq + 4 e + li) mod 32 -- the two lane groups of a half-wave (kq, kq + 1) take
// disjoint halves of the banks.  (80, the stride of rounds 1-2, put both on the same 16 banks: SQ_LDS_BANK_CONFLICT 0.3-0.4
// of the LDS cycles of the kernels with a k-major operand.)
constexpr int KSTR = CURLA_GEMM_KSTR;
// bf16x3 form (round 5, gemm_tile<..., B3 = true>): an operand tile is THREE bf16 images [part][row][32 k], rows of 64
// bytes = four 16-byte chunks (a lane's fragment is one chunk, a staging thread's four k half a chunk), chunk c of row r at
// slot c ^ b3_swz(r).  With that XOR the four 16-lane groups of a ds_read_b128 (MI355X_MICROARCH.md, LDS: {0-3, 12-15,
// 20-27}, ...) each read 16 different slots of the 256-byte bank row, and the 8-byte stores of a row-major operand (16
// lanes = 2 rows x 8 pieces) cover all 32 banks once; a k-major operand's stores (16 rows, one piece) are 2-way.  (The
// first two versions padded rows to 80 and 96 bytes: fragment reads 2-way at 80, stores 2- and 4-way at 96 -- PMC
// SQ_LDS_BANK_CONFLICT 0.30 / 0.50 of the LDS cycles of the 128 x 64 kernels.)
constexpr int kB3RowBytes = 64;
__device__ __forceinline__ int b3_swz(int row) { return (-((row >> 2) & 3)) & 3; }
constexpr int b3_part_bytes(int rows) { return rows * kB3RowBytes; }
constexpr int b3_tile_floats(int rows) { return 3 * b3_part_bytes(rows) / 4; }
constexpr int kGemmTileFloatsF32 = (BK * KSTR > BM * RSTR) ? BK * KSTR : BM * RSTR;
// floats of one operand tile buffer with `rows` rows (the f32 forms exist for up to 64 rows only)
constexpr int gemm_tile_floats(int rows) {
  return rows > 64 ? b3_tile_floats(rows) : (b3_tile_floats(64) > kGemmTileFloatsF32 ? b3_tile_floats(64) : kGemmTileFloatsF32);
}

// load one BK x ROWS operand tile into registers (ROWS/32 float4 per thread)
template <bool KMAJOR, int ROWS>
__device__ __forceinline__ void tile_load(const float* __restrict__ P, int ld, int rows_total, int r0, int k0, int kend,
                                          int vec, int tid, f32x4 (&reg)[ROWS / 32]) {
#pragma unroll
  for (int u = 0; u < ROWS / 32; ++u) {
    f32x4 v = {0, 0, 0, 0};
    if (!KMAJOR) {
      const int row = (tid >> 3) + 32 * u, k4 = (tid & 7) * 4;
      const int gr = r0 + row, gk = k0 + k4;
      if (gr < rows_total) {
        const float* p = P + (size_t)gr * ld + gk;
        if (vec && gk + 3 < kend) {
          v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (gk + i < kend) v[i] = p[i];
        }
      }
    } else {
      constexpr int TPR = ROWS / 4;  // threads per k-row
      const int k = tid / TPR + (256 / TPR) * u, r4 = (tid % TPR) * 4;
      const int gk = k0 + k, gr = r0 + r4;
      if (gk < kend) {
        const float* p = P + (size_t)gk * ld + gr;
        if (vec && gr + 3 < rows_total) {
          v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (gr + i < rows_total) v[i] = p[i];
        }
      }
    }
    reg[u] = v;
  }
}

// interior, aligned tiles: no bounds or alignment tests in the k loop
template <bool KMAJOR, int ROWS>
__device__ __forceinline__ void tile_load_fast(const float* __restrict__ P, int ld, int rows_total, int r0, int k0,
                                               int tid, f32x4 (&reg)[ROWS / 32]) {
#pragma unroll
  for (int u = 0; u < ROWS / 32; ++u) {
    if (!KMAJOR) {
      // rows past the matrix edge re-read the last row (their products are discarded by the epilogue)
      const int row = min(r0 + (tid >> 3) + 32 * u, rows_total - 1), k4 = (tid & 7) * 4;
      reg[u] = *reinterpret_cast<const f32x4*>(P + (size_t)row * ld + k0 + k4);
    } else {
      constexpr int TPR = ROWS / 4;
      const int k = tid / TPR + (256 / TPR) * u, r4 = (tid % TPR) * 4;
      reg[u] = *reinterpret_cast<const f32x4*>(P + (size_t)(k0 + k) * ld + r0 + r4);
    }
  }
}

template <bool KMAJOR, int ROWS>
__device__ __forceinline__ void tile_store(float* __restrict__ S, int tid, const f32x4 (&reg)[ROWS / 32]) {
#pragma unroll
  for (int u = 0; u < ROWS / 32; ++u) {
    if (!KMAJOR) {
      const int row = (tid >> 3) + 32 * u, k4 = (tid & 7) * 4;
      *reinterpret_cast<f32x4*>(S + row * RSTR + k4) = reg[u];
    } else {
      constexpr int TPR = ROWS / 4;
      const int k = tid / TPR + (256 / TPR) * u, r4 = (tid % TPR) * 4;
      *reinterpret_cast<f32x4*>(S + k * KSTR + r4) = reg[u];
    }
  }
}

// MFMA operand values of one lane for the 8 k-steps of a BK=32 tile.  k-step (j, e) multiplies
// k = 16j + 4kq + e on lane group kq (any k order is fine as long as A and B agree): a row-major
// tile delivers them with two ds_read_b128, a k-major tile with eight ds_read_b32.
template <bool KMAJOR>
__device__ __forceinline__ void frags(const float* __restrict__ S, int row, int kq, float (&v)[8]) {
  if (!KMAJOR) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(S + row * RSTR + 4 * kq);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(S + row * RSTR + 16 + 4 * kq);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = lo[e], v[4 + e] = hi[e];
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = S[(16 * j + 4 * kq + e) * KSTR + row];
  }
}

// ---- bf16x3 operands (the heads' 512 x 1024 x 1024 products ran at 0.6-0.7 of the f32-input MFMA: a barrier per 32-deep
// k tile with 32 matrix instructions of 32 cycles between two of them).  Every fp32 operand element is split ONCE, when
// its tile is staged into LDS, into three bf16 parts (x = xh + xm + xl exactly, conv_rwb.h); a k tile is then one k-step
// of v_mfma_f32_16x16x32_bf16 per term, six terms per fp32 product: 24 matrix instructions of 16 cycles per wave and
// tile instead of 32 of 32, and the split costs 5.5 VALU instructions per element against the 2 x 16 .. 4 x 16
// products the element takes part in.  Both operand kinds end in the same image: a row-major operand is loaded as
// float4 along k, a k-major one as four dword loads along k per thread (a wave reads 64 consecutive rows of one k: 256
// contiguous bytes), so a thread always holds four consecutive k of one row.
typedef short gbf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned gu32x4 __attribute__((ext_vector_type(4)));
typedef unsigned gu32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 gbf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned g_cvt_pk_bf16(float x0, float x1) {
  const f32x2 v = {x0, x1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, gbf16x2));
}

template <bool KMAJOR, int ROWS, int NT = 256>
__device__ __forceinline__ void tile_load_b3(const float* __restrict__ P, int ld, int rows_total, int r0, int k0, int tid,
                                             f32x4 (&reg)[ROWS * 8 / NT]) {
#pragma unroll
  for (int u = 0; u < ROWS * 8 / NT; ++u) {
    if (!KMAJOR) {
      const int row = min(r0 + (tid >> 3) + (NT / 8) * u, rows_total - 1), k4 = (tid & 7) * 4;
      reg[u] = *reinterpret_cast<const f32x4*>(P + (size_t)row * ld + k0 + k4);
    } else {
      const int row = tid % ROWS, k4 = 4 * (tid / ROWS + (NT / ROWS) * u);
      const float* p = P + (size_t)(k0 + k4) * ld + r0 + row;
#pragma unroll
      for (int e = 0; e < 4; ++e) reg[u][e] = p[(size_t)e * ld];
    }
  }
}

template <bool KMAJOR, int ROWS, int NT = 256>
__device__ __forceinline__ void tile_store_b3(float* __restrict__ S, int tid, const f32x4 (&reg)[ROWS * 8 / NT]) {
  char* base = reinterpret_cast<char*>(S);
#pragma unroll
  for (int u = 0; u < ROWS * 8 / NT; ++u) {
    const int row = KMAJOR ? tid % ROWS : (tid >> 3) + (NT / 8) * u;
    const int k4 = KMAJOR ? 4 * (tid / ROWS + (NT / ROWS) * u) : (tid & 7) * 4;
    gu32x2 h, m, l;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float x0 = reg[u][2 * q], x1 = reg[u][2 * q + 1];
      const unsigned hh = g_cvt_pk_bf16(x0, x1);
      const float r0 = x0 - __builtin_bit_cast(float, hh << 16), r1 = x1 - __builtin_bit_cast(float, hh & 0xFFFF0000u);
      const unsigned mm = g_cvt_pk_bf16(r0, r1);
      const float s0 = r0 - __builtin_bit_cast(float, mm << 16), s1 = r1 - __builtin_bit_cast(float, mm & 0xFFFF0000u);
      h[q] = hh, m[q] = mm, l[q] = g_cvt_pk_bf16(s0, s1);
    }
    char* p = base + row * kB3RowBytes + (((k4 >> 3) ^ b3_swz(row)) << 4) + ((k4 & 4) << 1);
    *reinterpret_cast<gu32x2*>(p) = h;
    *reinterpret_cast<gu32x2*>(p + b3_part_bytes(ROWS)) = m;
    *reinterpret_cast<gu32x2*>(p + 2 * b3_part_bytes(ROWS)) = l;
  }
}

struct Frag3 {
  gu32x4 h, m, l;
};

template <int ROWS>
__device__ __forceinline__ Frag3 frags_b3(const float* __restrict__ S, int row, int kq) {
  const char* p = reinterpret_cast<const char*>(S) + row * kB3RowBytes + ((kq ^ b3_swz(row)) << 4);
  Frag3 f;
  f.h = *reinterpret_cast<const gu32x4*>(p);
  f.m = *reinterpret_cast<const gu32x4*>(p + b3_part_bytes(ROWS));
  f.l = *reinterpret_cast<const gu32x4*>(p + 2 * b3_part_bytes(ROWS));
  return f;
}

// eight fp32 values (a lane's 8 consecutive k of one row) -> the three bf16 operands (x = h + m + l exactly)
__device__ __forceinline__ Frag3 g_split8(const f32x4 lo, const f32x4 hi) {
  Frag3 o;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = p < 2 ? lo[2 * p] : hi[2 * p - 4], x1 = p < 2 ? lo[2 * p + 1] : hi[2 * p - 3];
    const unsigned hh = g_cvt_pk_bf16(x0, x1);
    const float r0 = x0 - __builtin_bit_cast(float, hh << 16), r1 = x1 - __builtin_bit_cast(float, hh & 0xFFFF0000u);
    const unsigned mm = g_cvt_pk_bf16(r0, r1);
    const float s0 = r0 - __builtin_bit_cast(float, mm << 16), s1 = r1 - __builtin_bit_cast(float, mm & 0xFFFF0000u);
    o.h[p] = hh, o.m[p] = mm, o.l[p] = g_cvt_pk_bf16(s0, s1);
  }
  return o;
}

__device__ __forceinline__ f32x4 g_mfma_bf16(const gu32x4 a, const gu32x4 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gbf16x8, a), __builtin_bit_cast(gbf16x8, b), c, 0, 0, 0);
}

// NT = 256 threads = 2 x 2 waves, a wave computes (TBM/2) x (TBN/2) of the TBM x TBN tile; NT = 512 (the 128 x 64 bf16x3
// tile): 4 x 2 waves of 32 x 32 -- two waves per SIMD (with one wave per SIMD, 64 x 32 each, the k tile's phases ran
// back to back: 37 against 32 us for the twin critics' hidden layer).
// TBN = 32 doubles the workgroup count for the mid-sized GEMMs of the heads
// (512 x 1024 x 1024 is only 128 tiles of 64 x 64 on a 256-CU chip).
// The k loop is double-buffered in LDS (two operand tile pairs, 40 KB): while the waves multiply tile t out of one
// buffer, tile t+1 goes from registers into the other and tile t+2 is in flight from HBM/L2 -- ONE barrier per k tile,
// and the LDS write -> barrier -> fragment read latency of the next tile sits under the current tile's MFMAs.
template <int ROWS>
using GemmLds = float[2][gemm_tile_floats(ROWS)];

// one TBM x TBN output tile (tile column bx, tile row by, batch x split item z) by the 256 threads of a workgroup
template <bool AK, bool BKM, int TBM, int TBN, bool FAST, bool B3 = false, int NT = 256>
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, const int bx, const int by, const int z, float (*As)[gemm_tile_floats(TBM)],
                                          float (*Bs)[gemm_tile_floats(TBN)]) {
  static_assert(!B3 || FAST, "the bf16x3 form takes interior, aligned tiles only");
  static_assert(TBM <= 64 || B3, "tiles of more than 64 rows exist in the bf16x3 form only");
  static_assert(NT == 256 || B3, "the f32 forms are written for 256 threads");
  constexpr int WR = NT / 128;        // rows of waves (two columns of waves always)
  constexpr int WM = TBM / WR;        // rows per wave
  constexpr int MI = WM / 16;         // 16-row fragments per wave
  constexpr int RA = TBM * 8 / NT, RB = TBN * 8 / NT;  // staging registers (float4) per thread and operand
  constexpr int NJ = TBN / 32;
  constexpr int WN = TBN / 2;  // columns per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int batch = z / g.ksplit, ks = z - batch * g.ksplit;
  const int m0 = by * TBM, n0 = bx * TBN;
  const int bo = batch / g.nb_inner, bi = batch - bo * g.nb_inner;
  const float* A = g.nptr ? g.Ap[batch] : g.A + bi * g.sA + bo * g.sA2;
  const float* B = g.nptr ? g.Bp[batch] : g.B + bi * g.sB + bo * g.sB2;
  float* C = (g.nptr ? g.Cp[batch] : g.C + bi * g.sC + bo * g.sC2) + ks * g.sSplit;
  const int kbeg = ks * g.kchunk;
  const int kend = min(g.K, kbeg + g.kchunk);

  const bool epi = g.ksplit == 1;
  const float* bias = (epi && g.bias) ? g.bias + bi * g.sBias + bo * g.sBias2 : nullptr;
  const float* mask = (epi && g.mask) ? g.mask + bi * g.sMask + bo * g.sMask2 : nullptr;
  // The MFMA is issued with the N-side operand as its row operand, so a lane holds 4 CONSECUTIVE n
  // (rows 4kq..4kq+3 of the 16x16 tile) of ONE m (column li): C, bias and mask move as float4.
  const bool vec_c = (g.ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0) &&
                     (!mask || ((g.ldmask % 4 == 0) && ((reinterpret_cast<uintptr_t>(mask) & 15) == 0)));
  // the ReLU mask of a data-gradient product (as large as C itself for the fc layer) is requested before the k loop
  // and arrives under it, instead of being waited for between the last MFMA and the stores
  f32x4 mk[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      mk[i][j] = f32x4{1.f, 1.f, 1.f, 1.f};
      const int m = m0 + wm * WM + i * 16 + li;
      const int n = n0 + wn * WN + j * 16 + 4 * kq;
      if (mask && vec_c && m < g.M && n + 3 < g.N) mk[i][j] = *reinterpret_cast<const f32x4*>(mask + (size_t)m * g.ldmask + n);
    }

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  auto load = [&](int k0, f32x4 (&ra)[RA], f32x4 (&rb)[RB]) {
    if constexpr (B3) {
      tile_load_b3<AK, TBM, NT>(A, g.lda, g.M, m0, k0, tid, ra);
      tile_load_b3<BKM, TBN, NT>(B, g.ldb, g.N, n0, k0, tid, rb);
    } else if constexpr (FAST) {
      tile_load_fast<AK, TBM>(A, g.lda, g.M, m0, k0, tid, ra);
      tile_load_fast<BKM, TBN>(B, g.ldb, g.N, n0, k0, tid, rb);
    } else {
      tile_load<AK, TBM>(A, g.lda, g.M, m0, k0, kend, g.vecA, tid, ra);
      tile_load<BKM, TBN>(B, g.ldb, g.N, n0, k0, kend, g.vecB, tid, rb);
    }
  };
  auto stage = [&](int buf, const f32x4 (&ra)[RA], const f32x4 (&rb)[RB]) {
    if constexpr (B3) {
      tile_store_b3<AK, TBM, NT>(As[buf], tid, ra);
      tile_store_b3<BKM, TBN, NT>(Bs[buf], tid, rb);
    } else {
      tile_store<AK, TBM>(As[buf], tid, ra);
      tile_store<BKM, TBN>(Bs[buf], tid, rb);
    }
  };
  auto multiply = [&](int buf) {
    if constexpr (B3) {
      Frag3 xa[MI], xb[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) xa[i] = frags_b3<TBM>(As[buf], wm * WM + i * 16 + li, kq);
#pragma unroll
      for (int j = 0; j < NJ; ++j) xb[j] = frags_b3<TBN>(Bs[buf], wn * WN + j * 16 + li, kq);
      // six terms per product, smallest first; the (i, j) accumulators interleaved term by term
#pragma unroll
      for (int term = 0; term < 6; ++term)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const gu32x4& pb = term == 0 ? xb[j].l : (term == 2 || term == 3) ? xb[j].m : xb[j].h;
            const gu32x4& pa = (term == 0 || term == 3 || term == 5) ? xa[i].h : (term == 1) ? xa[i].l : xa[i].m;
            acc[i][j] = g_mfma_bf16(pb, pa, acc[i][j]);
          }
    } else {
    float fa[MI][8], fb[NJ][8];
#pragma unroll
    for (int i = 0; i < MI; ++i) frags<AK>(As[buf], wm * WM + i * 16 + li, kq, fa[i]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) frags<BKM>(Bs[buf], wn * WN + j * 16 + li, kq, fb[j]);
#pragma unroll
    for (int s = 0; s < BK / 4; ++s)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16(fb[j][s], fa[i][s], acc[i][j]);
    }
  };
  const int ntiles = (kend - kbeg + BK - 1) / BK;
  if (ntiles > 0) {
    f32x4 ra0[RA], rb0[RB], ra1[RA], rb1[RB];
    load(kbeg, ra0, rb0);
    load(ntiles > 1 ? kbeg + BK : kbeg, ra1, rb1);  // (a single-tile product re-reads its tile: keeps this branch-free)
    stage(0, ra0, rb0);
    __syncthreads();
    int k0 = kbeg, t = 0;
    // steady state: tile t in buffer 0, tile t+1 in the second register set; both refills unconditional so that the
    // compiler's vmcnt bookkeeping keeps the younger tile's loads in flight across each LDS store
    for (; t + 3 < ntiles; t += 2, k0 += 2 * BK) {
      load(k0 + 2 * BK, ra0, rb0);
      multiply(0);
      stage(1, ra1, rb1);
      __syncthreads();
      load(k0 + 3 * BK, ra1, rb1);
      multiply(1);
      stage(0, ra0, rb0);
      __syncthreads();
    }
    const int rem = ntiles - t;  // 1..3 tiles left: tile t in buffer 0, tile t+1 (if any) in the second register set
    if (rem >= 3) load(k0 + 2 * BK, ra0, rb0);
    multiply(0);
    if (rem >= 2) {
      stage(1, ra1, rb1);
      __syncthreads();
      multiply(1);
    }
    if (rem >= 3) {
      stage(0, ra0, rb0);  // (buffer 0 was last read before the barrier above)
      __syncthreads();
      multiply(0);
    }
  }

#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int m = m0 + wm * WM + i * 16 + li;
      const int n = n0 + wn * WN + j * 16 + 4 * kq;
      if (m >= g.M || n >= g.N) continue;
      f32x4 v = acc[i][j] * g.alpha;
      if (vec_c && n + 3 < g.N) {
        if (bias) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bias[n + r];
        }
        if (epi && g.relu) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (mask) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = mk[i][j][r] > 0.f ? v[r] : 0.f;
        }
        if (g.stream_c)
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(C + (size_t)m * g.ldc + n));
        else
          *reinterpret_cast<f32x4*>(C + (size_t)m * g.ldc + n) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n + r >= g.N) continue;
          float x = v[r] + (bias ? bias[n + r] : 0.f);
          if (epi && g.relu) x = fmaxf(x, 0.f);
          if (mask) x = mask[(size_t)m * g.ldmask + n + r] > 0.f ? x : 0.f;
          C[(size_t)m * g.ldc + n + r] = x;
        }
      }
    }
}

#ifndef CURLA_GEMM_XCD
#define CURLA_GEMM_XCD 1
#endif
// Workgroup b runs on XCD b mod 8 (each XCD has its own L2).  xcd_order gives XCD x the x-th eighth of the tile list, so
// that with the tiles listed row tile fastest, then column tile, then problem, an XCD's workgroups share a few column
// tiles of B and the rows of A of ONE problem instead of touching every problem's A.
__device__ __forceinline__ int xcd_order(int b, int total) {
  return (CURLA_GEMM_XCD && (total & 7) == 0) ? (b & 7) * (total >> 3) + (b >> 3) : b;
}

template <bool AK, bool BKM, int TBM, int TBN, bool FAST, bool B3 = false, int NT = 256>
__global__ __launch_bounds__(NT) void gemm_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) GemmLds<TBM> As;
  __shared__ __attribute__((aligned(16))) GemmLds<TBN> Bs;
  // one-dimensional grid: gx * gy * (nbatch * ksplit) workgroups in XCD order
  const int gx = (g.N + TBN - 1) / TBN, gy = (g.M + TBM - 1) / TBM;
  const int v = xcd_order(blockIdx.x, gx * gy * g.nbatch * g.ksplit);
  const int r = v / gy;
  gemm_tile<AK, BKM, TBM, TBN, FAST, B3, NT>(g, r % gx, v - r * gy, r / gx, As, Bs);
}

// Backward of a linear layer as ONE launch: the weight gradient dW = dy^T x (both operands k-major, k = the batch rows)
// and the data gradient dx = (dy W) masked (W k-major) are independent products over the same dy -- the first `n1`
// workgroups take the tiles of the first, the rest the tiles of the second (grids gx x gy x batch each).  Saves a
// launch's ramp and tail per layer and lets the second product's first workgroups fill the first one's last round.
template <int TM1, int TN1, int TM2, int TN2, bool B3 = false, bool SECOND_FIRST = false, int NT = 256>
__global__ __launch_bounds__(NT) void gemm_pair_kernel(GemmArgs g1, GemmArgs g2, int n1, int gx1, int gy1, int gx2,
                                                        int gy2, int n2) {
  constexpr int RA = TM1 > TM2 ? TM1 : TM2, RB = TN1 > TN2 ? TN1 : TN2;
  __shared__ __attribute__((aligned(16))) GemmLds<RA> As;
  __shared__ __attribute__((aligned(16))) GemmLds<RB> Bs;
  int bid = blockIdx.x;
  // XCD order inside each product (xcd_order), the second product's share of an XCD first when SECOND_FIRST (its tiles
  // are the longer ones: k = N against k = the batch rows -- the short ones then fill the last round)
  if (CURLA_GEMM_XCD && ((n1 | n2) & 7) == 0) {
    const int x = bid & 7, i = bid >> 3, s1 = n1 >> 3, s2 = n2 >> 3;
    const int fst = SECOND_FIRST ? s2 : s1;
    const bool in_first = i < fst;
    const bool second = SECOND_FIRST ? in_first : !in_first;
    const int j = in_first ? i : i - fst;
    bid = second ? n1 + x * s2 + j : x * s1 + j;
  } else if (SECOND_FIRST) {
    bid = bid < n2 ? bid + n1 : bid - n2;
  }
  if (bid < n1) {
    const int r = bid / gy1;
    gemm_tile<true, true, TM1, TN1, true, B3, NT>(g1, r % gx1, bid - r * gy1, r / gx1,
                                                  reinterpret_cast<float(*)[gemm_tile_floats(TM1)]>(&As[0][0]),
                                                  reinterpret_cast<float(*)[gemm_tile_floats(TN1)]>(&Bs[0][0]));
  } else {
    bid -= n1;
    const int r = bid / gy2;
    gemm_tile<false, true, TM2, TN2, true, B3, NT>(g2, r % gx2, bid - r * gy2, r / gx2,
                                                   reinterpret_cast<float(*)[gemm_tile_floats(TM2)]>(&As[0][0]),
                                                   reinterpret_cast<float(*)[gemm_tile_floats(TN2)]>(&Bs[0][0]));
  }
}
