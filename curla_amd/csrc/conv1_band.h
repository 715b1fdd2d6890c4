// First conv layer (3x3, stride 2, C -> 32, + bias + ReLU) in its forms that stage the crop in LDS, gfx950: the banded
// loop from a float tensor (conv1_fwd_kernel) or from the uint8 ring with the band kept as bytes (conv1_fwd_u8_kernel),
// and the hybrid (conv1_u8_walk_kernel: that byte staging, the row walk of conv1_u8_rw.h out of LDS).  Included by
// conv.hip inside its anonymous namespace, after conv1_u8_rw.h (kLdsPix, ABL, rw::Geom and the rw:: helpers come from there).
#pragma once

// ---------------------------------------------------------------------------
// first layer: Cin = C (9 or 12 ...), stride 2, input either the uint8 replay
// frames (gather by index + random-crop offsets + /255 fused into the load) or
// a float NCHW tensor in [0,255] (the reference's tensor contract).
// K index of the GEMM is k = dy*KR + (dx*C + c), KR = 3C rounded up to 4; the
// (dx,c) run is contiguous in an HWC row, so one LDS row holds it directly.
// ---------------------------------------------------------------------------
struct Conv1Args {
  const void* src;     // SRC_U8: frames [N][Hs][Ws][C] u8;  SRC_F32: [B][C][Hc][Wc] f32
  const int64_t* idx;  // [B] frame index (u8 source) or nullptr -> b
  const int32_t* h1;   // [B] crop row offset or nullptr -> 0
  const int32_t* w1;   // [B] crop col offset or nullptr -> 0
  const float* w;      // OIHW [32][C][3][3]
  const float* bias;   // [32]
  float* out;          // [B][Ho][Wo][32]
  int B, C, Hs, Ws, Hc, Wc, Ho, Wo, th, nbands;
  float scale;
  int dbg;
  // uint8 forward only: a second minibatch from the same ring with its own weights (B2 samples; 0 = none), whose
  // workgroups follow the first one's in the same launch
  const int64_t* idx2;
  const int32_t* h1_2;
  const int32_t* w1_2;
  const float* w2;
  const float* bias2;
  float* out2;
  int B2;
};

enum { SRC_U8 = 0, SRC_F32 = 1, SRC_NHWC = 2 };  // u8 ring / float NCHW tensor / float NHWC tensor

__device__ __forceinline__ int conv1_row_stride(int Wc, int C) { return ((Wc * C + 3) & ~3) + 4; }
__device__ __forceinline__ bool aligned16_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Stage input rows [r0, r0+rows) of sample b's (cropped) image into LDS as
// f32 HWC rows of stride RS, scaled by `scale`.
template <int SRC>
__device__ __forceinline__ void conv1_stage(float* lds, const void* src, const int64_t* idx, const int32_t* h1,
                                            const int32_t* w1, int b, int C, int Hs, int Ws, int Hc, int Wc, int r0,
                                            int rows, int RS, float scale, int tid, int nthreads) {
  const int rowf = Wc * C;
  if (SRC == SRC_U8) {
    const int64_t fi = idx ? idx[b] : b;
    const int oh = h1 ? h1[b] : 0, ow = w1 ? w1[b] : 0;
    const uint8_t* frame = static_cast<const uint8_t*>(src) + (size_t)fi * Hs * Ws * C;
    const int G = (rowf + 3) >> 2;
    for (int i = tid; i < rows * G; i += nthreads) {
      const int r = i / G, g = i - r * G;
      const uint8_t* p = frame + ((size_t)(oh + r0 + r) * Ws + ow) * C + 4 * g;
      // (pointer arithmetic, not an integer round trip: the loads stay global_load, not flat_load)
      const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
      const uint32_t d0 = q[0];
      const uint32_t d1 = sh ? q[1] : 0u;   // only touch the next dword when the run straddles it
      const uint32_t v = __builtin_amdgcn_alignbyte(d1, d0, sh);
      f32x4 o;
      o[0] = (float)(v & 0xff) * scale;
      o[1] = (float)((v >> 8) & 0xff) * scale;
      o[2] = (float)((v >> 16) & 0xff) * scale;
      o[3] = (float)(v >> 24) * scale;
      *reinterpret_cast<f32x4*>(lds + r * RS + 4 * g) = o;
    }
  } else if (SRC == SRC_NHWC) {
    // float NHWC minibatch (augmented observations): rows are contiguous runs of Wc*C floats
    const float* img = static_cast<const float*>(src) + ((size_t)b * Hc + r0) * rowf;
    if ((rowf & 3) == 0 && aligned16_dev(img)) {
      const int G = rowf >> 2;
      for (int i = tid; i < rows * G; i += nthreads) {
        const int r = i / G, g = i - r * G;
        f32x4 v = *reinterpret_cast<const f32x4*>(img + (size_t)r * rowf + 4 * g);
        *reinterpret_cast<f32x4*>(lds + r * RS + 4 * g) = v * scale;
      }
    } else {
      for (int i = tid; i < rows * rowf; i += nthreads) {
        const int r = i / rowf, e = i - r * rowf;
        lds[r * RS + e] = img[(size_t)r * rowf + e] * scale;
      }
    }
  } else {
    const float* img = static_cast<const float*>(src) + (size_t)b * C * Hc * Wc;
    const int n = rows * rowf;
    for (int i = tid; i < n; i += nthreads) {
      const int x = i % Wc;
      const int t = i / Wc;
      const int r = t % rows, c = t / rows;
      lds[r * RS + x * C + c] = img[((size_t)c * Hc + r0 + r) * Wc + x] * scale;
    }
  }
  // The k-steps of a tap row cover KR = 3C rounded up to 4 values: at an odd crop width the last pixel's run ends at
  // the row's end and its padding value is the float BEHIND the row.  Its weight is zero, but 0 x (whatever bit
  // pattern an earlier kernel left in LDS: NaN, Inf) is NaN, which the ReLU then turns into 0 -- a wrong, finite
  // output.  The slack behind every row is zeroed here (the uint8 path wrote whole groups of four: behind those).
#ifndef CURLA_TEST_NO_SLACK_ZERO  // (defined only by a one-off build that checks the regression test can fail)
  {
    const int first = SRC == SRC_U8 ? (rowf + 3) & ~3 : rowf;
    const int pad = RS - first;  // 4..7 floats
    for (int i = tid; i < rows * pad; i += nthreads) {
      const int r = i / pad, e = i - r * pad;
      lds[r * RS + first + e] = 0.f;
    }
  }
#endif
}

template <int SRC, int C>
__global__ __launch_bounds__(512) void conv1_fwd_kernel(Conv1Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KR = (3 * C + 3) & ~3;
  constexpr int NS = 3 * KR / 4;  // k-steps
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int RS = conv1_row_stride(a.Wc, C);

  constexpr int KQ = KR / 4;  // k-steps per tap row
  for (int i = tid; i < 32 * C * 9; i += 512) lds[i] = a.w[i];
  __syncthreads();
  // k = 4 s + kq of the GEMM is (dy, rr) = (s / KQ, 4 (s % KQ) + kq): KR is a multiple of 4, so the tap row is the
  // same for all lanes of a k-step and a lane's operand sits at a COMPILE-TIME offset (dy, 4 (s % KQ)) from its own
  // base (pixel, kq) -- one address per tile instead of one add per k-step (a VALU instruction is a cycle the f32
  // matrix pipe idles: conv_rw.h)
  float wr[NS][2];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int dy = s / KQ, rr = 4 * (s % KQ) + kq;
    const bool ok = rr < 3 * C;
    const int dx = ok ? rr / C : 0, c = ok ? rr - dx * C : 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) wr[s][mt] = ok ? lds[((mt * 16 + li) * C + c) * 9 + dy * 3 + dx] : 0.f;
  }
  f32x4 bias4[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) bias4[mt] = *reinterpret_cast<const f32x4*>(a.bias + mt * 16 + 4 * kq);
  __syncthreads();

  // persistent: the weight registers above are built once per workgroup, not once per band (a band is ~2 us of
  // tile work at 168x168x12 -- the per-band weight phase was a quarter of the kernel)
  const int nitems = a.B * a.nbands;
  const int qstep = 128 / a.Wo, rstep = 128 - qstep * a.Wo;  // 8 waves x 16 pixels further
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int band = item / a.B, b = item - band * a.B;  // band-major: every workgroup sees every band size
    const int y0 = band * a.th;
    const int tha = min(a.th, a.Ho - y0);
    conv1_stage<SRC>(lds, a.src, a.idx, a.h1, a.w1, b, C, a.Hs, a.Ws, a.Hc, a.Wc, 2 * y0, 2 * tha + 1, RS, a.scale, tid,
                     512);
    __syncthreads();

    const int npix = tha * a.Wo;
    const int ntiles = (npix + 15) >> 4;
    float* const out_item = a.out + ((size_t)(b * a.Ho + y0) * a.Wo) * 32 + 4 * kq;
    int ty = (wave * 16 + li) / a.Wo, x = (wave * 16 + li) - ty * a.Wo;  // walked incrementally: no division per tile
    for (int t = wave; t < ntiles; t += 8) {
      const bool pv = t * 16 + li < npix;
      if (!pv) ty = 0, x = 0;
      const float* base = lds + __mul24(2 * ty, RS) + __mul24(2 * x, C) + kq;
      // the 3 tap rows: RS is a run-time stride, so each row has its own base register; inside a row the k-steps are
      // immediates.  All NS reads of the tile are issued up front (they are independent of the accumulators).
      float bv[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) bv[s] = base[(s / KQ) * RS + 4 * (s % KQ)];
      f32x4 acc[2] = {bias4[0], bias4[1]};  // bias through the accumulators' initial values
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        float v = bv[s];
        // the last k-step of a tap row reaches past the window's 3 C floats into the NEXT pixel's first channels (the
        // zeroed slack at the row's end): their weight is zero, but 0 x NaN (or Inf) is NaN -- in an output whose
        // window does not hold that pixel.  (Selected where it is used: in front of the loop it made the first MFMA wait
        // for the last read.)
        if (KR > 3 * C && s % KQ == KQ - 1) v = 4 * (KQ - 1) + kq >= 3 * C ? 0.f : v;
        acc[0] = mfma16(wr[s][0], v, acc[0]);
        acc[1] = mfma16(wr[s][1], v, acc[1]);
      }
      if (pv) {
        float* o = out_item + (__mul24(ty, a.Wo) + x) * 32;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          f32x4 v = acc[mt];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = relu_keep_nan(v[r]);
          act_store(reinterpret_cast<f32x4*>(o + mt * 16), v);
        }
      }
      x += rstep, ty += qstep;  // at most one more wrap
      const bool wrap = x >= a.Wo;
      x = wrap ? x - a.Wo : x;
      ty = wrap ? ty + 1 : ty;
    }
    __syncthreads();  // every wave is done with the band before the next one is staged over it
  }
}

// ---------------------------------------------------------------------------
// first layer, uint8 ring source, bytes kept as bytes in LDS (4x less LDS than the float band: a whole
// 76x76x9 crop is 52 KB, so a workgroup takes one sample with no halo re-reads and two workgroups share a
// CU).  Staging is a pure byte copy: 16-byte runs of the (arbitrarily aligned) crop row are rebuilt from
// aligned dword loads with v_alignbyte; u8 -> f32 and the /255 happen when the MFMA B operand is read.
// k = 4s + kq of the GEMM is (dy, rr) = (s / (KR/4), 4 (s % (KR/4)) + kq): since KR is a multiple of 4 the
// tap row dy is wave-uniform per k-step and the byte offset inside the row differs per lane only by kq.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int conv1_row_bytes(int Wc, int C) { return ((Wc * C + 15) & ~15) + 16; }

// One pass of the byte staging, split into its two halves so that a kernel can put other work between the
// loads and the LDS stores: U 16-byte runs per thread, all their dword loads in flight together.
template <int U>
struct Conv1StageRegs {
  uint32_t dw[U][5], sh[U];
  int dst[U];
};

template <int U>
__device__ __forceinline__ void conv1_stage_u8_issue(Conv1StageRegs<U>& rg, const uint8_t* frame, int oh, int ow, int C,
                                                     int Ws, int Wc, int r0, int rows, int RSb, int i0, int tid,
                                                     int nthreads) {
  const int runs = (Wc * C + 15) >> 4;  // 16-byte runs per row
  const int total = rows * runs;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const int i = i0 + tid + k * nthreads;
    const bool ok = i < total;
    const int ic = ok ? i : 0;
    const int r = ic / runs, g = ic - r * runs;
    const uint8_t* p = frame + ((size_t)(oh + r0 + r) * Ws + ow) * C + 16 * g;
    // (pointer arithmetic, not an integer round trip: the loads stay global_load, not flat_load)
    rg.sh[k] = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - rg.sh[k]);
    rg.dst[k] = ok ? r * RSb + 16 * g : -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) rg.dw[k][e] = ok ? q[e] : 0u;
    rg.dw[k][4] = (ok && rg.sh[k]) ? q[4] : 0u;  // only touch the fifth dword when the run straddles it
  }
}

template <int U>
__device__ __forceinline__ void conv1_stage_u8_commit(const Conv1StageRegs<U>& rg, uint8_t* lds) {
#pragma unroll
  for (int k = 0; k < U; ++k) {
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(rg.dw[k][1], rg.dw[k][0], rg.sh[k]);
    o.y = __builtin_amdgcn_alignbyte(rg.dw[k][2], rg.dw[k][1], rg.sh[k]);
    o.z = __builtin_amdgcn_alignbyte(rg.dw[k][3], rg.dw[k][2], rg.sh[k]);
    o.w = __builtin_amdgcn_alignbyte(rg.dw[k][4], rg.dw[k][3], rg.sh[k]);
    if (rg.dst[k] >= 0) *reinterpret_cast<uint4*>(lds + rg.dst[k]) = o;
  }
}

__device__ __forceinline__ void conv1_stage_u8(uint8_t* lds, const uint8_t* frames, const int64_t* idx,
                                               const int32_t* h1, const int32_t* w1, int b, int C, int Hs, int Ws,
                                               int Wc, int r0, int rows, int RSb, int tid, int nthreads,
                                               int first_run = 0) {
  const int64_t fi = idx ? idx[b] : b;
  const int oh = h1 ? h1[b] : 0, ow = w1 ? w1[b] : 0;
  const uint8_t* frame = frames + (size_t)fi * Hs * Ws * C;
  const int total = rows * ((Wc * C + 15) >> 4);
  constexpr int U = 4;
  for (int i0 = first_run; i0 < total; i0 += nthreads * U) {
    Conv1StageRegs<U> rg;
    conv1_stage_u8_issue<U>(rg, frame, oh, ow, C, Ws, Wc, r0, rows, RSb, i0, tid, nthreads);
    conv1_stage_u8_commit<U>(rg, lds);
  }
}

// The same byte staging dealt out BY ROW: wave w of NW takes crop rows w, w + NW, ..., lane g the row's g-th 16-byte
// run (lanes past the row idle).  A row's address, its misalignment and its LDS offset are then wave-uniform -- scalar
// registers and scalar arithmetic -- and a run costs a lane one address add instead of an integer division by the run
// count and 64-bit pointer arithmetic (the element-per-thread form above: ~40 VALU instructions per run, ~3800 wave
// instructions per 76x76x9 crop against the 2700 of the multiply loop that follows).  UR rows per wave and call.
template <int UR>
struct Conv1RowRegs {
  uint32_t dw[UR][5];
  uint32_t sh[UR];  // (wave-uniform)
  int dst[UR];      // (wave-uniform row offset; < 0: no row)
};

template <int UR>
__device__ __forceinline__ void conv1_stage_rows_issue(Conv1RowRegs<UR>& rg, const uint8_t* crop, int pitch, int nbytes,
                                                       int rows, int RSb, int r_first, int wave, int nwaves, int lane) {
  const bool lane_on = 16 * lane < nbytes;
#pragma unroll
  for (int k = 0; k < UR; ++k) {
    const int r = r_first + wave + k * nwaves;  // (uniform)
    rg.dst[k] = r < rows ? r * RSb : -1;
    const uint8_t* p = crop + (size_t)min(r, rows - 1) * pitch;
    rg.sh[k] = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - rg.sh[k]) + 4 * lane;
    // (registers of rows / lanes that load nothing stay undefined: the commit never stores them)
    if (r < rows && lane_on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rg.dw[k][e] = q[e];
      if (rg.sh[k]) rg.dw[k][4] = q[4];  // only touch the fifth dword when the run straddles it
    }
  }
}

template <int UR>
__device__ __forceinline__ void conv1_stage_rows_commit(const Conv1RowRegs<UR>& rg, uint8_t* lds, int nbytes, int lane) {
  const bool lane_on = 16 * lane < nbytes;
#pragma unroll
  for (int k = 0; k < UR; ++k) {
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(rg.dw[k][1], rg.dw[k][0], rg.sh[k]);
    o.y = __builtin_amdgcn_alignbyte(rg.dw[k][2], rg.dw[k][1], rg.sh[k]);
    o.z = __builtin_amdgcn_alignbyte(rg.dw[k][3], rg.dw[k][2], rg.sh[k]);
    o.w = __builtin_amdgcn_alignbyte(rg.dw[k][4], rg.dw[k][3], rg.sh[k]);
    if (rg.dst[k] >= 0 && lane_on) *reinterpret_cast<uint4*>(lds + rg.dst[k] + 16 * lane) = o;
  }
}

// all rows [r_first, rows) of a crop, UR per wave and pass
template <int UR>
__device__ __forceinline__ void conv1_stage_rows(uint8_t* lds, const uint8_t* crop, int pitch, int nbytes, int rows,
                                                 int RSb, int r_first, int wave, int nwaves, int lane) {
  for (int r0 = r_first; r0 < rows; r0 += UR * nwaves) {
    Conv1RowRegs<UR> rg;
    conv1_stage_rows_issue<UR>(rg, crop, pitch, nbytes, rows, RSb, r0, wave, nwaves, lane);
    conv1_stage_rows_commit<UR>(rg, lds, nbytes, lane);
  }
}

// float4 copy of `n4` contiguous float4 from HBM into the pixel-padded LDS band layout (8 float4 per pixel ->
// stride kLdsPix floats), U loads in flight per thread per pass
__device__ __forceinline__ void stage_band_f32(float* lds_band, const float* src, int n4, int tid, int nthreads) {
  constexpr int U = 6;
  for (int f0 = 0; f0 < n4; f0 += nthreads * U) {
    f32x4 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int f = f0 + tid + k * nthreads;
      v[k] = f < n4 ? *reinterpret_cast<const f32x4*>(src + (size_t)f * 4) : f32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int f = f0 + tid + k * nthreads;
      if (f < n4) *reinterpret_cast<f32x4*>(lds_band + (f >> 3) * kLdsPix + (f & 7) * 4) = v[k];
    }
  }
}

template <int C>
__global__ __launch_bounds__(512) void conv1_fwd_u8_kernel(Conv1Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KR = (3 * C + 3) & ~3;
  constexpr int KQ = KR / 4;      // k-steps per tap row
  constexpr int NS = 3 * KQ;      // k-steps
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int RSb = conv1_row_bytes(a.Wc, C);

  // (two problems in one launch: the workgroups of the second minibatch follow the first's and take its weights)
  const int nitems1 = a.B * a.nbands;
  const bool second = (int)blockIdx.x >= nitems1;
  const int item = second ? blockIdx.x - nitems1 : blockIdx.x;
  const int Bc = second ? a.B2 : a.B;
  if (second) a.idx = a.idx2, a.h1 = a.h1_2, a.w1 = a.w1_2, a.w = a.w2, a.bias = a.bias2, a.out = a.out2;
  const int band = item / Bc, b = item - band * Bc;
  const int y0 = band * a.th;
  const int tha = min(a.th, a.Ho - y0);
  // the first staging pass (7 x 512 runs: a whole 76x76x9 crop) is issued before the weight phase, whose two
  // barriers and LDS gather then run under the loads' latency; its LDS stores come after (same LDS region)
  constexpr int U0 = 7;
  Conv1StageRegs<U0> rg0;
  const uint8_t* frame0;
  int oh0, ow0;
  {
    const int64_t fi = a.idx ? a.idx[b] : b;
    oh0 = a.h1 ? a.h1[b] : 0, ow0 = a.w1 ? a.w1[b] : 0;
    frame0 = static_cast<const uint8_t*>(a.src) + (size_t)fi * a.Hs * a.Ws * C;
    if (!ABL(1)) conv1_stage_u8_issue<U0>(rg0, frame0, oh0, ow0, C, a.Ws, a.Wc, 2 * y0, 2 * tha + 1, RSb, 0, tid, 512);
  }

  // weights -> MFMA A-operand registers through a k-major LDS image [dy][rr (KR, zero padded)][cout 32], rr = dx*C + c,
  // with the 1/255 of `obs / 255.` (encoder.py:78) folded in: the index arithmetic is paid once per weight while
  // staging (5 per thread), and every lane then reads its 2 x NS values at compile-time offsets from ONE base
  // (the per-register gather out of the OIHW image cost ~10 VALU for each of the 42 registers of every lane).
  for (int i = tid; i < 3 * KR * 32; i += 512) {
    const int co = i & 31, k = i >> 5;
    const int dy = k / KR, rr = k - dy * KR;
    const int dx = rr / C, c = rr - dx * C;
    lds[i] = rr < 3 * C ? a.w[(co * C + c) * 9 + dy * 3 + dx] * a.scale : 0.f;
  }
  __syncthreads();
  float wr[NS][2];
  {
    const float* wl = lds + kq * 32 + li;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) wr[s][mt] = wl[((s / KQ) * KR + 4 * (s % KQ)) * 32 + mt * 16];
  }
  f32x4 bias4[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) bias4[mt] = *reinterpret_cast<const f32x4*>(a.bias + mt * 16 + 4 * kq);
  __syncthreads();

  uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
  if (!ABL(1)) {
    conv1_stage_u8_commit<U0>(rg0, ldsb);
    conv1_stage_u8(ldsb, static_cast<const uint8_t*>(a.src), a.idx, a.h1, a.w1, b, C, a.Hs, a.Ws, a.Wc, 2 * y0,
                   2 * tha + 1, RSb, tid, 512, /*first_run=*/U0 * 512);  // taller bands: the rest
  }
  __syncthreads();

  const int npix = tha * a.Wo;
  const int ntiles = ABL(64) ? 0 : (npix + 15) >> 4;
  int ty = (wave * 16 + li) / a.Wo, x = (wave * 16 + li) - ty * a.Wo;
  const int qstep = 128 / a.Wo, rstep = 128 - qstep * a.Wo;
  for (int t = wave; t < ntiles; t += 8) {
    const bool pv = t * 16 + li < npix;
    if (!pv) ty = 0, x = 0;
    const uint8_t* base = ldsb + 2 * ty * RSb + 2 * x * C + kq;
    // all NS byte reads of the tile are issued first; each conversion is then placed one k-step ahead of the MFMA
    // pair that consumes it (left alone, the compiler emits read -> wait -> convert -> s_nop -> 2 MFMAs chains that
    // expose the LDS latency and a VALU->MFMA hazard stall on every k-step: tools/micro/conv1_loop.hip)
    uint32_t raw[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) raw[s] = base[(s / KQ) * RSb + 4 * (s % KQ)];
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[2] = {bias4[0], bias4[1]};  // bias through the accumulators' initial values
    // (the conversions are volatile asm so that instruction selection cannot sink them next to their users; the
    // first one carries the 2 wait states a VALU write needs before an MFMA reads it, every other one has the two
    // MFMAs of the previous k-step between itself and its reader: tools/check_asm_hazards.py scans the ISA)
    float cur;
    asm volatile("v_cvt_f32_ubyte0 %0, %1\n\ts_nop 1" : "=v"(cur) : "v"(raw[0]));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float nxt = cur;
      if (s + 1 < NS) asm volatile("v_cvt_f32_ubyte0 %0, %1" : "=v"(nxt) : "v"(raw[s + 1]));
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = mfma16(wr[s][0], cur, acc[0]);
      acc[1] = mfma16(wr[s][1], cur, acc[1]);
      __builtin_amdgcn_sched_barrier(0);
      cur = nxt;
    }
    if (pv && !ABL(4)) {
      const size_t g = ((size_t)(b * a.Ho + y0 + ty) * a.Wo + x) * 32 + 4 * kq;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x4 v = acc[mt];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = relu_keep_nan(v[r]);
        act_store(reinterpret_cast<f32x4*>(a.out + g + mt * 16), v);
      }
    }
    x += rstep, ty += qstep;  // 8 waves x 16 pixels further: qstep rows + rstep columns, at most one more wrap
    const bool wrap = x >= a.Wo;
    x = wrap ? x - a.Wo : x;
    ty = wrap ? ty + 1 : ty;
  }
}

// ---------------------------------------------------------------------------
// The same layer, HYBRID form: the banded kernel's input side (one workgroup per sample, the crop staged as bytes in
// LDS by one burst of aligned loads -- which is what makes that kernel indifferent to where the ring slots come from)
// with the row walk's compute loop (conv1_u8_rw.h: a wave owns 16 output columns and walks down; a lane group's
// E = ceil(3C/4) operand bytes of an input row are CONTIGUOUS, here read from LDS as aligned dwords + v_alignbyte, two
// new rows per 6 E MFMAs) instead of one byte read + one (row, column) walk per k-step.  The sample's steps (strips x
// rows, rw::Geom) are split evenly over the 8 waves.  Only for crops that fit one band (nbands == 1).
// ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(512, 2) void conv1_u8_walk_kernel(Conv1Args a, rw::Geom G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int E = (3 * C + 3) / 4, KR = 4 * E;
  constexpr int NLD = (E + 3 + 3) / 4;  // aligned dwords that hold a run starting at byte 0..3 of the first
  constexpr int NWD = (E + 3) / 4;      // dwords of the run once it starts at byte 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int RSb = conv1_row_bytes(a.Wc, C);
  const bool second = (int)blockIdx.x >= a.B;
  const int b = second ? blockIdx.x - a.B : blockIdx.x;
  if (second) a.idx = a.idx2, a.h1 = a.h1_2, a.w1 = a.w1_2, a.w = a.w2, a.bias = a.bias2, a.out = a.out2;
  // the crop's bytes: requested before the weight phase, stored to LDS after it (same region)
  constexpr int U0 = 10;  // rows per wave in flight across the weight phase (8 waves x 10 >= the 77 rows of a 76x76 crop)
  Conv1RowRegs<U0> rg0;
  const int crop_rows = 2 * a.Ho + 1, crop_bytes = a.Wc * C;
  const uint8_t* crop0;
  {
    const int64_t fi = a.idx ? rw::const_load(a.idx, b) : (int64_t)b;  // (scalar loads: b is wave-uniform)
    const int oh0 = a.h1 ? rw::const_load(a.h1, b) : 0, ow0 = a.w1 ? rw::const_load(a.w1, b) : 0;
    crop0 = static_cast<const uint8_t*>(a.src) + ((size_t)fi * a.Hs + oh0) * a.Ws * C + (size_t)ow0 * C;
  }
  conv1_stage_rows_issue<U0>(rg0, crop0, a.Ws * C, crop_bytes, crop_rows, RSb, 0, wave, 8, lane);  // (host: <= 64 runs per row)
  for (int i = tid; i < 3 * KR * 32; i += 512) {
    const int co = i & 31, k = i >> 5;
    const int dy = k / KR, rr = k - dy * KR;
    const int dx = rr / C, c = rr - dx * C;
    lds[i] = rr < 3 * C ? a.w[(co * C + c) * 9 + dy * 3 + dx] * a.scale : 0.f;
  }
  __syncthreads();
  float wr[3][E][2];  // lane (li = cout, kq): W[cout][dy][rr = E kq + e] * scale
  {
    const float* wl = lds + (E * kq) * 32 + li;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) wr[dy][e][mt] = wl[(dy * KR + e) * 32 + mt * 16];
  }
  f32x4 bias4[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) bias4[mt] = *reinterpret_cast<const f32x4*>(a.bias + mt * 16 + 4 * kq);
  __syncthreads();
  uint8_t* ldsb = reinterpret_cast<uint8_t*>(lds);
  conv1_stage_rows_commit<U0>(rg0, ldsb, crop_bytes, lane);
  conv1_stage_rows<4>(ldsb, crop0, a.Ws * C, crop_bytes, crop_rows, RSb, /*r_first=*/U0 * 8, wave, 8, lane);
  __syncthreads();

  const int lo = G.steps * wave / 8, hi = G.steps * (wave + 1) / 8;
  const int out_row = a.Wo * 128;
  const __amdgpu_buffer_rsrc_t rout = rw::uniform_rsrc(a.out + (size_t)b * a.Ho * a.Wo * 32, a.Ho * out_row);
  for (int g = lo; g < hi;) {
    int k, sb, n_strip;
    if (g < G.nfull * G.Ho) {
      k = g / G.Ho, sb = g - k * G.Ho, n_strip = G.Ho;
    } else {
      const int q = (g - G.nfull * G.Ho) / G.nr;
      k = G.nfull + q, sb = g - G.nfull * G.Ho - q * G.nr, n_strip = G.nr;
    }
    const int n = hi - g < n_strip - sb ? hi - g : n_strip - sb;
    g += n;
    int x, y0;
    bool lane_on;
    if (k < G.nfull) {
      x = 16 * k + li, y0 = 0, lane_on = true;
    } else {
      const int u = (k - G.nfull) * 16 + li;
      const int col = u / G.nseg, sg = u - col * G.nseg;
      lane_on = col < G.brem;
      x = 16 * G.nfull + col, y0 = sg * G.nr;
    }
    // (lanes without a column, and rows past the crop, read whatever sits in LDS: finite bytes; nothing of it is stored)
    const int Y = lane_on ? min(y0 + sb, a.Ho - 1) : 0;
    const int xx = lane_on ? x : 0;
    const unsigned run = (unsigned)(2 * Y * RSb + 2 * xx * C + E * kq);
    const unsigned sh = run & 3u;
    const uint8_t* rowp = ldsb + (run & ~3u);
    unsigned vo = lane_on ? (unsigned)(((y0 + sb) * a.Wo + x) * 128 + kq * 16) : 0x80000000u;
    const int rmax = 2 * a.Ho - 2 * Y;  // last crop row (relative to 2 Y) that exists in LDS
    struct Raw {
      uint32_t d[NLD];
    };
    struct Row {
      float v[E];
    };
    auto load_row = [&](Raw& R, int r) {  // crop row 2 Y + r (clamped into the staged image)
      const uint32_t* p = reinterpret_cast<const uint32_t*>(rowp + __mul24(min(r, rmax), RSb));  // (24-bit: no 64-bit mad)
#pragma unroll
      for (int j = 0; j < NLD; ++j) R.d[j] = p[j];
    };
    auto convert = [&](Row& F, const Raw& R) {
      rw::RawBytes<NWD> Wd;
#pragma unroll
      for (int j = 0; j < NWD; ++j) Wd.d[j] = __builtin_amdgcn_alignbyte(j + 1 < NLD ? R.d[j + 1 < NLD ? j + 1 : j] : 0u, R.d[j], sh);
#pragma unroll
      for (int e = 0; e < E; ++e) F.v[e] = rw::byte_f32<NWD>(Wd, e);
    };
    auto mma_row = [&](f32x4 (&acc)[2], const Row& F, const int dy) {
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[mt] = mfma16(wr[dy][e][mt], F.v[e], acc[mt]);
    };
    struct Pair {
      Raw a, b;
    };
    auto step = [&](const Row& r0, Row& r1, Row& r2, const Pair& cur, Pair& nxt, const int t) {
      load_row(nxt.a, 2 * t + 3);
      load_row(nxt.b, 2 * t + 4);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc[2] = {bias4[0], bias4[1]};
      mma_row(acc, r0, 0);
      __builtin_amdgcn_sched_barrier(0);
      convert(r1, cur.a);
      convert(r2, cur.b);
      __builtin_amdgcn_sched_barrier(0);
      mma_row(acc, r1, 1);
      mma_row(acc, r2, 2);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x4 v = acc[mt];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = relu_keep_nan(v[r]);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rout,
                                               vo + mt * 64u, 0, CURLA_ACT_STORE_POLICY);
      }
      vo += out_row;
    };
    Row S0, S1, S2, S3, S4;
    Pair P0, P1;
    {
      Raw R0;
      load_row(R0, 0), load_row(P0.a, 1), load_row(P0.b, 2);
      convert(S0, R0);
    }
    for (int t = 0;;) {  // rows of step t sit in sets (2t, 2t+1, 2t+2) mod 5, its bytes in pair t mod 2
      step(S0, S1, S2, P0, P1, t);
      if (++t >= n) break;
      step(S2, S3, S4, P1, P0, t);
      if (++t >= n) break;
      step(S4, S0, S1, P0, P1, t);
      if (++t >= n) break;
      step(S1, S2, S3, P1, P0, t);
      if (++t >= n) break;
      step(S3, S4, S0, P0, P1, t);
      if (++t >= n) break;
      step(S0, S1, S2, P1, P0, t);
      if (++t >= n) break;
      step(S2, S3, S4, P0, P1, t);
      if (++t >= n) break;
      step(S4, S0, S1, P1, P0, t);
      if (++t >= n) break;
      step(S1, S2, S3, P0, P1, t);
      if (++t >= n) break;
      step(S3, S4, S0, P1, P0, t);
      if (++t >= n) break;
    }
  }
}
