// Pixel augmentations that produce float observations (reference: augmentations.py:78-205).
//
// The reference implements ColorJiggle / NoisyCover with kornia (un-vendored, version un-pinned), so there is
// no reference arithmetic to pin against: the algorithm below is this build's own statement of kornia's
// documented behaviour (oracle/curla_oracle.py restates it on the CPU; parity is to that restatement only).
// Both kernels read the uint8 NHWC replay ring directly (gather by frame index fused in) and write the
// float32 NHWC minibatch [B][H][W][C] in [0,255] that the first conv kernel consumes (src kind 2).
#include "common.h"
#include "u8_mover.h"  // RandomShift, RandomTranslate and the crop; U8_UNROLL and u32x4 for RandomCutout below
#include "affine.h"    // RandomAffine: the one mover that resamples

namespace {

constexpr float kTwoPi = 6.283185307179586f;

// The colour-space round trips are the whole cost of the jitter kernel (VALU-bound: ~300 instructions per RGB pixel
// with IEEE divisions and integer modulos), so divisions are reciprocal multiplies (v_rcp_f32, 1 ulp) and the sector
// index uses the range the hue is known to be in; the differences to exact division are ~1e-7 relative.  Round 4: only
// the hue shift still makes the round trip; the saturation change is evaluated in RGB (jiggle_rgb).
__device__ __forceinline__ float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }

__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float& h, float& s, float& v) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  v = mx;
  float d = mx - mn;
  s = fminf(d * rcp_fast(mx + 1e-8f), 1.f);  // (the reciprocal's last-bit error must not push s past 1: v(1-s) >= 0)
  if (d == 0.f) d = 1.f;
  const float rc = mx - r, gc = mx - g, bc = mx - b;
  float hh;
  if (r == mx)          // first maximum wins, as argmax does
    hh = bc - gc;
  else if (g == mx)
    hh = (rc - bc) + 2.f * d;
  else
    hh = (gc - rc) + 4.f * d;
  hh = hh * rcp_fast(d) * (1.f / 6.f);
  hh = hh - floorf(hh);  // python-style % 1
  h = kTwoPi * hh;
}

// h in [0, 2 pi] (what rgb_to_hsv and the hue shift below produce)
__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float& r, float& g, float& b) {
  const float h6 = h * (6.f / kTwoPi);
  // sector floor(h6) % 6; h6 == 6 (hue rounded up to 2 pi) is sector 5 with f = 1, the same colour as sector 0, f = 0
  const int hi = min(max((int)h6, 0), 5);
  const float f = h6 - (float)hi;
  const float p = v * (1.f - s), q = v * (1.f - f * s), t = v * (1.f - (1.f - f) * s);
  r = (hi == 0 || hi == 5) ? v : (hi == 1) ? q : (hi == 4) ? t : p;
  g = (hi == 1 || hi == 2) ? v : (hi == 0) ? t : (hi == 3) ? q : p;
  b = (hi == 3 || hi == 4) ? v : (hi == 2) ? t : (hi == 5) ? q : p;
}

// One RGB pixel in [0,1] through the jitter chain.  p = (apply, contrast, saturation, hue_radians) of the pixel's
// frame; o0..o3 = the call's permutation of {0 brightness (factor 0: identity), 1 contrast, 2 saturation, 3 hue}.
__device__ __forceinline__ void jiggle_rgb(float& r, float& g, float& bl, const float* p, int o0, int o1, int o2,
                                           int o3) {
  if (p[0] == 0.f) return;
  const float con = p[1], sat = p[2], hue = p[3];
#pragma unroll
  for (int step = 0; step < 4; ++step) {
    const int op = step == 0 ? o0 : step == 1 ? o1 : step == 2 ? o2 : o3;
    if (op == 1) {
      r = fminf(fmaxf(r * con, 0.f), 1.f);
      g = fminf(fmaxf(g * con, 0.f), 1.f);
      bl = fminf(fmaxf(bl * con, 0.f), 1.f);
    } else if (op == 2) {
      // Saturation WITHOUT the HSV round trip.  RGB -> HSV -> (s <- clamp(s sat)) -> RGB leaves v and h alone and maps
      // every channel c = v (1 - k s) (k in {0, f, 1 - f, 1} by the hue sector) to v (1 - k s'), i.e.
      // c' = v - (v - c) s' / s: three FMAs instead of ~50 instructions of sector arithmetic and selects -- the same
      // function up to rounding (the restatement in oracle/curla_oracle.py keeps the round trip; agreement 1e-6).
      const float mx = fmaxf(r, fmaxf(g, bl)), mn = fminf(r, fminf(g, bl));
      const float s = fminf((mx - mn) * rcp_fast(mx + 1e-8f), 1.f);
      const float s2 = fminf(fmaxf(s * sat, 0.f), 1.f);
      const float ratio = s > 0.f ? s2 * rcp_fast(s) : 0.f;
      r = fmaxf(mx - (mx - r) * ratio, 0.f);  // (s' / s can exceed (mx + 1e-8) / d by an ulp: keep [0, v])
      g = fmaxf(mx - (mx - g) * ratio, 0.f);
      bl = fmaxf(mx - (mx - bl) * ratio, 0.f);
    } else if (op == 3) {
      float h, s, v;
      rgb_to_hsv(r, g, bl, h, s, v);
      h = h + hue;
      h = h - kTwoPi * floorf(h * (1.f / kTwoPi));  // fmod into [0, 2pi)
      h = fminf(fmaxf(h, 0.f), kTwoPi);
      hsv_to_rgb(h, s, v, r, g, bl);
    }
  }
}

// params[img] = (apply, contrast, saturation, hue_radians); order[4] = permutation of {0 brightness(identity),
// 1 contrast, 2 saturation, 3 hue}; one image = one RGB frame of the stack (augmentations.py:124-128).
__global__ void color_jiggle_kernel(const uint8_t* frames, const int64_t* idx, const float* params, const int* order,
                                    int B, int C, int H, int W, float* out) {
  const int k = C / 3;
  const size_t n = (size_t)B * H * W * k;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int o0 = order[0], o1 = order[1], o2 = order[2], o3 = order[3];
  for (; i < n; i += stride) {
    const int fr = i % k;
    const size_t pix = i / k;  // (b, y, x) flattened
    const int b = pix / ((size_t)H * W);
    const size_t yx = pix - (size_t)b * H * W;
    const int64_t fi = idx ? idx[b] : b;
    const uint8_t* src = frames + ((size_t)fi * H * W + yx) * C + 3 * fr;
    constexpr float k255 = 1.f / 255.f;
    float r = src[0] * k255, g = src[1] * k255, bl = src[2] * k255;  // `image_batch /= 255.0`, augmentations.py:118
    jiggle_rgb(r, g, bl, params + ((size_t)b * k + fr) * 4, o0, o1, o2, o3);
    float* dst = out + pix * C + 3 * fr;
    dst[0] = r * 255.f, dst[1] = g * 255.f, dst[2] = bl * 255.f;
  }
}

// The same with one thread per PIXEL (all K frames of the stack) and one grid row per sample: no 64-bit division per
// element (the flat form spends ~100 instructions on i % k, i / k, pix / (H W)), the pixel's 3 K bytes as aligned
// dwords when 3 K is a multiple of 4 (frame_stack 4: three dwords), its 3 K floats as 16-byte stores.  The arithmetic
// per RGB triple is the flat kernel's (jiggle_rgb), so the results are bit-identical.
template <int K>
__global__ __launch_bounds__(256) void color_jiggle_pixel_kernel(const uint8_t* frames, const int64_t* idx,
                                                                   const float* params, const int* order, int HW,
                                                                   float* out) {
  constexpr int C = 3 * K;
  const int b = blockIdx.y;
  const int p_raw = blockIdx.x * 256 + threadIdx.x;
  if ((p_raw & ~63) >= HW) return;             // (whole waves past the image leave; a partly covered wave stays whole:
  const int p = p_raw < HW ? p_raw : HW - 1;   //  its lanes past the image redo the last pixel and help with the stores)
  const int o0 = order[0], o1 = order[1], o2 = order[2], o3 = order[3];
  const int64_t fi = idx ? idx[b] : b;
  const uint8_t* src = frames + ((size_t)fi * HW + p) * C;
  uint8_t px[C];
  if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
    for (int u = 0; u < C / 4; ++u) {
      const uint32_t d = reinterpret_cast<const uint32_t*>(src)[u];
      px[4 * u] = d & 0xff, px[4 * u + 1] = (d >> 8) & 0xff, px[4 * u + 2] = (d >> 16) & 0xff, px[4 * u + 3] = d >> 24;
    }
  } else {
#pragma unroll
    for (int u = 0; u < C; ++u) px[u] = src[u];
  }
  float v[C];
  constexpr float k255 = 1.f / 255.f;
#pragma unroll
  for (int fr = 0; fr < K; ++fr) {
    float r = px[3 * fr] * k255, g = px[3 * fr + 1] * k255, bl = px[3 * fr + 2] * k255;
    jiggle_rgb(r, g, bl, params + ((size_t)b * K + fr) * 4, o0, o1, o2, o3);
    v[3 * fr] = r * 255.f, v[3 * fr + 1] = g * 255.f, v[3 * fr + 2] = bl * 255.f;
  }
  float* dst = out + ((size_t)b * HW + p) * C;
  if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    // A lane holds its pixel's C floats: stored directly, a wave's store instruction would write 16 bytes per lane
    // C * 4 bytes apart (a third of every 128-byte line per instruction at C = 12).  Through LDS instead: the wave's
    // 64 pixels are 64 C / 4 consecutive 16-byte chunks of the output; lane l stores chunks l, l + 64, ... -- whole lines.
    __shared__ __attribute__((aligned(16))) float stage[4][64 * C];
    float* mine = stage[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < C / 4; ++u)
      *reinterpret_cast<f32x4*>(mine + lane * C + 4 * u) = f32x4{v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int p0 = blockIdx.x * 256 + (threadIdx.x & ~63);  // the wave's first pixel
    const int nvalid = min(64, HW - p0);                    // pixels of this wave inside the image (> 0: p < HW here)
    float* wave_out = out + ((size_t)b * HW + p0) * C;
#pragma unroll
    for (int u = 0; u < C / 4; ++u) {
      const int chunk = lane + 64 * u;  // 16-byte chunk of the wave's output: floats [4 chunk, 4 chunk + 4)
      if (4 * chunk < nvalid * C) *reinterpret_cast<f32x4*>(wave_out + 4 * chunk) = *reinterpret_cast<const f32x4*>(mine + 4 * chunk);
    }
  } else if (p_raw < HW) {
#pragma unroll
    for (int u = 0; u < C; ++u) dst[u] = v[u];
  }
}

// the same on the reference's tensor contract: float NCHW [B][C][H][W] in [0,255] in and out
// (ColorJiggle.training_augmentation(image_batch), augmentations.py:105-136; in == out is allowed)
__global__ void color_jiggle_nchw_kernel(const float* in, const float* params, const int* order, int B, int C, int H,
                                         int W, float* out) {
  const int k = C / 3;
  const size_t plane = (size_t)H * W;
  const size_t n = (size_t)B * k * plane;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int o0 = order[0], o1 = order[1], o2 = order[2], o3 = order[3];
  for (; i < n; i += stride) {
    const size_t img = i / plane;  // b * k + frame
    const size_t yx = i - img * plane;
    const size_t base = img * 3 * plane + yx;
    constexpr float k255 = 1.f / 255.f;
    float r = in[base] * k255, g = in[base + plane] * k255, bl = in[base + 2 * plane] * k255;
    jiggle_rgb(r, g, bl, params + img * 4, o0, o1, o2, o3);
    out[base] = r * 255.f, out[base + plane] = g * 255.f, out[base + 2 * plane] = bl * 255.f;
  }
}

// rows [0,top) and [H-bottom,H) of every frame are painted with colors[c%3], then noise is added and the
// result clamped to [0,255] (augmentations.py:185-203)
__global__ void noisy_cover_kernel(const uint8_t* frames, const int64_t* idx, const float* noise, float c0, float c1,
                                   float c2, int top, int bottom, int B, int C, int H, int W, float* out) {
  const size_t n = (size_t)B * H * W * C;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int c = i % C;
    const size_t pix = i / C;
    const int b = pix / ((size_t)H * W);
    const size_t yx = pix - (size_t)b * H * W;
    const int y = yx / W;
    const int64_t fi = idx ? idx[b] : b;
    float v = (float)frames[((size_t)fi * H * W + yx) * C + c];
    if (y < top || y >= H - bottom) v = (c % 3 == 0) ? c0 : (c % 3 == 1) ? c1 : c2;
    v += noise[i];
    out[i] = fminf(fmaxf(v, 0.f), 255.f);
  }
}

// noisy_cover_kernel with the noise DRAWN here instead of read (augmentations.py:157,197: RandomGaussianNoise(0, std)):
// element i of the flat NHWC batch gets std * philox_normal(seed, offset, i) (common.h), so one thread owns one Philox
// counter = 4 consecutive elements: 4 source bytes in (one aligned dword where the frame and its address allow), one
// 16-byte store out -- 1 B read + 4 B written per element, where torch.randn + `* std` + noisy_cover_kernel move
// 4 + (4 + 4) + (1 + 4 + 4).  Cover rows need no pixel coordinates: inside a frame of H W C bytes row y < top is byte
// r < top W C and y >= H - bottom is r >= (H - bottom) W C; the colour channel is (r % C) % 3.
// rng_dev / colors_dev != nullptr: (seed, offset) / the three colours are read from device memory when the kernel
// RUNS (a captured graph is replayed with new values), the by-value ones are ignored.
struct CoverDraw {
  float std, c0, c1, c2;
  unsigned long long seed, offset;
  const unsigned long long* rng_dev;
  const float* colors_dev;
};

__global__ __launch_bounds__(256) void noisy_cover_rng_kernel(const uint8_t* frames, const int64_t* idx, CoverDraw a,
                                                                unsigned lo, unsigned hi, unsigned frame, unsigned C,
                                                                unsigned n, float* out, float* noise_out) {
  // v + std * z must round like the explicit-noise kernel fed noise_out (product first, then the sum): no fused
  // multiply-add across the two
#pragma clang fp contract(off)
  const unsigned long long seed = a.rng_dev ? a.rng_dev[0] : a.seed, offs = a.rng_dev ? a.rng_dev[1] : a.offset;
  const float c0 = a.colors_dev ? a.colors_dev[0] : a.c0, c1 = a.colors_dev ? a.colors_dev[1] : a.c1,
              c2 = a.colors_dev ? a.colors_dev[2] : a.c2;
  const unsigned groups = (n >> 2) + ((n & 3) != 0);
  const bool vec = ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(noise_out)) & 15) == 0;  // (null: aligned)
  for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < groups; j += gridDim.x * 256) {
    float z[4];
    philox_normal4(seed, offs + j, z);
    const unsigned e0 = 4 * j, cnt = min(4u, n - e0);
    unsigned b = e0 / frame, r = e0 - b * frame;  // sample and byte inside its frame of element e0
    const uint8_t* src = frames + (size_t)(idx ? idx[b] : (int64_t)b) * frame + r;
    unsigned px[4], rr[4];
    if (r + 4 <= frame && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
      const uint32_t d = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
      for (int e = 0; e < 4; ++e) px[e] = (d >> (8 * e)) & 0xffu, rr[e] = r + e;
    } else {  // the group straddles two samples (H W C not a multiple of 4), or the bytes are off a dword boundary
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        px[e] = 0, rr[e] = 0;
        if ((unsigned)e < cnt) {
          if (r == frame) r = 0, ++b, src = frames + (size_t)(idx ? idx[b] : (int64_t)b) * frame;
          px[e] = *src++, rr[e] = r++;
        }
      }
    }
    float nz[4], o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned ch = (rr[e] % C) % 3;
      float v = (float)px[e];
      if (rr[e] < lo || rr[e] >= hi) v = ch == 0 ? c0 : ch == 1 ? c1 : c2;
      nz[e] = a.std * z[e];
      o[e] = fminf(fmaxf(v + nz[e], 0.f), 255.f);
    }
    if (vec && cnt == 4) {
      *reinterpret_cast<f32x4*>(out + e0) = f32x4{o[0], o[1], o[2], o[3]};
      if (noise_out) *reinterpret_cast<f32x4*>(noise_out + e0) = f32x4{nz[0], nz[1], nz[2], nz[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((unsigned)e < cnt) {
          out[e0 + e] = o[e];
          if (noise_out) noise_out[e0 + e] = nz[e];
        }
    }
  }
}

// the same on the reference's tensor contract: float NCHW in [0,255] in, noise NCHW, out NCHW
// (NoisyCover.training_augmentation(image_batch), augmentations.py:170-205; in == out is allowed)
__global__ void noisy_cover_nchw_kernel(const float* in, const float* noise, float c0, float c1, float c2, int top,
                                        int bottom, int B, int C, int H, int W, float* out) {
  const size_t n = (size_t)B * C * H * W;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int y = (i / W) % H;
    const int c = (i / ((size_t)W * H)) % C;
    float v = in[i];
    if (y < top || y >= H - bottom) v = (c % 3 == 0) ? c0 : (c % 3 == 1) ? c1 : c2;
    v += noise[i];
    out[i] = fminf(fmaxf(v, 0.f), 255.f);
  }
}

// plain gather + u8 -> f32 (identity augmentation materialised as NHWC floats)
__global__ void gather_nhwc_kernel(const uint8_t* frames, const int64_t* idx, int B, size_t frame, float* out) {
  const size_t n = (size_t)B * frame;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int b = i / frame;
    const int64_t fi = idx ? idx[b] : b;
    out[i] = (float)frames[(size_t)fi * frame + (i - (size_t)b * frame)];
  }
}

// ---- RandomCutout (beyond the reference: RAD's cutout / cutout-color) ----
// out[s][y][x][c] = colour(s)[c % 3] inside the sample's box [y0, y0 + bh) x [x0, x0 + bw), frames[row(s)][y][x][c]
// elsewhere; uint8 NHWC in and out, all frames of a stack share the box.  Like the shift a byte mover whose thread owns
// 16 consecutive output bytes of a sample, but the source of a group is simply the same 16 bytes of the source frame:
// no address depends on the box (it is clamped into the frame besides), so whatever the block holds nothing is read or
// written outside a frame.  A group wholly outside the box is one 16-byte load and one 16-byte store; a group wholly
// inside is a store of the colour pattern without a load; a group that crosses a box edge (or straddles rows of which
// the box touches one) loads its 16 bytes like an outside group and replaces the bytes inside the box in registers
// (cut_blend) -- arithmetic only, no byte-wise memory access: in the shift kernel the byte loads of such groups set the
// time.  Byte-wise loads and stores are left to frames that are no whole number of groups and to an
// `out` off the 16-byte grid (vec == false), as there.
// The frame of the kernel (sample loop, byte loop, U8_UNROLL groups per trip with their loads before the first store) is
// u8_mover_kernel's written out once more: as an Op of that skeleton, with the same registers, LDS reads and occupancy
// as here, the cutout ran 48.3 us where this kernel runs 45.1 us (84 x 84 x 9, n = 1536).
struct CutGeom {
  unsigned rb, frame;  // bytes of a row / of a frame
  int C, y0, y1;       // box rows [y0, y1)
  unsigned xb0, xb1;   // box columns in bytes of a row [xb0, xb1)
  uint32_t col[3];
};

__device__ __forceinline__ bool cut_inside(const CutGeom& q, int yy, unsigned xb) {
  return yy >= q.y0 && yy < q.y1 && xb >= q.xb0 && xb < q.xb1;
}

__device__ __forceinline__ uint32_t cut_colour(const CutGeom& q, int c3) {  // (selects: no runtime-indexed array)
  return c3 == 0 ? q.col[0] : c3 == 1 ? q.col[1] : q.col[2];
}

// the 16 bytes `v` of the group at byte r = y rb + xb with the bytes inside the box replaced by their colour:
// (row, byte in row, channel) are stepped, not divided
__device__ __forceinline__ u32x4 cut_blend(const CutGeom& q, u32x4 v, unsigned y, unsigned xb) {
  int yy = (int)y, c = (int)(xb % (unsigned)q.C), c3 = c % 3;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int sh = 8 * (e & 3);
    if (cut_inside(q, yy, xb)) w[e >> 2] = (w[e >> 2] & ~(0xffu << sh)) | (cut_colour(q, c3) << sh);
    if (++c3 == 3) c3 = 0;
    if (++c == q.C) c = 0, c3 = 0;
    if (++xb == q.rb) xb = 0, ++yy;  // (rb is a multiple of C: c is 0 here)
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// one (possibly short) group byte by byte: frames of no whole number of groups, `out` off the 16-byte grid
__device__ __forceinline__ void cut_group_bytes(const uint8_t* src, uint8_t* dst, const CutGeom& q, unsigned r) {
  const unsigned cnt = min(16u, q.frame - r);
  const unsigned y = r / q.rb;
  unsigned xb = r - y * q.rb;
  int yy = (int)y, c = (int)(xb % (unsigned)q.C), c3 = c % 3;
  for (unsigned e = 0; e < cnt; ++e) {
    dst[r + e] = cut_inside(q, yy, xb) ? (uint8_t)cut_colour(q, c3) : src[r + e];
    if (++c3 == 3) c3 = 0;
    if (++c == q.C) c = 0, c3 = 0;
    if (++xb == q.rb) xb = 0, ++yy;
  }
}

__global__ __launch_bounds__(256) void cutout_u8_kernel(const uint8_t* frames, const int64_t* idx, int period,
                                                          const int32_t* y0, const int32_t* x0, const int32_t* size,
                                                          const int32_t* rgb, int n, int H, int W, int C,
                                                          unsigned groups, bool vec, uint8_t* out) {
  CutGeom q;
  q.C = C, q.rb = (unsigned)W * C, q.frame = (unsigned)H * q.rb;
  const bool c3ok = C % 3 == 0;  // then a byte's colour is (byte offset in row) % 3 and the pattern runs on across rows
  const unsigned stride = gridDim.x * 256;
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    const int p = s % period;
    const int64_t row = idx ? idx[p] : (int64_t)p;
    // whatever the block holds is clamped: the box lies inside the frame (an empty one is a plain copy)
    const uint32_t sz = (uint32_t)size[s], colour = (uint32_t)rgb[s];
    const int yc = min(max(y0[s], 0), H), xc = min(max(x0[s], 0), W);
    const int bh = min((int)(sz & 0xffffu), H - yc), bw = min((int)(sz >> 16), W - xc);
    const bool empty = bh == 0 || bw == 0;
    q.y0 = yc, q.y1 = empty ? yc : yc + bh;
    q.xb0 = (unsigned)(xc * C), q.xb1 = (unsigned)((xc + bw) * C);
    q.col[0] = colour & 0xffu, q.col[1] = (colour >> 8) & 0xffu, q.col[2] = (colour >> 16) & 0xffu;
    // the pattern of a group whose first byte has (byte offset in row) % 3 == k is {pat[k], pat[k + 1], pat[k + 2], pat[k]}
    // (indices mod 3): pat[m] = colours m, m + 1, m + 2, m
    uint32_t pat[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
      pat[m] = q.col[m] | (q.col[(m + 1) % 3] << 8) | (q.col[(m + 2) % 3] << 16) | (q.col[m] << 24);
    const uint8_t* src = frames + (size_t)row * q.frame;
    uint8_t* dst = out + (size_t)s * q.frame;
    if (!vec) {
      for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) cut_group_bytes(src, dst, q, 16 * g);
      continue;
    }
    for (unsigned g0 = blockIdx.x * 256 + threadIdx.x; g0 < groups; g0 += U8_UNROLL * stride) {
      u32x4 v[U8_UNROLL];
      int kind[U8_UNROLL];  // 0 outside the box, 1 inside, 2 both
      unsigned gy[U8_UNROLL], gxb[U8_UNROLL];
#pragma unroll
      for (int u = 0; u < U8_UNROLL; ++u) {
        const unsigned g = g0 + u * stride;
        kind[u] = 0, gy[u] = 0, gxb[u] = 0;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (g < groups) {
          const unsigned r = 16 * g;
          const unsigned y = r / q.rb, xb = r - y * q.rb;
          gy[u] = y, gxb[u] = xb;
          const unsigned last = xb + 15;  // the group's last byte, counted from the start of row y
          if (empty) {
            kind[u] = 0;
          } else if (last < q.rb) {  // one row
            const bool in_rows = (int)y >= q.y0 && (int)y < q.y1;
            if (!in_rows || last < q.xb0 || xb >= q.xb1) kind[u] = 0;
            else kind[u] = (xb >= q.xb0 && last < q.xb1) ? 1 : 2;
          } else if (last < 2 * q.rb) {  // rows y and y + 1
            const unsigned last2 = last - q.rb;
            const bool in0 = (int)y >= q.y0 && (int)y < q.y1, in1 = (int)y + 1 >= q.y0 && (int)y + 1 < q.y1;
            if ((!in0 || xb >= q.xb1) && (!in1 || last2 < q.xb0)) kind[u] = 0;
            else kind[u] = (in0 && in1 && q.xb0 == 0 && q.xb1 == q.rb) ? 1 : 2;
          } else {  // rows shorter than a group
            const unsigned ylast = (r + 15) / q.rb;
            kind[u] = ((int)ylast < q.y0 || (int)y >= q.y1) ? 0 : 2;
          }
          if (kind[u] != 1) __builtin_memcpy(&v[u], src + r, 16);  // inside the frame: frame % 16 == 0
        }
      }
#pragma unroll
      for (int u = 0; u < U8_UNROLL; ++u) {
        const unsigned g = g0 + u * stride;
        if (g < groups) {
          u32x4 o = v[u];
          if (kind[u] == 1 && c3ok) {
            const unsigned k = gxb[u] % 3;
            const uint32_t a = k == 0 ? pat[0] : k == 1 ? pat[1] : pat[2], b = k == 0 ? pat[1] : k == 1 ? pat[2] : pat[0],
                           c = k == 0 ? pat[2] : k == 1 ? pat[0] : pat[1];
            o = u32x4{a, b, c, a};
          } else if (kind[u] != 0) {
            o = cut_blend(q, o, gy[u], gxb[u]);
          }
          *reinterpret_cast<u32x4*>(dst + 16 * g) = o;
        }
      }
    }
  }
}

// ---- Compose(move, paint): a mover of u8_mover.h with the cutout's box painted over its output, in ONE launch ----
// out[s] = the inner Op's output frame with colour(s)[c % 3] inside the sample's box, the box in coordinates of the OUTPUT
// frame (Ho x Wo) and clamped into it exactly as cutout_u8_kernel clamps it.  A cutout is a pointwise repaint of what the
// mover produces, and the skeleton has each group's 16 bytes in registers before the store: the ring is read once and
// the scratch written once, where a mover launch followed by a cutout launch moves the minibatch through memory twice.
// Per group, by cutout_u8_kernel's three kinds (paint_kind): outside the box the inner Op's load and finish as they are;
// wholly inside nothing is loaded and the colour pattern is stored; across a box edge the inner Op's bytes are blended in
// registers (paint_blend: cut_blend's arithmetic).  Byte-wise (group_bytes) the inner Op writes its group and the bytes
// inside the box are painted over by the same thread.  The colours and pattern words are plain members selected BY VALUE
// (sel3): cut_colour's select between elements of q.col is a select of addresses that keeps the whole per-sample struct
// in memory -- LDS in cutout_u8_kernel, private memory for the larger struct here.
struct PaintGeom {
  unsigned rb, frame;       // bytes of a row / of a frame of the OUTPUT
  int C, y0, y1;            // box rows [y0, y1)
  unsigned xb0, xb1;        // box columns in bytes of a row [xb0, xb1)
  uint32_t c0, c1, c2;      // the colours of channels 0, 1, 2 (mod 3)
  uint32_t p0, p1, p2;      // pattern words: pm = colours m, m + 1, m + 2, m (indices mod 3), as in cutout_u8_kernel
  bool empty, c3ok;         // no box; C % 3 == 0
};

__device__ __forceinline__ uint32_t sel3(unsigned k, uint32_t a, uint32_t b, uint32_t c) {  // (copies: selects of values)
  return k == 0 ? a : k == 1 ? b : c;
}

__device__ __forceinline__ bool paint_inside(const PaintGeom& q, int yy, unsigned xb) {
  return yy >= q.y0 && yy < q.y1 && xb >= q.xb0 && xb < q.xb1;
}

// 0: the group at byte r = y rb + xb lies outside the box, 1: inside, 2: both (cutout_u8_kernel's classification)
__device__ __forceinline__ int paint_kind(const PaintGeom& q, unsigned r, unsigned y, unsigned xb) {
  const unsigned last = xb + 15;  // the group's last byte, counted from the start of row y
  if (q.empty) return 0;
  if (last < q.rb) {  // one row
    const bool in_rows = (int)y >= q.y0 && (int)y < q.y1;
    if (!in_rows || last < q.xb0 || xb >= q.xb1) return 0;
    return (xb >= q.xb0 && last < q.xb1) ? 1 : 2;
  }
  if (last < 2 * q.rb) {  // rows y and y + 1
    const unsigned last2 = last - q.rb;
    const bool in0 = (int)y >= q.y0 && (int)y < q.y1, in1 = (int)y + 1 >= q.y0 && (int)y + 1 < q.y1;
    if ((!in0 || xb >= q.xb1) && (!in1 || last2 < q.xb0)) return 0;
    return (in0 && in1 && q.xb0 == 0 && q.xb1 == q.rb) ? 1 : 2;
  }
  const unsigned ylast = (r + 15) / q.rb;  // rows shorter than a group
  return ((int)ylast < q.y0 || (int)y >= q.y1) ? 0 : 2;
}

// cut_blend's arithmetic with the colours by value
__device__ __forceinline__ u32x4 paint_blend(const PaintGeom& q, u32x4 v, unsigned y, unsigned xb) {
  int yy = (int)y, c = (int)(xb % (unsigned)q.C), c3 = c % 3;
  const uint32_t c0 = q.c0, c1 = q.c1, c2 = q.c2;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int sh = 8 * (e & 3);
    if (paint_inside(q, yy, xb)) w[e >> 2] = (w[e >> 2] & ~(0xffu << sh)) | (sel3((unsigned)c3, c0, c1, c2) << sh);
    if (++c3 == 3) c3 = 0;
    if (++c == q.C) c = 0, c3 = 0;
    if (++xb == q.rb) xb = 0, ++yy;  // (rb is a multiple of C: c is 0 here)
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// group bytes [lo, hi) as a mask of whole bytes (0 where the run is empty)
__device__ __forceinline__ u128 paint_run_mask(int lo, int hi) {
  return hi > lo ? (~(u128)0 >> (8 * (16 - (hi - lo)))) << (8 * lo) : (u128)0;
}

// paint_blend for C % 3 == 0 and rows no shorter than a group, without a walk over the bytes: the bytes of the box in
// the group are one run per row the group touches (two rows at most), and the colour of byte e is (xb + e) % 3 across
// the row end too (a row is a multiple of 3 bytes) -- the pattern words under a mask of two runs.
__device__ __forceinline__ u32x4 paint_blend_runs(const PaintGeom& q, u32x4 v, unsigned y, unsigned xb, u32x4 pattern) {
  const int x = (int)xb, rel = (int)q.rb - x;  // the group byte at which row y + 1 starts
  const int x0 = (int)q.xb0, x1 = (int)q.xb1;
  u128 m = 0;
  if ((int)y >= q.y0 && (int)y < q.y1) m = paint_run_mask(max(x0 - x, 0), min(min(x1 - x, rel), 16));
  if ((int)y + 1 >= q.y0 && (int)y + 1 < q.y1) m |= paint_run_mask(min(rel + x0, 16), min(rel + x1, 16));
  const u128 o = (__builtin_bit_cast(u128, v) & ~m) | (__builtin_bit_cast(u128, pattern) & m);
  return __builtin_bit_cast(u32x4, o);
}

template <class Inner>
struct PaintOp {
  Inner in;
  const int32_t *y0, *x0, *size, *rgb;
  int Ho, Wo, C;
  unsigned src_frame, out_frame;

  struct Geom {
    typename Inner::Geom g;
    PaintGeom p;
  };

  struct Held {
    typename Inner::Held h;
    unsigned yk = 0, xb = 0;  // the group's row y and its kind (paint_kind) as y << 2 | kind; its byte in that row
  };

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.g = in.sample(s);
    PaintGeom& b = q.p;
    b.C = C, b.rb = Inner::out_row(q.g), b.frame = out_frame, b.c3ok = C % 3 == 0;  // (the inner Op's row: ONE division per group)
    // whatever the block holds is clamped: the box lies inside the output frame (an empty one is a plain move)
    const uint32_t sz = (uint32_t)size[s], colour = (uint32_t)rgb[s];
    const int yc = min(max(y0[s], 0), Ho), xc = min(max(x0[s], 0), Wo);
    const int bh = min((int)(sz & 0xffffu), Ho - yc), bw = min((int)(sz >> 16), Wo - xc);
    b.empty = bh == 0 || bw == 0;
    b.y0 = yc, b.y1 = b.empty ? yc : yc + bh;
    b.xb0 = (unsigned)(xc * C), b.xb1 = (unsigned)((xc + bw) * C);
    const uint32_t c0 = colour & 0xffu, c1 = (colour >> 8) & 0xffu, c2 = (colour >> 16) & 0xffu;
    b.c0 = c0, b.c1 = c1, b.c2 = c2;
    b.p0 = c0 | (c1 << 8) | (c2 << 16) | (c0 << 24);
    b.p1 = c1 | (c2 << 8) | (c0 << 16) | (c1 << 24);
    b.p2 = c2 | (c0 << 8) | (c1 << 16) | (c2 << 24);
    return q;
  }

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    const unsigned y = r / q.p.rb;  // (below 2^29: the entry point refuses taller frames)
    h.xb = r - y * q.p.rb;
    const int kind = paint_kind(q.p, r, y, h.xb);
    h.yk = y << 2 | (unsigned)kind;
    if (kind != 1) Inner::load(q.g, src, r, h.h);
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t* src, unsigned r, const Held& h) {
    const unsigned kind = h.yk & 3;
    // C % 3 == 0: a byte's colour is (byte offset in row) % 3, and the pattern runs on across rows -- the group's words
    // are patterns k, k + 1, k + 2, k (mod 3)
    const unsigned k = h.xb % 3;
    const uint32_t a = sel3(k, q.p.p0, q.p.p1, q.p.p2);
    const u32x4 pattern = u32x4{a, sel3(k, q.p.p1, q.p.p2, q.p.p0), sel3(k, q.p.p2, q.p.p0, q.p.p1), a};
    if (kind == 1 && q.p.c3ok) return pattern;
    u32x4 o = u32x4{0u, 0u, 0u, 0u};
    if (kind != 1) o = Inner::finish(q.g, src, r, h.h);
    if (kind != 0) {
      if (q.p.c3ok && q.p.rb >= 16) o = paint_blend_runs(q.p, o, h.yk >> 2, h.xb, pattern);  // (uniform over the launch)
      else o = paint_blend(q.p, o, h.yk >> 2, h.xb);
    }
    return o;
  }

  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    Inner::group_bytes(q.g, src, dst, r);
    const PaintGeom& b = q.p;
    if (b.empty) return;
    const unsigned cnt = min(16u, b.frame - r);
    const unsigned y = r / b.rb;
    unsigned xb = r - y * b.rb;
    int yy = (int)y, c = (int)(xb % (unsigned)b.C), c3 = c % 3;
    for (unsigned e = 0; e < cnt; ++e) {
      if (paint_inside(b, yy, xb)) dst[r + e] = (uint8_t)sel3((unsigned)c3, b.c0, b.c1, b.c2);
      if (++c3 == 3) c3 = 0;
      if (++c == b.C) c = 0, c3 = 0;
      if (++xb == b.rb) xb = 0, ++yy;
    }
  }
};

// the plain mover where there is no box (size == nullptr), the mover with the box painted in where there is one
template <class Op>
int launch_move_cutout(const Op& op, const int32_t* y0, const int32_t* x0, const int32_t* size, const int32_t* rgb, int Ho,
                       int Wo, int C, const uint8_t* frames, const int64_t* idx, int period, int n, long long out_frame,
                       bool vec_extra, uint8_t* out, void* stream) {
  if (!size) return launch_u8_mover(op, frames, idx, period, n, out_frame, vec_extra, out, stream);
  const PaintOp<Op> paint{op, y0, x0, size, rgb, Ho, Wo, C, op.src_frame, op.out_frame};
  return launch_u8_mover(paint, frames, idx, period, n, out_frame, vec_extra, out, stream);
}

// ---- RandomConv (beyond the reference: the random convolution of RAD / "Network Randomization") ----
// out[s][y][x][3 f + co] = sum over ci, ky, kx of w[s][co][ci][ky][kx] * in[row(s)][y + ky - 1][x + kx - 1][3 f + ci], `in`
// zero outside the frame; one weight set per sample, shared by its frames; uint8 NHWC in, float NHWC out, not clamped.
// Every accumulator is ONE fmaf chain from 0 over (ky, kx, ci) in that order -- the NCHW kernel below runs the same chain,
// so the two agree bit for bit, and a filter of zeros and ones returns bytes exactly.
//
// Tiling.  A workgroup owns RC_TILE = 1024 consecutive pixels [p0, p0 + 1024) of ONE sample's flattened frame (thread t:
// pixels p0 + t + 256 i, so a wave's lanes are 64 neighbouring pixels).  Their 3x3 windows lie in pixels
// [p0 - W - 1, p0 + 1024 + W + 1) clipped to the frame, and in NHWC that is ONE contiguous run of bytes of the gathered
// row: it is copied to LDS once, as aligned 16-byte groups (byte-wise only at its two ends, so nothing before or behind
// the run -- hence the frame -- is read), and all nine reads of an input pixel are served from there.  Global traffic is
// (1024 + 2 W + 2) / 1024 of the frame's bytes (1.33 x at W = 168), a fifth of what is written.  The LDS image keeps the
// bytes' position on the 16-byte grid of global memory; a pixel's 3 KG bytes are read as the dwords that hold them
// and shifted into place (v_alignbit), which serves every C, also those whose pixels are no whole dwords (C = 9).
// The C floats of a pixel leave through LDS too, so that a wave stores whole lines (see the store below).
// The 81 weights are uniform over the workgroup: read once, into registers (scalar registers where the compiler can).
// Borders: which taps are inside the frame is decided from (y, x); a tap outside reads nothing of the frame -- its address
// is that of a run of zero bytes in front of the LDS image, so it contributes x = 0 through the same instructions (no
// branch and no select per tap, and no lane mask per tap to keep alive across the pixel loop).
constexpr int RC_TILE = 1024;

// acc = fma(w, x, acc) with the workgroup-uniform weight taken from a SCALAR register.  Written as an instruction because
// the compiler, given fmaf, pairs the chains into packed FMAs whose operand pairs push the 81 weights out of the scalar
// file (a v_readlane per FMA in the pixel loop) or, with the weights in vector registers, double them to 162 registers;
// a packed f32 FMA issues no faster than two plain ones here.  The same IEEE fused multiply-add either way.
__device__ __forceinline__ void rc_fmac(float& acc, float w, float x) {
  asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "s"(w), "v"(x));
}

template <int KG>  // frames of a pixel convolved at a time: the whole stack (K = KG <= 4), or one by one (KG = 1, any K)
__global__ __launch_bounds__(256) void random_conv_kernel(const uint8_t* __restrict__ frames,
                                                            const int64_t* __restrict__ idx,
                                                            const float* __restrict__ weights, int B, int K, int H, int W,
                                                            float* __restrict__ out, unsigned stage_off) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rc_tile[];
  constexpr int NB = 3 * KG;          // bytes / accumulators of a group
  constexpr int NW = (NB + 3) / 4;    // dwords of NB bytes in place
  constexpr int ND = (NB + 3 + 3) / 4;  // dwords that hold NB bytes starting 0..3 bytes into the first
  const int C = 3 * K, HW = H * W;
  // LDS: `zero` bytes of 0 (3 K + 16 rounded up to 16: what the read of an outside tap at any frame offset touches), then
  // the image
  const unsigned zero = (3u * (unsigned)K + 16u + 15u) & ~15u;
  uint8_t* tile8 = reinterpret_cast<uint8_t*>(rc_tile) + zero;
  for (unsigned j = threadIdx.x; j < zero / 4; j += 256) rc_tile[j] = 0u;
  const int p0 = blockIdx.x * RC_TILE;
  const int lo = max(p0 - W - 1, 0), hi = min(p0 + RC_TILE + W + 1, HW);  // the pixels staged: [lo, hi)
  const unsigned nbytes = (unsigned)(hi - lo) * (unsigned)C;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t fi = idx ? idx[b] : (int64_t)b;
    const uint8_t* g0 = frames + ((size_t)fi * HW + lo) * C;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(g0) & 15);  // LDS byte mis + j = g0[j]
    const unsigned head = mis ? min(16u - mis, nbytes) : 0u;                // bytes in front of the first whole group
    const unsigned nfull = (nbytes - head) >> 4;
    const unsigned tail0 = head + 16 * nfull;
    for (unsigned g = threadIdx.x; g < nfull; g += 256)
      *reinterpret_cast<u32x4*>(tile8 + mis + head + 16 * g) = *reinterpret_cast<const u32x4*>(g0 + head + 16 * g);
    if (threadIdx.x < head) tile8[mis + threadIdx.x] = g0[threadIdx.x];
    if (threadIdx.x < nbytes - tail0) tile8[mis + tail0 + threadIdx.x] = g0[tail0 + threadIdx.x];
    float w[81];
#pragma unroll
    for (int i = 0; i < 81; ++i) w[i] = weights[(size_t)b * 81 + i];
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < RC_TILE / 256; ++i) {
      const int p_raw = p0 + (int)threadIdx.x + 256 * i;
      const int pw0 = p_raw & ~63;             // the wave's first pixel (p0 is a multiple of 64)
      if (pw0 >= HW) break;                    // (whole waves past the image leave; a partly covered wave stays whole:
      const int p = p_raw < HW ? p_raw : HW - 1;  //  its lanes past the image redo the last pixel and help with the stores)
      const int y = p / W, x = p - y * W;
      unsigned tap[9];  // LDS byte address of each tap's pixel (inside: it lies in [lo, hi)), or 0: the zeros
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool inside = (unsigned)(y + ky - 1) < (unsigned)H && (unsigned)(x + kx - 1) < (unsigned)W;
          tap[3 * ky + kx] = inside ? zero + mis + (unsigned)(p + (ky - 1) * W + (kx - 1) - lo) * (unsigned)C : 0u;
        }
#pragma unroll 1
      for (int f0 = 0; f0 < K; f0 += KG) {
        float acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const unsigned a = tap[3 * ky + kx] + 3u * (unsigned)f0;
            const unsigned sh = 8 * (a & 3);
            uint32_t d[NW + 1];
            d[NW] = 0u;
#pragma unroll
            for (int m = 0; m < ND; ++m) d[m] = rc_tile[(a >> 2) + m];
            float xin[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              const uint32_t word = (uint32_t)((((uint64_t)d[j / 4 + 1] << 32) | d[j / 4]) >> sh);
              xin[j] = (float)((word >> (8 * (j % 4))) & 0xffu);
            }
#pragma unroll
            for (int fr = 0; fr < KG; ++fr)
#pragma unroll
              for (int co = 0; co < 3; ++co)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
                  rc_fmac(acc[3 * fr + co], w[((co * 3 + ci) * 3 + ky) * 3 + kx], xin[3 * fr + ci]);
          }
        }
        if (stage_off) {
          // (K == KG: the lane holds its pixel's C floats.)  Stored directly, a wave's store instruction would write NB
          // floats per lane 4 C bytes apart -- a fraction of every line per instruction.  Through LDS instead, as in the
          // jitter kernel: the wave's pixels are ONE run of the output, stored in whole 16-byte chunks, lane l the chunks
          // l, l + 64, ... (dwords where the run is off the 16-byte grid, and for what is left of a short last wave).
          float* mine = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(rc_tile) + stage_off) + (threadIdx.x >> 6) * (64 * NB);
          const int lane = threadIdx.x & 63;
          if (KG == 4) {
#pragma unroll
            for (int u = 0; u < 3; ++u)
              *reinterpret_cast<f32x4*>(mine + lane * NB + 4 * u) = f32x4{acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
          } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) mine[lane * NB + j] = acc[j];
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const int total = min(64, HW - pw0) * NB;  // floats of this wave inside the image (> 0)
          float* wave_out = out + ((size_t)b * HW + pw0) * NB;
          const int nvec = (reinterpret_cast<uintptr_t>(wave_out) & 15) == 0 ? total >> 2 : 0;
          for (int c = lane; c < nvec; c += 64)
            *reinterpret_cast<f32x4*>(wave_out + 4 * c) = *reinterpret_cast<const f32x4*>(mine + 4 * c);
          for (int e = 4 * nvec + lane; e < total; e += 64) wave_out[e] = mine[e];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next pixel's floats go where these are being read)
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else if (p_raw < HW) {  // stacks of more than 4 frames, frame by frame
          float* dst = out + ((size_t)b * HW + p) * C + 3 * f0;
#pragma unroll
          for (int j = 0; j < NB; ++j) dst[j] = acc[j];
        }
      }
    }
    __syncthreads();  // (the next sample's tile goes where this one's is still being read)
  }
}

// the same on the reference's tensor contract: float NCHW in and out, one grid row per RGB frame (so the weights are
// uniform over a workgroup here too); the taps come from global memory (L1 / L2 serve the re-reads) -- not the learner path
__global__ __launch_bounds__(256) void random_conv_nchw_kernel(const float* __restrict__ in,
                                                                 const float* __restrict__ weights, int n_img, int K, int H,
                                                                 int W, float* __restrict__ out) {
  const int HW = H * W;
  for (int img = blockIdx.y; img < n_img; img += gridDim.y) {
    float w[81];
#pragma unroll
    for (int i = 0; i < 81; ++i) w[i] = weights[(size_t)(img / K) * 81 + i];
    const float* src = in + (size_t)img * 3 * HW;
    float* dst = out + (size_t)img * 3 * HW;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
      const int y = p / W, x = p - y * W;
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool inside = (unsigned)(y + ky - 1) < (unsigned)H && (unsigned)(x + kx - 1) < (unsigned)W;
          float xin[3] = {0.f, 0.f, 0.f};
          if (inside) {
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) xin[ci] = src[(size_t)ci * HW + (p + (ky - 1) * W + (kx - 1))];
          }
#pragma unroll
          for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
              acc[co] = fmaf(w[((co * 3 + ci) * 3 + ky) * 3 + kx], xin[ci], acc[co]);
        }
      }
#pragma unroll
      for (int co = 0; co < 3; ++co) dst[(size_t)co * HW + p] = acc[co];
    }
  }
}

inline int blocks_for(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b < 8192 ? b : 8192);
}

}  // namespace

extern "C" {

int curla_color_jiggle(const uint8_t* frames, const int64_t* idx, const float* params, const int32_t* order, int B,
                       int C, int H, int W, float* out, void* stream) {
  CURLA_REQUIRE(frames && params && order && out && B > 0 && C > 0 && C % 3 == 0 && H > 0 && W > 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int K = C / 3, HW = H * W;
  if (K >= 1 && K <= 4 && B <= 65535 && (long long)H * W < (1LL << 30)) {
    const dim3 grid((HW + 255) / 256, B);
    if (K == 4) hipLaunchKernelGGL(color_jiggle_pixel_kernel<4>, grid, dim3(256), 0, st, frames, idx, params, order, HW, out);
    else if (K == 3) hipLaunchKernelGGL(color_jiggle_pixel_kernel<3>, grid, dim3(256), 0, st, frames, idx, params, order, HW, out);
    else if (K == 2) hipLaunchKernelGGL(color_jiggle_pixel_kernel<2>, grid, dim3(256), 0, st, frames, idx, params, order, HW, out);
    else hipLaunchKernelGGL(color_jiggle_pixel_kernel<1>, grid, dim3(256), 0, st, frames, idx, params, order, HW, out);
    return curla_launch_status();
  }
  hipLaunchKernelGGL(color_jiggle_kernel, dim3(blocks_for((size_t)B * H * W * (C / 3))), dim3(256), 0, st, frames, idx,
                     params, order, B, C, H, W, out);
  return curla_launch_status();
}

int curla_noisy_cover(const uint8_t* frames, const int64_t* idx, const float* noise, float c0, float c1, float c2,
                      int top, int bottom, int B, int C, int H, int W, float* out, void* stream) {
  CURLA_REQUIRE(frames && noise && out && B > 0 && C > 0 && H > 0 && W > 0 && top >= 0 && bottom >= 0);
  hipLaunchKernelGGL(noisy_cover_kernel, dim3(blocks_for((size_t)B * H * W * C)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), frames, idx, noise, c0, c1, c2, top, bottom, B, C, H, W, out);
  return curla_launch_status();
}

int curla_noisy_cover_rng(const uint8_t* frames, const int64_t* idx, float std, unsigned long long seed,
                          unsigned long long offset, const unsigned long long* rng_dev, float c0, float c1, float c2,
                          const float* colors_dev, int top, int bottom, int B, int C, int H, int W, float* out,
                          float* noise_out, void* stream) {
  CURLA_REQUIRE(frames && out && B > 0 && C > 0 && H > 0 && W > 0 && top >= 0 && bottom >= 0);
  CURLA_REQUIRE((reinterpret_cast<uintptr_t>(rng_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(colors_dev) & 3) == 0);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(noise_out)) & 3) == 0);
  const unsigned long long n = (unsigned long long)B * H * W * C;
  if (n >= (1ull << 32)) return CURLA_ERR_UNSUPPORTED;  // (elements are numbered in 32 bits, like the policy head's)
  const unsigned row = (unsigned)W * C;
  const CoverDraw a{std, c0, c1, c2, seed, offset, rng_dev, colors_dev};
  hipLaunchKernelGGL(noisy_cover_rng_kernel, dim3(blocks_for((size_t)((n + 3) / 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), frames, idx, a, (unsigned)(top < H ? top : H) * row,
                     (unsigned)(bottom < H ? H - bottom : 0) * row, (unsigned)H * row, (unsigned)C, (unsigned)n, out,
                     noise_out);
  return curla_launch_status();
}

int curla_color_jiggle_nchw(const float* in, const float* params, const int32_t* order, int B, int C, int H, int W,
                            float* out, void* stream) {
  CURLA_REQUIRE(in && params && order && out && B > 0 && C > 0 && C % 3 == 0 && H > 0 && W > 0);
  hipLaunchKernelGGL(color_jiggle_nchw_kernel, dim3(blocks_for((size_t)B * H * W * (C / 3))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, params, order, B, C, H, W, out);
  return curla_launch_status();
}

int curla_noisy_cover_nchw(const float* in, const float* noise, float c0, float c1, float c2, int top, int bottom,
                           int B, int C, int H, int W, float* out, void* stream) {
  CURLA_REQUIRE(in && noise && out && B > 0 && C > 0 && H > 0 && W > 0 && top >= 0 && bottom >= 0);
  hipLaunchKernelGGL(noisy_cover_nchw_kernel, dim3(blocks_for((size_t)B * H * W * C)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, noise, c0, c1, c2, top, bottom, B, C, H, W, out);
  return curla_launch_status();
}

int curla_random_shift_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* dy, const int32_t* dx,
                          int pad, int n, int C, int H, int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && dy && dx && out && n > 0 && period > 0 && pad >= 0 && C > 0 && H > 0 && W > 0);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (2LL * pad * C >= (1LL << 30)) return CURLA_ERR_UNSUPPORTED;  // (the byte shift (dx - pad) C is a 32-bit quantity in the kernel)
  const ShiftOp op{dy, dx, pad, H, W, C, (unsigned)frame, (unsigned)frame};
  return launch_u8_mover(op, frames, idx, period, n, frame, true, out, stream);
}

int curla_cutout_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* y0, const int32_t* x0,
                    const int32_t* size, const int32_t* rgb, int n, int C, int H, int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && y0 && x0 && size && rgb && out && n > 0 && period > 0 && C > 0 && H > 0 && W > 0);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(y0) | reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(size) |
                  reinterpret_cast<uintptr_t>(rgb)) & 3) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;  // (bytes inside a frame are 32-bit quantities in the kernel)
  const bool vec = frame % 16 == 0 && aligned16(out);
  const unsigned groups = (unsigned)((frame + 15) / 16);
  const unsigned per_block = vec ? 256 * U8_UNROLL : 256;
  const unsigned gx = (groups + per_block - 1) / per_block;
  const dim3 grid(gx < 64 ? gx : 64, n < 65535 ? n : 65535);
  hipLaunchKernelGGL(cutout_u8_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), frames, idx, period, y0, x0,
                     size, rgb, n, H, W, C, groups, vec, out);
  return curla_launch_status();
}

int curla_translate_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* ty, const int32_t* tx, int n,
                       int C, int H, int W, int Ho, int Wo, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && ty && tx && out && n > 0 && period > 0 && C > 0 && H > 0 && W > 0 && Ho >= H && Wo >= W);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(ty) | reinterpret_cast<uintptr_t>(tx)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long sframe = (long long)H * W * C, oframe = (long long)Ho * Wo * C;
  // (twice an output row is a 32-bit quantity in the kernel: the run arithmetic reaches 2 Wo C)
  if ((long long)Wo * C >= (1LL << 30)) return CURLA_ERR_UNSUPPORTED;
  const TrOp op{ty, tx, H, W, C, Ho, Wo, (unsigned)sframe, (unsigned)oframe};
  return launch_u8_mover(op, frames, idx, period, n, oframe, sframe >= 16, out, stream);  // (a load of 16 bytes must fit the source frame)
}

int curla_move_cutout_u8(const uint8_t* frames, const int64_t* idx, int period, int move, const int32_t* a,
                         const int32_t* b, int pad, const int32_t* y0, const int32_t* x0, const int32_t* size,
                         const int32_t* rgb, int n, int C, int H, int W, int Ho, int Wo, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && a && b && out && n > 0 && period > 0 && pad >= 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0);
  CURLA_REQUIRE(move >= 0 && move <= 2 && (!size || (y0 && x0 && rgb)));
  CURLA_REQUIRE(move == 0 ? (Ho <= H && Wo <= W) : move == 1 ? (Ho == H && Wo == W) : (Ho >= H && Wo >= W));
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  if (size)
    CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(y0) | reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(size) |
                    reinterpret_cast<uintptr_t>(rgb)) & 3) == 0);
  const long long sframe = (long long)H * W * C, oframe = (long long)Ho * Wo * C;
  if (size && Ho >= (1 << 29)) return CURLA_ERR_UNSUPPORTED;  // (PaintOp holds a group's row and kind in one word)
  if (move == 0) {
    // (bytes inside the source frame, the larger one here, and twice an output row are 32-bit quantities in the kernel)
    if (sframe >= (1LL << 31) - 16 || (long long)Wo * C >= (1LL << 30)) return CURLA_ERR_UNSUPPORTED;
    const CropOp op{a, b, H, W, C, Ho, Wo, (unsigned)sframe, (unsigned)oframe};
    return launch_move_cutout(op, y0, x0, size, rgb, Ho, Wo, C, frames, idx, period, n, oframe, true, out, stream);
  }
  if (move == 1) {
    if (2LL * pad * C >= (1LL << 30)) return CURLA_ERR_UNSUPPORTED;  // (as curla_random_shift_u8)
    const ShiftOp op{a, b, pad, H, W, C, (unsigned)sframe, (unsigned)sframe};
    return launch_move_cutout(op, y0, x0, size, rgb, Ho, Wo, C, frames, idx, period, n, sframe, true, out, stream);
  }
  if ((long long)Wo * C >= (1LL << 30)) return CURLA_ERR_UNSUPPORTED;  // (as curla_translate_u8)
  const TrOp op{a, b, H, W, C, Ho, Wo, (unsigned)sframe, (unsigned)oframe};
  return launch_move_cutout(op, y0, x0, size, rgb, Ho, Wo, C, frames, idx, period, n, oframe, sframe >= 16, out, stream);
}

int curla_dihedral_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* code, int n, int C, int H,
                      int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && code && out && n > 0 && period > 0 && C > 0 && H > 0 && W > 0);
  CURLA_REQUIRE((reinterpret_cast<uintptr_t>(code) & 3) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;  // (bytes inside a frame are 32-bit quantities in the kernel)
  const FlipOp op{code, H, W, C, (unsigned)frame, (unsigned)frame};
  return launch_dihedral_u8(op, frames, idx, period, n, frame, out, stream);
}

int curla_grayscale_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* grey, int n, int C, int H,
                       int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && grey && out && n > 0 && period > 0 && C > 0 && C % 3 == 0 && H > 0 && W > 0);
  CURLA_REQUIRE((reinterpret_cast<uintptr_t>(grey) & 3) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;  // (as curla_dihedral_u8)
  const GreyOp op{grey, (unsigned)frame, (unsigned)frame};
  return launch_u8_mover(op, frames, idx, period, n, frame, true, out, stream);
}

int curla_affine_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* m00, const int32_t* m01,
                    const int32_t* m02, const int32_t* m10, const int32_t* m11, const int32_t* m12, int fill, int n, int C,
                    int H, int W, uint8_t* out, void* stream) {
  CURLA_REQUIRE(frames && m00 && m01 && m02 && m10 && m11 && m12 && out && n > 0 && period > 0 && C > 0 && H > 0 && W > 0);
  CURLA_REQUIRE(fill == 0 || fill == 1);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(m00) | reinterpret_cast<uintptr_t>(m01) | reinterpret_cast<uintptr_t>(m02) |
                  reinterpret_cast<uintptr_t>(m10) | reinterpret_cast<uintptr_t>(m11) | reinterpret_cast<uintptr_t>(m12)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;  // (as curla_dihedral_u8)
  const AffOp op{{m00, m01, m02, m10, m11, m12}, fill, H, W, C, (unsigned)frame};
  return launch_affine_u8(op, frames, idx, period, n, frame, out, stream);
}

int curla_random_conv(const uint8_t* frames, const int64_t* idx, const float* weights, int B, int C, int H, int W,
                      float* out, void* stream) {
  CURLA_REQUIRE(frames && weights && out && B > 0 && C > 0 && C % 3 == 0 && H > 0 && W > 0);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(out)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(idx) & 7) == 0);
  const long long frame = (long long)H * W * C;
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;  // (pixels and bytes inside a frame are 32-bit quantities in the kernel)
  // the zeros of the outside taps, the staged run of (RC_TILE + 2 W + 2) pixels, up to 15 bytes in front of it (its place
  // on the 16-byte grid) and the dwords a read of the last pixel may touch behind it
  // ... and, for stacks of up to 4 frames, the four waves' output runs of 64 pixels (the stores go through LDS)
  const int K = C / 3;
  const long long image = ((C + 16 + 15) / 16 * 16) + (((long long)RC_TILE + 2LL * W + 2) * C + 15 + 16 + 15) / 16 * 16;
  const long long lds = image + (K <= 4 ? 4LL * 64 * C * 4 : 0);
  if (lds > 64 * 1024) return CURLA_ERR_UNSUPPORTED;  // (rows of more than ~1700 pixels at C = 12)
  const unsigned stage_off = K <= 4 ? (unsigned)image : 0u;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(((long long)H * W + RC_TILE - 1) / RC_TILE), B < 65535 ? B : 65535);
  if (K == 4) hipLaunchKernelGGL(random_conv_kernel<4>, grid, dim3(256), (size_t)lds, st, frames, idx, weights, B, K, H, W, out, stage_off);
  else if (K == 3) hipLaunchKernelGGL(random_conv_kernel<3>, grid, dim3(256), (size_t)lds, st, frames, idx, weights, B, K, H, W, out, stage_off);
  else if (K == 2) hipLaunchKernelGGL(random_conv_kernel<2>, grid, dim3(256), (size_t)lds, st, frames, idx, weights, B, K, H, W, out, stage_off);
  else hipLaunchKernelGGL(random_conv_kernel<1>, grid, dim3(256), (size_t)lds, st, frames, idx, weights, B, K, H, W, out, stage_off);
  return curla_launch_status();
}

int curla_random_conv_nchw(const float* in, const float* weights, int B, int C, int H, int W, float* out, void* stream) {
  CURLA_REQUIRE(in && weights && out && in != out && B > 0 && C > 0 && C % 3 == 0 && H > 0 && W > 0);
  CURLA_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(out)) & 3) == 0);
  const long long n_img = (long long)B * (C / 3);
  if ((long long)H * W * C >= (1LL << 31) - 16 || n_img >= (1LL << 31)) return CURLA_ERR_UNSUPPORTED;
  const long long gx = ((long long)H * W + 255) / 256;
  const dim3 grid((unsigned)(gx < 65535 ? gx : 65535), (unsigned)(n_img < 65535 ? n_img : 65535));
  hipLaunchKernelGGL(random_conv_nchw_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), in, weights, (int)n_img,
                     C / 3, H, W, out);
  return curla_launch_status();
}

int curla_gather_nhwc(const uint8_t* frames, const int64_t* idx, int B, int C, int H, int W, float* out, void* stream) {
  CURLA_REQUIRE(frames && out && B > 0 && C > 0 && H > 0 && W > 0);
  hipLaunchKernelGGL(gather_nhwc_kernel, dim3(blocks_for((size_t)B * H * W * C)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), frames, idx, B, (size_t)C * H * W, out);
  return curla_launch_status();
}

}  // extern "C"
