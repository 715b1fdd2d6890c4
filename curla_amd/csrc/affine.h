// ---- RandomAffine (beyond the reference: the rotate / zoom / sub-pixel shift of kornia's and torchvision's RandomAffine) ----
// The one uint8 kernel that RESAMPLES: every output byte is a blend of four source bytes.  The map is defined in integers,
// so the device, the host restatement (RandomAffine.warp) and the tests agree bit for bit.  Six int32 words per sample,
// m00 m01 m02 m10 m11 m12, are a 16.16 fixed-point inverse map from output pixel (y, x) to source coordinates:
//   X = wrap32(m00 x + m01 y + m02)          Y = wrap32(m10 x + m11 y + m12)        (two's-complement wrap-around)
//   x0 = X >> 16 (arithmetic: floor)         fx = (X >> 8) & 255
//   y0 = Y >> 16                             fy = (Y >> 8) & 255
//   out[y][x][c] = (P(y0, x0)[c] (256 - fx) (256 - fy) + P(y0, x0 + 1)[c] fx (256 - fy)
//                 + P(y0 + 1, x0)[c] (256 - fx) fy     + P(y0 + 1, x0 + 1)[c] fx fy     + 32768) >> 16
// with P(yy, xx) = in[clamp(yy, 0, H - 1)][clamp(xx, 0, W - 1)] under fill = 1 (edge) and, under fill = 0 (zero), in[yy][xx]
// inside [0, H) x [0, W) and 0 outside.  The accumulator fits 32 unsigned bits (at most 255 * 65536 + 32768); all
// channels of a stack share the map; the output frame has the source frame's size.  The rule is total: whatever six
// words the block holds, a tap's address is clamped into the source frame before it is read (a tap outside under zero
// fill keeps its clamped address and gets the weight 0), and every output byte is written.
//
// Shape: a band through LDS -- dihedral_u8_kernel's transposing form with a box instead of columns.  Neighbouring output
// pixels come from source addresses that do not step with the output address (under a rotation they lie rows apart), so
// no run of consecutive source bytes serves a 16-byte group, which is what every Op of the mover skeleton lives on; the
// registers-on-the-skeleton form would fetch 2 C bytes per pixel and tap row with unaligned 16-byte loads, 8 loads for
// the 16 bytes of a group at C = 9, and still need a byte path along all four borders.  Here a workgroup takes a BAND of
// up to AFF_BAND consecutive groups of one sample's output.  The band is a rectangle of output pixels (its rows, and
// between them the pixels of one row or all columns); X and Y are linear over it as long as nothing wraps, so its four
// corners bound the source rows and columns of every tap: the BOX (+1 for the second tap, clamped into the frame).  The
// corners are evaluated in 64 bits: if all four fit 32 bits so does every pixel between them and wrap32 is the identity.
// The box's rows are staged in LDS with 16-byte loads (row i at i * stride; the one chunk that would end behind the frame
// goes byte by byte: ring row 0 has nothing in front of it, the slack behind a ring is not relied on), then each thread
// puts half groups of 8 bytes together from LDS bytes -- the taps and weights of a pixel are computed once and serve its
// channels (aff_groups) -- and stores them whole.  HBM sees one read and one write of the frame; the box's overlap
// between bands (a band's box under a rotation by t is about (W sin t + h cos t) rows for h output rows) is served by L2.
// Where the box does not fit AFF_LDS the band is halved, down to AFF_MIN_BAND groups; a band that still does not fit (a
// wide frame under a large angle, strong minification) or whose corners wrap (words no RandomAffine makes) gathers its
// taps from global memory directly, with the same arithmetic and the frame as its box.  The sample, hence box and band,
// is uniform over a workgroup: every branch around a barrier is taken by whole workgroups.
// Byte-wise stores are left to frames of no whole number of groups and to an `out` off the 16-byte grid (vec == false).
// What bounds it: not HBM -- the integer work per output byte (two tap sets and two divisions per
// 8 bytes, then per byte the selects, four LDS byte reads and four multiply-adds), at two workgroups per CU.
#pragma once
#include "u8_mover.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned AFF_BAND = 256 * U8_UNROLL;  // groups of a band (what a workgroup takes per trip as a mover)
constexpr unsigned AFF_MIN_BAND = 256;          // a band is not halved below two half groups per thread
constexpr unsigned AFF_LDS = 64 * 1024;         // the box's budget: two workgroups per CU

struct AffOp {
  const int32_t* m[6];  // m00 m01 m02 m10 m11 m12, each [n]
  int fill, H, W, C;
  unsigned frame;
};

struct AffGeom {
  uint32_t m00, m01, m02, m10, m11, m12;  // the sample's words, as the unsigned numbers they are multiplied as
  int H, W, C;
  bool edge;
  unsigned rb, frame;  // bytes of a row / of a frame
};

// rows [y0, y1] x columns [x0, x1] of the source frame, row i of it at i * stride of the image (LDS: the staged box;
// global: the frame itself, stride = a row)
struct AffBox {
  int y0, y1, x0, x1;
  unsigned stride;
};

// the range [lo, hi] of source rows or columns, clamped into [0, last], that the taps of the output pixels
// [xa, xb] x [ya, yb] touch along one axis; false where a corner does not fit 32 bits (the map may wrap inside)
__device__ __forceinline__ bool aff_range(uint32_t mx, uint32_t my, uint32_t m2, unsigned xa, unsigned xb, unsigned ya,
                                          unsigned yb, int last, int& lo, int& hi) {
  const int64_t ax = (int64_t)(int32_t)mx, ay = (int64_t)(int32_t)my, a2 = (int64_t)(int32_t)m2;
  const int64_t c0 = ax * xa + ay * ya + a2, c1 = ax * xb + ay * ya + a2, c2 = ax * xa + ay * yb + a2,
                c3 = ax * xb + ay * yb + a2;  // (|word| <= 2^31, x and y < 2^31: no corner leaves 64 bits)
  const int64_t mn = min(min(c0, c1), min(c2, c3)), mxx = max(max(c0, c1), max(c2, c3));
  if (mn < -(1LL << 31) || mxx >= (1LL << 31)) return false;
  lo = min(max((int)(mn >> 16), 0), last), hi = min(max((int)(mxx >> 16) + 1, 0), last);
  return true;
}

// the box of the groups [g0, g1) of the output, and whether it may be staged in `lds_bytes` of LDS
__device__ __forceinline__ bool aff_box(const AffGeom& q, unsigned g0, unsigned g1, unsigned lds_bytes, AffBox& b) {
  const unsigned first = 16 * g0, last = min(16 * g1, q.frame) - 1;  // the band's first and last byte
  const unsigned ya = first / q.rb, yb = last / q.rb;
  unsigned xa = 0, xb = (unsigned)q.W - 1;
  if (ya == yb) xa = (first - ya * q.rb) / (unsigned)q.C, xb = (last - ya * q.rb) / (unsigned)q.C;
  if (!aff_range(q.m00, q.m01, q.m02, xa, xb, ya, yb, q.W - 1, b.x0, b.x1)) return false;
  if (!aff_range(q.m10, q.m11, q.m12, xa, xb, ya, yb, q.H - 1, b.y0, b.y1)) return false;
  b.stride = ((unsigned)(b.x1 - b.x0 + 1) * (unsigned)q.C + 15u) & ~15u;
  return (uint64_t)(unsigned)(b.y1 - b.y0 + 1) * b.stride <= lds_bytes;
}

// the four taps of an output pixel: the bytes of channel 0 in the image and the weights (0 for a tap outside the frame
// under zero fill: the weights are products of one factor per axis)
struct AffTaps {
  unsigned a00, a01, a10, a11;
  uint32_t w00, w01, w10, w11;
};

__device__ __forceinline__ AffTaps aff_taps(const AffGeom& q, const AffBox& b, unsigned x, unsigned y) {
  const int32_t X = (int32_t)(q.m00 * x + q.m01 * y + q.m02), Y = (int32_t)(q.m10 * x + q.m11 * y + q.m12);
  const int x0 = X >> 16, y0 = Y >> 16;  // (in [-32768, 32767]: x0 + 1 does not overflow)
  const uint32_t fx = (uint32_t)(X >> 8) & 255u, fy = (uint32_t)(Y >> 8) & 255u;
  uint32_t wx0 = 256u - fx, wx1 = fx, wy0 = 256u - fy, wy1 = fy;
  if (!q.edge) {
    if ((unsigned)x0 >= (unsigned)q.W) wx0 = 0u;
    if ((unsigned)(x0 + 1) >= (unsigned)q.W) wx1 = 0u;
    if ((unsigned)y0 >= (unsigned)q.H) wy0 = 0u;
    if ((unsigned)(y0 + 1) >= (unsigned)q.H) wy1 = 0u;
  }
  // (the box holds every clamped tap of its band; clamping into the BOX keeps the read inside the image regardless)
  const unsigned cx0 = (unsigned)(min(max(x0, b.x0), b.x1) - b.x0) * (unsigned)q.C,
                 cx1 = (unsigned)(min(max(x0 + 1, b.x0), b.x1) - b.x0) * (unsigned)q.C;
  const unsigned ry0 = (unsigned)(min(max(y0, b.y0), b.y1) - b.y0) * b.stride,
                 ry1 = (unsigned)(min(max(y0 + 1, b.y0), b.y1) - b.y0) * b.stride;
  AffTaps t;
  t.a00 = ry0 + cx0, t.a01 = ry0 + cx1, t.a10 = ry1 + cx0, t.a11 = ry1 + cx1;
  t.w00 = wx0 * wy0, t.w01 = wx1 * wy0, t.w10 = wx0 * wy1, t.w11 = wx1 * wy1;
  return t;
}

extern __shared__ __attribute__((aligned(16))) uint8_t aff_tile[];

// One tap set or the other, by value (selects of values: a select between members of two structs by address would keep
// both in memory, as sel3 of augment.hip notes)
__device__ __forceinline__ uint32_t aff_sel(bool second, uint32_t a, uint32_t b) { return second ? b : a; }

// The groups [g0, g1) of a sample, put together from the image (kLds: the box staged in aff_tile; else the frame at src).
// A thread owns HALF a group, 8 output bytes (one 8-byte store; a wave stores 512 consecutive bytes): neighbouring lanes
// then read LDS bytes 8 apart, a 2-way bank conflict where whole groups per lane make it 4-way, and the taps of a pixel
// serve fewer lanes' worth of idle work.  kTwo (C >= 7): the 8 bytes lie in two pixels at most, whose taps are computed
// once by every lane alike, and each byte selects its pixel's; narrower pixels step (y, x, c) and compute the taps of a
// pixel where it begins.
template <bool kLds, bool kTwo>
__device__ __forceinline__ void aff_groups(const AffGeom& q, const AffBox& b, const uint8_t* src, uint8_t* dst,
                                           unsigned g0, unsigned g1, bool vec) {
  const unsigned C = (unsigned)q.C, W = (unsigned)q.W;
  for (unsigned u = 2 * g0 + threadIdx.x; u < 2 * g1; u += 256) {
    const unsigned r = 8 * u;
    if (r >= q.frame) break;  // (the last group of a frame of no whole number of groups may lack its second half)
    const unsigned cnt = min(8u, q.frame - r);
    unsigned y = r / q.rb;
    const unsigned xb = r - y * q.rb;
    unsigned x = xb / C, c = xb - x * C;
    uint32_t w[2] = {0u, 0u};
    if (kTwo) {
      const AffTaps ta = aff_taps(q, b, x, y);
      unsigned x2 = x + 1, y2 = y;
      if (x2 == W) x2 = 0, ++y2;
      // (behind the frame's last pixel y2 == H: the taps are clamped into the box like any others, and no byte uses them)
      const AffTaps tb = aff_taps(q, b, x2, y2);
#pragma unroll
      for (unsigned e = 0; e < 8; ++e) {
        if (e < cnt) {
          const bool second = c + e >= C;
          const unsigned cc = second ? c + e - C : c + e;
          const unsigned a00 = aff_sel(second, ta.a00, tb.a00) + cc, a01 = aff_sel(second, ta.a01, tb.a01) + cc,
                         a10 = aff_sel(second, ta.a10, tb.a10) + cc, a11 = aff_sel(second, ta.a11, tb.a11) + cc;
          uint32_t p00, p01, p10, p11;
          if (kLds) {
            p00 = aff_tile[a00], p01 = aff_tile[a01], p10 = aff_tile[a10], p11 = aff_tile[a11];
          } else {
            p00 = src[a00], p01 = src[a01], p10 = src[a10], p11 = src[a11];
          }
          const uint32_t v = (p00 * aff_sel(second, ta.w00, tb.w00) + p01 * aff_sel(second, ta.w01, tb.w01) +
                              p10 * aff_sel(second, ta.w10, tb.w10) + p11 * aff_sel(second, ta.w11, tb.w11) + 32768u) >> 16;
          w[e >> 2] |= v << (8 * (e & 3));
        }
      }
    } else {
      AffTaps t = aff_taps(q, b, x, y);
#pragma unroll
      for (unsigned e = 0; e < 8; ++e) {
        if (e < cnt) {
          uint32_t p00, p01, p10, p11;
          if (kLds) {
            p00 = aff_tile[t.a00 + c], p01 = aff_tile[t.a01 + c], p10 = aff_tile[t.a10 + c], p11 = aff_tile[t.a11 + c];
          } else {
            p00 = src[t.a00 + c], p01 = src[t.a01 + c], p10 = src[t.a10 + c], p11 = src[t.a11 + c];
          }
          const uint32_t v = (p00 * t.w00 + p01 * t.w01 + p10 * t.w10 + p11 * t.w11 + 32768u) >> 16;
          w[e >> 2] |= v << (8 * (e & 3));
          if (++c == C) {
            c = 0;
            if (++x == W) x = 0, ++y;
            if (e + 1 < cnt) t = aff_taps(q, b, x, y);
          }
        }
      }
    }
    if (vec) {
      *reinterpret_cast<u32x2*>(dst + r) = u32x2{w[0], w[1]};  // (r is a multiple of 8 and `out` on the 16-byte grid)
    } else {
#pragma unroll
      for (unsigned e = 0; e < 8; ++e)
        if (e < cnt) dst[r + e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
    }
  }
}

__global__ __launch_bounds__(256) void affine_u8_kernel(const uint8_t* frames, const int64_t* idx, int period, int n,
                                                          unsigned groups, bool vec, const AffOp op, unsigned lds_bytes,
                                                          uint8_t* out) {
  AffGeom q;
  q.H = op.H, q.W = op.W, q.C = op.C, q.edge = op.fill != 0, q.rb = (unsigned)op.W * op.C, q.frame = op.frame;
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    const int p = s % period;
    const int64_t row = idx ? idx[p] : (int64_t)p;
    q.m00 = (uint32_t)op.m[0][s], q.m01 = (uint32_t)op.m[1][s], q.m02 = (uint32_t)op.m[2][s];
    q.m10 = (uint32_t)op.m[3][s], q.m11 = (uint32_t)op.m[4][s], q.m12 = (uint32_t)op.m[5][s];
    const uint8_t* src = frames + (size_t)row * q.frame;
    uint8_t* dst = out + (size_t)s * q.frame;
    const AffBox whole{0, q.H - 1, 0, q.W - 1, q.rb};  // the frame as the image of the global form
    for (unsigned g_lo = blockIdx.x * AFF_BAND; g_lo < groups; g_lo += gridDim.x * AFF_BAND) {
      const unsigned g_hi = min(g_lo + AFF_BAND, groups);
      unsigned len = AFF_BAND;
      for (unsigned g0 = g_lo; g0 < g_hi;) {
        AffBox b;
        unsigned g1;
        bool staged;
        for (;;) {  // (uniform: every thread halves alike)
          g1 = min(g0 + len, g_hi);
          staged = aff_box(q, g0, g1, lds_bytes, b);
          if (staged || len <= AFF_MIN_BAND) break;
          len >>= 1;
        }
        if (staged) {
          const unsigned nc = b.stride / 16, rows = (unsigned)(b.y1 - b.y0 + 1);  // 16-byte chunks of a row of the box
          const unsigned a0 = (unsigned)b.y0 * q.rb + (unsigned)b.x0 * (unsigned)q.C;
          for (unsigned ch = threadIdx.x; ch < rows * nc; ch += 256) {
            const unsigned i = ch / nc, m = ch - i * nc;
            const unsigned a = a0 + i * q.rb + 16 * m, at = i * b.stride + 16 * m;  // (a < frame: 16 m < the row's bytes)
            if (a + 16 <= q.frame) {
              u32x4 v;
              __builtin_memcpy(&v, src + a, 16);  // one unaligned global_load_dwordx4
              *reinterpret_cast<u32x4*>(aff_tile + at) = v;
            } else {
              for (unsigned k = 0; a + k < q.frame; ++k) aff_tile[at + k] = src[a + k];
            }
          }
          __syncthreads();
          if (q.C >= 7) aff_groups<true, true>(q, b, src, dst, g0, g1, vec);
          else aff_groups<true, false>(q, b, src, dst, g0, g1, vec);
          __syncthreads();  // (the next band's box goes where this one is still being read)
        } else {
          if (q.C >= 7) aff_groups<false, true>(q, whole, src, dst, g0, g1, vec);
          else aff_groups<false, false>(q, whole, src, dst, g0, g1, vec);
        }
        g0 = g1;
      }
    }
  }
}

// as launch_dihedral_u8: bands of AFF_BAND groups, and LDS for the largest box that is staged
inline int launch_affine_u8(const AffOp& op, const uint8_t* frames, const int64_t* idx, int period, int n, long long frame,
                            uint8_t* out, void* stream) {
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;
  const bool vec = frame % 16 == 0 && aligned16(out);
  const unsigned groups = (unsigned)((frame + 15) / 16);
  const unsigned gx = (groups + AFF_BAND - 1) / AFF_BAND;
  const dim3 grid(gx < 64 ? gx : 64, n < 65535 ? n : 65535);
  const long long whole = (((long long)op.W * op.C + 15) / 16 * 16) * op.H;  // the whole frame as a box
  const unsigned lds_bytes = (unsigned)(whole < (long long)AFF_LDS ? whole : (long long)AFF_LDS);
  hipLaunchKernelGGL(affine_u8_kernel, grid, dim3(256), (size_t)lds_bytes, static_cast<hipStream_t>(stream), frames, idx,
                     period, n, groups, vec, op, lds_bytes, out);
  return curla_launch_status();
}

}  // namespace
