// The uint8 byte movers RandomShift, RandomTranslate and the crop of augment.hip: one kernel skeleton and one launch path,
// and one `Op` per augmentation that says what a group of 16 output bytes loads and what becomes of it.  (RandomCutout is
// the same frame written out once more in augment.hip: on this skeleton it was measured 7 % slower, see there and
// DESIGN.md; PaintOp there wraps a mover Op and paints the cutout's box over its bytes before the store.)  Behind them,
// on the same skeleton: FlipOp (RandomFlip / RandomRotate: pixels in reversed order), with the transposing codes of the
// dihedral group in a kernel of their own shape (dihedral_u8_kernel: through LDS), and GreyOp (RandomGrayscale: an Op
// that changes the bytes it moves).  RandomAffine, the one kernel that resamples, is not a mover: affine.h, which borrows
// only the band form of dihedral_u8_kernel and this file's types.
//
// A mover gathers a frame of the uint8 NHWC ring per sample (row(s) = idx ? idx[s % period] : s % period) and writes a
// uint8 NHWC frame per sample (roof: HBM).  A thread owns 16 consecutive OUTPUT bytes of a sample, a "group" (one 16-byte
// store); grid row = sample, so the only division is r / (row bytes) once per group.  A thread takes U8_UNROLL groups per
// trip, a grid stride apart, and issues the loads of all of them before the first store: a wave has up to 4 KiB in
// flight.  Byte-wise stores are left to output frames of no whole number of groups and to an `out` off the 16-byte grid
// (vec == false; the last group of a sample is then short).
//
// An Op holds the entry point's pointers and geometry (it is a kernel argument and never written) and provides
//   src_frame, out_frame              bytes of a source / an output frame;
//   Geom sample(s)                    sample s's parameters, clamped so that whatever the parameter block holds nothing
//                                     outside a frame is read or written; passed by value to the three below, so that it
//                                     lives in registers (a mutated Op would live in private memory);
//   load(q, src, r, held)             the loads of the group at output byte r (a multiple of 16), into a Held;
//   u32x4 finish(q, src, r, held)     the group's 16 output bytes;
//   group_bytes(q, src, dst, r)       the (possibly short) group byte by byte.
//   out_row(q)                        bytes of an output row (for PaintOp of augment.hip, which wraps an Op).
#pragma once
#include "common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 u128;

constexpr int U8_UNROLL = 4;  // groups per thread and trip

template <class Op>
__global__ __launch_bounds__(256) void u8_mover_kernel(const uint8_t* frames, const int64_t* idx, int period, int n,
                                                         unsigned groups, bool vec, const Op op, uint8_t* out) {
  const unsigned stride = gridDim.x * 256;
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    const int p = s % period;
    const int64_t row = idx ? idx[p] : (int64_t)p;
    const typename Op::Geom q = op.sample(s);
    const uint8_t* src = frames + (size_t)row * op.src_frame;
    uint8_t* dst = out + (size_t)s * op.out_frame;
    if (!vec) {
      for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) Op::group_bytes(q, src, dst, 16 * g);
      continue;
    }
    for (unsigned g0 = blockIdx.x * 256 + threadIdx.x; g0 < groups; g0 += U8_UNROLL * stride) {
      typename Op::Held held[U8_UNROLL];
#pragma unroll
      for (int u = 0; u < U8_UNROLL; ++u) {
        const unsigned g = g0 + u * stride;
        if (g < groups) Op::load(q, src, 16 * g, held[u]);
      }
#pragma unroll
      for (int u = 0; u < U8_UNROLL; ++u) {
        const unsigned g = g0 + u * stride;
        if (g < groups) *reinterpret_cast<u32x4*>(dst + 16 * g) = Op::finish(q, src, 16 * g, held[u]);
      }
    }
  }
}

// u8_mover_kernel's share of ONE sample, for a kernel that takes another form for some of its samples
// (dihedral_u8_kernel).  The loop is written out once more because u8_mover_kernel calling this function compiles to
// other code than it has: the movers that exist keep theirs instruction for instruction.
template <class Op>
__device__ __forceinline__ void u8_mover_sample(const typename Op::Geom& q, const uint8_t* src, uint8_t* dst,
                                                unsigned groups, bool vec) {
  const unsigned stride = gridDim.x * 256;
  if (!vec) {
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) Op::group_bytes(q, src, dst, 16 * g);
    return;
  }
  for (unsigned g0 = blockIdx.x * 256 + threadIdx.x; g0 < groups; g0 += U8_UNROLL * stride) {
    typename Op::Held held[U8_UNROLL];
#pragma unroll
    for (int u = 0; u < U8_UNROLL; ++u) {
      const unsigned g = g0 + u * stride;
      if (g < groups) Op::load(q, src, 16 * g, held[u]);
    }
#pragma unroll
    for (int u = 0; u < U8_UNROLL; ++u) {
      const unsigned g = g0 + u * stride;
      if (g < groups) *reinterpret_cast<u32x4*>(dst + 16 * g) = Op::finish(q, src, 16 * g, held[u]);
    }
  }
}

// `out_frame` in 64 bits: bytes inside an output frame (hence inside a source frame, which only the crop has larger: its
// entry point checks that one) are 32-bit quantities in the kernel.  vec_extra: what the Op's 16-byte loads ask for beyond whole groups and an aligned `out`.
template <class Op>
int launch_u8_mover(const Op& op, const uint8_t* frames, const int64_t* idx, int period, int n, long long out_frame,
                    bool vec_extra, uint8_t* out, void* stream) {
  if (out_frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;
  const bool vec = out_frame % 16 == 0 && aligned16(out) && vec_extra;
  const unsigned groups = (unsigned)((out_frame + 15) / 16);
  const unsigned per_block = vec ? 256 * U8_UNROLL : 256;
  const unsigned gx = (groups + per_block - 1) / per_block;
  const dim3 grid(gx < 64 ? gx : 64, n < 65535 ? n : 65535);
  hipLaunchKernelGGL(u8_mover_kernel<Op>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), frames, idx, period, n,
                     groups, vec, op, out);
  return curla_launch_status();
}

// ---- RandomShift (beyond the reference: the pad-and-crop shift of DrQ / DrQ-v2) ----
// out[s][y][x][c] = in[row(s)][clamp(y + dy[s] - pad, 0, H - 1)][clamp(x + dx[s] - pad, 0, W - 1)][c]: a frame padded by
// `pad` replicated edge pixels on every side, then an H x W window cut at (dy, dx).  The shift is the same for every
// channel, so in bytes it is (dx - pad) C along a row and byte b of an output row comes from byte b + (dx - pad) C of the
// source row wherever that lies inside the row: a group that sits in ONE output row and whose 16 source bytes need no
// x-clamp is one unaligned 16-byte load (it cannot leave the source row, hence not the ring).  Row clamping only picks
// the source row.  Groups that straddle two rows or touch the replicated left / right pixels walk their bytes ((y, x, c)
// are stepped, not divided).  Measured: what sets the time is not the fast path but these byte-wise
// groups -- a wave that holds one runs the 16 byte loads for it, and at rows of 756 bytes (84 x 84 x 9: 47.25 groups)
// every wave holds a row-straddling group.
struct ShiftGeom {
  int H, W, C, oy, ox;  // oy / ox = dy - pad / dx - pad of the sample
  unsigned rb, frame;   // bytes of a row / of a frame
};

struct ShiftOp {
  using Geom = ShiftGeom;
  const int32_t *dy, *dx;
  int pad, H, W, C;
  unsigned src_frame, out_frame;

  struct Held {
    u32x4 v;
    bool fast = false;
  };

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.H = H, q.W = W, q.C = C, q.rb = (unsigned)W * C, q.frame = (unsigned)H * q.rb;
    // (offsets outside [0, 2 pad] are clamped into it: whatever the block holds, every read stays inside the frame)
    q.oy = min(max(dy[s], 0), 2 * pad) - pad, q.ox = min(max(dx[s], 0), 2 * pad) - pad;
    return q;
  }

  static __device__ __forceinline__ unsigned out_row(const Geom& q) { return q.rb; }  // bytes of an output row (PaintOp)

  // byte e of the group at byte r, read at its clamped source, for e < cnt: (y, x, c) of the first byte are stepped
  template <class Put>
  static __device__ __forceinline__ void walk(const Geom& q, const uint8_t* src, unsigned r, unsigned cnt, Put put) {
    const unsigned y = r / q.rb;
    const int xb = (int)(r - y * q.rb);
    int yy = (int)y, x = xb / q.C, c = xb - x * q.C;
#pragma unroll
    for (unsigned e = 0; e < 16; ++e) {
      if (e < cnt) {
        const int ys = min(max(yy + q.oy, 0), q.H - 1), xs = min(max(x + q.ox, 0), q.W - 1);
        put(e, src[(size_t)ys * q.rb + (unsigned)(xs * q.C + c)]);
        if (++c == q.C) {
          c = 0;
          if (++x == q.W) x = 0, ++yy;
        }
      }
    }
  }

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    const int sx = q.ox * q.C;
    const unsigned y = r / q.rb;
    const int xb = (int)(r - y * q.rb);
    if (xb + 16 <= (int)q.rb && xb + sx >= 0 && xb + sx + 16 <= (int)q.rb) {
      const int ys = min(max((int)y + q.oy, 0), q.H - 1);
      __builtin_memcpy(&h.v, src + (size_t)ys * q.rb + (xb + sx), 16);  // one unaligned global_load_dwordx4
      h.fast = true;
    }
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t* src, unsigned r, const Held& h) {
    if (h.fast) return h.v;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    walk(q, src, r, 16u, [&](unsigned e, uint8_t b) { w[e >> 2] |= (uint32_t)b << (8 * (e & 3)); });
    return u32x4{w[0], w[1], w[2], w[3]};
  }

  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    walk(q, src, r, min(16u, q.frame - r), [&](unsigned e, uint8_t b) { dst[r + e] = b; });
  }
};

// ---- RandomTranslate (beyond the reference: RAD's translate) ----
// out[s][y][x][c] = frames[row(s)][y - ty][x - tx][c] where 0 <= y - ty < H and 0 <= x - tx < W, 0 elsewhere: the H x W
// frame placed at (ty, tx) on a black Ho x Wo canvas; all channels of a stack share the offset (clamped into
// [0, Ho - H] x [0, Wo - W]).  The one byte mover whose output frame is larger than its source frame.  In output order
// the bytes of an output row that lie inside the image are ONE run, bytes [tx C, tx C + W C) of the row, and along such a
// run the source address steps with the output address.  So per output row that a group touches (two at most where rows
// are no shorter than a group) there is at most one run [lo, hi) of the group's bytes, with group byte e = source-frame
// byte base + e: ONE unaligned 16-byte load at base, masked to [lo, hi).  The three kinds of groups are then one code:
//   margin  no run: a store of zeros, nothing is loaded;
//   inside  one run [0, 16): the load is stored as it is;
//   mixed   (crosses the image's left / right edge or straddles two output rows) one or two runs: the loads are masked
//           and OR-ed in registers -- no byte-wise memory access (in the shift the byte loads of such groups set the time,
//           DESIGN.md section 4).
// `base` may lie up to 15 bytes in front of the source frame (the image's first row behind a left margin) or less than 16
// bytes in front of its end: the load address is clamped into [0, frame - 16] and the 16 bytes are shifted by the
// difference, so nothing outside the source frame is read -- ring row 0 has nothing in front of it, and the slack behind
// a ring is not relied on.  Where the canvas is no wider than the frame (Wo == W) the runs of two rows are one run of the
// source and take one load.  Groups that touch three or more rows (rows shorter than a group) walk their rows in a loop
// with the same run arithmetic.  Source frames shorter than a group go byte by byte as well (vec_extra).
struct TrGeom {
  int H, ty, txb;           // image rows [ty, ty + H) of the canvas, image columns in bytes of an output row from txb on
  int srb, orb;             // bytes of a source row / of an output row
  unsigned sframe, oframe;  // bytes of a source frame / of an output frame
  bool flat;                // no margin left or right: the image rows follow one another in the output too
};

// The run of output row yy inside a group: `rel` = the group byte at which row yy starts (negative: the row started in
// front of the group).  Group bytes [lo, hi) are the row's bytes inside the image, group byte e is source-frame byte
// base + e.  False: row yy has no image byte in the group.
__device__ __forceinline__ bool tr_run(const TrGeom& q, int yy, int rel, int& lo, int& hi, int& base) {
  lo = max(rel + q.txb, 0), hi = min(rel + q.txb + q.srb, 16);
  base = (yy - q.ty) * q.srb - rel - q.txb;
  return yy >= q.ty && yy < q.ty + q.H && lo < hi;
}

// The 16-byte load of a run, at its address clamped into the source frame; returns lo | hi << 8 | (d + 16) << 16 (never
// 0: hi >= 1), d = the bytes the load sits in front of (d > 0) or behind (d < 0) `base`.  Every byte of [lo, hi) is in
// the load: base + e is a byte of the frame, and the clamp moves the address only as far as the frame's ends.
__device__ __forceinline__ int u8_run_load(const uint8_t* src, int sframe, int lo, int hi, int base, u32x4& v) {
  const int a = min(max(base, 0), sframe - 16);
  __builtin_memcpy(&v, src + a, 16);  // one unaligned global_load_dwordx4
  return lo | (hi << 8) | ((base - a + 16) << 16);
}

__device__ __forceinline__ int tr_load(const uint8_t* src, const TrGeom& q, int lo, int hi, int base, u32x4& v) {
  return u8_run_load(src, (int)q.sframe, lo, hi, base, v);
}

// the loaded bytes moved to their places in the group (only the runs at the two ends of a frame are shifted), all
// others zero
__device__ __forceinline__ u128 tr_place(u32x4 v, int meta) {
  const int lo = meta & 0xff, hi = (meta >> 8) & 0xff, d = (meta >> 16) - 16;
  u128 x = __builtin_bit_cast(u128, v);
  if (d > 0) x >>= 8 * d;
  if (d < 0) x <<= -8 * d;
  if (hi - lo < 16) x &= (~(u128)0 >> (8 * (16 - (hi - lo)))) << (8 * lo);
  return x;
}

// a group that touches three or more output rows (rows shorter than a group): its rows one by one
__device__ __forceinline__ u128 tr_group_rows(const uint8_t* src, const TrGeom& q, unsigned r) {
  const unsigned y = r / (unsigned)q.orb;
  u128 o = 0;
  int yy = (int)y;
  for (int rel = (int)(y * (unsigned)q.orb) - (int)r; rel < 16; rel += q.orb, ++yy) {
    int lo, hi, base;
    if (tr_run(q, yy, rel, lo, hi, base)) {
      u32x4 v;
      const int meta = tr_load(src, q, lo, hi, base, v);
      o |= tr_place(v, meta);
    }
  }
  return o;
}

struct TrOp {
  using Geom = TrGeom;
  const int32_t *ty, *tx;
  int H, W, C, Ho, Wo;
  unsigned src_frame, out_frame;

  struct Held {
    u32x4 v[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    int meta[2] = {0, 0};  // of the runs of the group's first and second row; 0: no run
    bool rows3 = false;    // the group touches three or more rows
  };

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.H = H, q.srb = W * C, q.orb = Wo * C, q.sframe = src_frame, q.oframe = out_frame;
    q.flat = q.srb == q.orb;
    // (offsets outside their ranges are clamped into them: whatever the block holds, the image lies on the canvas)
    q.ty = min(max(ty[s], 0), Ho - H), q.txb = min(max(tx[s], 0), Wo - W) * C;
    return q;
  }

  static __device__ __forceinline__ unsigned out_row(const Geom& q) { return (unsigned)q.orb; }  // (PaintOp)

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    const unsigned y = r / (unsigned)q.orb;
    const int xb = (int)(r - y * (unsigned)q.orb);
    if (xb + 15 >= 2 * q.orb) {
      h.rows3 = true;
    } else {
      int lo0, hi0, b0, lo1, hi1, b1;
      const bool r0 = tr_run(q, (int)y, -xb, lo0, hi0, b0);
      bool r1 = tr_run(q, (int)y + 1, q.orb - xb, lo1, hi1, b1);  // (a group inside one row: lo1 >= 16, no run)
      if (q.flat && r0 && r1) hi0 = hi1, r1 = false;           // b1 == b0, lo1 == hi0: one run of the source
      if (r0) h.meta[0] = tr_load(src, q, lo0, hi0, b0, h.v[0]);
      if (r1) h.meta[1] = tr_load(src, q, lo1, hi1, b1, h.v[1]);
    }
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t* src, unsigned r, const Held& h) {
    u128 o = 0;
    if (h.rows3) {
      o = tr_group_rows(src, q, r);
    } else {
      if (h.meta[0]) o = tr_place(h.v[0], h.meta[0]);
      if (h.meta[1]) o |= tr_place(h.v[1], h.meta[1]);
    }
    return __builtin_bit_cast(u32x4, o);
  }

  // (row, byte in row) are stepped, not divided
  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    const unsigned cnt = min(16u, q.oframe - r);
    const unsigned y = r / (unsigned)q.orb;
    int yy = (int)y, xb = (int)(r - y * (unsigned)q.orb);
    for (unsigned e = 0; e < cnt; ++e) {
      const bool in = yy >= q.ty && yy < q.ty + q.H && xb >= q.txb && xb < q.txb + q.srb;
      dst[r + e] = in ? src[(size_t)(yy - q.ty) * q.srb + (unsigned)(xb - q.txb)] : (uint8_t)0;
      if (++xb == q.orb) xb = 0, ++yy;
    }
  }
};

// ---- the crop as a mover (Compose: RandomCrop + RandomCutout, curla_move_cutout_u8) ----
// out[s][y][x][c] = frames[row(s)][y + h1][x + w1][c]: the Ho x Wo window at (h1, w1) of the H x W frame, all channels of a
// stack sharing the offset (clamped into [0, H - Ho] x [0, W - Wo]).  The one byte mover whose output frame is SMALLER than
// its source frame.  Every output byte has a source byte, and along an output row the source address steps with the output
// address: per output row that a group touches there is one run [lo, hi) of the group's bytes with group byte e =
// source-frame byte base + e -- the translate's runs without margins.  A group inside one output row is ONE unaligned
// 16-byte load; a group that straddles two rows is two loads, masked and OR-ed in registers (tr_place): no byte-wise
// memory access.  Where the window is as wide as the frame (Wo == W) the two runs are one run of the
// source.  A load whose 16 bytes would end behind the source frame (the window's last row in the frame's last row) is
// moved back into the frame and shifted, as tr_load does: nothing in the slack behind a ring is read; no base lies in
// front of the frame.  Groups that touch three or more rows (rows shorter than a group) walk their rows in a loop.
struct CropGeom {
  int Ho, srb, orb;         // output rows; bytes of a source row / of an output row
  unsigned base0;           // source-frame byte of the window's first byte: h1 srb + w1 C
  unsigned sframe, oframe;  // bytes of a source frame / of an output frame
  bool flat;                // the window is as wide as the frame: its rows follow one another in the source too
};

// The run of output row yy inside a group, `rel` as for tr_run: group bytes [lo, hi) are the row's, group byte e is
// source-frame byte base + e (base >= 0: rel <= lo).  False: the group has no byte of row yy, or the frame no such row.
__device__ __forceinline__ bool crop_run(const CropGeom& q, int yy, int rel, int& lo, int& hi, int& base) {
  lo = max(rel, 0), hi = min(rel + q.orb, 16);
  base = (int)q.base0 + yy * q.srb - rel;
  return yy < q.Ho && lo < hi;
}

struct CropOp {
  using Geom = CropGeom;
  const int32_t *h1, *w1;
  int H, W, C, Ho, Wo;
  unsigned src_frame, out_frame;

  using Held = TrOp::Held;  // the runs of the group's first and second row, or rows3

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.Ho = Ho, q.srb = W * C, q.orb = Wo * C, q.sframe = src_frame, q.oframe = out_frame;
    q.flat = q.srb == q.orb;
    // (offsets outside their ranges are clamped into them: whatever the block holds, the window lies inside the frame)
    q.base0 = (unsigned)(min(max(h1[s], 0), H - Ho) * q.srb + min(max(w1[s], 0), W - Wo) * C);
    return q;
  }

  static __device__ __forceinline__ unsigned out_row(const Geom& q) { return (unsigned)q.orb; }  // (PaintOp)

  static __device__ __forceinline__ int run_load(const uint8_t* src, const Geom& q, int lo, int hi, int base, u32x4& v) {
    return u8_run_load(src, (int)q.sframe, lo, hi, base, v);
  }

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    const unsigned y = r / (unsigned)q.orb;
    const int xb = (int)(r - y * (unsigned)q.orb);
    if (xb + 15 >= 2 * q.orb) {
      h.rows3 = true;
    } else {
      int lo0, hi0, b0, lo1, hi1, b1;
      const bool r0 = crop_run(q, (int)y, -xb, lo0, hi0, b0);  // (always a run: the group's first byte is row y's)
      bool r1 = crop_run(q, (int)y + 1, q.orb - xb, lo1, hi1, b1);  // (a group inside one row: lo1 >= 16, no run)
      if (q.flat && r1) hi0 = hi1, r1 = false;                      // b1 == b0, lo1 == hi0: one run of the source
      if (r0) h.meta[0] = run_load(src, q, lo0, hi0, b0, h.v[0]);
      if (r1) h.meta[1] = run_load(src, q, lo1, hi1, b1, h.v[1]);
    }
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t* src, unsigned r, const Held& h) {
    u128 o = 0;
    if (h.rows3) {  // rows shorter than a group: its rows one by one
      const unsigned y = r / (unsigned)q.orb;
      int yy = (int)y;
      for (int rel = (int)(y * (unsigned)q.orb) - (int)r; rel < 16; rel += q.orb, ++yy) {
        int lo, hi, base;
        if (crop_run(q, yy, rel, lo, hi, base)) {
          u32x4 v;
          const int meta = run_load(src, q, lo, hi, base, v);
          o |= tr_place(v, meta);
        }
      }
    } else {
      if (h.meta[0]) o = tr_place(h.v[0], h.meta[0]);
      if (h.meta[1]) o |= tr_place(h.v[1], h.meta[1]);
    }
    return __builtin_bit_cast(u32x4, o);
  }

  // (row, byte in row) are stepped, not divided
  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    const unsigned cnt = min(16u, q.oframe - r);
    const unsigned y = r / (unsigned)q.orb;
    unsigned xb = r - y * (unsigned)q.orb, at = q.base0 + y * (unsigned)q.srb;  // source byte of row y's first byte
    for (unsigned e = 0; e < cnt; ++e) {
      dst[r + e] = src[at + xb];
      if (++xb == (unsigned)q.orb) xb = 0, at += (unsigned)q.srb;
    }
  }
};

// ---- RandomFlip / RandomRotate (beyond the reference: RAD's flip and rotate): the eight maps of the dihedral group ----
// A word per sample carries three bits, FX = 1, FY = 2, T = 4; with (a, b) = (x, y) if T is set, else (y, x):
//   out[s][y][x][c] = frames[row(s)][FY ? H - 1 - a : a][FX ? W - 1 - b : b][c]
// (1: mirrored left-right; 3: turned by 180 degrees; 5 / 6: turned by 90 / 270 degrees counter-clockwise, on square frames
// only).  The effective code is word & 7, and & 3 where H != W: whatever the block holds, every source pixel lies inside
// the frame.  Neither map is a translation: under FX the pixels of a row come in reversed order, under T neighbouring
// output pixels come from different source rows.
//
// Codes 0..3 (FlipOp) run on the mover skeleton.  What steps with the output address is a RUN: the C bytes of one pixel
// under FX (output pixel x of a row is source pixel W - 1 - x, its channels in order), the rest of the output row
// otherwise (FY only picks the source row).  Group byte e of a run is source-frame byte base + e, so a run is the
// translate's: ONE unaligned 16-byte load at base, its address clamped into the frame (u8_run_load), masked to the run's
// bytes [lo, hi) and OR-ed into the group in registers (tr_place) -- no byte-wise memory access, no permutation network.
// Under FX a group has floor(15 / C) + 2 runs at most (three for C >= 8: stacks of three and four RGB frames), whose
// loads overlap inside a span of 16 + 2 (C - 1) bytes and are served by the same lines of the vector L1.  The first
// FLIP_HELD runs of a group are loaded before the first store of the trip, like every mover's loads; the runs beyond
// them (narrow pixels, C < 8; rows shorter than a group) are loaded when the group is finished.  A group that straddles
// two rows needs nothing of its own: the walk steps from the last pixel of a row to the first of the next.
constexpr int FLIP_HELD = 3;

struct FlipGeom {
  int H, W, C, code;   // code: the effective one
  unsigned rb, frame;  // bytes of a row / of a frame
};

// the runs of the group at output byte r, one after the other: (y, byte in row) -- and (x, c) under FX -- are stepped
struct FlipWalk {
  unsigned y, xb, x, c;
  int e;  // the group byte at which the next run starts

  __device__ __forceinline__ FlipWalk(const FlipGeom& q, unsigned r) : y(r / q.rb), x(0), c(0), e(0) {
    xb = r - y * q.rb;
    if (q.code & 1) x = xb / (unsigned)q.C, c = xb - x * (unsigned)q.C;
  }

  // the next run: group bytes [lo, hi), group byte e = source-frame byte base + e
  __device__ __forceinline__ void next(const FlipGeom& q, int& lo, int& hi, int& base) {
    const unsigned ys = (q.code & 2) ? (unsigned)q.H - 1 - y : y;
    lo = e;
    if (q.code & 1) {
      hi = min(e + (q.C - (int)c), 16);
      base = (int)(ys * q.rb + ((unsigned)q.W - 1 - x) * (unsigned)q.C + c) - e;
      c = 0;
      if (++x == (unsigned)q.W) x = 0, ++y;
    } else {
      hi = (int)min((unsigned)e + (q.rb - xb), 16u);
      base = (int)(ys * q.rb + xb) - e;
      xb = 0, ++y;
    }
    e = hi;
  }
};

struct FlipOp {
  using Geom = FlipGeom;
  const int32_t* code;
  int H, W, C;
  unsigned src_frame, out_frame;

  struct Held {
    u32x4 v[FLIP_HELD];
    int meta[FLIP_HELD];  // of the group's first runs (u8_run_load); 0: no such run
    bool more = false;    // the group has further runs
  };

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.H = H, q.W = W, q.C = C, q.rb = (unsigned)W * C, q.frame = out_frame;
    q.code = code[s] & (H == W ? 7 : 3);  // (a frame that is not square cannot be transposed in place)
    return q;
  }

  static __device__ __forceinline__ unsigned out_row(const Geom& q) { return q.rb; }

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    FlipWalk w(q, r);
#pragma unroll
    for (int k = 0; k < FLIP_HELD; ++k) {
      h.meta[k] = 0;
      if (w.e < 16) {
        int lo, hi, base;
        w.next(q, lo, hi, base);
        h.meta[k] = u8_run_load(src, (int)q.frame, lo, hi, base, h.v[k]);
      }
    }
    h.more = w.e < 16;
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t* src, unsigned r, const Held& h) {
    u128 o = 0;
#pragma unroll
    for (int k = 0; k < FLIP_HELD; ++k)
      if (h.meta[k]) o |= tr_place(h.v[k], h.meta[k]);
    if (h.more) {  // the runs behind the held ones
      FlipWalk w(q, r);
      int lo, hi, base;
#pragma unroll
      for (int k = 0; k < FLIP_HELD; ++k) w.next(q, lo, hi, base);
      while (w.e < 16) {
        w.next(q, lo, hi, base);
        u32x4 v;
        const int meta = u8_run_load(src, (int)q.frame, lo, hi, base, v);
        o |= tr_place(v, meta);
      }
    }
    return __builtin_bit_cast(u32x4, o);
  }

  // (row, pixel, channel) are stepped, not divided
  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    const unsigned cnt = min(16u, q.frame - r);
    unsigned y = r / q.rb;
    const unsigned xb = r - y * q.rb;
    unsigned x = xb / (unsigned)q.C, c = xb - x * (unsigned)q.C;
    for (unsigned e = 0; e < cnt; ++e) {
      const unsigned ys = (q.code & 2) ? (unsigned)q.H - 1 - y : y, xs = (q.code & 1) ? (unsigned)q.W - 1 - x : x;
      dst[r + e] = src[ys * q.rb + xs * (unsigned)q.C + c];
      if (++c == (unsigned)q.C) {
        c = 0;
        if (++x == (unsigned)q.W) x = 0, ++y;
      }
    }
  }
};

// Codes 4..7 transpose (H == W = N): output row y is source COLUMN j = FX ? N - 1 - y : y, read downwards or (FY) upwards,
// so neighbouring output pixels lie a whole source row apart and no load of consecutive bytes serves a group.  A
// workgroup therefore takes a BAND of DH_BAND consecutive groups of the output (what it takes per trip as a mover), which
// lies in R output rows, i.e. needs R neighbouring source columns: from each of the N source rows one segment of R C
// bytes.  The segments are staged in LDS with 16-byte loads (row i at i * lds_stride; the one chunk that would end
// behind the frame goes byte by byte, so nothing outside the frame is read), and the band's groups are then put together
// from LDS bytes and stored whole.  R <= floor((16 DH_BAND - 1) / (N C)) + 2, so the image is about 16 DH_BAND + 2 N C
// bytes (18 KiB at 84 x 84 x 9) whatever the frame's size -- an 136 x 136 x 9 frame, larger than the LDS, takes the same
// path.  Only where N segments do not fit 64 KiB (thousands of rows, or pixels of hundreds of bytes) lds_stride is 0 and
// the bytes are gathered from global memory directly.  The sample, hence the code, is uniform over a workgroup: the
// branch between the mover and the transposing form is taken by whole workgroups, and so are the barriers.
constexpr unsigned DH_BAND = 256 * U8_UNROLL;

__global__ __launch_bounds__(256) void dihedral_u8_kernel(const uint8_t* frames, const int64_t* idx, int period, int n,
                                                            unsigned groups, bool vec, const FlipOp op,
                                                            unsigned lds_stride, uint8_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dh_tile[];
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    const int p = s % period;
    const int64_t row = idx ? idx[p] : (int64_t)p;
    const FlipGeom q = op.sample(s);
    const uint8_t* src = frames + (size_t)row * op.src_frame;
    uint8_t* dst = out + (size_t)s * op.out_frame;
    if (!(q.code & 4)) {
      u8_mover_sample<FlipOp>(q, src, dst, groups, vec);
      continue;
    }
    const unsigned N = (unsigned)q.H, C = (unsigned)q.C;
    const bool fx = q.code & 1, fy = q.code & 2;
    for (unsigned g_lo = blockIdx.x * DH_BAND; g_lo < groups; g_lo += gridDim.x * DH_BAND) {
      const unsigned g_hi = min(g_lo + DH_BAND, groups);
      const unsigned y_lo = 16 * g_lo / q.rb, y_hi = (min(16 * g_hi, q.frame) - 1) / q.rb;  // the band's output rows
      const unsigned j0 = fx ? N - 1 - y_hi : y_lo;                                          // its first source column
      if (lds_stride) {
        const unsigned seg = (y_hi - y_lo + 1) * C, nc = (seg + 15) / 16;  // bytes / 16-byte chunks of a segment
        for (unsigned ch = threadIdx.x; ch < N * nc; ch += 256) {
          const unsigned i = ch / nc, m = ch - i * nc;
          const unsigned a = i * q.rb + j0 * C + 16 * m, at = i * lds_stride + 16 * m;
          if (a + 16 <= q.frame) {
            u32x4 v;
            __builtin_memcpy(&v, src + a, 16);  // one unaligned global_load_dwordx4
            *reinterpret_cast<u32x4*>(dh_tile + at) = v;
          } else {
            for (unsigned b = 0; a + b < q.frame; ++b) dh_tile[at + b] = src[a + b];
          }
        }
        __syncthreads();
      }
      for (unsigned g = g_lo + threadIdx.x; g < g_hi; g += 256) {
        const unsigned r = 16 * g, cnt = min(16u, q.frame - r);
        unsigned y = r / q.rb;
        const unsigned xb = r - y * q.rb;
        unsigned x = xb / C, c = xb - x * C;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (unsigned e = 0; e < 16; ++e) {
          if (e < cnt) {
            const unsigned i = fy ? N - 1 - x : x, j = fx ? N - 1 - y : y;  // the source pixel (row i, column j)
            const uint32_t b = lds_stride ? dh_tile[i * lds_stride + (j - j0) * C + c] : src[i * q.rb + j * C + c];
            w[e >> 2] |= b << (8 * (e & 3));
            if (++c == C) {
              c = 0;
              if (++x == N) x = 0, ++y;
            }
          }
        }
        if (vec) {
          *reinterpret_cast<u32x4*>(dst + r) = u32x4{w[0], w[1], w[2], w[3]};
        } else {
#pragma unroll
          for (unsigned e = 0; e < 16; ++e)
            if (e < cnt) dst[r + e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
        }
      }
      if (lds_stride) __syncthreads();  // (the next band's segments go where these are still being read)
    }
  }
}

// as launch_u8_mover, with the LDS image of the transposing form where the frame is square
inline int launch_dihedral_u8(const FlipOp& op, const uint8_t* frames, const int64_t* idx, int period, int n,
                              long long frame, uint8_t* out, void* stream) {
  if (frame >= (1LL << 31) - 16) return CURLA_ERR_UNSUPPORTED;
  const bool vec = frame % 16 == 0 && aligned16(out);  // (a frame of whole groups holds the 16 bytes of a run's load)
  const unsigned groups = (unsigned)((frame + 15) / 16);
  const unsigned per_block = vec ? 256 * U8_UNROLL : 256;
  const unsigned gx = (groups + per_block - 1) / per_block;
  const dim3 grid(gx < 64 ? gx : 64, n < 65535 ? n : 65535);
  unsigned lds_stride = 0;
  if (op.H == op.W) {
    const long long rb = (long long)op.W * op.C;
    long long rows = (16LL * DH_BAND - 1) / rb + 2;  // output rows a band can touch
    if (rows > op.H) rows = op.H;
    const long long stride = (rows * op.C + 15) / 16 * 16;
    if (stride * op.H <= 64 * 1024) lds_stride = (unsigned)stride;
  }
  hipLaunchKernelGGL(dihedral_u8_kernel, grid, dim3(256), (size_t)lds_stride * op.H, static_cast<hipStream_t>(stream),
                     frames, idx, period, n, groups, vec, op, lds_stride, out);
  return curla_launch_status();
}

// ---- RandomGrayscale (beyond the reference: RAD's grayscale) ----
// out[s] = frames[row(s)] with every RGB triplet (R, G, B) replaced by (g, g, g), g = (77 R + 150 G + 29 B + 128) >> 8,
// where grey[s] != 0; a plain copy where it is 0.  (The weights sum to 256: a grey pixel stays what it is.)  C % 3 == 0, so
// the channel of frame byte r is r % 3 and the triplets tile the frame: no row or pixel arithmetic.  The first Op that
// CHANGES bytes from a neighbourhood off the 16-byte grid: the group at r needs bytes [r - r % 3, ceil((r + 16) / 3) 3),
// two bytes more on either side at most.  They are the group's own 16 bytes plus the dword in front of it and the dword
// behind it, each loaded only where it lies inside the frame (the first group needs none in front, r = 0 starts a
// triplet; the last none behind, the frame ends with one); the six triplets that touch the group are mixed in registers,
// with every byte position a constant of the group's phase r % 3 (grey_mix<K>).
struct GreyGeom {
  unsigned frame;
  bool grey;
};

__device__ __forceinline__ uint32_t grey_of(uint32_t R, uint32_t G, uint32_t B) {
  return (77u * R + 150u * G + 29u * B + 128u) >> 8;
}

// w = the 24 bytes from 4 in front of the group; K = r % 3, so triplet t starts at byte 4 - K + 3 t of w
template <int K>
__device__ __forceinline__ u32x4 grey_mix(const uint32_t (&w)[6]) {
  uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int b0 = 4 - K + 3 * t;
    uint32_t px[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) px[j] = (w[(b0 + j) >> 2] >> (8 * ((b0 + j) & 3))) & 0xffu;
    const uint32_t g = grey_of(px[0], px[1], px[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int e = b0 + j - 4;
      if (e >= 0 && e < 16) o[e >> 2] |= g << (8 * (e & 3));
    }
  }
  return u32x4{o[0], o[1], o[2], o[3]};
}

struct GreyOp {
  using Geom = GreyGeom;
  const int32_t* grey;
  unsigned src_frame, out_frame;

  struct Held {
    u32x4 v;
    uint32_t lo = 0u, hi = 0u;  // the dwords in front of and behind the group (greyed samples)
  };

  __device__ __forceinline__ Geom sample(int s) const {
    Geom q;
    q.frame = out_frame, q.grey = grey[s] != 0;
    return q;
  }

  static __device__ __forceinline__ void load(const Geom& q, const uint8_t* src, unsigned r, Held& h) {
    __builtin_memcpy(&h.v, src + r, 16);  // inside the frame: frame % 16 == 0
    if (q.grey) {
      if (r) __builtin_memcpy(&h.lo, src + r - 4, 4);
      if (r + 16 < q.frame) __builtin_memcpy(&h.hi, src + r + 16, 4);
    }
  }

  static __device__ __forceinline__ u32x4 finish(const Geom& q, const uint8_t*, unsigned r, const Held& h) {
    if (!q.grey) return h.v;
    const uint32_t w[6] = {h.lo, h.v.x, h.v.y, h.v.z, h.v.w, h.hi};
    const unsigned k = r % 3;
    return k == 0 ? grey_mix<0>(w) : k == 1 ? grey_mix<1>(w) : grey_mix<2>(w);
  }

  static __device__ __forceinline__ void group_bytes(const Geom& q, const uint8_t* src, uint8_t* dst, unsigned r) {
    const unsigned cnt = min(16u, q.frame - r);
    unsigned k = r % 3;  // the channel of byte r + e, stepped
    for (unsigned e = 0; e < cnt; ++e) {
      const unsigned at = r + e;
      dst[at] = q.grey ? (uint8_t)grey_of(src[at - k], src[at - k + 1], src[at - k + 2]) : src[at];
      if (++k == 3) k = 0;
    }
  }
};

}  // namespace
