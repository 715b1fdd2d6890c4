// curla_stage_frames_u8: the front of the batched acting path (CurlSacAgent.select_actions / sample_actions).
// Included by heads.hip inside its anonymous namespace, behind ring.h and per.h; the launches are in heads.hip
// (curla_stage_frames_u8).
//
// N planar uint8 observations [N][C][Hs][Ws] (what a vector of environments hands over) go into N consecutive NHWC
// slots, out[n][y][x][c] = nchw[n][c][top + y][left + x]: the CHW -> HWC transpose of ReplayBuffer.add for N frames
// per launch, with the centre crop of RandomCrop.evaluation_augmentation fused, so only the window the encoder reads
// is written.
//
// Form.  The N * Hd * Wd output pixels are numbered straight through and one thread moves 4 consecutive ones.  Their
// 4 * C bytes are C dwords at a dword-aligned offset whatever Wd is (the slots are contiguous), as in
// gather_stacks_kernel<FAST>.  Per plane the 4 pixels are 4 consecutive source bytes: the two aligned dwords around
// them, shifted.  Neighbouring threads read neighbouring dwords of a plane row, so every plane row is read once and
// coalesced at any `left` / Ws; the transpose happens in registers.  A group that straddles a row end reads its pixels
// one by one, and a last group of fewer than 4 pixels is written bytewise.  Nothing outside [0, src_bytes) is read and
// nothing outside the N slots is written.
#pragma once

// bytes at .. at+3 of `base` (a dword-aligned pointer, `at` a multiple of 4) as one little-endian word; bytes at or
// past nbytes read as 0
__device__ __forceinline__ uint32_t stage_word(const uint8_t* base, size_t at, size_t nbytes) {
  if (at + 4 <= nbytes) return *reinterpret_cast<const uint32_t*>(base + at);
  uint32_t v = 0;
  for (int b = 0; b < 4; ++b)
    if (at + b < nbytes) v |= (uint32_t)base[at + b] << (8 * b);
  return v;
}

// the same at any byte offset
__device__ __forceinline__ uint32_t stage_load_u8x4(const uint8_t* base, size_t off, size_t nbytes) {
  const size_t a = off & ~(size_t)3;
  const int s = (int)(off & 3);
  const uint32_t lo = stage_word(base, a, nbytes);
  if (s == 0) return lo;
  const uint32_t hi = stage_word(base, a + 4, nbytes);
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
}

// One group: the np (1..4) output pixels p0 .. p0 + np - 1 of the straight-through numbering, read from the planar frames
// and written as np * C bytes at `o8` (np == 4: C dwords, `o8` on a dword).  Shared by stage_frames_kernel and
// add_vec_kernel (add_vec.h), which differ only in where a group's bytes go.
template <int C>
__device__ __forceinline__ void stage_group(const uint8_t* nchw, size_t src_bytes, uint8_t* o8, uint32_t p0, int np, int Hs,
                                            int Ws, int top, int left, int Hd, int Wd) {
  const uint32_t HWd = (uint32_t)Hd * Wd;
  const size_t plane = (size_t)Hs * Ws;
  const uint32_t n = p0 / HWd, r = p0 - n * HWd;
  const uint32_t y = r / Wd, x = r - y * Wd;
  uint32_t ob[C];
#pragma unroll
  for (int w = 0; w < C; ++w) ob[w] = 0;
  if (np == 4 && x + 4 <= (uint32_t)Wd) {  // the 4 pixels sit side by side in one source row
    const size_t o = (size_t)n * C * plane + (size_t)(top + y) * Ws + left + x;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const uint32_t s = stage_load_u8x4(nchw, o + c * plane, src_bytes);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int db = p * C + c;  // byte of the 4 * C output bytes
        ob[db >> 2] |= ((s >> (8 * p)) & 0xffu) << (8 * (db & 3));
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p < np) {
        const uint32_t q = p0 + p;
        const uint32_t qn = q / HWd, qr = q - qn * HWd;
        const uint32_t qy = qr / Wd, qx = qr - qy * Wd;
        const size_t o = (size_t)qn * C * plane + (size_t)(top + qy) * Ws + left + qx;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int db = p * C + c;
          ob[db >> 2] |= (uint32_t)nchw[o + c * plane] << (8 * (db & 3));
        }
      }
    }
  }
  if (np == 4) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o8);
#pragma unroll
    for (int w = 0; w < C; ++w) o4[w] = ob[w];  // 4 pixels x C bytes = C dwords
  } else {
#pragma unroll
    for (int b = 0; b < 3 * C; ++b)
      if (b < np * C) o8[b] = (uint8_t)(ob[b >> 2] >> (8 * (b & 3)));
  }
}

template <int C>
__global__ void stage_frames_kernel(const uint8_t* nchw, size_t src_bytes, uint8_t* out, uint32_t npix, int Hs, int Ws,
                                    int top, int left, int Hd, int Wd) {
  const uint32_t groups = (npix + 3) >> 2;
  uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (; g < groups; g += stride) {
    const uint32_t p0 = 4 * g;
    stage_group<C>(nchw, src_bytes, out + (size_t)p0 * C, p0, (int)min(4u, npix - p0), Hs, Ws, top, left, Hd, Wd);
  }
}

// Output byte i of the straight-through NHWC numbering, from the planar frames: the byte-wise form of stage_group.
__device__ __forceinline__ uint8_t stage_byte(const uint8_t* nchw, size_t i, int C, int Hs, int Ws, int top, int left,
                                              int Hd, int Wd) {
  const size_t plane = (size_t)Hs * Ws;
  const int c = i % C;
  size_t t = i / C;
  const int x = t % Wd;
  t /= Wd;
  const int y = t % Hd;
  const size_t n = t / Hd;
  return nchw[(n * C + c) * plane + (size_t)(top + y) * Ws + left + x];
}

// the same bytes one at a time: any channel count, any pointer alignment
__global__ void stage_frames_bytes_kernel(const uint8_t* nchw, uint8_t* out, size_t nout, int C, int Hs, int Ws, int top,
                                          int left, int Hd, int Wd) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < nout; i += stride) out[i] = stage_byte(nchw, i, C, Hs, Ws, top, left, Hd, Wd);
}
