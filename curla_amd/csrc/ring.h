// The replay ring's frame movers: the crop materialiser for callers that want the reference's float NCHW minibatch
// tensors (crop_nchw_kernel), the frame store of ReplayBuffer.add (store_frame_kernel), the stack gather of the
// de-duplicated storage (gather_stacks_kernel<FAST>) and the NHWC -> NCHW copy of an activation
// (nhwc_to_nchw_kernel).  Included by heads.hip inside its anonymous namespace.
#pragma once

// out[b][c][i][j] = (float) frames[idx[b]][h1[b]+i][w1[b]+j][c]          (augmentations.py:47-75 + utils.py:161)
__global__ void crop_nchw_kernel(const uint8_t* frames, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                                 int B, int C, int Hs, int Ws, int Hc, int Wc, float* out_f32, uint8_t* out_u8) {
  const size_t n = (size_t)B * C * Hc * Wc;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int x = i % Wc;
    size_t t = i / Wc;
    const int y = t % Hc;
    t /= Hc;
    const int c = t % C;
    const int b = t / C;
    const int64_t fi = idx ? idx[b] : b;
    const int oh = h1 ? h1[b] : 0, ow = w1 ? w1[b] : 0;
    const uint8_t v = frames[(((size_t)fi * Hs + oh + y) * Ws + ow + x) * C + c];
    if (out_f32) out_f32[i] = (float)v;
    if (out_u8) out_u8[i] = v;
  }
}

// frames[slot][y][x][c] = chw[c][y][x]   (replay add: the reference stores CHW, utils.py:120-128)
__global__ void store_frame_kernel(const uint8_t* chw, uint8_t* frames, int64_t slot, int C, int H, int W) {
  const int n = C * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = i % C, p = i / C;
    frames[(size_t)slot * n + i] = chw[(size_t)c * H * W + p];
  }
}

// De-duplicated replay storage: every RGB frame is stored once ([F][H][W][3] uint8) and a transition keeps the k frame
// ids of its observation stack.  out[b][y][x][3f+c] = store[fid[idx[b]][f]][y][x][c] rebuilds the [B][H][W][3k] stacks
// of a minibatch (the layout the first conv's loader reads).  One thread moves 4 pixels: 3 aligned dwords from each
// of the k frames, 3k aligned dwords out (FAST); any other geometry goes byte by byte.
template <bool FAST>
__global__ void gather_stacks_kernel(const uint8_t* store, const int32_t* fid, int fid_stride, const int64_t* idx, int B,
                                     int K, int HW, uint8_t* out) {
  const int groups = (HW + 3) >> 2;
  const size_t n = (size_t)B * groups;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int C = 3 * K;
  for (; i < n; i += stride) {
    const int b = i / groups, g = i - (size_t)b * groups;
    const int32_t* ids = fid + (size_t)(idx ? idx[b] : b) * fid_stride;
    uint8_t* o = out + ((size_t)b * HW + 4 * (size_t)g) * C;
    if (FAST) {
      uint32_t ob[12];  // up to k = 4 frames: 4 pixels x 12 bytes
#pragma unroll
      for (int w = 0; w < 12; ++w) ob[w] = 0;
      for (int f = 0; f < K; ++f) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(store + ((size_t)ids[f] * HW + 4 * (size_t)g) * 3);
        const uint32_t s0 = src[0], s1 = src[1], s2 = src[2];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int sb = 3 * p + c;  // byte of the 12 source bytes
            const uint32_t v = ((sb < 4 ? s0 : sb < 8 ? s1 : s2) >> (8 * (sb & 3))) & 0xffu;
            const int db = p * C + 3 * f + c;  // byte of the 4*C output bytes
            ob[db >> 2] |= v << (8 * (db & 3));
          }
      }
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      for (int w = 0; w < C; ++w) o4[w] = ob[w];  // 4 pixels x C bytes = C dwords
    } else {
      const int np = min(4, HW - 4 * g);
      for (int f = 0; f < K; ++f) {
        const uint8_t* src = store + ((size_t)ids[f] * HW + 4 * (size_t)g) * 3;
        for (int p = 0; p < np; ++p)
          for (int c = 0; c < 3; ++c) o[p * C + 3 * f + c] = src[3 * p + c];
      }
    }
  }
}

// NHWC float activation -> NCHW (for callers that read encoder.outputs)
__global__ void nhwc_to_nchw_kernel(const float* in, float* out, int B, int H, int W, int C) {
  const size_t n = (size_t)B * H * W * C;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int x = i % W;
    size_t t = i / W;
    const int y = t % H;
    t /= H;
    const int c = t % C;
    const int b = t / C;
    out[i] = in[(((size_t)b * H + y) * W + x) * C + c];
  }
}
