// curla_add_vec: one vector step of N environments into the replay ring in ONE launch (ReplayBuffer.add_vec).  Included by
// heads.hip inside its anonymous namespace, behind stage.h, whose per-group transpose it shares; the launch is in
// heads.hip (curla_add_vec).
//
// The staged block (device copy of the pinned add block):
//   [N obs frames | N next_obs frames] planar uint8 [2N][C][H][W] | pad to 16 | N x (A + 2) float32 | 2N flag bytes
// goes to ring rows first .. first + N - 1 (first a multiple of N, so the run never straddles the ring's end):
//   frames   obs[first + e][y][x][c] = block frame e, next_obs[first + e] = block frame N + e -- the CHW -> HWC transpose of
//            stage_frames_kernel<C> (4 pixels per thread, C dwords out, coalesced plane reads) when a frame is a whole
//            number of 4-pixel groups, byte by byte otherwise (ADD_VEC_BYTES)
//   scalars  the N rows action | reward | not_done, contiguous on both sides
//   flags    cont[prev + e] = flag byte e (the previous vector step's run, prev = first - N modulo capacity; skipped when
//            there is none), cont[first + e] = flag byte N + e
// Work items are numbered straight through -- frame groups (or bytes), then scalars, then flags -- and a thread takes
// every (gridDim.x * blockDim.x)-th one.  Every store is a plain vector store; nothing outside the rows above is written.
#pragma once

constexpr int ADD_VEC_BYTES = 0;  // add_vec_kernel<ADD_VEC_BYTES>: any channel count, any frame size

struct AddVecArgs {
  const uint8_t* block;
  uint8_t *obs, *next;  // row 0 of the obs ring and of the next_obs ring (one allocation or two)
  float* sc;            // the ring's [capacity][A + 2] scalar rows
  uint8_t* cont;        // the ring's continuity flags; nullptr: the buffer keeps none and the block carries none
  long long first, prev;  // first row of the new run and of the previous step's run (-1: no previous flags to write)
  int N, C, H, W, A;
};

template <int C>
__global__ void add_vec_kernel(const AddVecArgs a) {
  const size_t HW = (size_t)a.H * a.W, frame = HW * a.C;
  const size_t nframe = 2 * (size_t)a.N * (C == ADD_VEC_BYTES ? frame : HW / 4);  // frame work items: bytes or groups
  const size_t sc_off = (2 * (size_t)a.N * frame + 15) & ~(size_t)15;
  const size_t nsc = (size_t)a.N * (a.A + 2);
  const size_t total = nframe + nsc + (a.cont ? 2 * (size_t)a.N : 0);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    if (i < nframe) {
      // block frame j, at `at` bytes into its ring row
      const size_t per = C == ADD_VEC_BYTES ? frame : HW / 4;
      const size_t j = i / per, at = C == ADD_VEC_BYTES ? i - j * per : (i - j * per) * 4 * a.C;
      uint8_t* o8 = (j < (size_t)a.N ? a.obs + ((size_t)a.first + j) * frame
                                     : a.next + ((size_t)a.first + j - a.N) * frame) + at;
      if constexpr (C == ADD_VEC_BYTES)
        *o8 = stage_byte(a.block, i, a.C, a.H, a.W, 0, 0, a.H, a.W);
      else
        stage_group<C>(a.block, 2 * (size_t)a.N * frame, o8, (uint32_t)(4 * i), 4, a.H, a.W, 0, 0, a.H, a.W);
    } else if (i < nframe + nsc) {
      const size_t s = i - nframe;
      a.sc[(size_t)a.first * (a.A + 2) + s] = reinterpret_cast<const float*>(a.block + sc_off)[s];
    } else {
      const size_t f = i - nframe - nsc;  // 0 .. N - 1: the previous run, N .. 2N - 1: the new one
      const uint8_t v = a.block[sc_off + 4 * nsc + f];
      if (f >= (size_t)a.N)
        a.cont[(size_t)a.first + f - a.N] = v;
      else if (a.prev >= 0)
        a.cont[(size_t)a.prev + f] = v;
    }
  }
}
