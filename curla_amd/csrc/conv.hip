// 3x3 convolution kernels of the CNNEncoder hot path, gfx950.
//
// Reference semantics: encoder.py:54-63 (Conv2d k=3, first layer stride 2, the
// rest stride 1, no padding) + encoder.py:77-90 (obs/255, relu(conv)).  The
// backward kernels are the autograd of those lines.
//
// Layout: activations are NHWC fp32 in HBM ([B][H][W][32]); conv weights stay
// in the reference OIHW layout (they are nn.Parameters shared with Adam) and
// are re-gathered into MFMA operand images at kernel start.  The stride-1 forward and data gradient run on the bf16
// matrix cores with fp32 operands as exact sums of three bf16 parts (conv_rwb.h, round 5: six exact bf16 products per
// fp32 product, fp32 accumulation); every other inner product runs on the exact-f32 matrix pipe
// (v_mfma_f32_16x16x4_f32), which has the same 157 TFLOP/s roof as the fp32 vector pipe but needs one operand VGPR
// per lane instead of 2 per FMA.  The stride-1 layers (forward, data gradient, weight gradient) are row-walk
// kernels (conv_rwb.h; conv_rw.h / conv_rw43.h: the f32-input forms, selectable; conv_rw_wgrad2.h / conv_rw_wgrad.h): 1-D
// Winograd F(2,3) along x (the weight gradient: F(3,2) in both directions), a wave walks down a strip of pixel-pair
// columns with the transformed filter streamed from LDS; the first
// layer has banded / hybrid forms (crop staged in LDS: conv1_band.h, conv1_wgrad.h) and row-walk forms (conv1_rw.h,
// conv1_u8_rw.h).  What bounds the
// f32-input loops is VALU issue time (a VALU instruction and an f32 MFMA cannot issue in the same cycle), so
// everything in them is counted in instructions.  (Rounds 1-3 also
// carried a banded LDS-tiled form of the stride-1 kernels; it was removed in round 4 once the row walk covered
// every shape -- DESIGN.md section 3.)
//
// This file: the __global__ wrappers round the kernel bodies of the headers above (each header is included in place,
// inside the anonymous namespace, where its wrappers stand) and the host side -- the launch helper and the
// channel-count dispatcher, one select_* function per choice between forms (options.h), the planning and launch
// functions that switch on those, and the C ABI (include/curla_hip.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "common.h"
#include "options.h"

namespace {

constexpr int kLdsPix = 36;   // floats per pixel in LDS (32 channels + 4 pad: conflict-free b128 reads)

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

// 128 bytes of zeros in HBM: where a lane with nothing to multiply points its operand load (a select on the loaded
// VALUE would make the wave wait for the load right behind it instead of one or more k-steps later)
__device__ float g_zero_px[32];

// Timing-only ablations for tools/kbench.py (results are wrong when set); compiled out of the product library.
#ifdef CURLA_ABLATE
int g_ablate = 0;
#define ABL(bit) (a.dbg & (bit))
#define ABL_HOST g_ablate
#else
#define ABL(bit) 0
#define ABL_HOST 0
#endif

#include "conv_rw.h"
#include "conv1_plan.h"  // (host-only: the first layer's plans; after conv_plan.h, which conv_rw.h includes)

// Row-walk kernels (conv_rw.h).  Forward: 512-thread workgroups, ONE per CU, persistent over the samples they own;
// 96 KB of LDS hold the transformed filters of both problems of a layer, so the eight waves draw their steps from one
// pool (minibatch one and two together) and nothing but the layer boundary synchronises them.
__global__ __launch_bounds__(512, 2) void conv_rw_fwd_kernel(rw::Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int l = 0; l < A.nlayers; ++l) {
    rw::build_filter<MODE_FWD, 512>(lds, A.p[l][0].w, A.p[l][1].B > 0 ? A.p[l][1].w : nullptr, threadIdx.x);
    __syncthreads();
    rw::run_layer<MODE_FWD, 8>(A.g[l], A.p[l][0], A.p[l][1], lds, blockIdx.x, gridDim.x);
    if (l + 1 < A.nlayers) {
      // this workgroup's outputs of layer l are (only) its own inputs of layer l + 1; the barrier also keeps the
      // filter in LDS until every wave has finished reading it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  }
}

#include "conv_rw43.h"

// The forward with Winograd F(4,3) along x (conv_rw43.h): 0.75 x the MFMAs; 256-thread workgroups, ONE wave per SIMD
// (the 144 accumulator + 96 window registers of a wave do not fit twice), 144 KB of LDS for the two filters.
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv_rw43_fwd_kernel(rw::Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int l = 0; l < A.nlayers; ++l) {
    rw43::build_filter<MODE_FWD, 256>(lds, A.p[l][0].w, A.p[l][1].B > 0 ? A.p[l][1].w : nullptr, threadIdx.x);
    __syncthreads();
    rw43::run_layer<MODE_FWD, 4>(A.g[l], A.p[l][0], A.p[l][1], lds, blockIdx.x, gridDim.x);
    if (l + 1 < A.nlayers) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  }
}

// ... and the data gradient in the same form (one wave per SIMD: it cannot share a launch with the 256-register weight
// gradient, so wide layers run the two as two launches -- at their size a launch boundary is noise)
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv_rw43_dgrad_kernel(rw::Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  rw43::build_filter<MODE_DGRAD, 256>(lds, A.p[0][0].w, nullptr, threadIdx.x);
  __syncthreads();
  rw43::run_layer<MODE_DGRAD, 4>(A.g[0], A.p[0][0], A.p[0][1], lds, blockIdx.x, gridDim.x);
}

#include "conv_rwb.h"

// The same layers on the bf16 matrix cores with fp32 operands split into three bf16 parts (conv_rwb.h): 512-thread
// workgroups, one per CU, 2 x rwb::kWBytes = 144 KB of LDS for the split filters of the two problems of a layer (72 KB
// each: 16 KB of headroom under the CU's 160 KB, asserted beside kMaxLds below).
#ifdef RWB_CLOCK
// diagnostic build (tools/clock_reconcile.sh: -DRWB_CLOCK): per workgroup, summed over launches, wave 0's shader cycles
// (s_memtime) and 100 MHz ticks (s_memrealtime) from its first instruction to its last, and the launch count.  Two
// stamps per workgroup and launch: nothing inside the loops (the per-step stamps of RWB_STAMP cost ~11 % of a wave).
__device__ unsigned long long g_rwb_clock[3 * 1024];
#endif

template <int NW>
__device__ __forceinline__ void rwb_fwd_body(const rw::Args& A) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds_h[];
#if defined(RWB_STAMP) || defined(RWB_CLOCK)
  const unsigned long long kt0 = __builtin_readcyclecounter(), kr0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (int l = 0; l < A.nlayers; ++l) {
#ifdef RWB_STAMP
    const unsigned long long k0 = __builtin_readcyclecounter();
#endif
    rwb::build_filter<MODE_FWD, 64 * NW>(lds_h, A.p[l][0].w, A.p[l][1].B > 0 ? A.p[l][1].w : nullptr, threadIdx.x);
    __syncthreads();
#ifdef RWB_STAMP
    const unsigned long long k1 = __builtin_readcyclecounter();
#endif
    rwb::run_layer<MODE_FWD, NW>(A.g[l], A.p[l][0], A.p[l][1], lds_h, blockIdx.x, gridDim.x);
#ifdef RWB_STAMP
    const unsigned long long k2 = __builtin_readcyclecounter();
#endif
    if (l + 1 < A.nlayers) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
#ifdef RWB_STAMP
    const unsigned long long k3 = __builtin_readcyclecounter();
    if (threadIdx.x == 0 && blockIdx.x == 7) {
      rwb::g_rwb_stamp[4] += k1 - k0, rwb::g_rwb_stamp[5] += k2 - k1, rwb::g_rwb_stamp[6] += k3 - k2, rwb::g_rwb_stamp[7] += 1;
    }
#endif
  }
#ifdef RWB_STAMP
  if (threadIdx.x == 0 && blockIdx.x == 7) {
    rwb::g_rwb_stamp[15] += __builtin_readcyclecounter() - kt0;
    rwb::g_rwb_stamp[14] += __builtin_amdgcn_s_memrealtime() - kr0;
  }
#endif
#ifdef RWB_CLOCK
  if (threadIdx.x == 0 && blockIdx.x < 1024) {
    g_rwb_clock[3 * blockIdx.x + 0] += __builtin_readcyclecounter() - kt0;
    g_rwb_clock[3 * blockIdx.x + 1] += __builtin_amdgcn_s_memrealtime() - kr0;
    g_rwb_clock[3 * blockIdx.x + 2] += 1;
  }
#endif
}

__global__ __launch_bounds__(512, 1) void conv_rwb_fwd_kernel(rw::Args A) { rwb_fwd_body<8>(A); }

__global__ __launch_bounds__(512, 1) void conv_rwb_dgrad_kernel(rw::Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds_h[];
  rwb::build_filter<MODE_DGRAD, 512>(lds_h, A.p[0][0].w, nullptr, threadIdx.x);
  __syncthreads();
  rwb::run_layer<MODE_DGRAD, 8>(A.g[0], A.p[0][0], A.p[0][1], lds_h, blockIdx.x, gridDim.x);
}

// data gradient alone (256-thread workgroups: the form that shares a launch with the weight gradient below)
__global__ __launch_bounds__(256, 2) void conv_rw_dgrad_kernel(rw::Args A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  rw::build_filter<MODE_DGRAD, 256>(lds, A.p[0][0].w, nullptr, threadIdx.x);
  __syncthreads();
  rw::run_layer<MODE_DGRAD, 4>(A.g[0], A.p[0][0], A.p[0][1], lds, blockIdx.x, gridDim.x);
}

#include "conv1_rw.h"

// first layer from a float NHWC minibatch in row-walk form (conv1_rw.h): 512-thread workgroups, one per CU, persistent
// over the samples they own (8 waves share a sample's steps: small minibatches still fill the SIMDs twice)
template <int C>
__global__ __launch_bounds__(512, 2) void conv1_rw_fwd_kernel(rw::Conv1Args a) {
  rw::conv1_body<C, 8>(a, blockIdx.x, gridDim.x);
}

template <int C>
__global__ __launch_bounds__(512, 2) void wgrad1_rw_kernel(rw::Wgrad1Args a) {
  rw::wgrad1_body<C, 8>(a, blockIdx.x, gridDim.x);
}

#include "conv1_u8_rw.h"

// workgroup shape of the uint8 row-walk forward: two 512-thread workgroups per CU (4 waves per SIMD).  Five 256-thread
// ones (5 waves per SIMD, what ~100 VGPRs allow) were slower inside update(): 402 against 407 update()/s
using conv1::kC1U8PerCU;
using conv1::kC1U8Threads;

// first layer straight from the uint8 ring in row-walk form (conv1_u8_rw.h): 512-thread workgroups, two per CU, equal
// shares of the pool of steps of both minibatches (the second with its own weights: both images sit in LDS)
template <int C>
__global__ __launch_bounds__(kC1U8Threads, kC1U8PerCU) void conv1_u8_rw_fwd_kernel(rw::Conv1U8Args a) {
  __shared__ __attribute__((aligned(16))) float lds_img[2 * rw::conv1_u8_image_floats<C>()];
  rw::conv1_u8_stage_weights<C, kC1U8Threads>(lds_img, a.p[0].w, a.p[0].bias, a.scale, threadIdx.x);
  if (a.p[1].B > 0)
    rw::conv1_u8_stage_weights<C, kC1U8Threads>(lds_img + rw::conv1_u8_image_floats<C>(), a.p[1].w, a.p[1].bias, a.scale,
                                                threadIdx.x);
  __syncthreads();
  if ((a.Ws * C) % 4 == 0)
    rw::conv1_u8_body<C, kC1U8Threads / 64, true>(a, lds_img, blockIdx.x, gridDim.x);
  else
    rw::conv1_u8_body<C, kC1U8Threads / 64, false>(a, lds_img, blockIdx.x, gridDim.x);
}

// ... and on the bf16 matrix cores (uint8 pixels are exact in bf16: one part for the pixels, three for the weights; C <= 10).
// The weight fragments take 72 registers (148 in all): three 256-thread workgroups per CU (3 waves per SIMD)
using conv1::kC1U8bPerCU;
using conv1::kC1U8bThreads;
template <int C>
__global__ __launch_bounds__(kC1U8bThreads, kC1U8bPerCU) void conv1_u8_rwb_fwd_kernel(rw::Conv1U8Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_imgb[2 * rw::kConv1U8B3ImageBytes];
  rw::conv1_u8b_stage_weights<C, kC1U8bThreads>(lds_imgb, a.p[0].w, a.p[0].bias, a.scale, threadIdx.x);
  if (a.p[1].B > 0)
    rw::conv1_u8b_stage_weights<C, kC1U8bThreads>(lds_imgb + rw::kConv1U8B3ImageBytes, a.p[1].w, a.p[1].bias, a.scale,
                                                  threadIdx.x);
  __syncthreads();
  if ((a.Ws * C) % 4 == 0)
    rw::conv1_u8b_body<C, kC1U8bThreads / 64, true>(a, lds_imgb, blockIdx.x, gridDim.x);
  else
    rw::conv1_u8b_body<C, kC1U8bThreads / 64, false>(a, lds_imgb, blockIdx.x, gridDim.x);
}

#include "conv1_band.h"

// ---------------------------------------------------------------------------
// weight gradient, stride-1 32->32:  dW[co][ci][tap] = sum_pixels g[p][co] * in[p+tap][ci]  (conv_rw_wgrad.h).
// Partial sums leave through one slab of kPartialS1 floats per workgroup and a deterministic second pass
// (wgrad_reduce_multi_kernel below).
// ---------------------------------------------------------------------------
constexpr int kPartialS1 = 32 * 288 + 32;

#include "conv_rw_wgrad.h"
#include "conv_rw_wgrad2.h"

// the weight-gradient body of a workgroup: Winograd along x (conv_rw_wgrad.h) or in both directions (conv_rw_wgrad2.h)
__device__ __forceinline__ void wgrad_any(const rw::WgradArgs& wa, const int bid, const int nblk) {
  if (wa.two_d)
    rw::wgrad2_body<4>(wa, bid, nblk);
  else
    rw::wgrad_body<4>(wa, bid, nblk);
}

// weight gradient in its row-walk form (conv_rw_wgrad.h), alone and in one launch with the row-walk data gradient
__global__ __launch_bounds__(256, 2) void wgrad_rw_kernel(rw::WgradArgs wa) {
  wgrad_any(wa, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256, 2) void bwd_rw2_kernel(rw::WgradArgs wa, rw::Args da, int nw) {
  if ((int)blockIdx.x < nw) {
    wgrad_any(wa, blockIdx.x, nw);
  } else {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    rw::build_filter<MODE_DGRAD, 256>(lds, da.p[0][0].w, nullptr, threadIdx.x);
    __syncthreads();
    rw::run_layer<MODE_DGRAD, 4>(da.g[0], da.p[0][0], da.p[0][1], lds, (int)blockIdx.x - nw, (int)gridDim.x - nw);
  }
}

// ... and with the data gradient in its bf16x3 form (conv_rwb.h) beside it: 256-thread workgroups of both kinds, the data
// gradient's with 72 KB of LDS for its split filter
__global__ __launch_bounds__(256, 2) void bwd_rwb2_kernel(rw::WgradArgs wa, rw::Args da, int nw) {
  if ((int)blockIdx.x < nw) {
    wgrad_any(wa, blockIdx.x, nw);
  } else {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds_hb[];
    rwb::build_filter<MODE_DGRAD, 256>(lds_hb, da.p[0][0].w, nullptr, threadIdx.x);
    __syncthreads();
    rwb::run_layer<MODE_DGRAD, 4>(da.g[0], da.p[0][0], da.p[0][1], lds_hb, (int)blockIdx.x - nw, (int)gridDim.x - nw);
  }
}

#include "conv1_wgrad.h"

#include "conv_wgrad_reduce.h"

// ------------------------------ host side: launching ------------------------------
constexpr int kMaxLds = 160 * 1024;
static_assert(2 * rwb::kWBytes <= kMaxLds, "the two problems' split filters of conv_rwb_fwd_kernel must fit one CU's LDS");
// Dynamic LDS limit of a kernel: raised once per (kernel, device) to the largest size this library ever asks for --
// never lowered, never set per launch (curla_set_dyn_lds, common.h).
template <typename K>
int set_lds(K kernel, size_t bytes) {
  if (bytes > (size_t)kMaxLds) return CURLA_ERR_UNSUPPORTED;
  return curla_set_dyn_lds(reinterpret_cast<const void*>(kernel), kMaxLds);
}

// Every launch of this file: raise the kernel's dynamic-LDS limit if (and only if) the launch uses dynamic LDS, launch,
// report the launch status.
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), int grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
  if (lds) {
    const int rc = set_lds(kernel, lds);
    if (rc != CURLA_OK) return rc;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
  return curla_launch_status();
}

// (the run-time channel count C -> template instance: dispatch_int<Cs...>, common.h -- the list at a call site names the
// instances it compiles; the bf16 first-layer forms exist for 3 C <= 32 only)

// the C ABI's src_kind of the first layer's input, and f(the kernels' SRC_* of it)
enum { kSrcF32Nchw = 0, kSrcU8Ring = 1, kSrcF32Nhwc = 2 };
template <typename F>
int dispatch_src(int src_kind, F&& f) {
  if (src_kind == kSrcU8Ring) return f(std::integral_constant<int, SRC_U8>{});
  if (src_kind == kSrcF32Nhwc) return f(std::integral_constant<int, SRC_NHWC>{});
  return f(std::integral_constant<int, SRC_F32>{});
}

// ------------------------------ host side: which form runs ------------------------------
// Each decision is made in ONE function below, "auto" resolved inside it; the launch functions switch on the result.

// Stride-1 forward AND data gradient (option s1_fwd).  auto = b3, the bf16-matrix-core form (conv_rwb.h: fp32 operands
// as three bf16 parts, Winograd F(2,3) in front): measured on the stacks update() launches (tools/s1_bench.py) it takes
// 365 / 253 us on configs[1]'s two stacks against 491 / 337 for F(2,3) and 451 / 309 for F(4,3) on the f32-input MFMA,
// and 5.99 / 4.01 ms against F(4,3)'s 7.15 / 4.71 on configs[4]'s.  f23 / f43 (conv_rw.h / conv_rw43.h) remain
// selectable: F(4,3) issues 0.78 x the f32 MFMAs of F(2,3) but ~0.9 VALU instructions per MFMA instead of 0.4 at one wave
// per SIMD, and wins among the two where rows hold at least one full strip of 16 pixel quads.  The data gradient as b3
// beside the weight gradient's workgroups in one launch takes configs[1] from 474.6 to 487.3 update()/s and configs[4]
// from 34.6 to 35.2 against the F(2,3) / F(4,3) forms.
enum class S1Form { F23, F43, B3 };
S1Form select_s1_form() {
  const int opt = curla_opt(kOptS1Fwd);
  return opt == kS1FwdF23 ? S1Form::F23 : opt == kS1FwdF43 ? S1Form::F43 : S1Form::B3;  // (auto = b3)
}

// Stride-1 backward launch shape (option bwd_split) where weight gradient and data gradient share a launch: 2 x CUs
// workgroups of each kind, run one kind after the other -- or ONE workgroup of each kind per CU side by side: the layer
// takes as long (a CU shared between the two kinds is no busier than one shared by two of a kind), but the weight
// gradient leaves half as many slabs for the reduction to read.  auto: beside the b3 data gradient always side by side
// (the faster split for long launches too: configs[4] 35.9 against 35.2 update()/s); beside the f23 one only for short
// launches -- long ones keep the 2 + 2 form: there a few percent of imbalance between the kinds (the tail runs at one
// workgroup per CU) costs more than the slabs (B = 1024 at 81 x 81: +0.3 ms per update).
enum class BwdShape { SideBySide, TwoAndTwo };
BwdShape select_bwd_shape(S1Form dgrad, int B, int Ho, int Wo) {
  const int opt = curla_opt(kOptBwdSplit);
  const bool side = opt == kBwdSplitAuto ? dgrad == S1Form::B3 || (long long)B * Ho * Wo <= (1LL << 20) : opt == kBwdSplitOn;
  return side ? BwdShape::SideBySide : BwdShape::TwoAndTwo;
}

// Stride-1 weight gradient (option s1_wgrad): Winograd F(3,2) along x, or in both directions (auto: a third fewer matrix
// instructions for ~40 instead of ~10 VALU instructions per step; alone 77 -> 69 us, beside the bf16x3 data gradient
// 125 -> 118 us for 512 samples of 35 x 35 gradients, 1179 -> 1080 us for 1024 of 79 x 79: tools/s1_bwd_bench.py)
enum class S1WgradForm { X, XY };
S1WgradForm select_s1_wgrad_form() { return curla_opt(kOptS1Wgrad) == kS1WgradX ? S1WgradForm::X : S1WgradForm::XY; }

// (the arithmetic of the first layer's plans and form choices is host-only code, conv1_plan.h: the functions below read
// the options and the CU count and hand them over)
using conv1::Conv1F32Form;
using conv1::Conv1U8Form;
using conv1::Wgrad1U8Form;

// First-layer forward from the uint8 ring (option conv1_u8).  Rw = the LDS-free row walk (conv1_u8_rw.h) and Rwb = the same
// on the bf16 matrix cores, where an input row's 3 C operand bytes are one k-step of 32; Hybrid = conv1_u8_walk_kernel
// (crop staged in LDS as bytes, row walk out of LDS); Band = the banded loop.  Measured on 1024 + 512 / 512 + 512 samples
// of configs[1]: alone, re-reading the same ring slots out of the Infinity Cache, the LDS-free walk takes 100 / 66 us
// against the banded loop's 128 / 86; on slots drawn afresh for every launch from a ring of gigabytes -- what update()
// does -- it was the slower one in rounds 3-4 (114 us on average against the hybrid's 102) and is the faster one since
// the stride-1 convs around it run on the bf16 matrix cores (round 5, whole update, alternating runs on one box:
// configs[1] 493.4 / 493.4 against 489.0 / 490.2 update()/s, configs[2] 634.3 against 632.0).
//   auto, rwb: Rwb where 3 C <= 32, else Rw;  rw: Rw;  hybrid, band: never a row walk.
//   A shape beyond the row walk's index limits, and hybrid / band, take Hybrid where the whole crop is one band of LDS
//   that leaves room for two workgroups per CU and a row is at most 64 16-byte runs (its staging gives a lane one run of
//   a row) -- unless the option says band; else Band.
Conv1U8Form select_conv1_u8_form(int C, int Hs, int Ws, int Wc, int Btotal, int Ho, int Wo) {
  return conv1::select_conv1_u8_form(curla_opt(kOptConv1U8), C, Hs, Ws, Wc, Btotal, Ho, Wo);
}

// First layer and its weight gradient from a float tensor (option conv1_f32): the row walk with nothing staged
// (conv1_rw.h) for NHWC minibatches within its 30-bit byte offsets, else the banded kernels.
Conv1F32Form select_conv1_f32_form(int src_kind, int C, int Hc, int Wc) {
  return conv1::select_conv1_f32_form(curla_opt(kOptConv1F32), src_kind == kSrcF32Nhwc, C, Hc, Wc);
}

// First-layer weight gradient from the uint8 ring, input band kept as bytes (option wgrad1_u8).  B16 = the
// bf16-matrix-core form (wgrad1_u8b_kernel, round 6) wherever a lane's 8 consecutive pixels wrap at most once (output rows
// of >= 8 pixels) and 3 C <= 32 (C = 12: nine tiles per channel half do not fit four waves per SIMD); F32 = the f32-input
// MFMA (wgrad1_u8_kernel), two 512-thread workgroups per CU.  F32FourWave (CURLA_ABLATE builds only) = four 256-thread
// ones: measured at 84x84x9, B = 512, 77.4 us against the 71.9 us of two 512-thread workgroups -- the shorter bands'
// extra halo rows and slabs cost more than the finer interleaving buys.
Wgrad1U8Form select_wgrad1_u8_form(int C, int Wc, int Wo) {
  return conv1::select_wgrad1_u8_form(curla_opt(kOptWgrad1U8), (ABL_HOST & 1024) != 0, C, Wc, Wo);
}

// ------------------------------ host side: stride-1 layers ------------------------------
// The row-walk forward keeps (pixel pair, 32 channels) of a whole row in flight per wave; any width works, the strips
// only get more numerous.  Limits: byte offsets inside one sample must fit 31 bits.
bool rw_supported(int Hi, int Wi) { return (long long)(Hi + 2) * (Wi + 2) * 128 < (1LL << 30); }

// the strips of a layer, and the LDS bytes of one problem's transformed filter, in each form
rw::Geom s1_plan(S1Form f, int Hi, int Wi, int Ho, int Wo) {
  return f == S1Form::B3 ? rwb::plan(Hi, Wi, Ho, Wo) : f == S1Form::F43 ? rw43::plan(Hi, Wi, Ho, Wo) : rw::plan(Hi, Wi, Ho, Wo);
}
size_t s1_filter_bytes(S1Form f) {
  return f == S1Form::B3 ? rwb::kWBytes : (f == S1Form::F43 ? rw43::kWFloats : rw::kWFloats) * sizeof(float);
}

int launch_rw_fwd(int nlayers, const float* in, const float* const* w, const float* const* bias, float* const* out, int B,
                  const float* in2, const float* const* w2, const float* const* bias2, float* const* out2, int B2, int Hi,
                  int Wi, bool owned, hipStream_t st) {
  const S1Form form = select_s1_form();
  rw::Args A;
  A.nlayers = nlayers;
  for (int l = 0; l < rw::kMaxLayers; ++l) {
    const bool on = l < nlayers;
    const int hi = Hi - 2 * l, wi = Wi - 2 * l;
    A.g[l] = on ? s1_plan(form, hi, wi, hi - 2, wi - 2) : rw::Geom{};
    A.p[l][0] = on ? rw::Problem{l == 0 ? in : out[l - 1], w[l], bias[l], out[l], B} : rw::Problem{};
    A.p[l][1] = (on && B2 > 0) ? rw::Problem{l == 0 ? in2 : out2[l - 1], w2[l], bias2[l], out2[l], B2} : rw::Problem{};
    if (on && (hi < 3 || wi < 3)) return CURLA_ERR_UNSUPPORTED;
  }
  if (!rw_supported(Hi, Wi)) return CURLA_ERR_UNSUPPORTED;
  // one workgroup per CU, the filters of both problems of a layer in LDS
  const int cus = curla_cu_count();
  const int grid = owned ? cus : std::min(B > B2 ? B : B2, cus);
  const size_t lds = (size_t)(B2 > 0 ? 2 : 1) * s1_filter_bytes(form);
  switch (form) {
    case S1Form::B3: return launch(conv_rwb_fwd_kernel, grid, 512, lds, st, A);
    case S1Form::F43: return launch(conv_rw43_fwd_kernel, grid, 256, lds, st, A);
    default: return launch(conv_rw_fwd_kernel, grid, 512, lds, st, A);
  }
}

// data-gradient arguments: input = the layer's output gradient [B][Ho][Wo][32], output [B][Ho+2][Wo+2][32]
rw::Args rw_dgrad_args(S1Form form, const float* g, const float* w, const float* act_below, float* gin, int B, int Ho,
                       int Wo) {
  rw::Args A;
  A.nlayers = 1;
  for (int l = 0; l < rw::kMaxLayers; ++l) A.g[l] = rw::Geom{}, A.p[l][0] = rw::Problem{}, A.p[l][1] = rw::Problem{};
  A.g[0] = s1_plan(form, Ho, Wo, Ho + 2, Wo + 2);
  A.p[0][0] = rw::Problem{g, w, act_below, gin, B};
  return A;
}

// the data gradient as a launch of its own: one workgroup per CU (f23: two 256-thread ones)
int launch_dgrad(S1Form form, const float* g, const float* w, const float* act_below, float* gin, int B, int Ho, int Wo,
                 hipStream_t st) {
  const rw::Args A = rw_dgrad_args(form, g, w, act_below, gin, B, Ho, Wo);
  const int cus = curla_cu_count();
  const size_t lds = s1_filter_bytes(form);
  switch (form) {
    case S1Form::B3: return launch(conv_rwb_dgrad_kernel, std::min(B, cus), 512, lds, st, A);
    case S1Form::F43: return launch(conv_rw43_dgrad_kernel, std::min(B, cus), 256, lds, st, A);
    default: return launch(conv_rw_dgrad_kernel, std::min(B, 2 * cus), 256, lds, st, A);
  }
}

int launch_conv_s1(int mode, const float* in, const float* w, const float* aux, float* out, int B, int Hs, int Ws,
                   hipStream_t st, const float* in2 = nullptr, const float* w2 = nullptr, const float* aux2 = nullptr,
                   float* out2 = nullptr, int B2 = 0) {
  if (!rw_supported(Hs, Ws)) return CURLA_ERR_UNSUPPORTED;
  if (mode == MODE_FWD) return launch_rw_fwd(1, in, &w, &aux, &out, B, in2, &w2, &aux2, &out2, B2, Hs, Ws, false, st);
  return launch_dgrad(select_s1_form(), in, w, aux, out, B, Hs, Ws, st);
}

rw::WgradArgs wgrad_args(const float* in, const float* g, float* workspace, int B, int Hi, int Wi, int Ho, int Wo) {
  const bool two_d = select_s1_wgrad_form() == S1WgradForm::XY;
  return rw::WgradArgs{in, g, workspace, B, Hi, Wi, Ho, Wo, two_d ? rw::plan4p(Hi, Wi, Ho, Wo) : rw::plan4(Hi, Wi, Ho, Wo),
                       two_d ? 1 : 0};
}

// ------------------------------ host side: first layer, banded forms ------------------------------
// band height of the float banded kernels within `lds_budget` (conv1_plan.h)
int plan_band_conv1(int Ho, int Wo, int Wc, int C, int g_px_per_row, size_t lds_budget) {
  return conv1::plan_band_conv1(Ho, Wo, Wc, C, g_px_per_row, lds_budget, kLdsPix);
}

// Conv1U8Form::Hybrid / Band: the band stays bytes in LDS, the tallest that leaves room for two workgroups per CU; the
// same bytes first hold the kernels' k-major weight image.  Fills a.th / a.nbands, returns the LDS bytes of the launch.
size_t plan_conv1_u8_band(Conv1Args& a) {
  const conv1::Bands b = conv1::plan_u8_bands(a.Ho, conv1::u8_row_bytes(a.Wc, a.C), conv1::kConv1U8BandBudget);
  a.th = b.th, a.nbands = b.nbands;
  return conv1::conv1_u8_band_lds(a.th, a.Wc, a.C);
}

// The uint8 weight gradient's bands (two 512-thread workgroups per CU of <= 76 KB of LDS each; F32FourWave: four
// 256-thread ones of <= 38 KB) and the LDS of its final cross-wave sum.  Fills a.th / a.nbands / a.lds_bytes, returns the
// LDS bytes of the launch.
size_t plan_wgrad1_u8(Wgrad1Args& a, Wgrad1U8Form form) {
  const int nwaves = form == Wgrad1U8Form::F32FourWave ? 4 : 8;
  const conv1::Bands b = conv1::plan_u8_bands(a.Ho, conv1::u8_row_bytes(a.Wc, a.C),
                                              nwaves == 4 ? conv1::kWgrad1U8BandBudget4 : conv1::kWgrad1U8BandBudget);
  a.th = b.th, a.nbands = b.nbands;
  const size_t lds = conv1::wgrad1_u8_lds(a.th, a.Wc, a.C, nwaves, form == Wgrad1U8Form::B16);
  a.lds_bytes = (unsigned)lds;
  return lds;
}

}  // namespace

// ------------------------------------ C ABI ------------------------------------
extern "C" {

#ifdef CURLA_ABLATE
void curla_debug_ablate(int flags) { g_ablate = flags; }
#endif
#ifdef RWB_CLOCK
int curla_debug_rwb_clock(unsigned long long* out, int n_workgroups, int reset) {
  if (n_workgroups < 1 || n_workgroups > 1024) return -1;
  if (reset) {
    static unsigned long long z[3 * 1024];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_rwb_clock), z, sizeof(z)) == hipSuccess ? 0 : -2;
  }
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rwb_clock), 3 * n_workgroups * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif
#ifdef RWB_STAMP
// timing-only debug build (tools/build_variant.sh stamp -DRWB_STAMP): cycle sums of wave 0 of workgroup 7 over its full steps
int curla_debug_rwb_stamps(unsigned long long* out8, int reset) {
  if (reset) {
    unsigned long long z[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(rwb::g_rwb_stamp), z, sizeof(z)) == hipSuccess ? 0 : -2;
  }
  return hipMemcpyFromSymbol(out8, HIP_SYMBOL(rwb::g_rwb_stamp), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif

}  // extern "C"  (re-opened below: the generic-width helpers are C++)
#include "conv_generic.h"

namespace {
// ---- filter counts other than 32: the plain kernels of conv_generic.h behind the same entry points -------------------
int gen_fwd_s1(const float* in, const float* w, const float* bias, float* out, int B, int Hi, int Wi, int C, hipStream_t st) {
  if (!gen::channels_ok(C)) return CURLA_ERR_UNSUPPORTED;
  const int Ho = Hi - 2, Wo = Wi - 2;
  gen::Src none{};
  return launch(gen::conv_fwd_kernel<false>, gen::grid_for((size_t)B * Ho * Wo * C), 256, 0, st, none, in, w, bias, out, B, Hi,
                Wi, C, Ho, Wo, C);
}

gen::Src gen_src(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1, int C, int Hs, int Ws,
                 int Hc, int Wc, float scale) {
  return gen::Src{src, src_kind, idx, h1, w1, C, Hs, Ws, Hc, Wc, scale};
}

int gen_fwd1(const gen::Src& s, const float* w, const float* bias, float* out, int B, int channels, hipStream_t st) {
  if (!gen::channels_ok(channels)) return CURLA_ERR_UNSUPPORTED;
  const int Ho = (s.Hc - 3) / 2 + 1, Wo = (s.Wc - 3) / 2 + 1;
  return launch(gen::conv_fwd_kernel<true>, gen::grid_for((size_t)B * Ho * Wo * channels), 256, 0, st, s,
                static_cast<const float*>(nullptr), w, bias, out, B, s.Hc, s.Wc, s.C, Ho, Wo, channels);
}

int gen_dgrad(const float* g, const float* w, const float* act_below, float* gin, int B, int Ho, int Wo, int C, hipStream_t st) {
  if (!gen::channels_ok(C)) return CURLA_ERR_UNSUPPORTED;
  return launch(gen::conv_dgrad_kernel, gen::grid_for((size_t)B * (Ho + 2) * (Wo + 2) * C), 256, 0, st, g, w, act_below, gin, B,
                Ho, Wo, C);
}

// (one slab: [channels * cin * 9 | channels])
int gen_wgrad_s1(const float* in, const float* g, float* slab, int B, int Hi, int Wi, int C, hipStream_t st, int* nslabs) {
  if (!gen::channels_ok(C)) return CURLA_ERR_UNSUPPORTED;
  gen::Src none{};
  *nslabs = 1;
  return launch(gen::conv_wgrad_kernel<false>, C * C + C, 256, 0, st, none, in, g, slab, B, Hi, Wi, C, Hi - 2, Wi - 2, C);
}

int gen_wgrad1(const gen::Src& s, const float* g, float* slab, int B, int channels, hipStream_t st, int* nslabs) {
  if (!gen::channels_ok(channels)) return CURLA_ERR_UNSUPPORTED;
  const int Ho = (s.Hc - 3) / 2 + 1, Wo = (s.Wc - 3) / 2 + 1;
  *nslabs = 1;
  return launch(gen::conv_wgrad_kernel<true>, channels * s.C + channels, 256, 0, st, s, static_cast<const float*>(nullptr), g,
                slab, B, s.Hc, s.Wc, s.C, Ho, Wo, channels);
}
}  // namespace

extern "C" {

int curla_conv3x3_s1_fwd(const float* in, const float* w, const float* bias, float* out, int B, int Hi, int Wi,
                         int channels, void* stream) {
  CURLA_REQUIRE(in && w && bias && out && B > 0 && Hi >= 3 && Wi >= 3);
  if (channels != 32) return gen_fwd_s1(in, w, bias, out, B, Hi, Wi, channels, static_cast<hipStream_t>(stream));
  CURLA_REQUIRE(aligned16(in) && aligned16(out) && aligned16(bias) && aligned16(w));
  return launch_conv_s1(MODE_FWD, in, w, bias, out, B, Hi, Wi, static_cast<hipStream_t>(stream));
}

int curla_conv3x3_s1_fwd2(const float* in, const float* w, const float* bias, float* out, int B, const float* in2,
                          const float* w2, const float* bias2, float* out2, int B2, int Hi, int Wi, int channels,
                          void* stream) {
  CURLA_REQUIRE(in && w && bias && out && B > 0 && in2 && w2 && bias2 && out2 && B2 > 0 && Hi >= 3 && Wi >= 3);
  if (channels != 32) {  // (generic width: the two problems one after the other)
    const int rc = gen_fwd_s1(in, w, bias, out, B, Hi, Wi, channels, static_cast<hipStream_t>(stream));
    return rc != CURLA_OK ? rc : gen_fwd_s1(in2, w2, bias2, out2, B2, Hi, Wi, channels, static_cast<hipStream_t>(stream));
  }
  CURLA_REQUIRE(aligned16(in) && aligned16(out) && aligned16(bias) && aligned16(w));
  CURLA_REQUIRE(aligned16(in2) && aligned16(out2) && aligned16(bias2) && aligned16(w2));
  return launch_conv_s1(MODE_FWD, in, w, bias, out, B, Hi, Wi, static_cast<hipStream_t>(stream), in2, w2, bias2, out2, B2);
}

int curla_conv3x3_s1_fwd_stack(int nlayers, const float* in, const float* const* w, const float* const* bias,
                               float* const* out, int B, const float* in2, const float* const* w2,
                               const float* const* bias2, float* const* out2, int B2, int Hi, int Wi, int channels,
                               void* stream) {
  CURLA_REQUIRE(nlayers > 0 && nlayers <= rw::kMaxLayers && in && w && bias && out && B > 0 && Hi >= 3 && Wi >= 3);
  CURLA_REQUIRE(B2 == 0 || (in2 && w2 && bias2 && out2));
  if (channels != 32) return CURLA_ERR_UNSUPPORTED;
  // ownership of samples by workgroups needs whole rounds of the grid (one workgroup per CU) over each minibatch
  const int G1 = curla_cu_count();
  if (B % G1 != 0 || B2 % G1 != 0) return CURLA_ERR_UNSUPPORTED;
  CURLA_REQUIRE(aligned16(in) && (!B2 || aligned16(in2)));
  for (int l = 0; l < nlayers; ++l) {
    CURLA_REQUIRE(w[l] && bias[l] && out[l] && aligned16(w[l]) && aligned16(bias[l]) && aligned16(out[l]));
    CURLA_REQUIRE(!B2 || (w2[l] && bias2[l] && out2[l] && aligned16(w2[l]) && aligned16(bias2[l]) && aligned16(out2[l])));
  }
  if (Hi - 2 * nlayers < 1 || Wi - 2 * nlayers < 1) return CURLA_ERR_UNSUPPORTED;
  return launch_rw_fwd(nlayers, in, w, bias, out, B, in2, w2, bias2, out2, B2, Hi, Wi, true,
                       static_cast<hipStream_t>(stream));
}

int curla_conv3x3_s1_stack_granule(void) { return curla_cu_count(); }

int curla_conv3x3_s1_dgrad(const float* g, const float* w, const float* act_below, float* gin, int B, int Ho, int Wo,
                           int channels, void* stream) {
  CURLA_REQUIRE(g && w && act_below && gin && B > 0 && Ho >= 1 && Wo >= 1);
  if (channels != 32) return gen_dgrad(g, w, act_below, gin, B, Ho, Wo, channels, static_cast<hipStream_t>(stream));
  CURLA_REQUIRE(aligned16(g) && aligned16(gin) && aligned16(act_below) && aligned16(w));
  return launch_conv_s1(MODE_DGRAD, g, w, act_below, gin, B, Ho, Wo, static_cast<hipStream_t>(stream));
}

static int conv1_common_check(const void* src, int src_kind, int B, int C, int Hs, int Ws, int Hc, int Wc) {
  CURLA_REQUIRE(src && B > 0 && Hc >= 3 && Wc >= 3 && src_kind >= 0 && src_kind <= 2);
  if (C != 9 && C != 12 && C != 6 && C != 3) return CURLA_ERR_UNSUPPORTED;  // 3 x frame_stack of 1..4
  if (src_kind == kSrcU8Ring) {
    CURLA_REQUIRE(Hs >= Hc && Ws >= Wc);
    // the loader rebuilds every 16-byte run from aligned dwords whatever its byte address, so frames of any size
    // work; only the ring's base must be dword-aligned (the first run would otherwise start before the buffer)
    CURLA_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0);
  }
  return CURLA_OK;
}

struct Conv1Second {
  const int64_t* idx;
  const int32_t* h1;
  const int32_t* w1;
  const float* w;
  const float* bias;
  float* out;
  int B;
};

// uint8 ring, row walk with nothing staged (conv1_u8_rw.h): Conv1U8Form::Rw / Rwb
static int launch_conv1_u8_rw(Conv1U8Form form, const Conv1Args& a, hipStream_t st) {
  rw::Conv1U8Args ra;
  ra.src = static_cast<const uint8_t*>(a.src);
  ra.p[0] = rw::Conv1U8Problem{a.idx, a.h1, a.w1, a.w, a.bias, a.out, a.B};
  ra.p[1] = rw::Conv1U8Problem{a.idx2, a.h1_2, a.w1_2, a.w2, a.bias2, a.out2, a.B2};
  ra.Hs = a.Hs, ra.Ws = a.Ws, ra.Ho = a.Ho, ra.Wo = a.Wo, ra.scale = a.scale;
  ra.g.Hi = a.Hc, ra.g.Wi = a.Wc, ra.g.Ho = a.Ho, ra.g.Wo = a.Wo;
  rw::plan_units(ra.g, a.Ho, a.Wo, 16);
  // kC1U8PerCU (bf16: kC1U8bPerCU) workgroups per CU; fewer when a workgroup's share of the pool of steps would drop
  // below 8 steps per wave (conv1_plan.h)
  const long long pool = (long long)(a.B + a.B2) * ra.g.steps;
  const bool b16 = form == Conv1U8Form::Rwb;
  const int threads = b16 ? kC1U8bThreads : kC1U8Threads;
  const int grid = conv1::conv1_u8_rw_grid(pool, threads, b16 ? kC1U8bPerCU : kC1U8PerCU, curla_cu_count());
  if (b16)
    return dispatch_int<9, 6, 3>(a.C, [&](auto cc) { return launch(conv1_u8_rwb_fwd_kernel<cc()>, grid, threads, 0, st, ra); });
  return dispatch_int<9, 12, 6, 3>(a.C, [&](auto cc) { return launch(conv1_u8_rw_fwd_kernel<cc()>, grid, threads, 0, st, ra); });
}

// uint8 ring, crop staged as bytes in LDS: Conv1U8Form::Hybrid / Band
static int launch_conv1_u8_band(Conv1U8Form form, Conv1Args& a, hipStream_t st) {
  const size_t lds = plan_conv1_u8_band(a);
  const int grid = (a.B + a.B2) * a.nbands;
  if (form == Conv1U8Form::Hybrid) {  // (nbands == 1: one workgroup per sample)
    rw::Geom G;
    G.Hi = a.Hc, G.Wi = a.Wc, G.Ho = a.Ho, G.Wo = a.Wo;
    rw::plan_units(G, a.Ho, a.Wo, 16);
    return dispatch_int<9, 12, 6, 3>(a.C, [&](auto cc) { return launch(conv1_u8_walk_kernel<cc()>, grid, 512, lds, st, a, G); });
  }
  return dispatch_int<9, 12, 6, 3>(a.C, [&](auto cc) { return launch(conv1_fwd_u8_kernel<cc()>, grid, 512, lds, st, a); });
}

// float NHWC minibatch, row walk with nothing staged (conv1_rw.h): Conv1F32Form::Rw
static int launch_conv1_rw(const Conv1Args& a, hipStream_t st) {
  rw::Conv1Args ra;
  ra.src = static_cast<const float*>(a.src), ra.w = a.w, ra.bias = a.bias, ra.out = a.out;
  ra.B = a.B, ra.Hc = a.Hc, ra.Wc = a.Wc, ra.Ho = a.Ho, ra.Wo = a.Wo, ra.scale = a.scale;
  ra.g.Hi = a.Hc, ra.g.Wi = a.Wc, ra.g.Ho = a.Ho, ra.g.Wo = a.Wo;
  rw::plan_units(ra.g, a.Ho, a.Wo, 16);
  const int grid = std::min(a.B, curla_cu_count());
  return dispatch_int<12, 9, 6, 3>(a.C, [&](auto cc) { return launch(conv1_rw_fwd_kernel<cc()>, grid, 512, 0, st, ra); });
}

// any source, band staged as floats in LDS (Conv1F32Form::Band): two workgroups per CU so one stages while the other
// computes
static int launch_conv1_band(int src_kind, Conv1Args& a, hipStream_t st) {
  a.th = plan_band_conv1(a.Ho, a.Wo, a.Wc, a.C, 0, conv1::kConv1F32BandBudget);
  a.nbands = (a.Ho + a.th - 1) / a.th;
  const size_t lds = conv1::f32_band_lds(a.th, a.Wc, a.C, conv1::conv1_weight_image_bytes(a.C));
  const int grid = std::min(a.B * a.nbands, 2 * curla_cu_count());
  return dispatch_int<9, 12, 6, 3>(a.C, [&](auto cc) {
    return dispatch_src(src_kind, [&](auto src) { return launch(conv1_fwd_kernel<src(), cc()>, grid, 512, lds, st, a); });
  });
}

static int conv1_fwd_impl(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                          const float* w, const float* bias, float* out, int B, int C, int Hs, int Ws, int Hc, int Wc,
                          int channels, float scale, void* stream, const Conv1Second* second) {
  CURLA_REQUIRE(w && bias && out);
  int rc = conv1_common_check(src, src_kind, B, C, Hs, Ws, Hc, Wc);
  if (rc != CURLA_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (second && src_kind != kSrcU8Ring) return CURLA_ERR_UNSUPPORTED;
  if (channels != 32) {  // generic width (conv_generic.h): the second minibatch, if any, as a launch of its own
    rc = gen_fwd1(gen_src(src, src_kind, idx, h1, w1, C, Hs, Ws, Hc, Wc, scale), w, bias, out, B, channels, st);
    if (rc == CURLA_OK && second)
      rc = gen_fwd1(gen_src(src, src_kind, second->idx, second->h1, second->w1, C, Hs, Ws, Hc, Wc, scale), second->w,
                    second->bias, second->out, second->B, channels, st);
    return rc;
  }
  Conv1Args a;
  a.src = src, a.idx = idx, a.h1 = h1, a.w1 = w1, a.w = w, a.bias = bias, a.out = out;
  a.B = B, a.C = C, a.Hs = Hs, a.Ws = Ws, a.Hc = Hc, a.Wc = Wc;
  a.Ho = (Hc - 3) / 2 + 1, a.Wo = (Wc - 3) / 2 + 1;
  a.scale = scale;
  a.dbg = ABL_HOST;
  a.idx2 = second ? second->idx : nullptr, a.h1_2 = second ? second->h1 : nullptr, a.w1_2 = second ? second->w1 : nullptr;
  a.w2 = second ? second->w : nullptr, a.bias2 = second ? second->bias : nullptr, a.out2 = second ? second->out : nullptr;
  a.B2 = second ? second->B : 0;
  if (src_kind == kSrcU8Ring) {
    switch (const Conv1U8Form form = select_conv1_u8_form(C, Hs, Ws, Wc, B + a.B2, a.Ho, a.Wo)) {
      case Conv1U8Form::Rwb:
      case Conv1U8Form::Rw: return launch_conv1_u8_rw(form, a, st);
      case Conv1U8Form::Hybrid:
      case Conv1U8Form::Band:
        if (!(ABL_HOST & 128)) return launch_conv1_u8_band(form, a, st);
        break;  // (timing-only ablation: the ring through the float band below)
    }
  } else if (select_conv1_f32_form(src_kind, C, Hc, Wc) == Conv1F32Form::Rw) {
    return launch_conv1_rw(a, st);
  }
  return launch_conv1_band(src_kind, a, st);
}

int curla_conv1_fwd(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                    const float* w, const float* bias, float* out, int B, int C, int Hs, int Ws, int Hc, int Wc,
                    int channels, float scale, void* stream) {
  return conv1_fwd_impl(src, src_kind, idx, h1, w1, w, bias, out, B, C, Hs, Ws, Hc, Wc, channels, scale, stream, nullptr);
}

int curla_conv1_fwd2(const uint8_t* ring, const int64_t* idx, const int32_t* h1, const int32_t* w1, const float* w,
                     const float* bias, float* out, int B, const int64_t* idx2, const int32_t* h1_2,
                     const int32_t* w1_2, const float* w2, const float* bias2, float* out2, int B2, int C, int Hs, int Ws,
                     int Hc, int Wc, int channels, float scale, void* stream) {
  CURLA_REQUIRE(w2 && bias2 && out2 && B2 > 0);
  Conv1Second sec{idx2, h1_2, w1_2, w2, bias2, out2, B2};
  return conv1_fwd_impl(ring, kSrcU8Ring, idx, h1, w1, w, bias, out, B, C, Hs, Ws, Hc, Wc, channels, scale, stream, &sec);
}

// workspace (floats) the weight-gradient kernels need for their per-workgroup slabs
size_t curla_conv_wgrad_workspace_floats(int cin) {
  return (size_t)4 * curla_cu_count() * ((size_t)32 * cin * 9 + 32);  // at most four workgroups (slabs) per CU
}

static int launch_wgrad_s1(const float* in, const float* g, float* workspace, int B, int Hi, int Wi, int channels,
                           hipStream_t st, int* nslabs) {
  CURLA_REQUIRE(in && g && workspace && B > 0 && Hi >= 3 && Wi >= 3);
  if (channels != 32) return gen_wgrad_s1(in, g, workspace, B, Hi, Wi, channels, st, nslabs);
  if (!rw_supported(Hi, Wi)) return CURLA_ERR_UNSUPPORTED;
  CURLA_REQUIRE(aligned16(in) && aligned16(g));
  const rw::WgradArgs ra = wgrad_args(in, g, workspace, B, Hi, Wi, Hi - 2, Wi - 2);
  *nslabs = std::min(B, 2 * curla_cu_count());
  return launch(wgrad_rw_kernel, *nslabs, 256, kPartialS1 * sizeof(float), st, ra);
}

// dW, db = the sum of `nslabs` slabs of [nw | channels] floats
static int launch_wgrad_reduce(const float* workspace, int nslabs, int nw, int channels, float* dw, float* db, hipStream_t st) {
  return launch(wgrad_reduce_kernel, (nw + channels + 31) / 32, 1024, 0, st, workspace, nslabs, nw, channels, dw, db);
}

int curla_conv3x3_s1_wgrad(const float* in, const float* g, float* dw, float* db, float* workspace, int B, int Hi,
                           int Wi, int channels, void* stream) {
  CURLA_REQUIRE(dw && db);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int nslabs = 0;
  const int rc = launch_wgrad_s1(in, g, workspace, B, Hi, Wi, channels, st, &nslabs);
  if (rc != CURLA_OK) return rc;
  return launch_wgrad_reduce(workspace, nslabs, channels * channels * 9, channels, dw, db, st);
}

int curla_conv3x3_s1_wgrad_slabs(const float* in, const float* g, float* workspace, int B, int Hi, int Wi, int channels,
                                 int* nslabs, void* stream) {
  CURLA_REQUIRE(nslabs);
  return launch_wgrad_s1(in, g, workspace, B, Hi, Wi, channels, static_cast<hipStream_t>(stream), nslabs);
}

int curla_conv3x3_s1_bwd_slabs(const float* in, const float* g, const float* w, float* gin, float* workspace, int B, int Hi,
                               int Wi, int channels, int* nslabs, void* stream) {
  CURLA_REQUIRE(in && g && w && gin && workspace && nslabs && B > 0 && Hi >= 3 && Wi >= 3);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (channels != 32) {  // generic width: the two gradients as two launches
    const int rc = gen_wgrad_s1(in, g, workspace, B, Hi, Wi, channels, st, nslabs);
    return rc != CURLA_OK ? rc : gen_dgrad(g, w, in, gin, B, Hi - 2, Wi - 2, channels, st);
  }
  CURLA_REQUIRE(aligned16(in) && aligned16(g) && aligned16(w) && aligned16(gin));
  const int Ho = Hi - 2, Wo = Wi - 2;
  if (!rw_supported(Hi, Wi)) return CURLA_ERR_UNSUPPORTED;
  const S1Form form = select_s1_form();
  if (form == S1Form::F43) {
    // the data gradient with Winograd F(4,3) runs one wave per SIMD: it cannot share a launch with the weight gradient
    const int rc = launch_wgrad_s1(in, g, workspace, B, Hi, Wi, channels, st, nslabs);
    return rc != CURLA_OK ? rc : launch_dgrad(form, g, w, in, gin, B, Ho, Wo, st);
  }
  // Weight gradient and data gradient of the layer in ONE launch (both only read the layer's output gradient): the
  // first n workgroups run the weight-gradient body, the next n the data-gradient body (f23, or b3 on the bf16 matrix
  // cores), each owning samples k, k + n, ... (the two do about the same number of MFMAs per sample).
  const int per_cu = select_bwd_shape(form, B, Ho, Wo) == BwdShape::SideBySide ? 1 : 2;
  const int n = std::min(B, per_cu * curla_cu_count());
  const rw::WgradArgs wr = wgrad_args(in, g, workspace, B, Hi, Wi, Ho, Wo);
  const rw::Args dr = rw_dgrad_args(form, g, w, in, gin, B, Ho, Wo);
  const size_t lds = std::max<size_t>(s1_filter_bytes(form), kPartialS1 * sizeof(float));
  *nslabs = n;
  return launch(form == S1Form::B3 ? bwd_rwb2_kernel : bwd_rw2_kernel, 2 * n, 256, lds, st, wr, dr, n);
}

int curla_wgrad_reduce_multi(int njobs, const float* const* slabs, const int* nslabs, const int* nw, const int* nb,
                             float* const* dw, float* const* db, void* stream) {
  CURLA_REQUIRE(njobs > 0 && njobs <= kMaxReduceJobs && slabs && nslabs && nw && dw && db);
  ReduceJobs J;
  int blocks = 0;
  for (int j = 0; j < njobs; ++j) {
    CURLA_REQUIRE(slabs[j] && dw[j] && db[j] && nslabs[j] > 0 && nw[j] > 0);
    J.partial[j] = slabs[j], J.dw[j] = dw[j], J.db[j] = db[j], J.nslabs[j] = nslabs[j], J.nw[j] = nw[j];
    J.nb[j] = nb ? nb[j] : 32;
    CURLA_REQUIRE(J.nb[j] > 0);
    J.first_block[j] = blocks;
    blocks += (nw[j] + J.nb[j] + 31) / 32;
  }
  J.first_block[njobs] = blocks;
  J.njobs = njobs;
  return launch(wgrad_reduce_multi_kernel, blocks, 1024, 0, static_cast<hipStream_t>(stream), J);
}

static int launch_wgrad1(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                         const float* g, float* workspace, int B, int C, int Hs, int Ws, int Hc, int Wc, int channels,
                         float scale, void* stream, int* nslabs) {
  CURLA_REQUIRE(g && workspace);
  const int rc = conv1_common_check(src, src_kind, B, C, Hs, Ws, Hc, Wc);
  if (rc != CURLA_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (channels != 32)
    return gen_wgrad1(gen_src(src, src_kind, idx, h1, w1, C, Hs, Ws, Hc, Wc, scale), g, workspace, B, channels, st, nslabs);
  CURLA_REQUIRE(aligned16(g));
  Wgrad1Args a;
  a.src = src, a.idx = idx, a.h1 = h1, a.w1 = w1, a.g = g, a.partial = workspace;
  a.B = B, a.C = C, a.Hs = Hs, a.Ws = Ws, a.Hc = Hc, a.Wc = Wc;
  a.Ho = (Hc - 3) / 2 + 1, a.Wo = (Wc - 3) / 2 + 1;
  a.scale = scale;
  a.lds_bytes = 0;
  a.dbg = ABL_HOST;
  const size_t slab_bytes = conv1::wgrad1_slab_bytes(C);
  int& grid = *nslabs;  // one slab per workgroup
  if (src_kind == kSrcU8Ring && !(ABL_HOST & 256)) {
    // uint8 ring, input band kept as bytes
    const Wgrad1U8Form form = select_wgrad1_u8_form(C, Wc, a.Wo);
    const size_t lds = plan_wgrad1_u8(a, form);
    grid = std::min(B * a.nbands, (form == Wgrad1U8Form::F32FourWave ? 4 : 2) * curla_cu_count());
    switch (form) {
      case Wgrad1U8Form::B16:
        return dispatch_int<9, 6, 3>(C, [&](auto cc) { return launch(wgrad1_u8b_kernel<cc(), 8>, grid, 512, lds, st, a); });
      case Wgrad1U8Form::F32FourWave:
        return dispatch_int<9, 12, 6, 3>(C, [&](auto cc) { return launch(wgrad1_u8_kernel<cc(), 4>, grid, 256, lds, st, a); });
      default:
        return dispatch_int<9, 12, 6, 3>(C, [&](auto cc) { return launch(wgrad1_u8_kernel<cc(), 8>, grid, 512, lds, st, a); });
    }
  }
  if (src_kind != kSrcU8Ring && select_conv1_f32_form(src_kind, C, Hc, Wc) == Conv1F32Form::Rw) {
    // float NHWC minibatch: row walk, nothing staged (conv1_rw.h)
    rw::Wgrad1Args ra;
    ra.src = static_cast<const float*>(src), ra.g = g, ra.partial = workspace;
    ra.B = B, ra.Hc = Hc, ra.Wc = Wc, ra.Ho = a.Ho, ra.Wo = a.Wo, ra.scale = scale;
    ra.gg.Hi = Hc, ra.gg.Wi = Wc, ra.gg.Ho = a.Ho, ra.gg.Wo = a.Wo;
    rw::plan_units(ra.gg, a.Ho, a.Wo, 4);
    grid = std::min(B, curla_cu_count());
    return dispatch_int<12, 9, 6, 3>(C, [&](auto cc) { return launch(wgrad1_rw_kernel<cc()>, grid, 512, slab_bytes, st, ra); });
  }
  // any source, band staged as floats in LDS: input rows only, one workgroup per CU
  a.th = plan_band_conv1(a.Ho, a.Wo, Wc, C, 0, conv1::kWgrad1F32BandBudget);
  a.nbands = (a.Ho + a.th - 1) / a.th;
  const size_t lds = conv1::f32_band_lds(a.th, Wc, C, slab_bytes);
  grid = std::min(B * a.nbands, curla_cu_count());
  return dispatch_int<9, 12, 6, 3>(C, [&](auto cc) {
    return dispatch_src(src_kind, [&](auto s) { return launch(wgrad1_kernel<s(), cc()>, grid, 512, lds, st, a); });
  });
}

int curla_conv1_wgrad(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                      const float* g, float* dw, float* db, float* workspace, int B, int C, int Hs, int Ws, int Hc,
                      int Wc, int channels, float scale, void* stream) {
  CURLA_REQUIRE(dw && db);
  int nslabs = 0;
  const int rc = launch_wgrad1(src, src_kind, idx, h1, w1, g, workspace, B, C, Hs, Ws, Hc, Wc, channels, scale, stream, &nslabs);
  if (rc != CURLA_OK) return rc;
  return launch_wgrad_reduce(workspace, nslabs, channels * C * 9, channels, dw, db, static_cast<hipStream_t>(stream));
}

int curla_conv1_wgrad_slabs(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                            const float* g, float* workspace, int B, int C, int Hs, int Ws, int Hc, int Wc, int channels,
                            float scale, int* nslabs, void* stream) {
  CURLA_REQUIRE(nslabs);
  return launch_wgrad1(src, src_kind, idx, h1, w1, g, workspace, B, C, Hs, Ws, Hc, Wc, channels, scale, stream, nslabs);
}

}  // extern "C"

#include "conv1_dgrad.h"  // curla_conv1_dgrad: the observation gradient of the differentiable encoder
