/* curla_hip.h -- C ABI of libcurla_hip.so: the MI355X (gfx950) kernels behind the
 * CURL/SAC learner hot path of paulvantieghem/curla.
 *
 * The reference has no native layer (it is pure PyTorch); what each entry point
 * replaces is therefore the ATen work dispatched by the cited reference lines
 * (paths relative to the reference checkout).  The boundary is deliberately
 * plain C: device pointers, sizes, a hipStream_t passed as void*.  No torch
 * types, no exceptions across the boundary, no allocation, no host sync -- every
 * call only enqueues kernels on `stream`, so callers may capture them into a
 * hipGraph.  Return value: CURLA_OK or a negative CURLA_ERR_* code.
 *
 * Layouts:
 *   activations        float32 NHWC  [B][H][W][32]
 *   replay frames      uint8   NHWC  [capacity][H][W][C]   (C = 3 * frame_stack)
 *   conv weights       float32 OIHW  (the reference's Parameter layout)
 *   dense weights      float32 [out][in] row-major (nn.Linear layout); the encoder
 *                      fc weight has its input columns in (y,x,c) order
 *   twin-Q tensors     two equally shaped blocks separated by a `twin_stride`
 *                      (floats; at least one block's length, else CURLA_ERR_ARG
 *                      before any launch)
 */
#ifndef CURLA_HIP_H
#define CURLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CURLA_OK 0
#define CURLA_ERR_ARG (-1)         /* null / misaligned pointer, non-positive size */
#define CURLA_ERR_LAUNCH (-2)      /* HIP reported a launch/attribute error */
#define CURLA_ERR_UNSUPPORTED (-3) /* shape outside what the kernels are built for (cf. NotImplementedError, encoder.py:47) */

const char* curla_version(void);

/* The C ABI's number: bumped whenever an entry point's argument list changes (round 4 put dyn / dyn64 / rng_dev
 * pointers into the middle of the Adam and policy-head calls: 4 -> 5 names that; 7 adds the autograd path's
 * curla_conv1_dgrad and curla_policy_head_bwd; 8 the batched acting path's curla_stage_frames_u8).  A binding written
 * for another number must refuse the library -- curla_amd/_lib.py does -- instead of calling with shifted arguments.
 * curla_noisy_cover_rng is a purely ADDITIVE entry point: no existing argument list moves, so a version-8 binding
 * calls a library that has it exactly as before and the number stays 8; a binding that needs it and meets an older
 * version-8 library fails at symbol lookup (curla_amd/_lib.py resolves every name when it loads), loudly, not with
 * shifted arguments. */
#define CURLA_ABI_VERSION 8
int curla_abi_version(void);

/* Run-time kernel-selection options (curla_amd/csrc/options.h).  Every option's default is the measured-best path;
 * the other values are fallbacks for shapes the default does not take or A/B partners for measurements, and every
 * value runs under the whole-update parity test (tests/test_gpu_switches.py).  The environment variable
 * CURLA_<NAME> sets the initial value (read once, at first use); afterwards only these calls change it.
 *   conv1_u8    auto | hybrid | band | rw | rwb   first layer from the uint8 ring (utils.py:151-166 + encoder.py:78-81); auto = rwb
 *                                      (LDS-free row walk on the bf16 matrix cores: a uint8 pixel is exact in bf16) where 3 C <= 32, else rw
 *   conv1_f32   rw | band              first layer and its weight gradient from a float NHWC minibatch
 *   s1_fwd      auto | f23 | f43 | b3  stride-1 forward / data gradient: Winograd F(2,3) or F(4,3) along x on the f32-input MFMA, or
 *                                      b3 (= auto): fp32 operands as three bf16 parts on the bf16 matrix cores behind F(2,3)
 *   bwd_split   auto | 0 | 1           stride-1 backward: 2 + 2 workgroups per CU, or 1 + 1 side by side
 *   gemm_tile   auto | 6464 | 6432 | 3232 | 12864   tile of the tiled GEMM (12864: the 128 x 64 bf16x3 tile wherever it applies)
 *   linear_bwd  pair | split           dW and dx of a linear layer in one launch or two
 *   gemm_mfma   auto | f32 | b3        arithmetic of the tiled GEMM (and of the encoder fc forward: bf16x3 unless f32): f32 = the
 *                                      f32-input MFMA; b3 = interior aligned tiles with fp32
 *                                      operands as three bf16 parts on the bf16 matrix cores, split once when a tile is staged;
 *                                      auto = b3 on 128 x 64 tiles where those give every CU a workgroup, f32 elsewhere
 *   s1_wgrad    auto | x | xy          stride-1 weight gradient: Winograd F(3,2) along x, or (auto) in both directions (2 x 2 gradient
 *                                      blocks: a third fewer f32 matrix instructions)
 *   wgrad1_u8   auto | f32 | b16       first-layer weight gradient from the uint8 ring: on the f32-input MFMA, or (auto, where
 *                                      3 C <= 32 and output rows hold >= 8 pixels) on the bf16 matrix cores -- a uint8 pixel is
 *                                      exact in one bf16, the gradient is split into three: nothing is dropped
 * curla_set_option returns CURLA_ERR_ARG for an unknown name or value; curla_get_option NULL for an unknown name. */
int curla_set_option(const char* name, const char* value);
const char* curla_get_option(const char* name);

/* ---- encoder convolutions (encoder.py:54-63 construction, :77-90 forward) ---- */

/* First layer: 3x3 stride 2, C -> 32, + bias + ReLU, with the minibatch assembly
 * fused into the load.  src_kind = 1: `src` is the uint8 replay ring
 * [N][Hs][Ws][C]; sample b reads frame idx[b] (NULL: b) cropped at
 * (h1[b], w1[b]) (NULL: 0) to Hc x Wc -- replaces utils.py:151-166 (gather,
 * RandomCrop.training_augmentation augmentations.py:47-75, .float()) and
 * encoder.py:78 (`obs / 255.`, pass scale = 1/255).  src_kind = 0: `src` is the
 * reference's float NCHW tensor [B][C][Hc][Wc] in [0,255]; src_kind = 2: a float
 * NHWC tensor [B][Hc][Wc][C] in [0,255] (what curla_color_jiggle / curla_noisy_cover
 * write).  C in {3, 6, 9, 12}.  The uint8 ring must be followed by >= 32 readable bytes (the row loader reads
 * whole aligned 16-byte runs) and start on a 4-byte boundary; frames may have any size. */
int curla_conv1_fwd(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                    const float* w, const float* bias, float* out, int B, int C, int Hs, int Ws, int Hc, int Wc,
                    int channels, float scale, void* stream);
/* The same for the first layer, both minibatches gathered from one uint8 ring (src_kind 1 of curla_conv1_fwd). */
int curla_conv1_fwd2(const uint8_t* ring, const int64_t* idx, const int32_t* h1, const int32_t* w1, const float* w,
                     const float* bias, float* out, int B, const int64_t* idx2, const int32_t* h1_2,
                     const int32_t* w1_2, const float* w2, const float* bias2, float* out2, int B2, int C, int Hs, int Ws,
                     int Hc, int Wc, int channels, float scale, void* stream);

/* Layers 2..L: 3x3 stride 1, 32 -> 32, + bias + ReLU (encoder.py:59-63,84-87). */
int curla_conv3x3_s1_fwd(const float* in, const float* w, const float* bias, float* out, int B, int Hi, int Wi,
                         int channels, void* stream);
/* Two forwards of the same geometry in ONE launch, each with its own weights (e.g. a minibatch through the online
 * encoder and another through the target encoder, curl_sac.py:350-358, 408-409): the second problem's items follow the
 * first's in the persistent grid and a workgroup re-builds its weight registers once.  A launch carries 4-9 us of
 * fixed cost at these sizes, so two 512-sample launches are slower than one of 1024. */
int curla_conv3x3_s1_fwd2(const float* in, const float* w, const float* bias, float* out, int B, const float* in2,
                          const float* w2, const float* bias2, float* out2, int B2, int Hi, int Wi, int channels,
                          void* stream);
/* The whole stack of stride-1 layers of one or two minibatches (B2 = 0: one) in ONE launch: layer l maps
 * [B][Hi-2l][Wi-2l][32] (in for l = 0, out[l-1] after) to out[l] with w[l], bias[l].  Every activation is written to HBM
 * as by the single-layer calls.  Needs B and B2 to be multiples of curla_conv3x3_s1_stack_granule() (a workgroup of the
 * persistent grid then owns its samples through all layers and only has to wait for itself); CURLA_ERR_UNSUPPORTED
 * otherwise -- fall back to one curla_conv3x3_s1_fwd2 per layer. */
int curla_conv3x3_s1_fwd_stack(int nlayers, const float* in, const float* const* w, const float* const* bias,
                               float* const* out, int B, const float* in2, const float* const* w2,
                               const float* const* bias2, float* const* out2, int B2, int Hi, int Wi, int channels,
                               void* stream);
/* Batch-size multiple curla_conv3x3_s1_fwd_stack needs: the size of its persistent grid on the current device (one
 * workgroup per CU in the row-walk form, two in the banded one). */
int curla_conv3x3_s1_stack_granule(void);

/* Autograd of the above (what critic_loss.backward() / loss.backward() run,
 * curl_sac.py:366,417).  `g` is the gradient w.r.t. the layer's pre-activation
 * (already ReLU-masked).  dgrad writes the pre-activation gradient of the layer
 * below: conv_transpose(g, w) zeroed where act_below <= 0. */
int curla_conv3x3_s1_dgrad(const float* g, const float* w, const float* act_below, float* gin, int B, int Ho, int Wo,
                           int channels, void* stream);
int curla_conv3x3_s1_wgrad(const float* in, const float* g, float* dw, float* db, float* workspace, int B, int Hi,
                           int Wi, int channels, void* stream);
int curla_conv1_wgrad(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                      const float* g, float* dw, float* db, float* workspace, int B, int C, int Hs, int Ws, int Hc,
                      int Wc, int channels, float scale, void* stream);
/* The weight-gradient kernels alone: every workgroup leaves its partial sums as one slab in `workspace` (*nslabs of
 * them, each 32*cin*9 + 32 floats) and nothing is reduced yet.  A backward pass runs one of these per conv layer, each
 * into its own workspace, and ONE curla_wgrad_reduce_multi at the end sums all layers' slabs (fixed order) into their
 * dW / db -- the per-layer reductions of curla_conv3x3_s1_wgrad / curla_conv1_wgrad would each be a launch of their
 * own.  njobs <= 8; nw[j] = channels*cin*9 of job j, nb[j] = its bias count = channels (NULL: 32 each).
 * FILTER COUNTS OTHER THAN 32 (the reference is generic in num_filters, encoder.py:54-63 / train.py:84): every conv
 * entry point above and below takes `channels` in 4 .. 256 (a multiple of 4); 32 runs the gfx950 row-walk kernels,
 * anything else plain direct convolutions on the vector ALU (csrc/conv_generic.h) -- the same results to fp32 rounding,
 * one to two orders of magnitude slower; their weight-gradient slabs are ONE slab of channels*cin*9 + channels floats.
 * curla_conv3x3_s1_fwd_stack stays 32-only (CURLA_ERR_UNSUPPORTED: one curla_conv3x3_s1_fwd / _fwd2 per layer). */
int curla_conv3x3_s1_wgrad_slabs(const float* in, const float* g, float* workspace, int B, int Hi, int Wi, int channels,
                                 int* nslabs, void* stream);
int curla_conv1_wgrad_slabs(const void* src, int src_kind, const int64_t* idx, const int32_t* h1, const int32_t* w1,
                            const float* g, float* workspace, int B, int C, int Hs, int Ws, int Hc, int Wc, int channels,
                            float scale, int* nslabs, void* stream);
/* Weight gradient (slabs, as curla_conv3x3_s1_wgrad_slabs) AND data gradient (as curla_conv3x3_s1_dgrad, ReLU mask =
 * the layer's input `in`) of one stride-1 layer in ONE launch: both only read the output gradient g. */
int curla_conv3x3_s1_bwd_slabs(const float* in, const float* g, const float* w, float* gin, float* workspace, int B, int Hi,
                               int Wi, int channels, int* nslabs, void* stream);
/* Gradient w.r.t. a float observation of the first (stride-2) layer (encoder.py:78,82: conv(obs / 255)):
 * dobs[n][c][y][x] = scale * sum g[n][oy][ox][o] * w[o][c][ky][kx] over y = 2 oy + ky, x = 2 ox + kx.  g = the layer's
 * pre-activation output gradient, NHWC [B][Ho][Wo][channels] (16-byte aligned; already ReLU-masked); w = OIHW weight;
 * dobs = float NCHW [B][C][H][W], every element written (pixels no output reaches are 0).  C in {3, 6, 9, 12},
 * channels a multiple of 4 up to 256 (32: one filter chunk per thread, others chunks of 4; csrc/conv1_dgrad.h).
 * The differentiable encoder's input gradient (curla_amd/autograd.py); update() never calls it. */
int curla_conv1_dgrad(const float* g, const float* w, float* dobs, int B, int C, int H, int W, int channels,
                      float scale, void* stream);
int curla_wgrad_reduce_multi(int njobs, const float* const* slabs, const int* nslabs, const int* nw, const int* nb,
                             float* const* dw, float* const* db, void* stream);
/* floats of `workspace` the two wgrad entry points need (per-workgroup partial slabs) */
size_t curla_conv_wgrad_workspace_floats(int cin);

/* ---- dense layers: encoder fc (encoder.py:66,98), actor trunk (curl_sac.py:70-74),
 * twin Q (curl_sac.py:129-139), CURL bilinear logits (curl_sac.py:219-220) ----
 * C[z] = epilogue(alpha * opA(A[z]) * opB(B[z])^T); a_kmajor/b_kmajor = operand is
 * stored [K][rows]; epilogue = +bias[n], ReLU, zero where mask <= 0.  ksplit > 1
 * writes partial products C + s*split_stride (no epilogue; reduce with
 * curla_splitk_reduce or curla_fc_ln_fwd). */
int curla_gemm(const float* A, int a_kmajor, int lda, long long strideA, const float* B, int b_kmajor, int ldb,
               long long strideB, float* C, int ldc, long long strideC, int M, int N, int K, int nbatch, int ksplit,
               long long split_stride, float alpha, const float* bias, long long strideBias, int relu,
               const float* mask, int ldmask, long long strideMask, void* stream);
/* Products with a small output and a long k (ceil(M/32) * ceil(N/32) * nbatch <= 128 tiles, K >= 256, K % 64 == 0, no
 * epilogue, no split) are computed by one workgroup per 16 x 16 tile whose waves split k; 1 if the shape qualifies. */
int curla_gemm_small_shape(int M, int N, int K, int nbatch);
/* Such a product plus colsum[z][m] = sum_k opA(A[z])[m][k] from the same launch -- a layer's weight gradient dy^T x
 * [N_out x N_in] with its bias gradient, the column sums of dy (curl_sac.py:70-74,129-133 backward): the workgroups
 * of the first column of tiles add up the A operands they load anyway.  Needs curla_gemm_small_shape(...);
 * CURLA_ERR_UNSUPPORTED otherwise. */
int curla_gemm_colsum(const float* A, int a_kmajor, int lda, long long strideA, const float* B, int b_kmajor, int ldb,
                      long long strideB, float* C, int ldc, long long strideC, int M, int N, int K, int nbatch,
                      float* colsum, long long strideColsum, void* stream);
/* Backward of a batched linear layer y = x W^T (curl_sac.py:70-74, 129-133: the hidden and first layers of the actor
 * trunk and of the twin Q functions) in ONE launch where the two products take the same kernel family, two otherwise:
 *   dW[z][n][k] = sum_b dy[z][b][n] x[z][b][k]          (db[z][n] = sum_b dy[z][b][n] when db != NULL: needs
 *                                                        curla_gemm_small_shape(N, K, B, nbatch), else UNSUPPORTED)
 *   dx[z][b][k] = sum_n dy[z][b][n] W[z][n][k], zeroed where mask[z][b][k] <= 0 (mask may be NULL)
 * dy [B][N], x / mask / dx [B][K], W / dW [N][K] row-major, batch strides in floats (0 = shared). */
int curla_linear_bwd(const float* dy, long long stride_dy, const float* x, long long stride_x, const float* W,
                     long long stride_W, const float* mask, long long stride_mask, float* dW, long long stride_dW,
                     float* db, long long stride_db, float* dx, long long stride_dx, int B, int N, int K, int nbatch,
                     void* stream);
/* curla_gemm with a two-level batch: item (outer, inner) at base + inner * stride + outer * stride2 (no split-K).  The
 * twin Q functions of the target critic and of the critic are one such batch of four: the twins a block apart inside a
 * flat parameter buffer, the two flat buffers wherever the allocator put them (curl_sac.py:353-358). */
int curla_gemm_nested(const float* A, int a_kmajor, int lda, long long strideA, long long strideA2, const float* B,
                      int b_kmajor, int ldb, long long strideB, long long strideB2, float* C, int ldc, long long strideC,
                      long long strideC2, int M, int N, int K, int nbatch, int nbatch2, float alpha, const float* bias,
                      long long strideBias, long long strideBias2, int relu, const float* mask, int ldmask,
                      long long strideMask, long long strideMask2, void* stream);
/* nprob <= 4 unrelated products of ONE shape in one launch, operands by pointer: C_i (+ split partials) =
 * A_i [M][K] * B_i [N][K]^T, no epilogue -- the fc layers of several encoders on several activation tensors (the
 * critic phase has three, curl_sac.py:350-358).  Each launch less is ~5 us. */
int curla_gemm_multi(int nprob, const float* const* A, const float* const* B, float* const* C, int lda, int ldb, int ldc,
                     int M, int N, int K, int ksplit, long long split_stride, void* stream);
/* The encoder fc layer's forward product as split-K partial sums, for up to four (x, W) pairs of one shape:
 * partial[i][s][b][f] = sum over the k of split s (32-wide slices, nsplit near-equal runs of them) of x[i][b][k] W[i][f][k],
 * split s at partial[i] + s * split_stride.  W [F][K] row-major; x [B][K] row-major (x_blocked = 0) or BLOCKED
 * [B / 16][K / 32][16][32] (x_blocked = 1: element (b, k) at ((b / 16) (K / 32) + k / 32) 512 + (b % 16) 32 + k % 32).
 * 50 <= F <= 64 even, B % 128 == 0, K % 32 == 0; other shapes: CURLA_ERR_UNSUPPORTED (curla_gemm_multi computes the same
 * sums from a row-major x in another order). */
int curla_fc_fwd_multi(int nprob, const float* const* x, const float* const* W, float* const* partial, int B, int F, int K,
                       int nsplit, long long split_stride, int x_blocked, void* stream);
int curla_splitk_reduce(const float* partial, int nsplit, long long split_stride, int M, int N, int ldp, float* C,
                        int ldc, const float* bias, int relu, void* stream);
/* Backward of the encoder fc layer z = fc(h) (encoder.py:98; autograd of the reference's nn.Linear), F <= 64 features,
 * K % 4 == 0 columns, 16-byte aligned matrices; CURLA_ERR_UNSUPPORTED otherwise (use curla_gemm):
 *   curla_fc_dx: dx[b][n] = (mask == NULL || mask[b][n] > 0) * sum_f dz[b][f] W[f][n]   (W [F][K] as stored by
 *                nn.Linear; mask = h, the ReLU output of the last conv layer: its backward fused in)
 *   curla_fc_dw: dW[f][n] = sum_b dz[b][f] x[b][n]
 * One workgroup per 64 columns, operands streamed from HBM/L2 straight into MFMA registers, 256-byte row pieces. */
int curla_fc_dx(const float* dz, const float* W, const float* mask, float* dx, int B, int F, int K, void* stream);
int curla_fc_dw(const float* dz, const float* x, float* dW, int B, int F, int K, void* stream);
/* Both at once (x doubles as the ReLU mask of dx: h = relu(conv) is the fc layer's input): one launch whose first
 * workgroups compute dx and whose rest compute dW. */
int curla_fc_bwd(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                 void* stream);
/* curla_fc_bwd / curla_fc_dw that also finish the LayerNorm parameter gradients curla_ln_bwd_partial left as partial sums
 * (dgamma[f], dbeta[f], dbias_in[f] = sum over the nparts partials, in order; dbias_in may be NULL). */
int curla_fc_bwd_ln(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                    const float* ln_partial, int nparts, float* dgamma, float* dbeta, float* dbias_in, void* stream);
int curla_fc_dw_ln(const float* dz, const float* x, float* dW, int B, int F, int K, const float* ln_partial, int nparts,
                   float* dgamma, float* dbeta, float* dbias_in, void* stream);
/* curla_fc_bwd_ln that also finishes a second set of partial sums in the same extra workgroup:
 * extra_out[i] = sum over p < extra_parts of extra_partial[p * extra_len + i] (the CURL head's dW partials). */
int curla_fc_bwd_ln2(const float* dz, const float* W, const float* x, float* dx, float* dW, int B, int F, int K,
                     const float* ln_partial, int nparts, float* dgamma, float* dbeta, float* dbias_in,
                     const float* extra_partial, int extra_parts, int extra_len, float* extra_out, void* stream);

/* Last layer of the actor trunk / the Q functions (curl_sac.py:73-74, 132-133): hidden -> N outputs, N <= 16
 * (Q: 1, actor: 2|A|), batched over `nbatch` identically laid-out networks `stride*` floats apart.
 *   fwd: out[z][m][n] = bias[z][n] + sum_k h[z][m][k] W[z][n][k]                       (K % 4 == 0)
 *   bwd: dh[z][m][k] = (h[z][m][k] > 0) * sum_n dy[z][m][n] W[z][n][k]   (ReLU mask of the layer below fused)
 *        dW[z][n][k] = sum_m dy[z][m][n] h[z][m][k]                      (dW may be NULL: data gradient only) */
int curla_mlp_out_fwd(const float* h, long long strideH, const float* W, long long strideW, const float* bias,
                      long long strideBias, float* out, long long strideOut, int M, int N, int K, int nbatch,
                      void* stream);
int curla_mlp_out_fwd_nested(const float* h, long long strideH, long long strideH2, const float* W, long long strideW,
                             long long strideW2, const float* bias, long long strideBias, long long strideBias2,
                             float* out, long long strideOut, long long strideOut2, int M, int N, int K, int nbatch,
                             int nbatch2, void* stream);
int curla_mlp_out_bwd(const float* dy, long long strideDy, const float* h, long long strideH, const float* W,
                      long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int M, int N,
                      int K, int nbatch, void* stream);
/* ... and (each optional) the bias gradient of this layer, db_out[z][n] = sum_m dy[z][m][n], and of the layer below,
 * db_hidden[z][k] = sum_m dh[z][m][k]; both with batch stride strideDb */
int curla_mlp_out_bwd_bias(const float* dy, long long strideDy, const float* h, long long strideH, const float* W,
                           long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int M, int N,
                           int K, int nbatch, float* db_out, float* db_hidden, long long strideDb, void* stream);

/* One problem of curla_fc_ln_fwd_multi (fields as curla_fc_ln_fwd's arguments; fc_out, xhat, rstd, xa, act optional;
 * xa without act: only the feature columns of the rows are written). */
typedef struct CurlaFcLnJob {
  const float *partial, *bias, *gamma, *beta;
  float *fc_out, *y, *xhat, *rstd, *xa;
  const float* act;
  int tanh_out;
} CurlaFcLnJob;
/* curla_mlp_out_bwd_bias for the twin Q functions' last layer (one output, two twins `twin_stride` floats apart in q /
 * target_q_twin / dq) with the output gradient computed in place of being read: the launch of the loss kernel that
 * would produce it goes away, its scalar results are written by the same launch.
 *   kind 1 (update_critic, curl_sac.py:350-362, = curla_critic_td_loss): target = reward + not_done * discount *
 *           (min(target_q_twin) - alpha * log_pi); dq = 2 (q - target) / B; scalars[0] = the critic loss; target_q [B]
 *   kind 2 (update_actor_and_alpha, curl_sac.py:378-399, = curla_actor_loss): dq = d(-min(Q1, Q2))/dQ / B;
 *           scalars[0..3] = actor loss, alpha loss, entropy, alpha; *dlog_alpha = d(alpha loss)/d(log_alpha)
 * dq [2][twin_stride] is also written out (bias-gradient fallbacks, tests). */
typedef struct CurlaLossArgs {
  int kind, A;
  long long twin_stride;
  const float *q, *target_q_twin, *log_pi, *reward, *not_done, *log_std;
  const double* log_alpha;
  double* dlog_alpha;
  float *target_q, *scalars, *dq;
  float discount, target_entropy;
} CurlaLossArgs;
int curla_mlp_out_bwd_loss(const CurlaLossArgs* loss, const float* h, long long strideH, const float* W,
                           long long strideW, float* dh, long long strideDh, float* dW, long long strideDW, int B, int K,
                           float* db_out, float* db_hidden, long long strideDb, void* stream);
/* fc split-K reduce + bias + LayerNorm(eps) [+ tanh] (encoder.py:98-107).  Saves
 * xhat / rstd for the backward when non-NULL.  F <= 256.  `xa` (optional, with `act` [B][A]): also writes the Q
 * functions' input rows xa[b] = [ y[b] | act[b] ], i.e. torch.cat([obs, action], dim=1) (curl_sac.py:138). */
int curla_fc_ln_fwd(const float* partial, int nsplit, long long split_stride, int ldp, const float* bias,
                    const float* gamma, const float* beta, int B, int F, float eps, float* fc_out, float* y,
                    float* xhat, float* rstd, int tanh_out, float* xa, const float* act, int A, void* stream);
/* up to 4 such problems of one shape (same B, F, nsplit, strides, eps, A) in one launch: the features of several
 * encoders over their own split-K partials (actor / target critic / critic, curl_sac.py:350-358) */
int curla_fc_ln_fwd_multi(int njobs, const CurlaFcLnJob* jobs, int nsplit, long long split_stride, int ldp, int B,
                          int F, float eps, int A, void* stream);
/* dx, and (when non-NULL) dgamma, dbeta; dbias_in (optional, needs dgamma/dbeta) = column sums of dx = the gradient of
 * the fc bias feeding the LayerNorm */
int curla_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int B, int F, float* dx,
                 float* dgamma, float* dbeta, float* dbias_in, void* stream);
/* The same with the incoming gradient the sum of two strided row blocks dy[b*ld_dy + f] + dy2[b*ld_dy + f] (dy2 may
 * be NULL): the two halves of the twin-Q input gradient [2][B][F + A], torch.cat's backward (curl_sac.py:138), read in
 * place. */
int curla_ln_bwd_twin(const float* dy, const float* dy2, int ld_dy, const float* xhat, const float* rstd,
                      const float* gamma, int B, int F, float* dx, float* dgamma, float* dbeta, float* dbias_in,
                      void* stream);
/* curla_ln_bwd_twin without the launch that finishes the parameter gradients: dx as above, and per-workgroup partial sums
 * of dgamma / dbeta / the fc bias gradient into `partial` ([*nparts][3][F] floats, *nparts = ceil(B / 4)).  The fc
 * backward that follows (curla_fc_bwd_ln / curla_fc_dw_ln) adds them up in one extra workgroup of its own launch. */
int curla_ln_bwd_partial(const float* dy, const float* dy2, int ld_dy, const float* xhat, const float* rstd,
                         const float* gamma, int B, int F, float* dx, float* partial, int* nparts, void* stream);
/* LayerNorm(eps) + ReLU behind a hidden layer of the Q functions' MLPs, in place: the reference's trunk
 * (curl_sac.py:129-139) extended to Linear - LayerNorm - ReLU per hidden layer (CurlSacAgent(critic_layer_norm=True)).
 * h[o][z] [B][H] at h + z * strideH + o * strideH2 (z < nbatch twins, o < nbatch2 groups of twins) holds the Linear's
 * output, bias included, and receives relu(xhat * gamma[o][z] + beta[o][z]); gamma / beta [H] at
 * + z * strideP + o * strideP2, addressed like the weights of curla_gemm_nested.  xhat / rstd (both or neither; NULL:
 * a no-grad pass writes neither): saved for the groups o >= save_first only, dense, xhat[o - save_first][z][B][H] and
 * rstd[o - save_first][z][B] (0 <= save_first < nbatch2: the groups in front are no-grad passes in the same launch, the
 * target critic's).  One wave per row; H <= 1024, CURLA_ERR_UNSUPPORTED above.  CURLA_ERR_ARG on a NULL h / gamma / beta,
 * B < 1, H < 1, nbatch < 1, nbatch2 < 1, one of xhat / rstd without the other, save_first out of range.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_mlp_ln_relu_fwd(float* h, long long strideH, long long strideH2, const float* gamma, const float* beta,
                          long long strideP, long long strideP2, float* xhat, float* rstd, int save_first, int B, int H,
                          int nbatch, int nbatch2, float eps, void* stream);
/* Its backward (curl_sac.py:129-139 as extended above), in place: dh[z] [B][H] at dh + z * strideDh arrives as the
 * gradient of the LayerNorm's output, the ReLU's mask already applied by the layer behind (whose mask is h > 0 with h the
 * post-LayerNorm activation), and leaves as the gradient of the Linear's output,
 * rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = dh * gamma[z]; xhat [nbatch][B][H], rstd [nbatch][B] dense as
 * the forward saved them, gamma [H] at + z * strideP.  dgamma, dbeta, dbias ([H] at + z * strideG; all three with
 * `partial`, or all four NULL: the data gradient only) = sum_b dh_in * xhat, sum_b dh_in, sum_b dh_out -- the last is
 * the bias gradient of the Linear in front.  `partial`: nbatch * ceil(B / 4) * 3 * H floats of workspace; a workgroup's
 * four rows are added in row order and a second small launch adds the workgroups' sums in order: no atomics, the
 * same bits run to run.  H <= 1024, CURLA_ERR_UNSUPPORTED above.  CURLA_ERR_ARG on a NULL dh / xhat / rstd / gamma,
 * B < 1, H < 1, nbatch < 1, or some but not all of partial / dgamma / dbeta / dbias.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_mlp_ln_bwd(float* dh, long long strideDh, const float* xhat, const float* rstd, const float* gamma,
                     long long strideP, int B, int H, int nbatch, float* partial, float* dgamma, float* dbeta,
                     float* dbias, long long strideG, void* stream);
/* curla_mlp_ln_relu_fwd with DroQ's dropout in front of the LayerNorm (CurlSacAgent(critic_layer_norm=True,
 * critic_dropout=p): the trunk of curl_sac.py:129-139 as Linear - Dropout(p) - LayerNorm - ReLU per hidden layer):
 * h receives relu(LN(m * h * s)), s = 1.0f / (1.0f - p), and xhat / rstd are those of the dropped activation.  The keep
 * mask m is not stored; element (twin z, row r, feature f) of group o is kept where u >= p, with
 * u = (word >> 8) * 2^-24 and word = output (f >> 6) & 3 of Philox4x32-10 under the key `seed` on the counter
 * (e & 0xffffffff, e >> 32, counter & 0xffffffff, (((counter >> 32) << 8) | (tag + 2 o)) & 0xffffffff),
 * e = ((z * B + r) * ceil(H / 256) + (f >> 8)) * 64 + (f & 63).  rng_dev (NULL, or 8-byte aligned device memory): seed
 * and counter are rng_dev[0] and rng_dev[1], read when the kernel RUNS (captured graphs), and the two by-value arguments
 * are ignored.  The arguments in front of p and their rules are curla_mlp_ln_relu_fwd's; in addition CURLA_ERR_ARG on
 * p outside [0, 1), tag outside 1..255, tag + 2 (nbatch2 - 1) > 255, a misaligned rng_dev.  CURLA_ERR_UNSUPPORTED on
 * H > 1024; an argument error comes first.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_mlp_drop_ln_relu_fwd(float* h, long long strideH, long long strideH2, const float* gamma, const float* beta,
                               long long strideP, long long strideP2, float* xhat, float* rstd, int save_first, int B,
                               int H, int nbatch, int nbatch2, float eps, float p, unsigned long long seed,
                               unsigned long long counter, const unsigned long long* rng_dev, int tag, void* stream);
/* Its backward (curl_sac.py:129-139 as extended above), in place: curla_mlp_ln_bwd with the mask of the forward call
 * under the same (p, seed, counter or rng_dev, tag) computed again; dh leaves as the gradient of the Linear's output,
 * m * s times the gradient of the LayerNorm's input, and dbias sums THAT; dgamma and dbeta as without dropout.  A row
 * that was dropped entirely leaves as exact zeros.  No mask buffer, no atomics: the same bits run to run.  The
 * arguments in front of p and their rules are curla_mlp_ln_bwd's; in addition CURLA_ERR_ARG on p outside [0, 1), tag
 * outside 1..255, a misaligned rng_dev.  CURLA_ERR_UNSUPPORTED on H > 1024; an argument error comes first.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_mlp_drop_ln_bwd(float* dh, long long strideDh, const float* xhat, const float* rstd, const float* gamma,
                          long long strideP, int B, int H, int nbatch, float* partial, float* dgamma, float* dbeta,
                          float* dbias, long long strideG, float p, unsigned long long seed, unsigned long long counter,
                          const unsigned long long* rng_dev, int tag, void* stream);
/* out[z][n] = sum_m X[z][m][n] (bias gradients) */
int curla_colsum(const float* X, int M, int N, int ldx, long long strideX, float* out, long long strideOut, int nbatch,
                 void* stream);

/* the three bias gradients of a (batched) 3-layer MLP backward in one launch: out_i[z][n] = sum_m X_i[z][m][n],
 * X_i dense [nbatch][M][N_i], out_i batches `strideOut` floats apart (curl_sac.py:70-74,129-133 backward) */
int curla_colsum3(const float* X0, int N0, const float* X1, int N1, const float* X2, int N2, int M, float* out0,
                  float* out1, float* out2, long long strideOut, int nbatch, void* stream);

/* ---- squashed-Gaussian policy head (curl_sac.py:20-35, 87-108) ----
 * trunk_out [B][2A] = [mu | raw log_std]; `noise` replaces torch.randn_like
 * (curl_sac.py:97); NULL noise = compute_pi False (select_action).  `pi_xa` (optional, with noise): pi is also
 * (or, with pi NULL, only) written at pi_xa[b * xa_ld + a] -- the action columns of the Q functions' input rows
 * [features | action] (curl_sac.py:138, 353). */
int curla_actor_head_fwd(const float* trunk_out, const float* noise, int B, int A, float log_std_min,
                         float log_std_max, float* mu, float* pi, float* log_pi, float* log_std, float* tanh_ls,
                         float* pi_xa, int xa_ld, void* stream);
/* The actor trunk's last layer and the policy head in one launch (curl_sac.py:79-108): trunk_out [B][2A] =
 * h [B][K] @ W [2A][K]^T + bias is written out and the head's outputs follow from it as in curla_actor_head_fwd
 * (2A <= 16, K % 4 == 0; CURLA_ERR_UNSUPPORTED otherwise). */
int curla_mlp_out_head_fwd(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                           const float* noise, float log_std_min, float log_std_max, float* mu, float* pi,
                           float* log_pi, float* log_std, float* tanh_ls, float* pi_xa, int xa_ld, void* stream);
/* The two forms above with the standard-normal noise of `torch.randn_like(mu)` (curl_sac.py:97) drawn INSIDE the launch
 * instead of read: element i = b * A + a is Box-Muller on outputs (i % 4) & 2, + 1 of Philox4x32-10 with key `seed` and
 * counter `offset + i / 4` (cos branch for even i, sin for odd), and is also stored to noise_out [B][A] (the backward
 * pass reads it).  The caller advances `offset` by ceil(B A / 4) per call.  rng_dev != NULL (8-byte aligned device
 * memory): seed = rng_dev[0] and offset = rng_dev[1] are read when the kernel RUNS and the by-value pair is ignored -- a
 * captured hipGraph is replayed with new stream positions (CurlSacAgent.enable_update_graphs). */
int curla_actor_head_fwd_rng(const float* trunk_out, float* noise_out, unsigned long long seed,
                             unsigned long long offset, const unsigned long long* rng_dev, int B, int A,
                             float log_std_min, float log_std_max, float* mu, float* pi, float* log_pi, float* log_std,
                             float* tanh_ls, float* pi_xa, int xa_ld, void* stream);
int curla_mlp_out_head_fwd_rng(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                               float* noise_out, unsigned long long seed, unsigned long long offset,
                               const unsigned long long* rng_dev, float log_std_min, float log_std_max, float* mu,
                               float* pi, float* log_pi, float* log_std, float* tanh_ls, float* pi_xa, int xa_ld,
                               void* stream);
/* gradient w.r.t. trunk_out of sum(gpi*pi) + glp*log_pi; glp = glp_rows[b] or glp_scale*exp(*log_alpha);
 * gpi[b][a] is read at gpi[b*gpi_ld + a] (+ gpi2[b*gpi_ld + a] when gpi2 is not NULL: the action columns of the twin-Q
 * input gradient summed over the twin in place) */
int curla_actor_head_bwd(const float* gpi, const float* gpi2, int gpi_ld, const float* glp_rows, const double* log_alpha,
                         float glp_scale, const float* noise, const float* pi, const float* log_std,
                         const float* tanh_ls, int B, int A, float log_std_min, float log_std_max, float* dtrunk_out,
                         void* stream);
/* General backward of the squashed-Gaussian head (curl_sac.py:20-35 gaussian_logprob / squash, :87-108 forward): the
 * gradient w.r.t. trunk_out [B][2A] = [mu | raw log_std] of sum(dmu*mu + dpi*pi + dlog_std*log_std) + sum_b
 * dlog_pi[b]*log_pi[b] for the outputs curla_actor_head_fwd wrote -- mu = tanh(mu), log_std rescaled from tanh (:85-87),
 * pi = tanh(mu + noise*std), log_pi with squash's log(relu(1 - pi^2) + 1e-6) correction (:32).  noise is a constant.
 * Any of dmu, dpi, dlog_pi (length B), dlog_std may be NULL (= zero).  Needs tanh_ls always, mu when dmu is given, and
 * noise / pi / log_std when dpi or dlog_pi is (the saved forward outputs).  The autograd path (curla_amd/autograd.py). */
int curla_policy_head_bwd(const float* dmu, const float* dpi, const float* dlog_pi, const float* dlog_std,
                          const float* noise, const float* mu, const float* pi, const float* log_std,
                          const float* tanh_ls, int B, int A, float log_std_min, float log_std_max, float* dtrunk_out,
                          void* stream);

/* ---- deterministic policy head (DrQ-v2; CurlSacAgent(policy="deterministic")) ----
 * trunk_out [B][A] = o, the A pre-squash means (no log_std half).  With s = *std, a float32 read from DEVICE memory when
 * the kernel runs (a schedule of s is data: a captured hipGraph never holds it), c = clip >= 0 (+inf: none) and
 * lim = float32(1 - 1e-6):   mu = tanh(o);   pi = clamp(mu + clamp(s noise, -c, c), -lim, lim);   log_pi[b] = 0;
 * log_std = log(s) (the float32 nearest to it).  Every output is optional as in curla_actor_head_fwd, pi_xa / xa_ld and
 * NULL noise (mu and log_std only) likewise.  The _rng forms draw the noise inside the launch from the stream of
 * curla_actor_head_fwd_rng -- same counters, same rng_dev -- and store it to noise_out.  The mlp_out forms run the
 * actor trunk's last layer h [B][K] @ W [A][K]^T + bias in the same launch (K % 4 == 0; CURLA_ERR_UNSUPPORTED otherwise)
 * and write the same bits as the two-launch form.  CURLA_ERR_ARG before any launch: A < 1 or A > 8, B < 1, a NULL
 * trunk_out / std (h / W; noise_out in the _rng forms), clip < 0 or NaN.  No atomics: a rerun writes the same bits.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_det_head_fwd(const float* trunk_out, const float* noise, const float* std, float clip, int B, int A, float* mu,
                       float* pi, float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream);
int curla_det_head_fwd_rng(const float* trunk_out, float* noise_out, unsigned long long seed, unsigned long long offset,
                           const unsigned long long* rng_dev, const float* std, float clip, int B, int A, float* mu,
                           float* pi, float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream);
int curla_mlp_out_det_head_fwd(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                               const float* noise, const float* std, float clip, float* mu, float* pi, float* log_pi,
                               float* log_std, float* pi_xa, int xa_ld, void* stream);
int curla_mlp_out_det_head_fwd_rng(const float* h, const float* W, const float* bias, float* trunk_out, int B, int A, int K,
                                   float* noise_out, unsigned long long seed, unsigned long long offset,
                                   const unsigned long long* rng_dev, const float* std, float clip, float* mu, float* pi,
                                   float* log_pi, float* log_std, float* pi_xa, int xa_ld, void* stream);
/* dtrunk_out [B][A] = gpi (1 - mu^2): the gradient of sum(gpi*pi) through the head above -- straight through the outer
 * clamp, the noise a constant.  gpi is addressed as curla_actor_head_bwd's (gpi_ld, gpi2: the twin's action columns in
 * place); mu is the forward's output. */
int curla_det_head_bwd(const float* gpi, const float* gpi2, int gpi_ld, const float* mu, int B, int A, float* dtrunk_out,
                       void* stream);
/* The general form (curla_amd/autograd.py): dtrunk_out = (dmu + dpi)(1 - mu^2), dmu / dpi [B][A], either may be NULL. */
int curla_det_policy_head_bwd(const float* dmu, const float* dpi, const float* mu, int B, int A, float* dtrunk_out,
                              void* stream);

/* torch.cat([z, action], 1) (curl_sac.py:138) and its backward summed over the twin */
int curla_concat(const float* z, const float* act, int B, int F, int A, float* xa, void* stream);
int curla_split_sum(const float* dxa, long long twin_stride, int B, int F, int A, float* dz, float* dact,
                    void* stream);

/* ---- SAC targets and losses ---- */
/* target_Q = r + not_done*discount*(min(tq1,tq2) - exp(log_alpha)*log_pi) (curl_sac.py:353-355) */
int curla_td_target(const float* tq, long long twin_stride, const float* log_pi, const float* reward,
                    const float* not_done, const double* log_alpha, float discount, int B, float* target_q,
                    void* stream);
/* loss = mse(q1,tQ)+mse(q2,tQ) and dq = dloss/dq (curl_sac.py:359) */
int curla_critic_loss(const float* q, long long twin_stride, const float* target_q, int B, float* loss, float* dq,
                      void* stream);
/* the two above in one launch: target_Q from the target critic's `tq`, then the loss and dq of the critic's `q` */
int curla_critic_td_loss(const float* q, const float* tq, long long twin_stride, const float* log_pi,
                         const float* reward, const float* not_done, const double* log_alpha, float discount, int B,
                         float* target_q, float* loss, float* dq, void* stream);
/* curla_critic_td_loss over two augmented views of every transition (DrQ, Kostrikov et al. 2021, K = 2 and M = 2): B is
 * even and positions b and b + B/2 are one transition under two augmentations.  Each position's target is formed as
 * above, the pair's mean tbar = 0.5 (t_b + t_{b+B/2}) is written to both places of target_q, loss = (1 / (B/2)) * the
 * sum over all B positions and both twins of (q - tbar)^2 (the two views' MSEs over B/2 transitions, summed) and dq =
 * 2 (q - tbar) / (B/2).  One workgroup, fixed-order sums, nothing written between the twins' blocks.  CURLA_ERR_ARG on
 * a NULL pointer, B < 2, an odd B or twin_stride < B.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_critic_td_loss_views(const float* q, const float* tq, long long twin_stride, const float* log_pi,
                               const float* reward, const float* not_done, const double* log_alpha, float discount,
                               int B, float* target_q, float* loss, float* dq, void* stream);
/* actor_loss, alpha_loss, entropy, alpha -> scalars4; dq = d actor_loss/dq; dlog_alpha (float64 like the
 * reference's log_alpha, curl_sac.py:292) (curl_sac.py:378-399) */
int curla_actor_loss(const float* q, long long twin_stride, const float* log_pi, const float* log_std, int A,
                     const double* log_alpha, float target_entropy, int B, float* scalars4, float* dq,
                     double* dlog_alpha, void* stream);
/* Truncated quantile critics (Kuznetsov et al. 2020) in place of curla_critic_td_loss, for Q functions with M output
 * atoms (curl_sac.py:129-139 with a last layer of M rows; q, tq, dq are [2][B][M], their twins the given element strides
 * apart, each >= B M).  Per row: the 2M atoms of `tq` are pooled and ranked (ties in index order), the K = 2 (M - d)
 * smallest kept, y_j = reward + not_done * discount * (z'_(j) - exp(log_alpha) * log_pi); with u = y_j - q[n][b][i],
 * tau_i = (2 i + 1) / (2 M), w = |tau_i - [u < 0]| and the Huber loss h (0.5 u^2 for |u| <= 1, |u| - 0.5 beyond):
 * row_loss[b] = sum_{n,i,j} w h(u) / (2 M K), dq[n][b][i] = -sum_j w clamp(u, -1, 1) / (B 2 M K), and `loss` (may be
 * NULL) the fixed-order mean of row_loss.  No atomics: a rerun writes the same bits.  CURLA_ERR_ARG on a NULL required
 * pointer, B < 1, M < 1, M > 32 (the 2M pooled atoms of a row are one wave's lanes), d < 0, d >= M or a stride below B M.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_tqc_critic_loss(const float* q, long long q_twin_stride, const float* tq, long long tq_twin_stride,
                          const float* log_pi, const float* reward, const float* not_done, const double* log_alpha,
                          float discount, int B, int M, int d, float* dq, long long dq_twin_stride, float* row_loss,
                          float* loss, void* stream);
/* curla_actor_loss for Q functions with M output atoms (curl_sac.py:129-139 with a last layer of M rows): the row's Q
 * term is the mean of its 2M atoms (no min), dq[n][b][i] = -1 / (2 M B) everywhere; scalars4 and dlog_alpha as
 * curla_actor_loss leaves them.  CURLA_ERR_ARG on a NULL required pointer, B < 1, A < 1, M < 1, M > 32 or a stride
 * below B M.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_tqc_actor_loss(const float* q, long long q_twin_stride, const float* log_pi, const float* log_std, int A,
                         const double* log_alpha, float target_entropy, int B, int M, float* scalars4, float* dq,
                         long long dq_twin_stride, double* dlog_alpha, void* stream);
/* The categorical HL-Gauss critic (Imani & White 2018; Farebrother et al. 2024) in place of curla_critic_td_loss, for Q
 * functions whose last layer outputs M logits over the bins of [v_min, v_max] (q, tq, dq are [2][B][M], their twins the
 * given element strides apart, each >= B M).  w = (v_max - v_min) / M, edges e_j = v_min + j w, centres
 * c_j = v_min + (j + 1/2) w, Q = sum_j softmax(l)_j c_j.  Per row b: y = reward + not_done * discount *
 * (min(Q'_0, Q'_1) - exp(log_alpha) * log_pi) from the target logits `tq`; with views != 0 (B even, H = B / 2) positions
 * p and p + H both take 0.5 (y_p + y_{p+H}), one value bit for bit; y is clamped to [v_min, v_max] and written to
 * target_q[b]; t_j = (Phi((e_{j+1} - y) / sigma) - Phi((e_j - y) / sigma)) / (Phi((e_M - y) / sigma) - Phi((e_0 - y) / sigma));
 * row_loss[b] = -sum_n sum_j t_j log_softmax(q[n][b])_j, dq[n][b][j] = (softmax(q[n][b])_j - t_j) / N and `loss` (may be
 * NULL) = sum_b row_loss[b] / N in a fixed order, N = B (H with views).  No atomics: a rerun writes the same bits.
 * CURLA_ERR_ARG on a NULL required pointer, B < 1, M < 2, M > 256, a non-finite bound, v_min >= v_max, sigma <= 0 or not
 * finite, a stride below B M, views not 0 or 1, or views with an odd B.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_hlg_critic_loss(const float* q, long long q_twin_stride, const float* tq, long long tq_twin_stride,
                          const float* log_pi, const float* reward, const float* not_done, const double* log_alpha,
                          float discount, int B, int M, float v_min, float v_max, float sigma, int views, float* dq,
                          long long dq_twin_stride, float* target_q, float* row_loss, float* loss, void* stream);
/* curla_actor_loss for the same Q functions: Q_n = sum_j softmax(q[n][b])_j c_j, the row's Q term min(Q_0, Q_1), written
 * to row_q[b] (a [B] scratch the scalars are then summed from in a fixed order); dq[n][b][j] = g_n p_{n,j} (c_j - Q_n)
 * with curla_actor_loss's g_n (-1 / B for the smaller network, -0.5 / B each on an exact tie, 0 for the larger); scalars4
 * and dlog_alpha (may be NULL) as curla_actor_loss leaves them.  CURLA_ERR_ARG on a NULL required pointer, B < 1, A < 1,
 * M < 2, M > 256, a non-finite bound, v_min >= v_max or a stride below B M.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_hlg_actor_loss(const float* q, long long q_twin_stride, const float* log_pi, const float* log_std, int A,
                         const double* log_alpha, float target_entropy, int B, int M, float v_min, float v_max,
                         float* row_q, float* scalars4, float* dq, long long dq_twin_stride, double* dlog_alpha,
                         void* stream);
/* CrossEntropyLoss(logits, arange(B)) and d/dlogits (curl_sac.py:221,411-413); `loss` (the mean of row_loss) may be
 * NULL when the scalar is not going to be logged */
int curla_curl_ce(const float* logits, int B, int ld, float* row_loss, float* loss, float* dlogits, void* stream);
/* curla_curl_ce for a minibatch of two augmented views per transition (B even): row a's partner column (a + B/2) % B
 * holds the other view of the anchor's own transition and is no negative -- it is left out of the row's logsumexp and
 * its dlogits entry is exactly 0; everything else as above (the mean is still over the B rows).  What curla_curl_ce
 * gives on logits whose partner entries are -inf, bit for bit.  CURLA_ERR_ARG on an odd B.  Additive: CURLA_ABI_VERSION
 * stays 8. */
int curla_curl_ce_views(const float* logits, int B, int ld, float* row_loss, float* loss, float* dlogits,
                        void* stream);
/* The CURL head in one launch (curl_sac.py:211-222,406-417 and their autograd), given the anchor features z_a, the
 * positives' z_pos and wz = (W z_pos^T)^T = z_pos W^T, all [B][F]: logits = z_a wz^T (optionally stored), row_loss[a] =
 * logsumexp(logits[a]) - logits[a][a] (their mean into `loss` when it is not NULL), dlogits = (softmax - I) / B
 * (optionally stored), dz = dlogits wz (optionally stored), dfc = the LayerNorm backward of dz with the anchor encoder's
 * (xhat, rstd, gamma), and per block of 16 rows the partial sums of dgamma / dbeta / fc-bias gradient (ln_partial
 * [*nparts][3][F], *nparts = B / 16) and of dW[i][k] = sum_a z_a[a][i] (dlogits z_pos)[a][k] (w_partial [*nparts][F * F]),
 * which curla_fc_bwd_ln2 adds up.  B % 128 == 0, B <= 1024, 49 <= F <= 52; else CURLA_ERR_UNSUPPORTED (the separate
 * launches compute the same quantities). */
int curla_curl_head(const float* z_a, const float* z_pos, const float* wz, const float* xhat, const float* rstd,
                    const float* gamma, int B, int F, float* row_loss, float* loss, float* dfc, float* ln_partial,
                    int* nparts, float* w_partial, float* logits, float* dlogits, float* dz, void* stream);
/* The self-predictive latent loss (SPR, Schwarzer et al. 2021; BYOL's normalised regression) of the predictor's output
 * p against the target encoder's latent t, both [B][F], forward and gradient in one kernel.  Per row b, with eps = 1e-12:
 * ph = p / max(|p|, eps), th = t / max(|t|, eps) (torch's F.normalize), row_loss[b] = sum_f (ph_f - th_f)^2 (= 2 - 2 cos
 * where neither vector is zero), `loss` (may be NULL) the fixed-order mean of row_loss, dp[b] = (2 / B) (I - ph ph^T)
 * (ph - th) / |p| for |p| >= eps and (2 / B) (ph - th) / eps below it (the clamp's branch: a zero row is defined and
 * finite); t gets no gradient.  Norms are float32 square roots of float32 sums of squares: inputs whose squares overflow or
 * underflow float32 are outside the contract; a non-finite input makes its own row's outputs non-finite and no other's.
 * One wave per row, no atomics: a rerun writes the same bits.  CURLA_ERR_ARG on a NULL required pointer, B < 1, F < 1 or
 * F > 1024.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_pred_loss(const float* p, const float* t, int B, int F, float* row_loss, float* loss, float* dp, void* stream);
int curla_mean(const float* x, int n, float* out, void* stream);

/* target <- tau*param + (1-tau)*target over a flat parameter block (utils.py:37-41) */
int curla_soft_update(const float* param, float* target, size_t n, float tau, float one_minus_tau, void* stream);
/* one flat block with two rates: elements [0, split) use tau_a, [split, n) tau_b (encoder_tau | critic_tau,
 * curl_sac.py:442-445) */
int curla_soft_update2(const float* param, float* target, size_t n, size_t split, float tau_a, float one_minus_tau_a,
                       float tau_b, float one_minus_tau_b, void* stream);
/* Shrink and perturb for network resets (Nikishin et al. 2022; D'Oro et al. 2023): one flat block with
 * curla_soft_update2's range convention -- elements [0, split) use (keep_a, new_a), [split, n) (keep_b, new_b).
 *   0 < keep < 1 : param[i] = keep * param[i] + new * fresh[i], the two products and the sum rounding once each (no
 *                  fused multiply-add); target[i] (target may be NULL) the same formula on its own old value
 *   keep == 0    : param[i] = target[i] = fresh[i] by selection: the old values are not read (a NaN does not survive)
 *   keep == 1    : the element is neither read nor written, in either array
 * The caller forms new = (float)(1 - keep) in double.  16-byte accesses when param, target and fresh are 16-byte
 * aligned, element-wise otherwise.  CURLA_ERR_ARG: a NULL param or fresh, n == 0, split > n, a keep outside [0, 1] or
 * NaN.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_shrink_perturb2(float* param, float* target, const float* fresh, size_t n, size_t split, float keep_a,
                          float new_a, float keep_b, float new_b, void* stream);

/* Dormant-neuron scores and ReDo recycling (Sokar et al. 2023) for the hidden layers of the 3-layer MLPs (the actor trunk,
 * the Q functions).  Three launches' worth of entry points; no atomics, every sum in a fixed order: a rerun writes the
 * same bits.
 * curla_dormant_colsum: sums[n][j] = sum over b of |h[n][b][j]| in float32, b in index order, for the nb networks of
 * h [nb][B][H] (post-ReLU activations; network n `h_stride` elements in, >= B H) into sums (network n `sums_stride`
 * elements in, >= H).  A launch of its own so that data-parallel ranks can add their sums up before thresholding.
 * CURLA_ERR_ARG on a NULL pointer, B < 1, H < 1, nb < 1 or a stride below the extent it spans.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_dormant_colsum(const float* h, long long h_stride, int nb, int B, int H, float* sums, long long sums_stride,
                         void* stream);
/* Per layer l of sums [L][H] (dense): total = sum_j (double) sums[l][j] in a fixed order, mean = total / H,
 * score[l][j] = (float)((double) sums[l][j] / mean), mask[l][j] (int32: 1 dormant, 0 not) = mean == 0 or
 * score[l][j] <= tau compared in float32 -- a NaN sum or total masks nothing --, count[l] (int32) the masked units and
 * fraction[l] = (float)((double) count[l] / H).  CURLA_ERR_ARG on a NULL pointer, L < 1, H < 1, tau negative or NaN.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_dormant_mask(const float* sums, int L, int H, float tau, float* score, int* mask, int* count, float* fraction,
                       void* stream);
/* ReDo's recycling over flat parameter blocks.  param, m, v (Adam's moments) and fresh share one layout; network n of
 * the nb lies `stride` elements in.  A segment is a [rows][cols] matrix (a vector: cols 1) `offset` elements into the
 * block with the mask row of its output units, row_layer, and of its input units, col_layer (-1: it has none; network n
 * takes mask rows row_layer + n * mask_twin and col_layer + n * mask_twin of mask [L][H], curla_dormant_mask's).  Per
 * element (i, j), r = the row mask of i, c = the column mask of j:
 *   c      : param = 0            (the outgoing weights of a dormant unit; zero wins where a row and a column cross)
 *   else r : param = fresh        (the incoming weights, the bias, a LayerNorm's weight / bias)
 *   else   : not written          (a stored -0.0 or NaN stays)
 * and m = v = 0 exactly where param is written.  param, m and v are never read.  16-byte accesses in a segment when the
 * four arrays and mask are 16-byte aligned and stride, its offset and cols are multiples of 4, element-wise otherwise
 * (tested per launch and per segment).  CURLA_ERR_ARG on a NULL pointer, nb < 1, H < 1, L < 1, nsegs outside
 * 1 .. CURLA_REDO_MAX_SEGS, a segment with rows < 1, cols < 1, offset < 0, a layer outside -1 .. L - 1 - (nb - 1)
 * mask_twin, rows != H under a row mask or cols != H under a column mask, mask_twin < 0, or (nb > 1) a stride below the
 * end of a segment.  Additive: CURLA_ABI_VERSION stays 8. */
#define CURLA_REDO_MAX_SEGS 12
typedef struct CurlaRedoSeg {
  long long offset;
  int rows, cols;
  int row_layer, col_layer;
} CurlaRedoSeg;
int curla_redo_recycle(float* param, float* m, float* v, const float* fresh, long long stride, int nb,
                       const CurlaRedoSeg* segs, int nsegs, const int* mask, int L, int H, int mask_twin, void* stream);

/* One torch.optim.Adam step (weight_decay 0, amsgrad off; the reference's five optimizers, curl_sac.py:299-313) over a
 * flat run of n fp32 parameters with their gradient and moment runs: replaces torch's multi-tensor Adam launches
 * (~70 workgroups on a 256-CU chip).  `step` is the 1-based count of this step; the hyper-parameters are doubles as in the
 * optimizer's param_group (the bias corrections and lr/(1-beta1^step) are evaluated in double on the host, like
 * torch's single-tensor Adam, and rounded to float once).
 * dyn != NULL (device memory, 2 floats): the two step-dependent factors -- dyn[0] = (float)(lr / (1 - beta1^step)),
 * dyn[1] = (float)sqrt(1 - beta2^step) -- are read when the kernel RUNS instead of being evaluated from `step`: a captured
 * hipGraph is replayed with new step counts (the host writes the same two floats it would have passed by value). */
int curla_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                    double beta1, double beta2, double eps, long long step, const float* dyn, void* stream);
/* curla_adam_step plus, in the same launch, the soft update of the target copy of the same flat run with the freshly
 * stepped parameters (critic_optimizer.step() ... soft_update_params x3, curl_sac.py:367,442-445): target[i] <- tau p[i]
 * + (1 - tau) target[i], elements [0, split) with (tau_a, one_minus_tau_a), the rest with (tau_b, one_minus_tau_b);
 * the same arithmetic as curla_adam_step followed by curla_soft_update2. */
int curla_adam_step_lerp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                         double beta1, double beta2, double eps, long long step, const float* dyn, float* target,
                         size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                         void* stream);
/* curla_adam_step plus, in the same launch, the Adam step of ONE float64 scalar parameter with its own optimizer state
 * and hyper-parameters (log_alpha, stepped right after the actor: curl_sac.py:393-404), in double.  dyn64 (device memory,
 * 2 doubles, or NULL): the scalar's two step-dependent factors, as `dyn` for the flat run. */
int curla_adam_step_scalar64(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                             double beta1, double beta2, double eps, long long step, const float* dyn, double* param64,
                             const double* grad64, double* exp_avg64, double* exp_avg_sq64, double lr64, double beta1_64,
                             double beta2_64, double eps64, long long step64, const double* dyn64, void* stream);
/* A float64 scalar riding in a float32 all-reduce bucket (data parallel: log_alpha's gradient inside the actor's bucket
 * instead of an 8-byte collective of its own; the reference has no counterpart -- its one float64
 * parameter is curl_sac.py:284-286, stepped at :404).  curla_f64_pack writes *value as CURLA_F64_WORDS float32 words:
 * signed 20-bit fixed-point digits, most significant first, digit j worth 2^(8 - 20 j); exact for |value| < 2^28 (larger
 * magnitudes, inf and nan travel in word 0 alone, inexactly).  Sums of the words over <= 16 ranks are exact in float32.
 * curla_f64_unpack: *value = RN(sum of (words[j] * n_mul) * 2^(8 - 20 j)) / n_div with ONE rounding of the exact sum --
 * n_mul undoes an average taken by the collective (ncclAvg: n_mul = world size), n_div = world size gives the mean. */
#define CURLA_F64_WORDS 8
int curla_f64_pack(const double* value, float* words, void* stream);
int curla_f64_unpack(const float* words, double n_mul, double n_div, double* value, void* stream);
/* Two such steps of two optimizers on the same parameters with the same gradient, one after the other, in one pass
 * (encoder_optimizer.step(); cpc_optimizer.step(), curl_sac.py:418-423).  exp_avg2 / exp_avg_sq2 cover n elements, the
 * first n_pre of which (CURL.W) take the second step only; exp_avg1 / exp_avg_sq1 cover the remaining n - n_pre.
 * dyn (device memory, 4 floats, or NULL): (lr1 / (1 - beta1_1^step1), sqrt(1 - beta2_1^step1)) then the same for the
 * second optimizer, as in curla_adam_step. */
int curla_adam_step2(float* param, const float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2,
                     float* exp_avg_sq2, size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1, double eps1,
                     long long step1, double lr2, double beta1_2, double beta2_2, double eps2, long long step2,
                     const float* dyn, void* stream);
/* Clipping by the global gradient norm inside the Adam launches: torch.nn.utils.clip_grad_norm_(params, max_norm,
 * norm_type=2.0, error_if_nonfinite=False) right in front of the optimizer's step, without a host read.
 * curla_grad_sqsum writes n_partials (1 .. CURLA_CLIP_MAX_PARTIALS) float64 partial sums of squares of one flat gradient
 * run, one per workgroup: partials[b] = sum of grad[i]^2 over workgroup b's grid-stride share, accumulated in double in a
 * fixed order (no atomics: the partials are a function of the gradient's bytes, n, n_partials and whether `grad` is
 * 16-byte aligned).  A step over several runs calls it once per run, with disjoint slots of ONE partials buffer.
 * The four curla_adam_step*_clip entry points are their namesakes with four more arguments in front of `stream`: the
 * partials of ALL the runs of the step and their total count, max_norm (> 0; inf allowed) and a two-float stats slot.
 * Every workgroup sums the partials in the same fixed order, in double: norm = sqrt(sum), coef = min(1, max_norm /
 * (norm + 1e-6)) rounded to float once.  coef != 1: grad[i] <- coef * grad[i] (one rounding; written back, so the
 * gradient buffer afterwards holds what Adam consumed, as with torch) and the step runs on the result -- in
 * curla_adam_step2_clip both steps; coef == 1: nothing is written to `grad` and the step is the unclipped one, bit for
 * bit.  A non-finite norm propagates as in torch.  stats[0] = (float)norm (before clipping), stats[1] = coef.
 * CURLA_ERR_ARG before any launch on: a NULL pointer (dyn / dyn64 may be NULL), a float pointer off 4 bytes, a double
 * pointer off 8, n == 0, n_partials outside 1 .. CURLA_CLIP_MAX_PARTIALS, max_norm <= 0 or NaN, and whatever the
 * unclipped namesake refuses.  Additive: CURLA_ABI_VERSION stays 8. */
#define CURLA_CLIP_MAX_PARTIALS 256
int curla_grad_sqsum(const float* grad, size_t n, double* partials, int n_partials, void* stream);
int curla_adam_step_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                         double beta2, double eps, long long step, const float* dyn, const double* partials,
                         int n_partials, double max_norm, float* stats, void* stream);
int curla_adam_step_lerp_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                              double beta1, double beta2, double eps, long long step, const float* dyn, float* target,
                              size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                              const double* partials, int n_partials, double max_norm, float* stats, void* stream);
int curla_adam_step_scalar64_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                  double beta1, double beta2, double eps, long long step, const float* dyn,
                                  double* param64, const double* grad64, double* exp_avg64, double* exp_avg_sq64,
                                  double lr64, double beta1_64, double beta2_64, double eps64, long long step64,
                                  const double* dyn64, const double* partials, int n_partials, double max_norm,
                                  float* stats, void* stream);
int curla_adam_step2_clip(float* param, float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2,
                          float* exp_avg_sq2, size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1,
                          double eps1, long long step1, double lr2, double beta1_2, double beta2_2, double eps2,
                          long long step2, const float* dyn, const double* partials, int n_partials, double max_norm,
                          float* stats, void* stream);
/* Decoupled weight decay inside the Adam launches: torch.optim.AdamW, i.e. torch.optim.Adam with
 * decoupled_weight_decay=True.  The four curla_adamw_* entry points are the curla_adam_*_clip namesakes with a `double
 * weight_decay` right behind each `eps` of the flat run (curla_adamw_step2: one per optimizer; the float64 scalar's eps64
 * gets none -- the scalar belongs to another optimizer and is never decayed).  Per element: param[i] <- param[i] * d
 * first, ONE multiply with one rounding, d = (float)(1.0 - lr * weight_decay) formed here on the host in double as torch
 * forms it; then the Adam update on the decayed parameter.  The gradient, the clip coefficient and the moments do not see
 * d; the target lerp reads the stepped, decayed parameter.  curla_adamw_step2, in torch's order for first.step();
 * second.step(): elements behind n_pre take param *= d1, Adam 1, param *= d2, Adam 2; the first n_pre take param *= d2,
 * Adam 2.  So a launch equals, bit for bit, param *= d over the run followed by the namesake's launch, and with
 * weight_decay == 0 (d == 1) it equals the namesake's launch.
 * partials == NULL: the unclipped step -- n_partials must then be 0, max_norm and stats are ignored and `grad` is not
 * written.  partials != NULL: clipped, as the _clip namesake.
 * dyn / dyn64 as in the namesakes.  d is evaluated from `lr` and passed to the kernel BY VALUE; it is not part of dyn: a
 * captured hipGraph holds it, so a graph captured with weight_decay != 0 must be captured again when lr changes.
 * CURLA_ERR_ARG before any launch on: weight_decay negative, NaN or infinite; partials == NULL with n_partials != 0; and
 * whatever the _clip namesake refuses.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                     double beta2, double eps, double weight_decay, long long step, const float* dyn,
                     const double* partials, int n_partials, double max_norm, float* stats, void* stream);
int curla_adamw_step_lerp(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                          double beta2, double eps, double weight_decay, long long step, const float* dyn, float* target,
                          size_t split, float tau_a, float one_minus_tau_a, float tau_b, float one_minus_tau_b,
                          const double* partials, int n_partials, double max_norm, float* stats, void* stream);
int curla_adamw_step_scalar64(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                              double beta1, double beta2, double eps, double weight_decay, long long step,
                              const float* dyn, double* param64, const double* grad64, double* exp_avg64,
                              double* exp_avg_sq64, double lr64, double beta1_64, double beta2_64, double eps64,
                              long long step64, const double* dyn64, const double* partials, int n_partials,
                              double max_norm, float* stats, void* stream);
int curla_adamw_step2(float* param, float* grad, float* exp_avg1, float* exp_avg_sq1, float* exp_avg2, float* exp_avg_sq2,
                      size_t n, size_t n_pre, double lr1, double beta1_1, double beta2_1, double eps1,
                      double weight_decay1, long long step1, double lr2, double beta1_2, double beta2_2, double eps2,
                      double weight_decay2, long long step2, const float* dyn, const double* partials, int n_partials,
                      double max_norm, float* stats, void* stream);

/* ---- augmentations that produce float observations (augmentations.py:78-205; kornia arithmetic is not
 * vendored by the reference: PARITY UNPINNED, the algorithm is this build's statement of kornia's documented
 * behaviour, see oracle/curla_oracle.py color_jiggle / noisy_cover).  Output: float NHWC [B][H][W][C] in [0,255].
 * color_jiggle: params[B*C/3][4] = (apply, contrast, saturation, hue_radians) per RGB frame, order[4] = permutation
 * of {0 brightness (identity), 1 contrast, 2 saturation, 3 hue}.  noisy_cover: rows [0,top) and [H-bottom,H) painted
 * with (c0,c1,c2) per RGB channel, + noise (float NHWC), clamped to [0,255].  gather_nhwc: identity (u8 -> float). */
int curla_color_jiggle(const uint8_t* frames, const int64_t* idx, const float* params, const int32_t* order, int B,
                       int C, int H, int W, float* out, void* stream);
int curla_noisy_cover(const uint8_t* frames, const int64_t* idx, const float* noise, float c0, float c1, float c2,
                      int top, int bottom, int B, int C, int H, int W, float* out, void* stream);
int curla_gather_nhwc(const uint8_t* frames, const int64_t* idx, int B, int C, int H, int W, float* out, void* stream);
/* curla_noisy_cover with the noise drawn INSIDE the launch (augmentations.py:157,197: kornia's
 * RandomGaussianNoise(mean 0, std) applied after the cover is painted) -- no B H W C float noise tensor is written by
 * one launch and read back by the next.  Element i of the flat NHWC batch gets std * z_i, z_i = Box-Muller on outputs
 * (i % 4) & 2, + 1 of Philox4x32-10 with key `seed` and counter `offset + i / 4` (cos for even i, sin for odd): the
 * policy head's stream (curla_actor_head_fwd_rng).  The caller advances `offset` by ceil(B H W C / 4) per call.
 * rng_dev != NULL (8-byte aligned device memory): seed = rng_dev[0], offset = rng_dev[1] are read when the kernel RUNS
 * and the by-value pair is ignored; colors_dev != NULL (3 floats of device memory): likewise for (c0, c1, c2) -- a
 * captured hipGraph is replayed with new values.  noise_out (optional, NULL in production; float NHWC): receives
 * std * z_i, so that out equals curla_noisy_cover fed noise_out bit for bit.  Everything else as curla_noisy_cover.
 * B H W C >= 2^32: CURLA_ERR_UNSUPPORTED (elements are numbered in 32 bits).  PARITY UNPINNED for the noise stream. */
int curla_noisy_cover_rng(const uint8_t* frames, const int64_t* idx, float std, unsigned long long seed,
                          unsigned long long offset, const unsigned long long* rng_dev, float c0, float c1, float c2,
                          const float* colors_dev, int top, int bottom, int B, int C, int H, int W, float* out,
                          float* noise_out, void* stream);
/* The two augmentations on the reference's own tensor contract -- what ColorJiggle.training_augmentation(image_batch)
 * and NoisyCover.training_augmentation(image_batch) take and return (augmentations.py:105-136,170-205): float NCHW
 * [B][C][H][W] in [0,255], same arithmetic as the ring forms above; `out` may alias `in`. */
int curla_color_jiggle_nchw(const float* in, const float* params, const int32_t* order, int B, int C, int H, int W,
                            float* out, void* stream);
int curla_noisy_cover_nchw(const float* in, const float* noise, float c0, float c1, float c2, int top, int bottom,
                           int B, int C, int H, int W, float* out, void* stream);
/* RandomConv (beyond the reference: the random convolution of RAD and of Lee et al., "Network Randomization").  Every
 * sample's k = C / 3 RGB frames go through ONE 3x3, 3 -> 3 channel filter weights[b][co][ci][ky][kx] (float [B][81], 4-byte
 * aligned, device memory -- read when the kernel RUNS, so a captured hipGraph is replayed with new values):
 *   out[b][y][x][3 f + co] = sum over ci, ky, kx of  w[co][ci][ky][kx] * in[b][y + ky - 1][x + kx - 1][3 f + ci]
 * cross-correlation (no flip), `in` = 0 outside the frame, the stored bytes as floats in [0,255]; the result is NOT clamped.
 * Each output is one float32 fused-multiply-add chain from 0 over (ky, kx, ci), ky slowest: a filter of zeros and ones
 * returns bytes exactly, and the two forms below agree bit for bit.  In general |out - exact| <= g sum |w_i| |x_i| with
 * g = 27 u / (1 - 27 u), u = 2^-24.
 * curla_random_conv: uint8 NHWC ring rows idx[b] (idx == NULL: rows 0..B-1), as curla_color_jiggle takes them, to float
 * NHWC [B][H][W][C]; nothing outside the B frames is read.  Frames of 2^31 - 16 bytes or more, and rows so long that
 * the LDS image of (1024 + 2 W + 2) C bytes and the staged output of 1024 C bytes exceed 64 KiB (W > ~1700 at C = 12):
 * CURLA_ERR_UNSUPPORTED.
 * curla_random_conv_nchw: the reference's tensor contract, float NCHW in and out (RandomConv.training_augmentation).
 * Unlike the jitter this kernel reads a pixel's NEIGHBOURS: `out` must NOT alias or overlap `in` (in == out:
 * CURLA_ERR_ARG; a partial overlap is not detected).  Additive: CURLA_ABI_VERSION stays 8. */
int curla_random_conv(const uint8_t* frames, const int64_t* idx, const float* weights, int B, int C, int H, int W,
                      float* out, void* stream);
int curla_random_conv_nchw(const float* in, const float* weights, int B, int C, int H, int W, float* out, void* stream);

/* ---- replay ring helpers ---- */
/* float/uint8 NCHW crops exactly as sample_cpc returns them (utils.py:151-166) */
int curla_crop_nchw(const uint8_t* frames, const int64_t* idx, const int32_t* h1, const int32_t* w1, int B, int C,
                    int Hs, int Ws, int Hc, int Wc, float* out_f32, uint8_t* out_u8, void* stream);
/* actions / rewards / not_dones of the sampled transitions (utils.py:159-166): rows idx[b] of the ring's
 * [capacity][A+2] scalar block (action | reward | not_done) into three dense outputs */
int curla_gather_transition_scalars(const float* scalars, const int64_t* idx, int B, int A, float* action, float* reward,
                                    float* not_done, void* stream);
/* The same, fed from pinned host memory: `host_block` (device-visible address of a pinned buffer, see
 * curla_host_device_pointer) holds the minibatch's index block -- B int64 ring rows first, then whatever else the
 * caller lays out (crop offsets, utils.py:151-156), nbytes in all, a multiple of 8.  The kernel reads it over PCIe,
 * writes it to `device_block` and gathers the scalar rows: the only host->device traffic of an update, without a
 * copy-engine transfer in the stream.  The host buffer must stay untouched until the launch has executed. */
int curla_sample_stage(const void* host_block, void* device_block, long long nbytes, const float* scalars, int B, int A,
                       float* action, float* reward, float* not_done, void* stream);
/* n-step returns (beyond the reference: ReplayBuffer(n_step=n), the multi-step TD target of DrQ-v2).  `cont`: one
 * uint8 per ring row, 1 when row (r + 1) % capacity continues row r's episode.  For sample b, starting at ring row
 * r0 = idx[b] (the block's first B int64), in fp32, every product and sum rounded on its own (no FMA), in this order:
 *   R = reward[r0]; g = 1; r = r0; m = 1
 *   while m < n and cont[r]:  r = (r + 1) % capacity; g = g * discount; R = R + g * reward[r]; m += 1
 *   reward[b] = R;  not_done[b] = not_done[r] * g;  action[b][:] = action[r0][:]
 *   block int64 [B + b] = capacity + r   (the bootstrap frame's row in the double ring, next_obs half)
 *   block int64 [next_row_offset / 8 + b] = r
 * so that reward + not_done * discount * (...) of the TD kernels is the n-step target; n = 1 gives what
 * curla_gather_transition_scalars gives and idx + capacity.  curla_nstep_compose works on a `device_block` that has
 * been staged already (its words B .. 2B - 1 and the next_row words are overwritten, nothing else of it is);
 * curla_sample_stage_nstep is curla_sample_stage with the composition in the same launch (the copy leaves out the
 * words the composition writes; the row indices are read from the pinned block).  CURLA_ERR_ARG on a NULL pointer,
 * n < 1, capacity < 1, a next_row_offset that is not a multiple of 8, overlaps the 2 B index words or (staging form)
 * does not leave room for B words inside nbytes.  Rows are not range-checked: idx[b] in [0, capacity), as for the
 * gathers above.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_nstep_compose(void* device_block, long long next_row_offset, const float* scalars, const uint8_t* cont,
                        long long capacity, int n, float discount, int B, int A, float* action, float* reward,
                        float* not_done, void* stream);
int curla_sample_stage_nstep(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                             const float* scalars, const uint8_t* cont, long long capacity, int n, float discount, int B,
                             int A, float* action, float* reward, float* not_done, void* stream);
/* Temporal positives for the CURL head (beyond the reference: ReplayBuffer(pos_offset=k); the positive selection of
 * ATC, Stooke et al. 2021).  For sample b, starting at ring row r0 = idx[b] (the block's first B int64), with `cont` as
 * above:
 *   r = r0;  repeat k - 1 times: if not cont[r]: stop;  r = (r + 1) % capacity
 *   block int64 [pos_offset / 8 + b]     = r              (the positive is next_obs of row r)
 *   block int64 [pos_offset / 8 + B + b] = capacity + r   (the same row in the double ring's next_obs half)
 * and, unless run_offset is -1, one run of 3 B double-ring rows obs | next_obs | pos for a single gather of 3 B frames:
 *   block int64 [run_offset / 8 + b]         = r0
 *   block int64 [run_offset / 8 + B + b]     = capacity + (r0 walked n - 1 links the same way: the n-step bootstrap row)
 *   block int64 [run_offset / 8 + 2 B + b]   = capacity + r
 * k = 1 gives r = r0 and reads no flag.  curla_pos_walk works on a `device_block` that has been staged already (behind
 * curla_nstep_compose and curla_per_sample where they run; it reads the B idx words and writes the pos and run words,
 * nothing else); `next_row_offset` (-1: the block has none) only takes part in the checks.  curla_sample_stage_pos is
 * curla_sample_stage (next_row_offset == -1, then n must be 1) or curla_sample_stage_nstep (next_row_offset >= 0) with
 * the walk in the same launch: the copy leaves out every word a walk writes, each such word has one writer, and the
 * start rows are read from the pinned block.  k and n are unrelated.
 * CURLA_ERR_ARG before any launch on: a NULL pointer (`cont` may be NULL only when nothing reads it: k == 1 and, where n
 * is used, n == 1); k < 1, n < 1, capacity < 1; an offset (-1 aside, where allowed) that is not a multiple of 8, lies
 * inside the 2 B index words, does not leave room for its words (2 B, 3 B, B) inside nbytes (stand-alone form: inside
 * 1 GiB; the caller's block must hold them), or overlaps another of the three regions.  Rows are not range-checked.
 * Additive: CURLA_ABI_VERSION stays 8. */
int curla_pos_walk(void* device_block, long long pos_offset, long long run_offset, long long next_row_offset,
                   const uint8_t* cont, long long capacity, int k, int n, int B, void* stream);
int curla_sample_stage_pos(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                           long long pos_offset, long long run_offset, const float* scalars, const uint8_t* cont,
                           long long capacity, int n, float discount, int k, int B, int A, float* action, float* reward,
                           float* not_done, void* stream);
/* The four walks above for a ring that several environments share (ReplayBuffer(n_envs=N)): environment e owns rows
 * e, e + N, e + 2 N, ... -- a lane of stride N -- and `cont[r] == 1` means that row (r + stride) % capacity continues row
 * r's episode.  Each entry point is its namesake with `long long stride` behind `capacity`: every `(r + 1) % capacity`
 * of the definitions above reads `(r + stride) % capacity`, nothing else changes, and stride == 1 gives the namesake's
 * bits (the namesakes are these with stride 1).  CURLA_ERR_ARG before any launch on what the namesake refuses and on
 * stride < 1 or capacity % stride != 0.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_nstep_compose_strided(void* device_block, long long next_row_offset, const float* scalars, const uint8_t* cont,
                                long long capacity, long long stride, int n, float discount, int B, int A, float* action,
                                float* reward, float* not_done, void* stream);
int curla_sample_stage_nstep_strided(const void* host_block, void* device_block, long long nbytes,
                                     long long next_row_offset, const float* scalars, const uint8_t* cont,
                                     long long capacity, long long stride, int n, float discount, int B, int A,
                                     float* action, float* reward, float* not_done, void* stream);
int curla_pos_walk_strided(void* device_block, long long pos_offset, long long run_offset, long long next_row_offset,
                           const uint8_t* cont, long long capacity, long long stride, int k, int n, int B, void* stream);
int curla_sample_stage_pos_strided(const void* host_block, void* device_block, long long nbytes, long long next_row_offset,
                                   long long pos_offset, long long run_offset, const float* scalars, const uint8_t* cont,
                                   long long capacity, long long stride, int n, float discount, int k, int B, int A,
                                   float* action, float* reward, float* not_done, void* stream);
/* Proportional prioritized replay (beyond the reference: ReplayBuffer(prioritized=True); Schaul et al. 2016).
 * Storage, all on the device: `s` float [capacity], the stored value p_i^alpha of every ring row (0 = never written:
 * never drawn) | `sums` double [ceil(capacity / CURLA_PER_CHUNK)], one sum per chunk of CURLA_PER_CHUNK consecutive
 * rows | `vmax` float [1], the largest value ever given (the caller initialises it, to 1), which new transitions take.
 *
 * curla_per_set writes the values of n rows -- rows[i] (int64, device), or with rows == NULL the run first_row,
 * first_row + 1, ... modulo capacity -- to values[i], or with values == NULL to *vmax.  A row that occurs several
 * times takes the maximum of its values; values are finite and non-negative (a negative one, -0 or a NaN stores +0,
 * +inf stores FLT_MAX, so the sign bit is clear and every sum stays finite); *vmax is raised
 * to the largest given value, never lowered.  Afterwards the sum of every chunk that holds a row of the call is the
 * float64 sum of that chunk's current values in one fixed order (lane l of a wave adds rows l, l + 64, l + 128,
 * l + 192, then an xor tree 32 .. 1 over the lanes).  Up to three stream-ordered launches (clear, write, re-sum): no
 * chunk is summed before every row of the call is written.  CURLA_ERR_ARG before any launch on: s, sums or vmax NULL;
 * s, vmax or values off 4 bytes; sums or rows off 8; n < 1; capacity < 1; rows == NULL and first_row outside
 * [0, capacity).  rows[i] are not range-checked (as for the gathers above).
 *
 * curla_per_sample draws B rows: for sample k, with u = the float64 at byte u_offset + 8 k of `device_block`
 * (0 <= u < 1) and total = the sum of `sums`, the smallest row i whose cumulative sum of s exceeds u total -- strictly --,
 * cumulative sums in float64.  Found in three levels (64 runs of chunk sums, the chunks of one run, the rows of one
 * chunk), each a sequential prefix sum; the levels associate their sums differently and may round differently, and where
 * a level's walk would pass its end the last entry with a positive value is taken, so a row with s == 0 is never drawn;
 * sums that are exact in float64 (integers, say) give the rows of a sequential cumulative sum exactly.  One workgroup per sample reads ceil(capacity / CURLA_PER_CHUNK) * 8 +
 * CURLA_PER_CHUNK * 4 bytes.  Writes int64 [k] = i and [B + k] = capacity + i at the start of the block (the index run
 * every loader reads) and the float s[i] / total at byte prob_offset + 4 k.  With total == 0: row 0, probability 0.
 * CURLA_ERR_ARG before the launch on: a NULL pointer; s off 4 bytes; sums or device_block off 8; B < 1; capacity < 1;
 * u_offset not a multiple of 8 or prob_offset of 4; either inside the 16 B index bytes, not below 2^30, or the two
 * fields overlapping.
 *
 * curla_per_td, behind the critic's TD loss (q, target_q and dq as curla_critic_td_loss leaves them; prob from
 * curla_per_sample), in one launch of one workgroup:
 *   w[k] = (min_j prob[j] / prob[k])^beta;  dq[k] *= w[k], dq[twin_stride + k] *= w[k]  (beta == 0: dq keeps its bits;
 *          prob[k] == 0, which only a draw from a ring without any mass gives: w[k] = 0)
 *   loss[0] = (1/B) sum_k w[k] ((q[k] - t[k])^2 + (q[twin_stride + k] - t[k])^2)
 *   value[k] = (0.5 (|q[k] - t[k]| + |q[twin_stride + k] - t[k]|) + eps)^alpha   -- what curla_per_set then stores.
 * CURLA_ERR_ARG before the launch on: a NULL pointer or one off 4 bytes; B < 1; twin_stride < B; beta outside [0, 1];
 * eps <= 0; alpha < 0.  All three are additive: CURLA_ABI_VERSION stays 8. */
#define CURLA_PER_CHUNK 256
int curla_per_set(float* s, double* sums, float* vmax, long long capacity, const int64_t* rows, long long first_row,
                  const float* values, int n, void* stream);
int curla_per_sample(const float* s, const double* sums, long long capacity, void* device_block, long long u_offset,
                     long long prob_offset, int B, void* stream);
int curla_per_td(const float* q, long long twin_stride, const float* target_q, const float* prob, float beta, float eps,
                 float alpha, int B, float* dq, float* loss, float* w, float* value, void* stream);
/* device-visible address of a pinned (hipHostMalloc'd / registered) host pointer; CURLA_ERR_ARG if it is not */
int curla_host_device_pointer(void* host, void** device);
/* ReplayBuffer.add: one CHW uint8 observation into ring slot `slot` (utils.py:120-128) */
int curla_store_frame(const uint8_t* chw, uint8_t* frames, long long slot, int C, int H, int W, void* stream);
/* Acting on N observations at once (CurlSacAgent.select_actions / sample_actions; one by one: curl_sac.py:330-347 with
 * the centre crop of augmentations.py:26-45 in front): `nchw` holds N planar uint8 frames [N][C][Hs][Ws] as the
 * environments hand them over; the window (top, left), Hd x Wd, of each goes into ring slots first_slot ..
 * first_slot + N - 1 of `frames` ([slot][Hd][Wd][C], what curla_conv1_fwd reads with src_kind 1):
 *   frames[first_slot + n][y][x][c] = nchw[n][c][top + y][left + x],   0 <= y < Hd, 0 <= x < Wd.
 * One launch replaces N curla_store_frame calls and N host-side crops and transposes.  C in {3, 6, 9, 12} with both
 * pointers on a 4-byte boundary moves whole dwords on both sides, at any Hs, Ws, Hd, Wd, top and left; every other
 * case gives the same bytes one at a time.  CURLA_ERR_ARG when the window reaches outside the source or N < 1 or
 * C < 1.  Reads only the N source frames and writes only the N slots (the caller owns the ring's size and its 32
 * bytes of loader slack). */
int curla_stage_frames_u8(const uint8_t* nchw, uint8_t* frames, long long first_slot, int N, int C, int Hs, int Ws,
                          int top, int left, int Hd, int Wd, void* stream);
/* ReplayBuffer.add_vec: one step of N environments into ring rows first .. first + N - 1 in ONE launch.  `block` is the
 * device copy of the staged add block,
 *   [N obs | N next_obs] planar uint8 [2 N][C][H][W] | pad to 16 bytes | float [N][A + 2] | uint8 [2 N] flags,
 * the flag bytes present only when `cont` is not NULL.  `obs_ring` / `next_ring`: row 0 of the two rings,
 * [capacity][H][W][C] each (one allocation, next_ring = obs_ring + capacity H W C, or two); `scalars`: the ring's [capacity][A + 2] rows.
 *   obs_ring[first + e][y][x][c] = block frame e at [c][y][x],  next_ring[first + e] likewise from block frame N + e
 *   scalars[first + e][:] = block row e
 *   cont[first + e] = flag N + e;  has_prev != 0: cont[prev + e] = flag e, prev = (first - N) modulo capacity, the run
 *   of the step before (it may sit at the ring's end)
 * C in {3, 6, 9, 12} with H W a multiple of 4 and both rings on a 4-byte boundary moves whole dwords (the transpose of
 * curla_stage_frames_u8); every other case gives the same bytes one at a time.  Writes the rows named above and nothing
 * else.  CURLA_ERR_ARG before the launch on: block, obs_ring, next_ring or scalars NULL; block or scalars off 4 bytes;
 * N < 1, C < 1, H < 1, W < 1, A < 1; capacity % N != 0, first < 0, first % N != 0, first + N > capacity; has_prev with
 * cont NULL or capacity == N; 2 N H W >= 2^31.  Additive: CURLA_ABI_VERSION stays 8. */
int curla_add_vec(const uint8_t* block, uint8_t* obs_ring, uint8_t* next_ring, float* scalars, uint8_t* cont,
                  long long capacity, long long first, int has_prev, int N, int C, int H, int W, int A, void* stream);
/* De-duplicated frame store (next_obs[t] shares k-1 of its k frames with obs[t], and equals obs[t+1]
 * inside an episode, utils.py:238-268): `store` holds every RGB frame once, uint8 [F][H][W][3]; row idx[b] (NULL: b) of
 * `fid` (int32, `fid_stride` entries per row) lists the K frame ids of a stack.  Writes the minibatch of stacks
 * out[b][y][x][3f+c] = store[fid[idx[b]][f]][y][x][c] -- uint8 [B][H][W][3K], what curla_conv1_fwd reads (src_kind 1,
 * idx NULL); `out` needs the same 32 bytes of slack as a ring. */
int curla_gather_stacks(const uint8_t* store, const int32_t* fid, int fid_stride, const int64_t* idx, int B, int K,
                        int H, int W, uint8_t* out, void* stream);
int curla_nhwc_to_nchw(const float* in, float* out, int B, int H, int W, int C, void* stream);
/* RandomShift, the pad-and-crop shift of DrQ / DrQ-v2 (beyond the reference: its augmentations.py has no such class).
 * Every frame is padded by `pad` pixels on each side with its edge pixels repeated, then an H x W window is cut at the
 * sample's (dy, dx), 0 <= dy, dx <= 2 pad -- all channels of a stack share the draw:
 *   out[s][y][x][c] = frames[row(s)][clamp(y + dy[s] - pad, 0, H - 1)][clamp(x + dx[s] - pad, 0, W - 1)][c],  0 <= s < n
 * uint8 NHWC in ([rows][H][W][C]) and out ([n][H][W][C]): a shifted minibatch is still a uint8 ring, read by
 * curla_conv1_fwd (src_kind 1) with zero crop offsets; like a ring, `out` needs 32 bytes of slack behind it for that.
 * row(s) = idx[s % period] (idx NULL: s % period): with period = 2 B over a block's (obs rows | next_obs rows) run one
 * launch of n = 3 B serves obs, next_obs and pos, which reads the obs rows again.  dy / dx: int32 [n] (values outside
 * [0, 2 pad] are clamped into it).  A frame of a multiple of 16 bytes with `out` on a 16-byte boundary moves 16 bytes
 * per lane (one unaligned load where the group lies in one row and needs no x-clamp); every other case gives the same
 * bytes one at a time.  Additive like curla_noisy_cover_rng: CURLA_ABI_VERSION stays 8.  CURLA_ERR_UNSUPPORTED when
 * H W C or 2 pad C does not fit 31 / 30 bits. */
int curla_random_shift_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* dy, const int32_t* dx,
                          int pad, int n, int C, int H, int W, uint8_t* out, void* stream);
/* RandomCutout, the cutout / cutout-color of RAD (beyond the reference: its augmentations.py has no such class).  One
 * box per sample, shared by all channels of a stack, is painted onto an otherwise untouched frame:
 *   out[s][y][x][c] = colour(s)[c % 3]           if y0c <= y < y0c + bhc and x0c <= x < x0c + bwc,
 *                     frames[row(s)][y][x][c]    otherwise,                                            0 <= s < n
 * uint8 NHWC in ([rows][H][W][C]) and out ([n][H][W][C], 32 bytes of slack behind it like a ring), row(s) = idx[s % period]
 * (idx NULL: s % period) as for curla_random_shift_u8.  y0 / x0: int32 [n], the box's first row / column; size: int32 [n],
 * bh | bw << 16; rgb: int32 [n], r | g << 8 | b << 16 (the top byte is ignored; 0 = black).  Whatever they hold is clamped
 * in the kernel: y0c = clamp(y0, 0, H), bhc = clamp(bh, 0, H - y0c), likewise in x -- an empty box is a plain copy, every
 * output byte is written exactly once and no address depends on the box.  A frame of a multiple of 16 bytes with `out` on
 * a 16-byte boundary moves 16 bytes per lane (no load for a group inside the box); every other case gives the same bytes
 * one at a time.  Any C > 0.  Additive: CURLA_ABI_VERSION stays 8.  CURLA_ERR_UNSUPPORTED when H W C does not fit 31 bits. */
int curla_cutout_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* y0, const int32_t* x0,
                    const int32_t* size, const int32_t* rgb, int n, int C, int H, int W, uint8_t* out, void* stream);
/* RandomTranslate, the translate of RAD (beyond the reference: its augmentations.py has no such class).  The H x W frame is
 * placed at the sample's (ty, tx) on a black Ho x Wo canvas, Ho >= H and Wo >= W -- all channels of a stack share the draw,
 * every source pixel is kept and none is invented:
 *   out[s][y][x][c] = frames[row(s)][y - tyc][x - txc][c]   if 0 <= y - tyc < H and 0 <= x - txc < W,
 *                     0                                     otherwise,                                  0 <= s < n
 * uint8 NHWC in ([rows][H][W][C]) and out ([n][Ho][Wo][C], 32 bytes of slack behind it like a ring: a translated minibatch
 * is a uint8 ring of larger frames), row(s) = idx[s % period] (idx NULL: s % period) as for curla_random_shift_u8.
 * ty / tx: int32 [n]; whatever they hold is clamped in the kernel, tyc = clamp(ty, 0, Ho - H), txc = clamp(tx, 0, Wo - W):
 * every output byte is written exactly once, nothing is read outside the source frame (neither in front of it nor in the
 * slack behind a ring) and nothing is written outside `out`.  An output frame of a multiple of 16 bytes with `out` on a
 * 16-byte boundary (and a source frame of at least 16 bytes) moves 16 bytes per lane: no load for a group in the margin,
 * one unaligned load for a group inside the image, at most two loads combined in registers for a group that crosses an
 * image edge or straddles two rows; every other case gives the same bytes one at a time.  Any C > 0.  Additive:
 * CURLA_ABI_VERSION stays 8.  CURLA_ERR_UNSUPPORTED when Ho Wo C does not fit 31 bits or a row Wo C does not fit 30. */
int curla_translate_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* ty, const int32_t* tx, int n,
                       int C, int H, int W, int Ho, int Wo, uint8_t* out, void* stream);
/* Compose(move, paint): a geometric uint8 move with RandomCutout's box painted over its OUTPUT, in one launch -- the ring is
 * read once and `out` written once, where a mover launch followed by curla_cutout_u8 moves the minibatch twice:
 *   mid[s] = move(frames[row(s)])                          (Ho x Wo; the mover's own formula and clamps)
 *   out[s][y][x][c] = colour(s)[c % 3]   if y0c <= y < y0c + bhc and x0c <= x < x0c + bwc,   mid[s][y][x][c] otherwise
 * `move` selects the mover and what (a, b), int32 [n] each, mean:
 *   0  crop       (a, b) = (h1, w1): mid[y][x][c] = frames[row(s)][y + h1c][x + w1c][c], h1c = clamp(h1, 0, H - Ho), w1c =
 *                 clamp(w1, 0, W - Wo).  Needs Ho <= H and Wo <= W; `pad` is not used.
 *   1  shift      (a, b) = (dy, dx) and `pad`, as curla_random_shift_u8.  Needs Ho == H and Wo == W.
 *   2  translate  (a, b) = (ty, tx), as curla_translate_u8.  Needs Ho >= H and Wo >= W; `pad` is not used.
 * uint8 NHWC in ([rows][H][W][C]) and out ([n][Ho][Wo][C], 32 bytes of slack behind it like a ring), row(s) = idx[s % period]
 * (idx NULL: s % period) as for curla_random_shift_u8.  y0 / x0 / size / rgb: int32 [n] as for curla_cutout_u8, the box in
 * coordinates of the OUTPUT frame and clamped into it in the kernel (y0c = clamp(y0, 0, Ho), bhc = clamp(bh, 0, Ho - y0c),
 * likewise in x); an empty box is a plain move.  size NULL: no box -- y0, x0 and rgb are ignored and the launch is the
 * plain mover (for move 1 and 2 the kernels of curla_random_shift_u8 / curla_translate_u8; for move 0 the crop on its
 * own).  Nothing is read outside a source frame (neither in front of it nor in the slack behind a ring) and nothing is
 * written outside `out`.  An output frame of a multiple of 16 bytes with `out` on a 16-byte boundary moves 16 bytes per
 * lane: no load for a group wholly inside the box, the mover's loads for every other group, the box's bytes replaced in
 * registers where a group crosses a box edge; every other case gives the same bytes one at a time.  Any C > 0.  Additive:
 * CURLA_ABI_VERSION stays 8.  CURLA_ERR_ARG on an unknown move, a NULL required pointer, n < 1, C < 1, pad < 0 or sizes that
 * do not fit the move; CURLA_ERR_UNSUPPORTED when H W C or Ho Wo C does not fit 31 bits, 2 pad C (move 1) or a row Wo C
 * (move 0 and 2) does not fit 30, or, with a box, Ho does not fit 29. */
int curla_move_cutout_u8(const uint8_t* frames, const int64_t* idx, int period, int move, const int32_t* a, const int32_t* b,
                         int pad, const int32_t* y0, const int32_t* x0, const int32_t* size, const int32_t* rgb, int n, int C,
                         int H, int W, int Ho, int Wo, uint8_t* out, void* stream);
/* RandomFlip / RandomRotate, the flip and rotate of RAD (beyond the reference: its augmentations.py has neither): one of
 * the eight maps of the dihedral group per sample, shared by all channels of a stack.  code: int32 [n], three bits
 * FX = 1, FY = 2, T = 4; with (a, b) = (x, y) if T is set, else (y, x):
 *   out[s][y][x][c] = frames[row(s)][FY ? H - 1 - a : a][FX ? W - 1 - b : b][c],  0 <= s < n
 * (1 mirrors left-right, 2 upside down; 5, 3, 6 turn by 90, 180, 270 degrees counter-clockwise, as np.rot90 over (H, W)).
 * uint8 NHWC in ([rows][H][W][C]) and out ([n][H][W][C], 32 bytes of slack behind it like a ring), row(s) = idx[s % period]
 * (idx NULL: s % period) as for curla_random_shift_u8.  The effective code is code[s] & 7, and additionally & 3 where
 * H != W (only a square frame can be transposed in place): whatever the words hold, every output byte is written exactly
 * once, nothing is read outside the source frame and nothing is written outside `out`.  One launch, mixed codes in it:
 * codes 0..3 move 16 bytes per lane from unaligned 16-byte loads combined in registers (a frame of a multiple of 16 bytes
 * with `out` on a 16-byte boundary; every other case gives the same bytes one at a time); codes 4..7 stage the source
 * columns of a band of output rows in LDS (gathered from global memory directly where H segments do not fit 64 KiB).
 * Any C > 0.  Additive: CURLA_ABI_VERSION stays 8.  CURLA_ERR_ARG on a NULL pointer, `code` off 4 bytes, `idx` off 8, or
 * n, period, C, H or W < 1; CURLA_ERR_UNSUPPORTED when H W C does not fit 31 bits; both before any launch. */
int curla_dihedral_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* code, int n, int C, int H,
                      int W, uint8_t* out, void* stream);
/* RandomGrayscale, the grayscale of RAD (beyond the reference: its augmentations.py has no such class).  Where grey[s] != 0
 * every RGB triplet of the sample, in all frames of the stack, becomes (g, g, g):
 *   g = (77 R + 150 G + 29 B + 128) >> 8        (weights that sum to 256: (v, v, v) stays (v, v, v), the map is idempotent)
 * and where grey[s] == 0 the frame is copied.  uint8 NHWC in ([rows][H][W][C]) and out ([n][H][W][C], 32 bytes of slack
 * behind it like a ring), row(s) = idx[s % period] (idx NULL: s % period) as for curla_random_shift_u8.  grey: int32 [n].
 * C must be a multiple of 3.  No address depends on the words: nothing is read outside the source frame and nothing is
 * written outside `out`.  A frame of a multiple of 16 bytes with `out` on a 16-byte boundary moves 16 bytes per lane (the
 * triplets that straddle a group's ends come from the dword in front of and behind it); every other case gives the same
 * bytes one at a time.  Additive: CURLA_ABI_VERSION stays 8.  CURLA_ERR_ARG on a NULL pointer, `grey` off 4 bytes, `idx`
 * off 8, n, period, C, H or W < 1 or C % 3 != 0; CURLA_ERR_UNSUPPORTED when H W C does not fit 31 bits; both before any
 * launch. */
int curla_grayscale_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* grey, int n, int C, int H,
                       int W, uint8_t* out, void* stream);
/* RandomAffine, the rotate / zoom / sub-pixel shift of kornia's and torchvision's RandomAffine (beyond the reference: its
 * augmentations.py resamples nothing): one inverse affine map per sample, shared by all channels of a stack, bilinear in
 * integers.  m00 m01 m02 m10 m11 m12: int32 [n] each, 16.16 fixed point, from output pixel (y, x) to source coordinates:
 *   X = wrap32(m00 x + m01 y + m02)          Y = wrap32(m10 x + m11 y + m12)       (two's-complement wrap-around)
 *   x0 = X >> 16 (arithmetic: floor)         fx = (X >> 8) & 255
 *   y0 = Y >> 16                             fy = (Y >> 8) & 255
 *   out[s][y][x][c] = (P(y0, x0)[c] (256 - fx) (256 - fy) + P(y0, x0 + 1)[c] fx (256 - fy)
 *                    + P(y0 + 1, x0)[c] (256 - fx) fy     + P(y0 + 1, x0 + 1)[c] fx fy     + 32768) >> 16
 * with P(yy, xx) = frames[row(s)][clamp(yy, 0, H - 1)][clamp(xx, 0, W - 1)] under fill = 1 (edge); under fill = 0 (zero)
 * frames[row(s)][yy][xx] inside [0, H) x [0, W) and 0 outside.  The identity words are (65536, 0, 0, 0, 65536, 0).  uint8
 * NHWC in ([rows][H][W][C]) and out ([n][H][W][C]: the source frame's size), row(s) = idx[s % period] (idx NULL:
 * s % period) as for curla_random_shift_u8.  The rule is total: whatever the words hold, nothing is read outside the source
 * frame (nor in the slack behind a ring), every output byte is written exactly once and nothing is written outside `out`.
 * One launch: a workgroup stages the source box of a band of output bytes in LDS with 16-byte loads and blends from there
 * (from global memory directly where no band's box fits 64 KiB, or where the words wrap inside a band); 8 bytes per lane
 * and store for a frame of a multiple of 16 bytes with `out` on a 16-byte boundary, the same bytes one at a time
 * otherwise.  Any C > 0.
 * Additive: CURLA_ABI_VERSION stays 8.  CURLA_ERR_ARG on a NULL pointer, a word array off 4 bytes, `idx` off 8, n, period,
 * C, H or W < 1, or fill not 0 or 1; CURLA_ERR_UNSUPPORTED when H W C does not fit 31 bits; both before any launch. */
int curla_affine_u8(const uint8_t* frames, const int64_t* idx, int period, const int32_t* m00, const int32_t* m01,
                    const int32_t* m02, const int32_t* m10, const int32_t* m11, const int32_t* m12, int fill, int n, int C,
                    int H, int W, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CURLA_HIP_H */
