/* libdrqv2_hip.so -- C ABI of the MI355X-native DrQ-v2 update path.
 *
 * The reference (johannah/drqv2) has no native boundary of its own: DrQV2Agent.update()
 * (drqv2.py:230-262) reaches ATen/cuDNN through torch.nn / torch.optim.  Each entry point below
 * replaces the ATen kernels behind the cited reference lines; the Python host (drqv2.py, utils.py at
 * the repo root, drqv2_amd/) binds them with ctypes.  Conventions:
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller (PyTorch-ROCm);
 *   - every call is enqueued on `stream` (a hipStream_t, passed as void*), nothing synchronises;
 *   - return 0 = ok, <0 = argument/shape/workspace error, >0 = hipError_t of the launch;
 *   - no allocation and no state that outlives a call, except two host-side caches indexed by the current HIP
 *     device: the CU count (with the test override of drq_set_num_cus), and "dynamic-LDS attribute already set" flags
 *     of the weight-gradient kernels;
 *   - the library is built with -fvisibility=hidden: the functions declared here are ALL it exports
 *     (tests/test_cpu_interface.py checks both directions);
 *   - tensors are fp32 row-major / NCHW unless stated.
 */
#ifndef DRQV2_HIP_H
#define DRQV2_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* drq_stream_t; /* hipStream_t */

#define DRQ_OK 0
#define DRQ_EARG (-1)
#define DRQ_EWS (-2)

int drq_abi_version(void);

/* ---- The CU count the library plans with.  Every launch sizes its grid from the CU count of the current HIP device,
 * and so do the XCD-aware workgroup orders, the shares of a merged grid, the split-K factors and the grid-stride caps.
 * drq_num_cus_in_effect(): the count every planner sees on the current device: the override below where one is set,
 * else the hardware's (hipDeviceProp_t::multiProcessorCount, asked once per device).
 * drq_set_num_cus(n): a per-device override for tests, which makes a whole device plan like a partition of it (an
 * MI355X in CPX / QPX / DPX mode shows 32 / 64 / 128 CUs).  n == 0 clears the override of the current device;
 * 1 <= n <= the hardware count sets it; anything else returns DRQ_EARG and changes nothing.  Returns DRQ_OK or DRQ_EARG.
 * A count above the hardware's is refused on purpose: a smaller count only shrinks grids, a larger one could enlarge
 * them past what is resident at once.  The workspace-size entries (drq_conv3x3_wgrad_ws_bytes, drq_step_ws_bytes,
 * drq_explore_knn_ws_bytes, drq_act_ws_bytes) do not depend on the count, so a workspace sized under an override serves
 * the launches made under it and under any smaller one.  Both entries launch nothing and take no stream.  The
 * override is plain process-wide state per device, NOT thread-safe against concurrent launches: set it while no other
 * thread is inside the library, and restore it (n = 0) before anything else runs.  Results under an override are as correct as without one; only grids (and with them the
 * summation order of the kernels that leave per-workgroup partial sums) change. */
int drq_num_cus_in_effect(void);
int drq_set_num_cus(int n);

/* ---- RandomShiftsAug.forward (drqv2.py:19-45) [+ Encoder's obs/255-0.5, drqv2.py:64, if fuse_norm]
 * obs u8 [n][c][hw][hw]; shift_xy f32 [n][2] = the torch.randint(0,2*pad+1,(n,1,1,2)) draw (x,y);
 * base_grid f32 [hw] = linspace(-1+1/S,1-1/S,S)[:hw]; out f32 [n][c][hw][hw]. */
int drq_aug_fwd(const uint8_t* obs, const float* shift_xy, const float* base_grid, float* out, int n, int c,
                int hw, int pad, int fuse_norm, drq_stream_t stream);
int drq_aug_fwd_f32(const float* x, const float* shift_xy, const float* base_grid, float* out, int n, int c,
                    int hw, int pad, drq_stream_t stream);

/* ---- RandomShiftsAug of BOTH views (drqv2.py:241-242) + obs/255-0.5 (:64) + the first encoder layer
 * Conv2d(9,32,3,stride 2)+ReLU (:55) in one launch that reads the uint8 frames once (frame_stack 3, 84x84, pad 4).
 * obs / obs1 u8 [n][9][84][84] (4-byte aligned), shift / shift1 f32 [n][2], base_grid f32 [84], w [32][9][3][3],
 * bias [32].  y f32 [2n][32][41][41]: frames [0,n) = obs view, [n,2n) = obs1 view.  xaug f32 [2n][9][84][84]:
 * the augmented, normalised encoder input of frames [0, n_store) is also written there (the update stores the
 * obs view, n_store = n, for conv1's weight gradient; tests store both views; 0 = none, xaug may be NULL).
 * Values are bit-identical to drq_aug_fwd(fuse_norm=1) followed by drq_conv3x3_fwd. */
int drq_conv1_aug_fwd(const uint8_t* obs, const float* shift, const uint8_t* obs1, const float* shift1,
                      const float* base_grid, const float* w, const float* bias, float* xaug, float* y, int n,
                      int n_store, drq_stream_t stream);
/* the same with the layer's products on the bf16 MFMA (the bf16 update path, see the bf16 conv entries below): the
 * augmentation and the stored encoder input are the fp32 ones, bit for bit; y = relu(conv(bf16(x), bf16(w)) + b). */
/* the same with the two views given as rows idx[b] / idx1[b] of frame stores (a device-resident replay ring): the batch
 * of replay_buffer.py:142-160 is never materialised; results are bit-identical to drq_conv1_aug_fwd on the gathered
 * frames. */
int drq_conv1_aug_fwd_indexed(const uint8_t* frames, const int64_t* idx, const float* shift, const uint8_t* frames1,
                              const int64_t* idx1, const float* shift1, const float* base_grid, const float* w,
                              const float* bias, float* xaug, float* y, int n, int n_store, drq_stream_t stream);
/* the same with both views taken from ONE ring of single frames ("single-frame step-major replay" below): frames u8
 * [R N][3][84][84], first u8 [R N]; idx[b] / idx1[b] in [0, R N) are the slots of the NEWEST frame of row b's two stacks,
 * the launch finds the other two frames by the flags.  Bit-identical to drq_conv1_aug_fwd on the stacks
 * drq_vec_stack_gather produces for idx and idx1; _bf16: likewise to drq_conv1_aug_fwd_bf16.  DRQ_EARG also for null
 * first / idx / idx1, R, N <= 0 or R N > INT32_MAX. */
int drq_conv1_aug_fwd_frames(const uint8_t* frames, const uint8_t* first, long R, long N, const int64_t* idx,
                             const float* shift, const int64_t* idx1, const float* shift1, const float* base_grid,
                             const float* w, const float* bias, float* xaug, float* y, int n, int n_store,
                             drq_stream_t stream);
int drq_conv1_aug_fwd_frames_bf16(const uint8_t* frames, const uint8_t* first, long R, long N, const int64_t* idx,
                                  const float* shift, const int64_t* idx1, const float* shift1, const float* base_grid,
                                  const float* w, const float* bias, float* xaug, float* y, int n, int n_store,
                                  drq_stream_t stream);
int drq_conv1_aug_fwd_bf16(const uint8_t* obs, const float* shift, const uint8_t* obs1, const float* shift1,
                           const float* base_grid, const float* w, const float* bias, float* xaug, float* y, int n,
                           int n_store, drq_stream_t stream);
/* the same with y in the bf16 [2n][41][41][32 channels] layout of the bf16 update (see drq_conv3x3_fwd_bf16_nhwc):
 * the values of drq_conv1_aug_fwd_bf16's y, rounded to bf16 */
int drq_conv1_aug_fwd_bf16_nhwc(const uint8_t* obs, const float* shift, const uint8_t* obs1, const float* shift1,
                                const float* base_grid, const float* w, const float* bias, float* xaug, void* y_nhwc,
                                int n, int n_store, drq_stream_t stream);

/* ---- Encoder conv layers (drqv2.py:55-59): Conv2d(cin,32,3,stride)+ReLU, 32 output channels.
 * Supported (cin,hin,stride): (9,84,2) (32,41,1) (32,39,1) (32,37,1).  y element (b,co,oy,ox) is
 * written at y[y_off + b*y_bs + co*y_cs + oy*y_rs + ox]. */
int drq_conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int nb, int cin, int hin,
                    int stride, int relu, long y_bs, long y_cs, long y_rs, long y_off, drq_stream_t stream);
/* autograd of the same layers.  dy_pad = gradient w.r.t. the pre-activation, stored zero-padded by 2:
 * [nb][32][hout+4][hout+4].  dx (size hout+2) = conv_transpose(dy, w) * (mask > 0), strided store. */
int drq_conv3x3_dgrad(const float* dy_pad, const float* w, const float* mask, float* dx, int nb, int hout,
                      long dx_bs, long dx_cs, long dx_rs, long dx_off, drq_stream_t stream);
/* The 32->32 layers (hin 41/39/37, stride 1) and their input gradient in Winograd F(2x2,3x3) form: same contracts as
 * drq_conv3x3_fwd / drq_conv3x3_dgrad, 2.25x fewer matrix FLOPs, fp32 throughout; the result differs from the
 * direct form by rounding only (same error level against fp64).  This is what DrQV2Agent.update runs. */
int drq_conv3x3_fwd_wino(const float* x, const float* w, const float* bias, float* y, int nb, int hin, int relu,
                         long y_bs, long y_cs, long y_rs, long y_off, drq_stream_t stream);
int drq_conv3x3_dgrad_wino(const float* dy_pad, const float* w, const float* mask, float* dx, int nb, int hout,
                           long dx_bs, long dx_cs, long dx_rs, long dx_off, drq_stream_t stream);
/* drq_conv3x3_dgrad_wino on a budget of workgroup slots: the launch takes at most `budget` workgroups (counted in
 * sixteens, at least 16; 0 or more than two per CU = the whole chip, which is drq_conv3x3_dgrad_wino) and leaves the
 * other slots of the chip to launches of other streams.  dx is the same bit for bit whatever the budget.  The
 * overlapped schedule of the update (DRQ_STEP_OVERLAP_ACTOR) runs its three input gradients this way. */
int drq_conv3x3_dgrad_wino_budget(const float* dy_pad, const float* w, const float* mask, float* dx, int nb, int hout,
                                  long dx_bs, long dx_cs, long dx_rs, long dx_off, int budget, drq_stream_t stream);
/* ... and their weight / bias gradient in the same form: the contract of drq_conv3x3_wgrad for cin = 32, stride 1, with
 * ONE more precondition: dy must be the interior of a ZERO-PADDED buffer (the kernel reads row and column `hout` of
 * every plane as the empty half of the last 2x2 tile), i.e. dy_rs >= hout+1, dy_cs >= (hout+1)*dy_rs and zeros there --
 * the update's [nb][32][hout+4][hout+4] gradient buffers (pad 2) satisfy it.  A contiguous dy returns DRQ_EARG. */
int drq_conv3x3_wgrad_wino(const float* x, const float* dy, float* dw, float* db, int nb, int hin, long dy_bs,
                           long dy_cs, long dy_rs, long dy_off, float* ws, size_t ws_bytes, drq_stream_t stream);
/* dw [32][cin][3][3], db [32]; dy addressed as dy[dy_off + b*dy_bs + co*dy_cs + oy*dy_rs + ox]. */
int drq_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, int nb, int cin, int hin,
                      int stride, long dy_bs, long dy_cs, long dy_rs, long dy_off, float* ws, size_t ws_bytes,
                      drq_stream_t stream);
size_t drq_conv3x3_wgrad_ws_bytes(void);

/* ---- bf16-MFMA variants of the 32->32 channel layers (conv2..4), BASELINE configs[4] ("bf16").  New functionality:
 * the reference is fp32 only.  Same arguments, layouts and fp32 storage as the entries above; every MFMA operand is
 * rounded to bf16 (nearest even) when staged, products are exact, accumulation is fp32: the result is the
 * fp32-accumulated convolution of the bf16-rounded operands.  hin in {41,39,37} (fwd, wgrad); hout+4 in {39,41,43}. */
int drq_conv3x3_fwd_bf16(const float* x, const float* w, const float* bias, float* y, int nb, int hin, int relu,
                         long y_bs, long y_cs, long y_rs, long y_off, drq_stream_t stream);
int drq_conv3x3_dgrad_bf16(const float* dy_pad, const float* w, const float* mask, float* dx, int nb, int hout,
                           long dx_bs, long dx_cs, long dx_rs, long dx_off, drq_stream_t stream);
int drq_conv3x3_wgrad_bf16(const float* x, const float* dy, float* dw, float* db, int nb, int hin, long dy_bs,
                           long dy_cs, long dy_rs, long dy_off, float* ws, size_t ws_bytes, drq_stream_t stream);
/* The same three launches with activations in the layout the bf16 update keeps between the encoder layers (round 3):
 * bf16 [frame][y][x][32 channels], 64 bytes per pixel, 16-byte aligned.  A value stored in that layout is the bf16
 * rounding the entries above apply when they stage it, in the same place of the same sums, so results are identical
 * bit for bit.  fwd: x in that layout when x_nhwc (else fp32 NCHW), y in that layout when y_nhwc (else contiguous fp32
 * NCHW); dgrad: the mask in that layout ([nb][hout+2][hout+2][32]); dy_nhwc: dy_pad is bf16 [nb][hout+4][hout+4][32]
 * with its zero border; dx_nhwc: dx is the INTERIOR of a bf16 [nb][hout+6][hout+6][32] buffer padded by 2 whose
 * border the caller keeps zero (the strides are ignored); wgrad: x in that layout; dy_nhwc: dy is the base of such a
 * padded bf16 [nb][hin+2][hin+2][32] buffer (strides ignored) and db sums the bf16 values. */
int drq_conv3x3_fwd_bf16_nhwc(const void* x, const float* w, const float* bias, void* y, int nb, int hin, int relu,
                              int x_nhwc, int y_nhwc, drq_stream_t stream);
int drq_conv3x3_dgrad_bf16_nhwc(const void* dy_pad, const float* w, const void* mask_nhwc, void* dx, int nb, int hout,
                                int dy_nhwc, int dx_nhwc, long dx_bs, long dx_cs, long dx_rs, long dx_off,
                                drq_stream_t stream);
int drq_conv3x3_wgrad_bf16_nhwc(const void* x_nhwc, const void* dy, float* dw, float* db, int nb, int hin, int dy_nhwc,
                                long dy_bs, long dy_cs, long dy_rs, long dy_off, float* ws, size_t ws_bytes,
                                drq_stream_t stream);

/* ---- nn.Linear forward / backward (drqv2.py:74-81,100-111) as one strided, batched GEMM:
 *   C[b][m][n] = epi( sum_k A_b(m,k) * B_b(k,n) ),  epi(v) = relu?(v + bias[n]) * (aux[m][n] > 0)?
 *   a_kc: A(m,k)=A[m*lda+k] else A[k*lda+m];  b_kc: B(k,n)=B[n*ldb+k] else B[k*ldb+n].
 *   scatter_hw>0: C index = zero-padded (pad 2) NCHW gradient layout of a [M][32*hw*hw] feature map.
 *   tile: block tile (rows x columns) of the LDS-staged kernel: 0 auto, 1 = 32x32, 2 = 64x64, 3 = 64x32, 4 = 32x64
 *   (k-tile 32), 5 = 32x32 and 6 = 64x64 with a k-tile of 64 (one barrier per 64 k).  Any tile != 0 or splitk != 0
 *   keeps the call on that kernel (0 / 0 lets the shape-specific kernels take eligible shapes).  Every tile takes every
 *   shape and alignment; splitk: 0 auto, else the number of K slices asked for (rounded to slices of whole multiples
 *   of 64; needs ws when more than one remains). */
int drq_gemm_f32(const float* A, long lda, int a_kc, const float* B, long ldb, int b_kc, float* C, long ldc,
                 int M, int N, int K, int nbatch, long a_bs, long b_bs, long c_bs, const float* bias, long bias_bs,
                 int relu, const float* aux, int ldaux, long aux_bs, int scatter_hw, int tile, int splitk,
                 float* ws, size_t ws_bytes, drq_stream_t stream);

/* same GEMM for nbatch (<= 8) problems of one shape with independent pointers (host arrays of device
 * pointers; bias / aux / rowsum arrays may be NULL).  rowsum[b] != NULL (needs a_kc == 0): also writes
 * rowsum[b][m] = sum_k A_b(m,k), i.e. the bias gradient of a wgrad GEMM, without a second pass. */
int drq_gemm_batched_f32(int nbatch, const float* const* A, long lda, int a_kc, const float* const* B, long ldb,
                         int b_kc, float* const* C, long ldc, int M, int N, int K, const float* const* bias, int relu,
                         const float* const* aux, int ldaux, float* const* rowsum, int scatter_hw, int tile,
                         int splitk, float* ws, size_t ws_bytes, drq_stream_t stream);

/* bf16-MFMA variant of drq_gemm_batched_f32 (BASELINE configs[4]; new functionality, see the conv entries): fp32
 * storage, operands rounded to bf16 when staged, fp32 accumulation; rowsum sums the unrounded values. */
int drq_gemm_batched_bf16(int nbatch, const float* const* A, long lda, int a_kc, const float* const* B, long ldb,
                          int b_kc, float* const* C, long ldc, int M, int N, int K, const float* const* bias, int relu,
                          const float* const* aux, int ldaux, float* const* rowsum, int scatter_hw, int splitk,
                          float* ws, size_t ws_bytes, drq_stream_t stream);

/* Forward form only (both operands k-contiguous, a_kc = b_kc = 1) with the split-K sum left to the caller: when
 * *splitk_out > 1 the result is ws[(b*splitk + s)*M*N + m*N + n], s < splitk, WITHOUT bias (the consumer, e.g. the
 * LayerNorm kernel of the trunk, sums the records and adds the bias itself); *splitk_out == 1: C holds the result
 * with bias.  This is the entry DrQV2Agent.update uses for the trunk Linear(39200 -> feature_dim) (drqv2.py:74,100). */
int drq_gemm_batched_partial(int nbatch, const float* const* A, long lda, int a_kc, const float* const* B, long ldb,
                             int b_kc, float* const* C, long ldc, int M, int N, int K, const float* const* bias,
                             float* ws, size_t ws_bytes, int* splitk_out, drq_stream_t stream);

/* ---- hidden layers of the policy / Q MLPs, nn.Linear(hidden, hidden)+ReLU (drqv2.py:77-81,103-111) on the LDS-DMA
 * ring kernel (csrc/gemm3.hip): fp32, nbatch (<= 8) problems of one shape, every dimension a multiple of 64 (K of
 * the forward / dgrad forms: of 32), 16-byte aligned operands, leading dimensions multiples of 4.  DRQ_EARG = shape
 * not eligible (callers fall back to drq_gemm_batched_f32).
 * drq_mlp_fwd: y_b [M][ldy] = relu?(x_b [M][ldx] w_b[N][ldw]^T + bias_b).  qw / qpart (both or neither): the weight
 * row [N] of a FOLLOWING Linear(N, 1) (the Q heads' output layer, drqv2.py:106,111): qpart_b [M][*nq_out] receives the
 * partial dots  sum_{n in column tile j} y_b[m][n] qw_b[n];  that layer's output is their sum in index order + bias.
 * drq_mlp_dgrad: dx_b [M][lddx] = (dy_b [M][lddy] w_b [K][ldw]) * (mask_b [M][ldmask] > 0)?   (N columns).
 * drq_mlp_wgrad_dgrad: both gradients of one layer in ONE launch: dw_b [Nout][Kin] = dy_b^T x_b, db_b [Nout] =
 * column sums of dy_b (db may be NULL), dx_b [Brows][lddx] = (dy_b w_b [Nout][ldw]) * (mask_b > 0)?. */
int drq_mlp_fwd(int nbatch, const float* const* x, long ldx, const float* const* w, long ldw, float* const* y,
                long ldy, int M, int N, int K, const float* const* bias, int relu, const float* const* qw,
                float* const* qpart, int* nq_out, drq_stream_t stream);
int drq_mlp_dgrad(int nbatch, const float* const* dy, long lddy, const float* const* w, long ldw, float* const* dx,
                  long lddx, int M, int N, int K, const float* const* mask, int ldmask, drq_stream_t stream);
int drq_mlp_wgrad_dgrad(int nbatch, const float* const* dy, long lddy, const float* const* x, long ldx,
                        float* const* dw, float* const* db, const float* const* w, long ldw, float* const* dx,
                        long lddx, const float* const* mask, int ldmask, int Brows, int Nout, int Kin,
                        drq_stream_t stream);

/* ---- row-local stages fused with the first MLP layer that consumes them (csrc/rowblock.hip), fp32.
 * drq_ln_l1_fwd: njobs (<= 4) problems  h_j = tanh(LayerNorm(z_j)) (drqv2.py:74-75,100-101; eps 1e-5, F <= 256), with
 * z_j given either as z[j] [rows_j][F] (splitk == 0) or as the split-K records of drq_gemm_batched_partial (splitk > 0:
 * element (s, row, f) of problem j at part[j][(s*slab) + row*F + f], plus bias[j][f]); out[j] [rows_j][ldo_j] receives
 * h_j in columns [0,F) and, if tail[j] is given, tail[j] [rows_j][tail_ld_j] in columns [F, F+tail_n_j) (the critic's
 * [h, action] input, drqv2.py:117); xhat[j] / rstd[j] (optional) as drq_ln_tanh_fwd writes them -- all bit-identical
 * to drq_ln_tanh_fwd.  nheads[j] in {0,1,2}: y[2j+h] [rows_j][H] = relu(out_j[:, :F+tail_n_j] w[2j+h]^T + b[2j+h]),
 * w [H][F+tail_n_j] (16-byte aligned), the first layers of the policy / Q MLPs (drqv2.py:77,103,108); F+tail_n <= 128.
 * drq_policy_out_l1_fwd: p3 [rows][A] = p2 [rows][H] w3[A][H]^T + b3 (drqv2.py:81; H % 256 == 0, A <= 32); rows >=
 * srow0 ("hi", the next_obs rows): mu = tanh(p3), a' = clampST(mu + clamp(noise_hi*std, +-clip)) (utils.py:117-126)
 * written to columns [F, F+A) of ha_hi [rows-srow0][lda_hi] (mu_hi optional), and with nheads == 2
 * y[h] [rows-srow0][H] = relu([ha_hi[:, :F], a'] w[h]^T + b[h]); rows < srow0 ("lo"): the same sample with noise_lo into
 * ha_lo / mu_lo when noise_lo is given. */
int drq_ln_l1_fwd(int njobs, const float* const* part, const float* const* z, const float* const* bias,
                  const float* const* gamma, const float* const* beta, float* const* out, const int* ldo,
                  float* const* xhat, float* const* rstd, const float* const* tail, const int* tail_ld,
                  const int* tail_n, const int* rows, const int* nheads, const float* const* w, const float* const* b,
                  float* const* y, int F, int H, int splitk, long slab, drq_stream_t stream);
int drq_policy_out_l1_fwd(const float* p2, const float* w3, const float* b3, float* p3, int rows, int srow0, int H, int A,
                          int F, float std, float clip, int use_clip, const float* noise_hi, float* mu_hi, float* ha_hi,
                          long lda_hi, const float* noise_lo, float* mu_lo, float* ha_lo, long lda_lo, int nheads,
                          const float* const* w, const float* const* b, float* const* y, drq_stream_t stream);

/* ---- output layer of the Q heads, nn.Linear(hidden, 1) (drqv2.py:106,111), nz (<= 8) problems per launch:
 * q = h w^T + b;  backward: dh = (dq w) * (h > 0), and if dw/db are given dw = dq^T h, db = sum dq. */
int drq_qout_fwd(int nz, const float* const* h, const float* const* w, const float* const* b, float* const* q, int B,
                 int H, drq_stream_t stream);
int drq_qout_bwd(int nz, const float* const* dq, const float* const* h, const float* const* w, float* const* dh,
                 float* const* dw, float* const* db, int B, int H, drq_stream_t stream);

/* ---- nn.LayerNorm(F)+nn.Tanh (drqv2.py:74-75,100-101), eps 1e-5, F <= 256 */
int drq_ln_tanh_fwd(const float* z, int ldz, const float* gamma, const float* beta, float* out, int ldo,
                    float* xhat, float* rstd, int rows, int F, drq_stream_t stream);
int drq_ln_tanh_fwd2(const float* z0, const float* z1, int ldz, const float* gamma0, const float* beta0,
                     const float* gamma1, const float* beta1, float* out0, int ldo0, float* out1, int ldo1,
                     float* xhat0, float* rstd0, float* xhat1, float* rstd1, int rows, int F, drq_stream_t stream);
int drq_ln_tanh_fwd_multi(int n, const float* const* z, int ldz, const float* const* gamma, const float* const* beta,
                          float* const* out, const int* ldo, float* const* xhat, float* const* rstd, int rows, int F,
                          drq_stream_t stream);
int drq_ln_tanh_bwd(const float* dh0, int ld0, const float* dh1, int ld1, const float* h, int ldh,
                    const float* xhat, const float* rstd, const float* gamma, float* dz, float* dln,
                    float* dgamma, float* dbeta, int rows, int F, drq_stream_t stream);

/* ---- bias gradients: out[b][n] = sum_m dy[b][m][n] */
int drq_colsum(const float* dy, long ld, long dy_bs, float* out, long out_bs, int M, int N, int nbatch,
               drq_stream_t stream);

/* ---- Actor head + utils.TruncatedNormal.sample (drqv2.py:88-92, utils.py:112-126):
 * mu = tanh(pre_tanh); a = clamp(mu + clamp(noise*std, +-clip), +-(1-1e-6)); a -> a_out[b*lda_out + j]. */
int drq_trunc_normal_sample(const float* pre_tanh, const float* noise, float std, float clip, int use_clip,
                            float* mu_out, float* a_out, long lda_out, int B, int A, drq_stream_t stream);
int drq_copy_cols(const float* src, int ld_src, float* dst, long ld_dst, int B, int A, drq_stream_t stream);

/* ---- update_critic loss (drqv2.py:185-189): y = r + d*min(tq1,tq2); dq_k = 2(q_k-y)*inv_global_B;
 * sums[0..4] = sum r, sum y, sum q1, sum q2, sum((q1-y)^2+(q2-y)^2) over the LOCAL batch. */
int drq_td_mse(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
               const float* discount, float* dq1, float* dq2, float* sums, int B, float inv_global_B,
               drq_stream_t stream);
/* The same loss with a weight per row (prioritized replay; new functionality, these definitions are the contract).
 * With w [B] and y as above:  critic_loss = mean_i w_i (q1_i - y_i)^2 + mean_i w_i (q2_i - y_i)^2,
 *   dq_k[i] = (2 (q_k,i - y_i) inv_global_B) w_i   -- multiplied by w_i LAST: w_i == 1.0f gives drq_td_mse's bits --
 *   td_abs[i] = (|q1_i - y_i| + |q2_i - y_i|) / 2  (unweighted: what the priorities are made of),
 *   sums[4] = sum_i w_i ((q1_i-y_i)^2 + (q2_i-y_i)^2);  sums[0..3] are unweighted, as drq_td_mse leaves them. */
int drq_td_mse_w(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
                 const float* discount, const float* w, float* dq1, float* dq2, float* td_abs, float* sums, int B,
                 float inv_global_B, drq_stream_t stream);
/* ---- update_actor loss (drqv2.py:212-216,225): sums[5] = sum -min(q1,q2), sums[6] = sum log_prob */
int drq_actor_loss(const float* q1, const float* q2, const float* a, long lda, const float* mu, float std,
                   float* dq1, float* dq2, float* sums, int B, int A, float inv_global_B, drq_stream_t stream);
int drq_actor_dmu(const float* dha1, const float* dha2, long ld, int col0, const float* mu, float* dpre, int B,
                  int A, drq_stream_t stream);

/* ---- DrQ+BC: the actor loss of TD3+BC on DrQ-v2's actor step (offline training from a fixed dataset).  New
 * functionality: the reference has no such loss; these definitions are the contract.  With a the sample of
 * drqv2.py:210-211 (its gradient passes straight through to mu), a_beh the batch's action and Qmin = min(Q1, Q2)(a):
 *   lambda = alpha / mean_i |Qmin_i|  (a constant of the backward, no epsilon),  bc = mean over [B][A] of (a - a_beh)^2,
 *   loss = -lambda mean_i Qmin_i + bc;  dq_k[i] = -lambda * inv_global_B on the head that holds the minimum (ties split
 *   as in the plain loss);  dmu = da_1 + da_2 + bc_scale (a - a_beh), bc_scale = 2 / (B_global A);  dpre = dmu (1 - mu^2).
 * lambda needs sum |Qmin| over the whole batch before any dq: every workgroup that needs it adds the B values itself in
 * one fixed order, so all workgroups of all four entries and all runs see the same bits.  Single GPU: B is the global batch.
 * `sums` holds at least 11 floats: sums[5] = sum -Qmin and sums[6] = sum log_prob as the plain loss leaves them,
 * sums[9] = sum (a - a_beh)^2, sums[10] = sum |Qmin|; slots 7 and 8 are not written.  a [B][lda], a_beh [B][ldb].
 * The loss as a launch of its own (BC form of the plain loss entry above), and as the first launch of the actor
 * backward: the twin Q output layer's input gradient dh[k] = (dq_k w[k]) * (h[k] > 0) with dq never stored, h / w / dh
 * host arrays of two device pointers ([B][H], [H], [B][H]); (B + 5184) floats of LDS, else DRQ_EARG. */
int drq_actor_loss_bc(const float* q1, const float* q2, const float* a, long lda, const float* a_beh, long ldb,
                      const float* mu, float std, float alpha, float* dq1, float* dq2, float* sums, int B, int A,
                      float inv_global_B, drq_stream_t stream);
int drq_qout_bwd_actor_bc(const float* q1, const float* q2, const float* act, long lda, const float* a_beh, long ldb,
                          const float* mu, float std, float alpha, int A, float inv_global_B, float* sums,
                          const float* const* h, const float* const* w, float* const* dh, int B, int H,
                          drq_stream_t stream);
/* The policy output layer's backward with the BC pull in dmu, in the two shapes the update uses.  The elementwise form
 * (BC form of the dmu entry above) writes dpre [B][A].  The fused form (A <= 32, (B A + 4096) floats of LDS) computes dpre
 * in LDS and from it dp2 [B][H] = (dpre w) * (p2 > 0), dw [A][H] = dpre^T p2, db [A] = column sums of dpre, for the layer
 * Linear(H, A) with weight w [A][H] and post-ReLU input p2 [B][H]; da1 / da2 are read as columns [col0, col0 + A) of
 * [B][ld] buffers or, when `part` is given, as the sums of splitk partial records [2 splitk][B][A] of the two
 * input-gradient GEMMs (head 1's records first). */
int drq_actor_dmu_bc(const float* dha1, const float* dha2, long ld, int col0, const float* mu, const float* act,
                     long lda, const float* a_beh, long ldb, float bc_scale, float* dpre, int B, int A,
                     drq_stream_t stream);
int drq_policy_out_bwd_bc(const float* da1, const float* da2, long ld, int col0, const float* mu, const float* act,
                          long lda, const float* a_beh, long ldb, float bc_scale, const float* p2, const float* w,
                          float* dp2, float* dw, float* db, int B, int H, int A, const float* part, int splitk,
                          drq_stream_t stream);

/* ---- torch.optim.Adam.step (drqv2.py:148-150,201-202,221; defaults) over a flat arena; optional fused
 * utils.soft_update_params (utils.py:42-45) into tgt.  g is multiplied by gscale first (1 = exact). */
int drq_adam_flat(float* p, const float* g, float* m, float* v, long n, double lr, long step, float gscale,
                  float* tgt, double tau, drq_stream_t stream);
/* ---- data-parallel exchanges on a fully connected xGMI node (new): the `world` ranks' copies of this rank's
 * slice of a gradient bucket, as an all-to-all delivers them (copy r at in[r*stride + i]), are added in RANK ORDER (the
 * same order everywhere: every rank ends with bit-identical sums).  drq_sum_slices writes the sum; drq_adam_reduce_flat
 * (ZeRO-1: sharded optimiser state) feeds it straight into torch.optim.Adam's arithmetic (drq_adam_flat's, bit for bit)
 * for the n parameters this rank owns -- the summed gradient never returns to memory. */
int drq_sum_slices(const float* in, long stride, int world, float* out, long n, drq_stream_t stream);
int drq_adam_reduce_flat(float* p, const float* recv, long stride, int world, float* m, float* v, long n, double lr,
                         long step, float gscale, drq_stream_t stream);
int drq_ema_flat(const float* p, float* t, long n, double tau, drq_stream_t stream);
int drq_fill(float* p, long n, float v, drq_stream_t stream);
/* obs/255-0.5 on raw uint8 frames (drqv2.py:64 as reached from act(), drqv2.py:165-166); y = tanh(x) */
int drq_u8_normalize(const uint8_t* x, float* y, long n, drq_stream_t stream);

/* ---- replay batch assembly on the device (replay_buffer.py:142-160 `_sample`) ----
 * A flat store of steps in HBM (each episode contiguous, its first step the dummy reset transition):
 * frames [n][frame_bytes] u8 (frame_bytes % 16 == 0), action [n][A], reward [n], discount [n].
 * Row b of the batch is the transition at store index pos[b] (device array, the reference's `idx`):
 *   obs = frames[pos-1], action = action[pos], next_obs = frames[pos+nstep-1],
 *   reward/discount = the n-step accumulation in the reference's float32 order
 *   (reward += discount*r[pos+i]; discount *= d[pos+i]*gamma). */
int drq_nstep_gather(const uint8_t* frames, const float* action, const float* reward, const float* discount,
                     const long* pos, int B, int A, long frame_bytes, int nstep, float gamma, uint8_t* obs,
                     float* act_out, float* rew_out, float* disc_out, uint8_t* next_obs, drq_stream_t stream);
int drq_tanh(const float* x, float* y, long n, drq_stream_t stream);

/* ---- proportional prioritized replay (Schaul et al. 2016) on the store above.  New functionality: the reference's
 * replay is uniform; these definitions are the contract.
 * `tree` is double [2 L], L the smallest power of two >= the store's slots: node 1 is the root, the children of node k
 * are 2k and 2k+1, the leaf of slot s is tree[L + s].  Every inner node holds exactly tree[2k] + tree[2k+1]: it is always
 * recomputed from its children, never adjusted by a difference.  tree[0] is the largest leaf value a priority update
 * ever wrote (the caller initialises it, to 1.0).  A leaf is 0 for a slot that must not be drawn, p^alpha otherwise.
 * Each entry is one launch of one workgroup, plain loads and stores, no atomics; the caller orders them on one stream.
 *
 * drq_per_fill: the leaves of slots [lo, hi) become 0 (mode 0) or tree[0] (mode 1: a new episode's drawable
 *   positions), then every ancestor of the range is rebuilt; no other node is touched.  lo == hi: nothing, DRQ_OK.
 *   DRQ_EARG: null tree, L no power of two, not 0 <= lo <= hi <= L, another mode.
 * drq_per_sample: B stratified draws.  u is double [B] in [0, 1); row i aims at the mass (i + u[i]) / B * tree[1] and
 *   descends from the root: at node k with left = tree[2k], right = tree[2k+1] it goes left if
 *   (m < left && left > 0) || right == 0, else m -= left and it goes right.  While the root is positive this never ends
 *   on a zero leaf.  idx_out is int64 [3][B] = pos - 1, pos + nstep - 1, pos (obs frame, next_obs frame, transition:
 *   row 2 is drq_nstep_gather's `pos`).  weight_out is float [B] = (n_valid leaf / tree[1])^(-beta) divided by the largest
 *   such value of the batch, evaluated in double and rounded once; the largest weight is exactly 1.  n_valid is the
 *   caller's count of drawable positions.  A root of 0 must be refused by the caller BEFORE the launch.
 *   DRQ_EARG: null pointers, B <= 0, L no power of two, nstep <= 0, n_valid <= 0, beta < 0.
 * drq_per_update: leaf[pos[i]] = pow((double)td_abs[i] + eps, alpha) for pos int64 [B] and td_abs float [B], both on the
 *   device (a NaN or negative td_abs counts as 0, an infinite one as FLT_MAX).  Where one position occurs in several
 *   rows the row with the HIGHEST index wins, on every run.  Positions outside [0, L) are skipped.  Then the ancestors
 *   are rebuilt and tree[0] = max(tree[0], the leaves written).  Any B.
 *   DRQ_EARG: null pointers, B <= 0, L no power of two, alpha <= 0, eps < 0. */
int drq_per_fill(double* tree, long L, long lo, long hi, int mode, drq_stream_t stream);
int drq_per_sample(const double* tree, long L, const double* u, int B, int nstep, long n_valid, double beta,
                   long* idx_out, float* weight_out, drq_stream_t stream);
int drq_per_update(double* tree, long L, const long* pos, const float* td_abs, int B, double alpha, double eps,
                   drq_stream_t stream);

/* ---- step-major replay for vectorised environments.  New functionality: the reference stores whole episodes of one
 * environment; these definitions are the contract.
 * A ring of R rows x N environments.  Absolute row numbers t = 0, 1, 2, ... count the rows added; row t of environment e
 * lives in slot (t mod R) * N + e of
 *   frames u8 [R N][frame_bytes] (frame_bytes % 16 == 0), action f32 [R N][A], reward f32 [R N], discount f32 [R N],
 *   first u8 [R N].
 * Row t holds the observation after step t and the action, reward and discount that led to it (the reference's episode
 * layout, replay_buffer.py:76-98).  first == 1 marks the dummy reset transition of a new episode (index 0 of an episode
 * file); row 0 always is one.  The transition at (t, e), first[t, e] == 0: obs = frame (t-1, e), action = action[t, e],
 * and the n-step window accumulates over rows t, t+1, ... in the reference's float32 order (reward += discount * r;
 * discount *= d * gamma; one rounding per operation, drq_nstep_gather's arithmetic) but stops early, after k < nstep
 * steps, at the first i > 0 with first[t+i, e] == 1; next_obs = frame (t+k-1, e), steps = k.  A window no reset cuts is
 * replay_buffer.py:142-160 on that environment's episode, a cut one the same with nstep = k, both bit for bit.
 * Drawable rows are lo <= t <= hi, chosen by the caller: with T rows added, hi = T - nstep (the head never cuts a
 * window) and lo = max(1, T - R + 1 + guard_rows) (row t-1 is still in the ring, and guard_rows more rows may be added
 * before a batch whose frames travel as indices is consumed).
 *
 * drq_vec_add: one launch writes row t mod R of the five arrays from device sources for all N environments: src_obs u8
 *   [N][frame_bytes] (16-byte aligned, like frames), src_action [N][A], src_reward [N], src_discount [N], src_first u8 [N]
 *   (non-zero = reset; NULL = all 0).  t == 0 stores first = 1 for every environment whatever src_first says.
 *   DRQ_EARG, nothing written: null pointers (but src_first), R, N, A <= 0, frame_bytes <= 0 or % 16 != 0, t < 0,
 *   misaligned frames / src_obs.
 * drq_vec_sample: one launch draws B transitions.  u is double [B][K] in [0, 1): with M = (hi - lo + 1) N, candidate j
 *   of batch row b is c = min((long)(u[b][j] M), M - 1), t = lo + c / N, e = c % N.  The first candidate that is no
 *   reset row is taken; if all K are reset rows, candidate 0 is walked cyclically through t+1 .. hi, lo .. t-1 of its
 *   environment to the first row that is none.  idx_out int64 [3][B] = the slots of (t-1, e), (t+k-1, e), (t, e): obs
 *   frame, next_obs frame, transition.  act_out [B][A], rew_out [B], disc_out [B], steps_out int32 [B] = k.  If the
 *   environment of candidate 0 has no drawable row at all (a violated precondition) the row gets steps = 0, reward = 0,
 *   discount = 0, all three indices and the action row those of candidate 0's slot; nothing is read out of range.
 *   frames / obs_out / next_obs_out: all NULL (the frames stay in the store) or all given: obs_out, next_obs_out u8
 *   [B][frame_bytes] receive frames[idx_out[0][b]], frames[idx_out[1][b]].
 *   DRQ_EARG, nothing written: null required pointers, R, N, A, B, K, nstep <= 0, frame_bytes <= 0 or % 16 != 0, lo < 1,
 *   hi < lo, hi - lo + 1 + nstep > R (rows lo-1 .. hi+nstep-1 must be distinct ring rows), some but not all of frames /
 *   obs_out / next_obs_out, one of them misaligned. */
int drq_vec_add(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R, long N, int A,
                long frame_bytes, long t, const uint8_t* src_obs, const float* src_action, const float* src_reward,
                const float* src_discount, const uint8_t* src_first, drq_stream_t stream);
int drq_vec_sample(const uint8_t* first, const float* action, const float* reward, const float* discount, long R, long N,
                   int A, long frame_bytes, long lo, long hi, const double* u, int B, int K, int nstep, float gamma,
                   long* idx_out, float* act_out, float* rew_out, float* disc_out, int* steps_out, const uint8_t* frames,
                   uint8_t* obs_out, uint8_t* next_obs_out, drq_stream_t stream);

/* ---- demonstrations in the step-major replay: a frozen partition behind the ring and batches that mix the two (the
 * symmetric sampling of RLPD, the demonstration buffer of DDPGfD).  New functionality; these definitions are the
 * contract.
 * The five arrays of "step-major replay" hold (R + D) N slots.  Rows 0 .. R-1 are the ring, as above: row t of
 * environment e in slot (t mod R) N + e, and nothing that writes or reads the ring knows of the rest.  Rows R .. R+D-1
 * are the PARTITION: linear, never wrapped, never evicted; demonstration row d of lane e lives in slot (R + d) N + e.
 * Its rows are laid out like the ring's (first == 1: a reset or pad row; row 0 always is one) and written by
 * drq_vec_fill called on the partition's base pointers (frames + R N frame_bytes, action + R N A, ...) with R = D and
 * T = Td, the rows filled so far; Td <= D.  Its drawable rows are 1 .. Td - nstep.
 *
 * drq_vec_sample_mixed: one launch, shaped like drq_vec_sample, draws B transitions: batch rows b < Bd from the
 *   partition, rows b >= Bd from the ring.  Every row is drq_vec_sample's row for its own geometry -- the ring with
 *   (R, lo, hi), the partition with (D, 1, Td - nstep) -- from its own u[b][0 .. K): the K candidates, the walk along
 *   candidate 0's lane, the steps = 0 row, the window, the n-step sum.  idx_out int64 [3][B] indexes the WHOLE allocation:
 *   a ring row's three slots are < R N, a partition row's are R N + its slots in the partition; obs_out / next_obs_out,
 *   if given, receive frames[idx_out[0][b]], frames[idx_out[1][b]].  Bd = 0 is drq_vec_sample on the ring, Bd = B a
 *   draw from the partition alone, for which lo and hi are not read (no live row need exist).  Plain vector stores, no
 *   atomics, nothing crosses workgroups.
 *   DRQ_EARG, nothing written: everything drq_vec_sample refuses (the ring's lo / hi only when Bd < B); D <= 0, Td < 0,
 *   Td > D, Bd < 0, Bd > B; Bd > 0 with Td - nstep < 1; Bd < B with no drawable ring row (hi < lo). */
int drq_vec_sample_mixed(const uint8_t* first, const float* action, const float* reward, const float* discount, long R,
                         long D, long N, int A, long frame_bytes, long lo, long hi, long Td, const double* u, int B,
                         int Bd, int K, int nstep, float gamma, long* idx_out, float* act_out, float* rew_out,
                         float* disc_out, int* steps_out, const uint8_t* frames, uint8_t* obs_out, uint8_t* next_obs_out,
                         drq_stream_t stream);

/* ---- prioritized step-major replay: proportional prioritization (the definitions of "proportional prioritized replay"
 * above) on the ring of "step-major replay".  New functionality; these definitions are the contract.
 * `tree` is the sum tree of drq_per_*: double [2 L], L the smallest power of two >= R N, the leaf of slot s at tree[L + s],
 * every inner node recomputed as tree[2k] + tree[2k+1], never adjusted; tree[0] the largest leaf a priority update ever
 * wrote (the caller initialises it to 1.0, and every leaf to 0).  T is the number of rows added so far, lo .. hi the
 * drawable rows (hi = T - nstep, lo = max(1, T - R + 1 + guard_rows)).  Ring row r holds the absolute row
 * t(r) = T-1 - ((T-1-r) mod R); a slot p is DRAWABLE if 0 <= p < R N, lo <= t(p / N) <= hi and first[p] == 0.
 * Invariant the caller keeps by calling drq_vec_per_advance after every drq_vec_add: a leaf is > 0 iff its slot is
 * drawable (eps > 0); every other leaf -- the padding above R N, guard rows, head rows, reset rows -- is exactly 0.
 * Each entry is one launch of one workgroup of 1,024 threads, plain loads and stores, no atomics; the caller orders
 * them, and drq_vec_add, on one stream.  Any N and any B.
 *
 * drq_vec_per_advance: an add moves hi and lo by at most one row.  enter_t = the absolute row that became drawable (the
 *   new hi, if hi >= lo), leave_t = the one that stopped being (the old lo, if lo advanced), -1 = none; the caller knows
 *   both from T, R, nstep and guard_rows alone.  The N leaves of row enter_t become first ? 0 : tree[0] (the flags were
 *   written by the drq_vec_add of that row, nstep - 1 adds earlier), those of row leave_t 0, and the ancestors of both
 *   ranges are recomputed.  Both -1: DRQ_OK without a launch.
 *   DRQ_EARG: null pointers, L no power of two or < R N, R, N, T <= 0, enter_t / leave_t outside [-1, T) or no longer in
 *   the ring (< T - R), enter_t == leave_t >= 0.
 * drq_vec_per_sample: B stratified draws, u double [B] in [0, 1): drq_per_sample's descent, verbatim, to a slot p;
 *   e = p % N, t = t(p / N); from there drq_vec_sample's outputs for the transition (t, e): the window k cut at the
 *   first reset row, idx_out int64 [3][B] = the slots of (t-1, e), (t+k-1, e), (t, e), act_out [B][A], rew_out, disc_out
 *   [B] in the same float32 operation order, steps_out int32 [B] = k.  weight_out float [B] =
 *   (n leaf / tree[1])^(-beta) divided by the largest such value of the batch (evaluated in double, rounded once, the
 *   largest exactly 1), n = (hi - lo + 1) N: the nominal count, reset rows included -- it cancels against the maximum,
 *   so no count of the valid positions is needed.  The tree is not written.  An empty tree (tree[1] == 0: every
 *   drawable row is a reset row, which the host cannot know) gives every batch row all three indices and the action row
 *   of slot(lo, 0), steps = 0, reward = 0, discount = 0, weight = 1; so does a row whose descent ends on a slot that is
 *   not drawable (a broken invariant).  Nothing is read out of range, no NaN.
 *   DRQ_EARG, nothing written: null pointers, L no power of two or < R N, R, N, A, B, nstep <= 0, beta < 0, lo < 1,
 *   hi < lo, hi - lo + 1 + nstep > R, hi + nstep > T, lo - 1 < T - R.
 * drq_vec_per_update: leaf[pos[i]] = pow(clamp(td_abs[i]) + eps, alpha) as drq_per_update (NaN / negative -> 0,
 *   inf -> FLT_MAX; the row with the HIGHEST index of a repeated position wins), but ONLY where pos[i] is drawable at
 *   the time of the call: a row that is not writes nothing and does not count for tree[0].  Then the ancestors of every
 *   pos[i] in [0, L) are recomputed (those of a skipped row get the sums they held) and tree[0] = max(tree[0], the
 *   leaves written).  The caller drops a whole batch once its slots may have been overwritten (guard_rows rows added).
 *   DRQ_EARG: null pointers, L no power of two or < R N, R, N, B <= 0, alpha <= 0, eps < 0, lo < 1, hi < lo,
 *   hi - lo + 2 > R, hi + 1 > T, lo - 1 < T - R. */
int drq_vec_per_advance(double* tree, long L, const uint8_t* first, long R, long N, long T, long enter_t, long leave_t,
                        drq_stream_t stream);
int drq_vec_per_sample(const double* tree, long L, const uint8_t* first, const float* action, const float* reward,
                       const float* discount, long R, long N, int A, long T, long lo, long hi, const double* u, int B,
                       int nstep, float gamma, double beta, long* idx_out, float* act_out, float* rew_out,
                       float* disc_out, int* steps_out, float* weight_out, drq_stream_t stream);
int drq_vec_per_update(double* tree, long L, const uint8_t* first, long R, long N, long T, long lo, long hi,
                       const long* pos, const float* td_abs, int B, double alpha, double eps, drq_stream_t stream);

/* ---- single-frame step-major replay: the ring stores ONE frame per slot and a frame stack is put together where it is
 * read.  New functionality (the reference stacks in the environment wrapper, dmc.py:87-109, and stores every stack
 * whole: two thirds of each slot repeat its neighbours); these definitions are the contract.
 * Storage: the ring of "step-major replay", R rows x N environments, with frames u8 [R N][fb], fb = 3*84*84 = 21168: one
 *   CHW frame per slot, the newest frame of the observation after step t.  action, reward, discount and first are
 *   unchanged, and so are drq_vec_add (frame_bytes = fb), drq_vec_sample (without frame outputs) and the
 *   drq_vec_per_* entries.
 * The stack at (t, e) is what FrameStackWrapper holds after step t (dmc.py:87-88, 98-109): three frames concatenated
 *   along the channel axis, oldest first, refilled with the first frame on reset.  With p0 = slot(t, e),
 *   p1 = slot(t-1, e), p2 = slot(t-2, e), rows modulo R:
 *     first[p0] != 0       -> (p0, p0, p0)
 *     else first[p1] != 0  -> (p1, p1, p0)
 *     else                 -> (p2, p1, p0)
 *   Row 0 is always a reset row, so no row below 0 is ever addressed; whatever the flags hold, every slot read lies in
 *   the ring, and first[p1] is read only where first[p0] does not decide.
 * Transitions are as before: at (t, e), obs is the stack at (t-1, e), next_obs the stack at (t+k-1, e); idx_out[0] and
 *   idx_out[1] of the draws are the slots of the NEWEST frame of each stack.
 * Drawable rows: hi = T - nstep, lo = max(1, T - R + 1 + guard_rows + 2).  The two extra rows keep the oldest frame of an
 *   obs stack (row t-3) inside the ring while guard_rows rows are added; R >= nstep + guard_rows + 4.
 *
 * drq_vec_stack_gather: one launch writes out u8 [n][3 frame_bytes], row b = the stack whose newest frame is slot
 *   slots[b] (int64 [n] on the device, each in [0, R N); a slot outside leaves its row unwritten and reads nothing).
 *   slots == NULL: the n = N stacks of absolute row t >= 0, environment b in row b -- the observations after step t.
 *   16-byte loads and stores; any frame_bytes % 16 == 0.
 *   DRQ_EARG, nothing written: null frames / first / out, R, N, n, frame_bytes <= 0, frame_bytes % 16 != 0, frames or out
 *   not 16-byte aligned, slots not 8-byte aligned; without slots: t < 0 or n != N. */
int drq_vec_stack_gather(const uint8_t* frames, const uint8_t* first, long R, long N, long frame_bytes,
                         const int64_t* slots, long t, int n, uint8_t* out, drq_stream_t stream);

/* ---- renderer images: an add on the single-frame ring above that takes the image as a GPU renderer hands it out and
 * resizes it on the way in.  New functionality (the reference renders 84 x 84 on the host, dmc.py); these definitions
 * are the contract.
 * src_image is u8 [N][S][S][Cin], channels last, square, S = 84 .. 336, Cin = 3 or 4; a fourth channel (alpha, padding)
 * is never read.  The frame written is u8 [3][84][84], the exact area average in integer arithmetic, no float anywhere:
 *   Measure an image axis in units of 1/84 input pixel: input pixel i covers [84 i, 84 (i+1)), output pixel o covers
 *   [S o, S (o+1)), and the weight of i in o is their overlap
 *     w(o, i) = max(0, min(S (o+1), 84 (i+1)) - max(S o, 84 i)).
 *   Every row of w sums to S, every column to 84, and a row has at most 5 non-zero entries for S <= 336 (at most 4
 *   for S <= 256 and for S = 336; 5 first at S = 257).
 *     frame[e][c][y][x] = (sum_i sum_j w(y, i) w(x, j) image[e][i][j][c] + (S S) / 2) / (S S),   c = 0, 1, 2,
 *   both divisions integer divisions (round half up).  The sum is at most 255 S^2, and with the rounding term
 *   255.5 * 336^2 = 28,844,928 < 2^31: 32-bit integers hold it.  S ends at 336 = 4 * 84: up to there a row of w has
 *   at most 5 entries and the input rows of 4 output rows, with their horizontal sums, take 41 KB of LDS at most.
 *   Consequences: S = 84 is the plain HWC -> CHW transposition; S = 84 k gives the mean of each k x k block rounded half
 *   up, (sum + k^2 / 2) / k^2; a constant image stays constant.
 *
 * drq_vec_add_render: drq_vec_add for a ring with frame_bytes = 21168 whose frame source is such an image: one launch
 *   writes frames[(t mod R) N + e][21168] by the rule above for all N environments, and row t mod R of action, reward,
 *   discount and first exactly as drq_vec_add does from the same sources (t == 0 stores first = 1 for every environment;
 *   src_first NULL = all 0).  Nothing outside the image is read, nothing outside the row is written.
 *   DRQ_EARG, nothing written: null pointers (but src_first), R, N, A <= 0, t < 0, S outside 84 .. 336, Cin not 3 or 4,
 *   frames not 16-byte aligned, src_image not 4-byte aligned; N > INT32_MAX / 21 (one workgroup per environment and
 *   band of 4 output rows). */
int drq_vec_add_render(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R, long N,
                       int A, long t, const uint8_t* src_image, int S, int Cin, const float* src_action,
                       const float* src_reward, const float* src_discount, const uint8_t* src_first,
                       drq_stream_t stream);

/* ---- single frames in the episode store: the flat store of "replay batch assembly on the device" with ONE frame per
 * slot.  It is the ring above with N = 1 and R = the store's slots: frames u8 [R][frame_bytes], action f32 [R][A], reward
 * and discount f32 [R], first u8 [R].  Every episode is contiguous, its first slot (the dummy reset transition) carries
 * first = 1 and its other slots first = 0; the flags of slots no live episode covers hold whatever an evicted episode
 * left.  The stack whose newest frame is slot p0 follows the rule above (p1 = p0 - 1, p2 = p0 - 2), and equals what
 * FrameStackWrapper held at that step.  Stale flags are harmless: a flag is read only for slots of the live episode
 * that holds the position drawn, at or before the slot drawn; p2 is read only where first[p0] == first[p1] == 0, that is
 * two slots or more past the episode's start; an episode that starts at slot 0 has first[0] = 1.  So no read leaves
 * the episode and the modulo wrap of the rule is never taken.  drq_conv1_aug_fwd_frames, drq_update_phase_frames and
 * drq_vec_stack_gather serve this store unchanged (N = 1).
 *
 * drq_nstep_gather_frames: drq_nstep_gather on such a store, one launch.  Row b of the batch is the transition at
 *   pos[b] (int64 [B] on the device): obs[b] = the stack whose newest frame is slot pos[b]-1, next_obs[b] = the stack at
 *   pos[b]+nstep-1, each 3 frame_bytes bytes, oldest frame first (obs, next_obs u8 [B][3 frame_bytes]); act_out [B][A] =
 *   action[pos], rew_out / disc_out [B] = the n-step accumulation in drq_nstep_gather's float32 operation order, bit
 *   for bit what that entry yields.  obs == NULL && next_obs == NULL: the scalars only.  16-byte loads and stores; any
 *   frame_bytes % 16 == 0.  A pos[b] < 1 or > R - nstep (slot pos-1 or the window pos .. pos+nstep-1 would leave
 *   [0, R)) leaves every output of its row unwritten and reads nothing; whatever the flags hold, every slot read lies in
 *   [0, R).
 *   DRQ_EARG, nothing launched: a null pointer (obs and next_obs: exactly one of the two), R, B, A, nstep,
 *   frame_bytes <= 0, frame_bytes % 16 != 0 (or beyond 85 MB), frames / obs / next_obs not 16-byte aligned, pos not
 *   8-byte aligned, a float array not 4-byte aligned. */
int drq_nstep_gather_frames(const uint8_t* frames, const uint8_t* first, long R, const float* action,
                            const float* reward, const float* discount, const long* pos, int B, int A, long frame_bytes,
                            int nstep, float gamma, uint8_t* obs, float* act_out, float* rew_out, float* disc_out,
                            uint8_t* next_obs, drq_stream_t stream);

/* ---- episode statistics for vectorised collection.  New functionality: the reference adds up episode_reward and
 * episode_step of its one environment on the host (train.py:133,186,189) and logs them per finished episode
 * (:147-155); for N lockstep environments the sums live on the device, fed by the reward and first tensors of
 * "step-major replay", and the host never reads a flag.  These definitions are the contract.  No store is involved.
 * State, all on the device:
 *   per environment e: ret f32 [N] the running return, len i32 [N] the running length, done i32 [N] the episodes of e
 *     closed so far (counted or not; it stops at INT32_MAX);
 *   header, 64 bytes, 8-byte aligned: rows i64 @0 (the number of step calls), episodes i64 @8, length_sum i64 @16,
 *     return_sum f64 @24, min_return f32 @32 (+inf at the start), max_return f32 @36 (-inf), 24 reserved bytes (0);
 *   a log of W records kept as four arrays: log_return f32 [W], log_length i32 [W], log_env i32 [W], log_row i64 [W].
 * The step at call number t = row (the caller counts the calls; the entry stores rows = row + 1), for every e:
 *   f = (t == 0) || (first != NULL && first[e] != 0): call 0 is a reset row for every environment, as row 0 of the ring.
 *   If f and len[e] >= 1 the running episode of e is finished (a reset with len[e] == 0 -- the first row, two resets in a
 *     row -- closes nothing): if limit == 0 || done[e] < limit it is COUNTED, a record (ret[e], len[e], e, t) and the
 *     header totals; done[e] += 1 in either case.
 *   If f: ret[e] = 0, len[e] = 0, and reward[e], a dummy, is not read.  Otherwise ret[e] = ret[e] + reward[e], ONE float32
 *     add per step in step order (train.py:186 on float32 rewards), and len[e] += 1.
 * Records.  The episodes counted by one call get the consecutive global numbers j = episodes_before + rank, rank = the
 *   number of counted environments with a smaller index; record j lives at index j mod W.  The log so holds the newest
 *   min(episodes, W) episodes in the order (row, env), deterministically.
 * Totals.  episodes, length_sum, min_return and max_return are exact; return_sum adds the counted float32 returns in
 *   float64, within a call in the kernel's own order.
 * limit = k > 0 (evaluation): only the first k episodes of every environment are counted, later ones still reset ret and
 *   len; the statistics are complete when episodes == k N.
 * Each entry is one launch of one workgroup of 1,024 threads, plain loads and stores, no atomics; the caller orders them
 * on one stream.  Any N up to INT32_MAX, any W.
 *
 * drq_vec_stats_step: the step above.  reward f32 [N] (may be NULL on row 0), first u8 [N] or NULL = no flags.
 *   DRQ_EARG, nothing launched: a null state pointer, N < 1 or > INT32_MAX, W < 1, limit < 0, row < 0, a null reward with
 *   row > 0, header or log_row not 8-byte aligned.
 * drq_vec_stats_publish: copies header and log into host_mirror (pinned host memory, 8-byte aligned), laid out as
 *   [header 64 bytes | log_return f32 [W] | log_length i32 [W] | log_env i32 [W] | 4 bytes of padding if W is odd |
 *    log_row i64 [W] | seq u32]: 64 + 20 W + 4 (W odd ? 2 : 1) bytes.  Then __threadfence_system(), a workgroup barrier,
 *   and a system-scope release store of seq by one lane (the protocol of drq_publish_sums): a host that reads seq reads
 *   the state of every step enqueued before.
 *   DRQ_EARG, nothing launched: a null pointer, W < 1, header / log_row / host_mirror not 8-byte aligned.
 * drq_vec_stats_reset: one launch puts ret, len, done, the header and the log back to the initial state (zeros; min +inf,
 *   max -inf); the caller's next step is row 0 again.  DRQ_EARG as for the step. */
int drq_vec_stats_step(float* ret, int* len, int* done, void* header, float* log_return, int* log_length, int* log_env,
                       long* log_row, long N, long W, int limit, long row, const float* reward, const uint8_t* first,
                       drq_stream_t stream);
int drq_vec_stats_publish(const void* header, const float* log_return, const int* log_length, const int* log_env,
                          const long* log_row, long W, void* host_mirror, unsigned seq, drq_stream_t stream);
int drq_vec_stats_reset(float* ret, int* len, int* done, void* header, float* log_return, int* log_length, int* log_env,
                        long* log_row, long N, long W, drq_stream_t stream);

/* ---- device environment.  New functionality: the reference steps one dm_control environment on the host (dmc.py,
 * train.py:160-190); this is a small pixel task that lives on the device and steps N lockstep environments with one
 * launch, the reference producer of what "single-frame step-major replay", "renderer images" and "episode statistics"
 * consume.  It is no benchmark task.  These definitions are the contract; they are exact to the bit.
 * The task ("reach"): a point in the square [-1, 1]^2 must reach a target.  State per environment e, all on the device:
 *   pos f32 [N][2], target f32 [N][2], t i32 [N] (the steps taken in this episode), episode u32 [N] (counts the episodes
 *   of e; 0 before the first reset), over u8 [N] (1 = the last step ended the episode).
 * Every float operation below is ONE IEEE float32 operation, in the written order, never fused.
 * Reset of e (when reset_all = 1, or in a step when over[e] == 1):
 *   episode += 1 (mod 2^32), t = 0, over = 0; four draws k = 0 .. 3 give pos.x, pos.y, target.x, target.y:
 *     h = fmix32(seed ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ k * 0xC2B2AE35) in uint32 arithmetic, episode the new count,
 *     fmix32 the murmur3 finaliser (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16);
 *     u = float(h >> 8) * 2^-24;  v = (u * 2 - 1) * 0.9f
 *   outputs: first = 1, reward = 0, discount = 1, the frame of the new state.  The action of e is not read.
 * Step of e (every environment that is not being reset):
 *   a = action[e][0 .. 1]; a NaN becomes 0, otherwise a < -1 becomes -1 and a > 1 becomes 1; columns 2 .. A-1 are not read
 *   pos = clamp(pos + a * 0.1f, -1, 1) per component (a multiply, an add, the clamp);  t += 1
 *   dx = pos.x - target.x, dy = pos.y - target.y;  d2 = dx * dx + dy * dy;  r = 1 - d2;  reward = r > 0 ? r : 0
 *   d2 <= 0.01f: discount = 0, over = 1 (reached: a true terminal);  else t == episode_length: discount = 1, over = 1
 *   (the time limit);  else discount = 1.  first = 0.
 * Frame of a state, u8 [3][84][84], pixel (i, j) = row i, column j:
 *   cx = (int)floorf((x + 1) * 41.5f + 0.5f) and cy likewise from y, for pos (the agent) and for target: 0 .. 83
 *   background 32 + ((i + j) >> 2) in all three channels;  the target, a disc (j-cx)^2 + (i-cy)^2 <= 25 in (64, 255, 64);
 *   the agent drawn over it, a disc <= 16 in (255, 64, 64).  Integers after the two centres.
 *
 * drq_vec_reach_step: one launch advances all N states by the rules above and writes frame u8 [N][3][84][84], reward and
 *   discount f32 [N], first u8 [N]: every byte of the four, nothing else but the state.  reset_all = 1 resets every
 *   environment (action may be NULL then).  N workgroups of 256 threads, one per environment: every lane reads the old
 *   state, a workgroup barrier, one lane stores the new state and the scalars, all store the frame as 16-byte pieces.
 *   No state of one environment is touched by another's workgroup; the caller orders the launches on one stream.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 2,
 *   episode_length < 1, reset_all not 0 or 1, frame not 16-byte aligned, a float / int array not 4-byte aligned.
 * drq_vec_reach_render: the frames of the states as they are, u8 [N][3][84][84], by the frame rule above: every byte of
 *   frame, nothing else -- pos and target are only read, t / episode / over are not involved.  After a step or a reset it
 *   writes exactly the frame that call wrote (the same device function); it is what a restored environment shows before
 *   its next step.  N workgroups of 256 threads, 16-byte pieces, like the frame part of drq_vec_reach_step.
 *   DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX, frame not 16-byte aligned, pos or target not
 *   4-byte aligned.
 * drq_vec_reach_image: the renderer-shaped image of such frames, u8 [N][S][S][C], S = 84 k, k = 1 .. 4, C = 3 or 4:
 *   image[e][y][x][c] = frame[e][c][y / k][x / k] for c < 3 and 255 for c == 3 -- every pixel k x k times, channels last.
 *   The area average of "renderer images" returns the frame exactly ((k^2 v + k^2 / 2) / k^2 = v).
 *   DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX, S not 84, 168, 252 or 336, C not 3 or 4, frame or
 *   image not 16-byte aligned.
 *
 * Tasks and action repeat.  drq_vec_task_step steps a family of tasks over the same square, each launch a MACRO step of up
 * to `repeat` sub-steps -- the ActionRepeatWrapper of dmc.py:35-50 inside the launch, since an environment that ends in
 * the middle of a repeat must stop there.  task: DRQ_TASK_REACH (0), the task above, or DRQ_TASK_POINTMASS (1).
 * Macro step of e:
 *   reset row (reset_all = 1, or over[e] == 1): the reset above, and vel = 0 for the point mass.  Outputs first = 1,
 *     reward = 0, discount = 1, substeps = 0.  The action is not read.
 *   otherwise: reward = 0, discount = 1, the action sanitised ONCE as above (NaN becomes 0, then the clamp to [-1, 1]).
 *     For i = 0 .. repeat-1: one sub-step of the task gives (r_i, d_i, over);
 *       reward = reward + r_i * discount (one multiply, then one add);  discount = discount * d_i;
 *       stop after the sub-step that set over.
 *     first = 0, substeps = the sub-steps executed (1 .. repeat).  t counts sub-steps, so episode_length is in simulator
 *     steps, as in DMC.  The frame is drawn once, from the state after the last executed sub-step, by the frame rule above.
 *   repeat = 1 is the step above bit for bit: 0 + r * 1 = r for r >= 0, and 1 * d = d.
 * Sub-step of reach: "Step of e" above without the sanitising: the move, t += 1, reward r_i, d_i = 0 with over when
 *   reached, else d_i = 1 and over at the time limit.
 * Sub-step of the point mass.  State vel f32 [N][2] beside the rest.  Per axis, a the sanitised action of that axis:
 *   v = v * 0.9f;  v = v + a * 0.02f;  p = pos + v
 *   p < -1: pos = -1, v = 0;  p > 1: pos = 1, v = 0;  otherwise pos = p          (a wall stops the axis that hit it)
 *   then t += 1;  d2 and r_i = max(0, 1 - d2) as in reach;  d_i = 1 always: touching the target does not end the episode;
 *   over only when t == episode_length.  Reset draws and frame rule are those of reach: velocity is in no frame.
 * drq_vec_task_step: writes every byte of frame, reward, discount, first and substeps (i32 [N]) and the state -- vel only
 *   for the point mass; for reach vel is neither read nor written and may be NULL.  The launch shape is that of
 *   drq_vec_reach_step, which is this entry with task reach, repeat 1 and no substeps output; the trip count of the
 *   sub-step loop is uniform across a workgroup.  drq_vec_reach_render and drq_vec_reach_image serve both tasks.
 *   DRQ_EARG, nothing launched: every condition of drq_vec_reach_step, an unknown task, repeat < 1 or
 *   > DRQ_TASK_MAX_REPEAT, a null substeps, a null vel for the point mass, vel or substeps not 4-byte aligned. */
enum { DRQ_TASK_REACH = 0, DRQ_TASK_POINTMASS = 1 };
#define DRQ_TASK_MAX_REPEAT 16
int drq_vec_task_step(int task, float* pos, float* target, float* vel, int* t, unsigned* episode, uint8_t* over, long N,
                      int A, const float* action, unsigned seed, int episode_length, int repeat, int reset_all,
                      uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps, drq_stream_t stream);
int drq_vec_reach_step(float* pos, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                       const float* action, unsigned seed, int episode_length, int reset_all, uint8_t* frame,
                       float* reward, float* discount, uint8_t* first, drq_stream_t stream);
int drq_vec_reach_render(const float* pos, const float* target, long N, uint8_t* frame, drq_stream_t stream);
int drq_vec_reach_image(const uint8_t* frame, uint8_t* image, long N, int S, int C, drq_stream_t stream);

/* Cartpole.  A third task of the device environment, with entries of its own: a cart on a rail carries a free pole, the
 * action pushes the cart.  swing_up = 1 starts every episode with the pole hanging down (the reference's
 * cartpole_swingup, cfgs/task/easy.yaml), swing_up = 0 with the pole near upright (cartpole_balance).  The action acts
 * through second-order coupled dynamics, and upright is an unstable equilibrium.  These definitions are the contract; they
 * are exact to the bit.  Every float operation below is ONE correctly rounded IEEE float32 operation (+, -, *, / or
 * sqrt), in the written order, never fused; there is no sin, cos or exp anywhere: the pole's angle theta, measured from
 * upright, is held as the unit vector (c, s) = (cos theta, sin theta).
 * State per environment e: phys f32 [N][5] = (x, xdot, c, s, omega): the cart's position and velocity, the pole's unit
 *   vector and angular velocity; t i32 [N], episode u32 [N], over u8 [N] as above.
 * normalise(c, s):  n = sqrt(c * c + s * s);  c = c / n;  s = s / n;  then one correction by the defect of the length,
 *   which leaves c * c + s * s within 1 ulp of 1 (the five operations before it leave it within 3):
 *   split(a):  t = a * 4097;  hi = t - (t - a);  lo = a - hi              (Veltkamp: hi * hi, hi * lo, lo * lo are exact)
 *   square(a): p = a * a;  q = hi * lo;  err = ((hi * hi - p) + (q + q)) + lo * lo      (Dekker: p + err = a * a exactly)
 *   (pc, ec) = square(c);  (ps, es) = square(s);  d = (1 - pc) - ps if pc >= ps, otherwise d = (1 - ps) - pc;
 *   d = d - (ec + es);  g = d * 0.5f;  c = c + c * g;  s = s + s * g.
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; two draws v_0, v_1 as above
 *   (the same hash of (seed, e, episode, k), v = (u * 2 - 1) * 0.9f):
 *   x = v_0 * 0.1f;  xdot = 0;  omega = 0;  c = -1 for swing_up, 1 for balance;  s = v_1 * 0.05f;  normalise(c, s).
 *   Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The action is not read.
 * Sub-step, a the sanitised action (a = action[e][0]; NaN becomes 0, then the clamp to [-1, 1]; columns 1 .. A-1 are not
 *   read).  dt = 0.01, force 10 a, cart mass 1, pole mass 0.1, pole half-length 0.5, g = 9.8; the frictionless equations:
 *   F = a * 10;  t1 = omega * omega;  t1 = 0.05f * t1;  t1 = t1 * s;  temp = (F + t1) / 1.1f
 *   num = 9.8f * s - c * temp                                  (two multiplies, then the subtraction)
 *   q = c * c;  q = 0.1f * q;  q = q / 1.1f;  den = 1.3333334f - q;  den = 0.5f * den;  thacc = num / den
 *   r = 0.05f * thacc;  r = r * c;  r = r / 1.1f;  xacc = temp - r
 *   omega = clamp(omega + thacc * 0.01f, -32, 32);  xdot = clamp(xdot + xacc * 0.01f, -16, 16)        (semi-implicit Euler)
 *   p = x + xdot * 0.01f;  p < -1.8f: x = -1.8f, xdot = 0;  p > 1.8f: x = 1.8f, xdot = 0;  otherwise x = p  (the rail ends)
 *   h = omega * 0.01f;  c' = c - s * h;  s' = s + c * h  (both from the old c and s);  (c, s) = normalise(c', s')
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always.  Every reachable state is finite: den >= 0.62,
 *   |omega|, |xdot| and |x| are bounded, and n >= 1 up to rounding.
 *   Reward r_i in [0, 1], of the new state and a -- DMC cartpole's product with rational sigmoids for its Gaussian ones:
 *   up = (c + 1) * 0.5f;  ce = 1 / (1 + x * x);  ce = (1 + ce) * 0.5f;  co = (4 + (1 - a * a)) / 5
 *   w = omega / 5;  sl = 1 / (1 + w * w);  sl = (1 + sl) * 0.5f;  r_i = ((up * ce) * co) * sl
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1: reward = reward + r_i for up to `repeat` sub-steps,
 *   stopping after the one that set over; discount = 1, first = 0, substeps = the sub-steps executed.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel; pixel (i, j) has its centre at
 *   (16 j + 8, 16 i + 8).  320 units (20 pixels) are one unit of x and the pole's length, so the pole is fully visible
 *   for |x| <= 0.9, half the rail.  The pivot is (X0, 672), the pole's tip (X1, Y1), each rounded once:
 *   xs = x * 320;  X0 = (int)floorf(xs + 672.5f);  X1 = (int)floorf((xs + s * 320) + 672.5f);  Y1 = (int)floorf(672.5f - c * 320)
 *   Everything after that is integer arithmetic.  Per pixel, with P = (16 j + 8, 16 i + 8), later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels;
 *   the rail, i == 42 and |P.x - 672| <= 576, in (64, 64, 255);
 *   the cart, |P.x - X0| <= 96 and |P.y - 672| <= 48, in (64, 255, 64);
 *   the pole, a capsule of radius 24 around the segment pivot -- tip, in (255, 64, 64): with v = P - pivot, d = tip - pivot,
 *     dot = v.d, dd = d.d (int32):  dot <= 0: |v|^2 <= 576;  dot >= dd: |P - tip|^2 <= 576;  otherwise
 *     cross = v.x * d.y - v.y * d.x and cross * cross <= 576 * dd, both sides in int64 (cross^2 reaches about 10^12).
 *   Shapes that leave the frame are clipped by the pixel loop itself.
 *
 * drq_vec_cartpole_step: one launch, N workgroups of 256 threads with the shape of drq_vec_task_step: every lane computes the
 *   macro step in registers (the trip count is uniform across a workgroup), a workgroup barrier, one lane stores the state
 *   and the scalars, all store the frame as 1,323 pieces of 16 bytes.  Writes every byte of frame, reward, discount, first,
 *   substeps and the state, nothing else.  No LDS, no atomics, nothing crosses workgroups.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 1, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all or swing_up not 0 or 1, frame not 16-byte aligned, a float /
 *   int array not 4-byte aligned.
 * drq_vec_cartpole_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; phys is only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX,
 *   frame not 16-byte aligned, phys not 4-byte aligned.  drq_vec_reach_image serves these frames as it serves any. */
int drq_vec_cartpole_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                          unsigned seed, int episode_length, int repeat, int reset_all, int swing_up, uint8_t* frame,
                          float* reward, float* discount, uint8_t* first, int* substeps, drq_stream_t stream);
int drq_vec_cartpole_render(const float* phys, long N, uint8_t* frame, drq_stream_t stream);

/* Reacher.  A fourth task of the device environment, with entries of its own: a planar arm of two links, seen from above
 * (no gravity), driven by a torque at the shoulder and one at the elbow; the fingertip must be brought into a target
 * disc of radius target_radius.  sparse = 1 pays 1 while the fingertip is inside the disc and 0 otherwise -- in the image
 * of the reference's reacher_easy and reacher_hard (the files under cfgs/task; target_radius about 0.15 and 0.05), not a port of
 * them; sparse = 0 pays a dense shaping of the same distance.  These definitions are the contract; they are exact to the
 * bit.  Every float operation below is ONE correctly rounded IEEE float32 operation (+, -, *, / or sqrt), in the written
 * order, never fused; there is no sin, cos or exp anywhere: the shoulder's angle is held as the unit vector (c1, s1), the
 * elbow's angle, relative to the upper arm, as (c2, s2).  normalise, the draws v_k and the sanitising are those above.
 * State per environment e: phys f32 [N][6] = (c1, s1, w1, c2, s2, w2), w the angular velocities; target f32 [N][2];
 *   t i32 [N], episode u32 [N], over u8 [N] as above.  0.02 <= target_radius <= 0.3.
 * Geometry.  Both links have length 0.5:  c12 = c1 * c2 - s1 * s2;  s12 = s1 * c2 + c1 * s2  (the forearm's direction);
 *   tip.x = 0.5f * c1 + 0.5f * c12;  tip.y = 0.5f * s1 + 0.5f * s12         (two multiplies, then the add, per component)
 * direction(v), the unit vector of a draw v in [-0.9, 0.9]: a walk round the diamond |x| + |y| = 1, normalised:
 *   u = clamp(v * 1.1111112f, -1, 1);  x = 1 - 2 * |u|;  y = 1 - |x|, negated for u < 0;
 *   x * x + y * y < 0.25f: (1, 0)  (a degenerate pair; no point of the diamond is one);  otherwise normalise(x, y).
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; four draws v_0 .. v_3:
 *   (c1, s1) = direction(v_0);  (c2, s2) = direction(v_1);  w1 = w2 = 0;
 *   (gx, gy) = direction(v_2);  f = 0.5f + v_3 * 0.5f;  rho = (1 - target_radius) * f;  target = (rho * gx, rho * gy)
 *   f is in [0.05, 0.95], so |target| + target_radius < 1: the whole disc lies where the fingertip can go.
 *   Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The action is not read.
 * Sub-step, (a1, a2) the sanitised action (action[e][0] the shoulder's torque, action[e][1] the elbow's, each NaN to 0,
 *   then the clamp to [-1, 1]; columns 2 .. A-1 are not read).  Two point masses of 1 at the ends of the links, dt = 0.01,
 *   torque K = 2 per unit of action, viscous damping b = 0.5 at both joints:
 *   M11 = 0.75f + 0.5f * c2;  M12 = 0.25f + 0.25f * c2;  h = 0.25f * s2                              (M22 = 0.25)
 *   cor = (2 * w1) * w2 + w2 * w2
 *   tau1 = (a1 * 2 - 0.5f * w1) + h * cor;  tau2 = (a2 * 2 - 0.5f * w2) - h * (w1 * w1)
 *   det = M11 * 0.25f - M12 * M12                          (= 0.125 - 0.0625 c2^2 >= 0.0625 up to rounding: never near 0)
 *   al1 = (0.25f * tau1 - M12 * tau2) / det;  al2 = (M11 * tau2 - M12 * tau1) / det
 *   w1 = clamp(w1 + al1 * 0.01f, -16, 16);  w2 = clamp(w2 + al2 * 0.01f, -16, 16)                (semi-implicit Euler)
 *   per joint, with its new w:  k = w * 0.01f;  k == 0: (c, s) stay as they are (an arm at rest stays at rest to the bit);
 *   otherwise c' = c - s * k;  s' = s + c * k  (both from the old c and s);  (c, s) = normalise(c', s').  No joint limits.
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always: the task never ends an episode itself.
 *   Reward r_i of the new state:  dx = tip.x - target.x;  dy = tip.y - target.y;  d2 = dx * dx + dy * dy;
 *   sparse:  r_i = d2 <= target_radius * target_radius ? 1 : 0;     dense:  r_i = 1 / (1 + 4 * d2), in (0, 1]
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1: reward = reward + r_i for up to `repeat` sub-steps,
 *   stopping after the one that set over; discount = 1, first = 0, substeps = the sub-steps executed.  In the sparse form
 *   the reward is an exact small integer, 0 .. repeat.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel; pixel (i, j) has its centre at
 *   (16 j + 8, 16 i + 8).  576 units (36 pixels) are one unit of length, y points up, the shoulder is at (672, 672): the
 *   reach of the arm and the fingertip's radius stay inside the frame (672 - 576 - 32 >= 0).  Each coordinate is rounded once:
 *   ax = c1 * 288;  ay = s1 * 288;  EX = (int)floorf(ax + 672.5f);  EY = (int)floorf(672.5f - ay)               (the elbow)
 *   TX = (int)floorf((ax + c12 * 288) + 672.5f);  TY = (int)floorf(672.5f - (ay + s12 * 288))                   (the tip)
 *   GX = (int)floorf(target.x * 576 + 672.5f);  GY = (int)floorf(672.5f - target.y * 576)                       (the target)
 *   GR = (int)floorf(target_radius * 576 + 0.5f)
 *   Everything after that is integer arithmetic.  Per pixel, with P = (16 j + 8, 16 i + 8), later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels;
 *   the target, |P - G|^2 <= GR * GR, in (64, 255, 64);
 *   the upper arm, the capsule of radius 24 around the segment shoulder -- elbow, in (64, 64, 255);
 *   the forearm, the capsule of radius 24 around the segment elbow -- tip, in (255, 64, 64);
 *   the fingertip, |P - T|^2 <= 1024, in (255, 255, 64).
 *   A capsule is the cartpole's: with v = P - start, d = end - start, dot = v.d, dd = d.d (int32):  dot <= 0: |v|^2 <= 576;
 *     dot >= dd: |P - end|^2 <= 576;  otherwise cross = v.x * d.y - v.y * d.x and cross * cross <= 576 * dd, in int64.
 *   Neither velocity is in a frame.  A shape pixel holds 64 and 255 only and never three equal channels.
 *
 * drq_vec_reacher_step: one launch, N workgroups of 256 threads with the shape of drq_vec_cartpole_step.  Writes every byte
 *   of frame, reward, discount, first, substeps and the state (phys and target), nothing else.  No LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 2, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all or sparse not 0 or 1, target_radius outside [0.02, 0.3] or
 *   NaN, frame not 16-byte aligned, a float / int array not 4-byte aligned.
 * drq_vec_reacher_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; phys and target are only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or
 *   > INT32_MAX, target_radius as for the step, frame not 16-byte aligned, phys or target not 4-byte aligned. */
int drq_vec_reacher_step(float* phys, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                         const float* action, unsigned seed, int episode_length, int repeat, int reset_all,
                         float target_radius, int sparse, uint8_t* frame, float* reward, float* discount, uint8_t* first,
                         int* substeps, drq_stream_t stream);
int drq_vec_reacher_render(const float* phys, const float* target, long N, float target_radius, uint8_t* frame,
                           drq_stream_t stream);

/* Maze.  A fifth task of the device environment, with entries of its own: a point in the square [-1, 1]^2, which walls cut
 * into G x G cells, must find the goal cell.  The walls are generated on the device for every episode, fresh or from a
 * finite pool of layouts, so the world itself differs between episodes and a reward sits behind walls.  These
 * definitions are the contract; they are exact to the bit.  The generator, the flood fill, the sparse reward and the frame
 * are integer arithmetic; every float operation below is ONE IEEE float32 operation (+, -, *, a compare or floorf; the
 * dense reward has the one correctly rounded division), in the written order, never fused.
 * Geometry.  G = size is 3, 4, 6, 7 or 8: the sizes that divide the 1344 sixteenths of a pixel of a frame side.  Cell
 *   (r, c), row 0 at the top of the frame (y = 1), column 0 at the left (x = -1), is bit 8 r + c of a 64-bit board, stride 8
 *   whatever G is.  The walls are two boards: east, bit (r, c) set = a wall between (r, c) and (r, c + 1), c <= G - 2;
 *   south, bit (r, c) set = a wall between (r, c) and (r + 1, c), r <= G - 2.  The outer boundary is always wall; bits
 *   outside these ranges are 0 as generated and are ignored when read.
 *   hg = G * 0.5f (exact);  cw = 2 / G rounded once: 0.6666667f, 0.5f, 0.33333334f, 0.2857143f, 0.25f.
 *   col(x) = clamp((int)floorf((x + 1) * hg), 0, G - 1);  row(y) = clamp((int)floorf((1 - y) * hg), 0, G - 1);
 *   cell(pos) = 8 * row(y) + col(x).
 * State per environment e: pos f32 [N][2]; walls u64 [N][2] = (east, south); cells i32 [N][2] = (start, goal), each
 *   8 r + c; t i32 [N], episode u32 [N], over u8 [N] as above.  The walls are state: nothing re-derives them.
 * The integer draw k of (s, e, episode):  h_k = fmix32(s ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ k * 0xC2B2AE35), the
 *   integer behind the draws v_k above.
 * walls(s, e, episode), the generator:
 *   every interior wall closed; then every cell but (0, G - 1) opens one passage, to the north or to the east: a cell of
 *   row 0 to the east, a cell of column G - 1 to the north, any other cell (r, c) to the north when bit 8 r + c of the
 *   64-bit word (h_4 << 32 | h_3) is set and to the east when it is clear.  (The binary tree: G * G - 1 open sides, every
 *   cell connected to the top-right corner.)
 *   then the symmetry sym = h_5 & 7, applied to the maze as a set of walls between cells, in this order:
 *     sym & 1: the transpose, (r, c) -> (c, r);  sym & 2: the columns mirrored, (r, c) -> (r, G - 1 - c);
 *     sym & 4: the rows mirrored, (r, c) -> (G - 1 - r, c)
 *   then, for loops > 0, every wall still closed is opened when (h_k & 255) < loops, with k = 16 + 8 r + c for the east
 *   wall of (r, c) and k = 80 + 8 r + c for its south wall, (r, c) in the board after the symmetry.  loops = 255 opens
 *   every wall, whatever its draw: the one value for which the comparison is not the whole rule.
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; with the draws of (seed, e, episode):
 *   i0 = h_0 mod G * G;  i1 = h_1 mod G * G;  i1 == i0: i1 = (i1 + 1) mod G * G;  a linear index i is the cell (i / G, i mod G);
 *   start = cell i0, goal = cell i1;
 *   layouts = 0: (east, south) = walls(seed, e, episode);  layouts = K > 0: (east, south) = walls(layout_seed, 0, h_2 mod K)
 *   pos, the centre of the start cell (r, c):  x = ((float)c + 0.5f) * cw - 1;  y = 1 - ((float)r + 0.5f) * cw
 *   Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The action is not read.
 * Sub-step, (ax, ay) the sanitised action (action[e][0 .. 1], each NaN to 0, then the clamp to [-1, 1]; columns 2 .. A-1
 *   are not read).  x moves first, in the cell the point is in; then the cell is taken again and y moves:
 *   move(p, d, wall_hi, edge_hi, wall_lo, edge_lo):  n = p + d;
 *     d > 0 and wall_hi:  lim = edge_hi - 0.04f;  lim < p: lim = p;  n > lim: n = lim
 *     d < 0 and wall_lo:  lim = edge_lo + 0.04f;  lim > p: lim = p;  n < lim: n = lim           (an open side does not clamp)
 *   c = col(x), r = row(y);  x = move(x, ax * 0.05f, c == G - 1 or east bit (r, c), (float)(c + 1) * cw - 1,
 *                                                      c == 0 or east bit (r, c - 1), (float)c * cw - 1)
 *   c = col(x), r = row(y);  y = move(y, ay * 0.05f, r == 0 or south bit (r - 1, c), 1 - (float)r * cw,
 *                                                      r == G - 1 or south bit (r, c), 1 - (float)(r + 1) * cw)
 *   A move is along one axis inside one row or column and 0.05 is less than a cell minus both margins, so no wall is
 *   crossed and no corner is cut: a move keeps the cell or enters the neighbour behind an open side.
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always: the task never ends an episode itself.
 *   Reward r_i of the new state:  sparse:  r_i = cell(pos) == goal ? 1 : 0, a compare of integers;
 *   dense:  r_i = (float)(G * G - d) / (float)(G * G), d = geodesic(cell(pos), goal).
 * geodesic(from, to), a flood fill on the boards:  reach = the bit of `from`;  d = 0;  while the bit of `to` is not in reach:
 *   reach = reach | the cells east, west, south and north of a cell of reach through an open side (all four from the
 *   old reach);  d += 1;  a fill that stops growing before it covers `to` gives d = G * G (only walls written by a
 *   caller can cut a cell off).  Cells are taken & 63.
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1: reward = reward + r_i for up to `repeat` sub-steps,
 *   stopping after the one that set over; discount = 1, first = 0, substeps = the sub-steps executed.  In the sparse form
 *   the reward is an exact small integer, 0 .. repeat.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel, y downwards; pixel (i, j) has its centre at
 *   P = (16 j + 8, 16 i + 8);  W = 1344 / G is a cell's side, cell (r, c) the square [c W, (c + 1) W] x [r W, (r + 1) W].
 *   Per pixel, later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels;
 *   the goal cell (r, c), an inset square:  c W + W / 4 <= P.x < (c + 1) W - W / 4 and likewise P.y with r, in (64, 255, 64);
 *   the walls, in (255, 255, 255): P within 12 in both coordinates of the nearest point of a closed segment -- for the wall
 *     east of (r, c), x = (c + 1) W and r W <= y <= (r + 1) W:  |P.x - (c + 1) W| <= 12 and r W - 12 <= P.y <= (r + 1) W + 12;
 *     for the wall south of (r, c) likewise with the axes exchanged; the four sides of the boundary are closed segments;
 *   the agent, |P - A|^2 <= 729 (a radius of 0.04), in (255, 64, 255), with each coordinate rounded once:
 *     A.x = (int)floorf(x * 672 + 672.5f);  A.y = (int)floorf(672.5f - y * 672)
 *   A pixel holds 32 .. 73, 64 or 255.
 *
 * drq_vec_maze_step: one launch, N workgroups of 256 threads with the shape of drq_vec_cartpole_step; every lane computes
 *   the reset or the macro step in registers.  Writes every byte of frame, reward, discount, first, substeps and the
 *   state (pos, walls, cells), nothing else.  No LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 2, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all or sparse not 0 or 1, size not 3, 4, 6, 7 or 8, loops outside
 *   0 .. 255, layouts outside 0 .. 65535, frame not 16-byte aligned, walls not 8-byte aligned, a float / int array not
 *   4-byte aligned.
 * drq_vec_maze_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; the state is only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or
 *   > INT32_MAX, size as for the step, frame not 16-byte aligned, walls not 8-byte aligned, pos or cells not 4-byte aligned.
 * drq_vec_maze_geodesic: out i32 [N] = geodesic(cell(pos), goal) per environment -- the length of the shortest path that is
 *   left, for an evaluation to report beside the return.  One launch, one lane per environment; the state is only read.
 *   DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX, size as for the step, walls not 8-byte aligned,
 *   pos, cells or out not 4-byte aligned. */
int drq_vec_maze_step(float* pos, uint64_t* walls, int* cells, int* t, unsigned* episode, uint8_t* over, long N, int A,
                      const float* action, unsigned seed, int episode_length, int repeat, int reset_all, int size,
                      int loops, int layouts, unsigned layout_seed, int sparse, uint8_t* frame, float* reward,
                      float* discount, uint8_t* first, int* substeps, drq_stream_t stream);
int drq_vec_maze_render(const float* pos, const uint64_t* walls, const int* cells, long N, int size, uint8_t* frame,
                        drq_stream_t stream);
int drq_vec_maze_geodesic(const uint64_t* walls, const int* cells, const float* pos, long N, int size, int* out,
                          drq_stream_t stream);

/* Catch.  A sixth task of the device environment, with entries of its own: a cup is driven in the plane, a ball hangs from
 * it on a string that is either slack or taut, and the ball must be swung up and caught.  sparse = 1 pays 1 while the ball's
 * centre is inside the cup and 0 otherwise -- in the image of the reference's cup_catch (cfgs/task/cup_catch.yaml, DMC's
 * ball-in-cup), not a port of it; sparse = 0 pays a dense shaping of the distance to the cup's interior.  The one task here
 * with a unilateral constraint (the string pulls and never pushes), contacts between moving bodies and dynamics that
 * switch regime inside an episode.  These definitions are the contract; they are exact to the bit.  Every float operation
 * below is ONE correctly rounded IEEE float32 operation (+, -, *, / or sqrt), in the written order, never fused.  The draws
 * v_k and the sanitising are those above.
 * World: the square [-1, 1]^2, y upwards, gravity 4 along -y, dt = 0.01.
 * State per environment e: phys f32 [N][8] = (cx, cy, vcx, vcy, bx, by, vbx, vby): the cup's position (the middle of its
 *   floor's segment) and velocity, the ball's centre and velocity; t i32 [N], episode u32 [N], over u8 [N] as above.  The
 *   geometry is launch arguments and constants:  0.16 <= cup_width <= 0.4;  hw = cup_width * 0.5f.
 * Geometry.  The cup is three capsules of radius 0.02 that move with it: the left wall, the segment (cx - hw, cy) --
 *   (cx - hw, cy + 0.15f); the right wall, the same at cx + hw; the floor, (cx - hw, cy) -- (cx + hw, cy).  The ball is a
 *   disc of radius 0.05, so ball and capsule touch at 0.07.  The tether has length 0.5 and is tied to the anchor
 *   (cx, ay), ay = cy + 0.02f: the middle of the cup's inside floor.  The cup's range is |cx|, |cy| <= 0.4.
 *   0.4 + 0.02 + 0.5 + 0.05 <= 1 on both axes: the ball stays in the world, which has no walls.
 *   No tunnelling: the ball's speed is at most 4, the cup's at most 1.5 per axis, and (4 + 1.5 * sqrt(2)) * 0.01 < 0.07.
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; three draws v_0 .. v_2:
 *   cx = v_0 * 0.4f;  cy = v_1 * 0.4f;  ay = cy + 0.02f;  o = v_2 * 0.25f;  n = sqrt(o * o + 1);
 *   bx = cx + (o / n) * 0.5f;  by = ay - (1 / n) * 0.5f   (the ball hangs at the tether's length, a little off the vertical)
 *   every velocity 0.  Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The
 *   action is not read.
 * Sub-step, (a1, a2) the sanitised action (action[e][0] drives the cup along x, action[e][1] along y, each NaN to 0, then
 *   the clamp to [-1, 1]; columns 2 .. A-1 are not read), in this order:
 *   1. the cup, x with a1, then y with a2:  v = clamp(v * 0.9f + a * 0.3f, -1.5f, 1.5f);  q = c + v * 0.01f;
 *      q < -0.4f: c = -0.4f, v = 0;  q > 0.4f: c = 0.4f, v = 0;  otherwise c = q               (a stop at either end)
 *   2. the ball's free flight:  vby = vby - 0.04f;  s2 = vbx * vbx + vby * vby;
 *      s2 > 16: k = 4 / sqrt(s2);  vbx = vbx * k;  vby = vby * k                                  (the clamp on its speed)
 *      bx = bx + vbx * 0.01f;  by = by + vby * 0.01f                                               (semi-implicit Euler)
 *   3. the tether, with the cup of step 1:  ay = cy + 0.02f;  dx = bx - cx;  dy = by - ay;  d2 = dx * dx + dy * dy;
 *      d2 > 0.25f: d = sqrt(d2);  nx = dx / d;  ny = dy / d;  bx = cx + nx * 0.5f;  by = ay + ny * 0.5f;
 *        vn = (vbx - vcx) * nx + (vby - vcy) * ny;  vn > 0: vbx = vbx - vn * nx;  vby = vby - vn * ny
 *      (back onto the circle, the outward part of the velocity relative to the cup removed: inelastic).  Otherwise the
 *      string is slack and does nothing.
 *   4. the contacts, left wall, right wall, floor, each with the ball as the one before left it:
 *      xl = cx - hw;  xr = cx + hw;  top = cy + 0.15f;  T, the closest point of the segment, is a clamp:
 *      left wall T = (xl, clamp(by, cy, top));  right wall T = (xr, clamp(by, cy, top));  floor T = (clamp(bx, xl, xr), cy)
 *      contact(T):  ex = bx - T.x;  ey = by - T.y;  e2 = ex * ex + ey * ey;  e2 < 0.0049f:
 *        e2 == 0: (nx, ny) = (0, 1)  (the centre on the segment: pushed upwards);  otherwise e = sqrt(e2);  nx = ex / e;  ny = ey / e
 *        bx = T.x + nx * 0.07f;  by = T.y + ny * 0.07f;                                    (out along the normal to touching)
 *        vn = (vbx - vcx) * nx + (vby - vcy) * ny;  vn < 0: vbx = vbx - vn * nx;  vby = vby - vn * ny      (restitution 0)
 *      A ball in contact is within 0.31 of the anchor, so no contact stretches the tether again.
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always: the task never ends an episode itself.
 *   Reward r_i of the new state:  ux = bx - cx;  inner = hw - 0.02f;
 *   sparse:  r_i = (ux >= -inner and ux <= inner and by >= cy + 0.02f and by <= cy + 0.15f) ? 1 : 0   (between the walls,
 *   above the floor, below the rim);     dense:  uy = by - (cy + 0.085f);  d2 = ux * ux + uy * uy;  r_i = 1 / (1 + 4 * d2)
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1: reward = reward + r_i for up to `repeat` sub-steps,
 *   stopping after the one that set over; discount = 1, first = 0, substeps = the sub-steps executed.  In the sparse form
 *   the reward is an exact small integer, 0 .. repeat.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel; pixel (i, j) has its centre at
 *   (16 j + 8, 16 i + 8).  672 units (42 pixels) are one unit of length, y points up, the world's centre is at (672, 672):
 *   the frame is the world, and every shape of every reachable state stays inside it (the cup: 0.4 + 0.2 + 0.02 <= 1; the
 *   ball: 0.4 + 0.02 + 0.5 + 0.05 <= 1).  X(x) = (int)floorf(x * 672 + 672.5f);  Y(y) = (int)floorf(672.5f - y * 672); each
 *   coordinate is rounded once:  LX = X(cx - hw);  RX = X(cx + hw);  CY = Y(cy);  TY = Y(cy + 0.15f);  AX = X(cx);
 *   AY = Y(cy + 0.02f);  BX = X(bx);  BY = Y(by).  Everything after that is integer arithmetic.  Per pixel, with
 *   P = (16 j + 8, 16 i + 8), later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels;
 *   the tether, the capsule of radius 10 around the segment A -- B (the cartpole's capsule: the cross product squared in
 *     int64; a segment of length 0 is a disc), in (64, 255, 255);
 *   the left wall, |P - (LX, clamp(P.y, TY, CY))|^2 <= 169, in (64, 64, 255);
 *   the right wall, |P - (RX, clamp(P.y, TY, CY))|^2 <= 169, in (255, 64, 255);
 *   the floor, |P - (clamp(P.x, LX, RX), CY)|^2 <= 169, in (64, 255, 64);
 *   the ball, |P - B|^2 <= 1156, in (255, 255, 64).
 *   No velocity is in a frame.  A shape pixel holds 64 and 255 only and never three equal channels.
 *
 * drq_vec_catch_step: one launch, N workgroups of 256 threads with the shape of drq_vec_cartpole_step.  Writes every byte of
 *   frame, reward, discount, first, substeps and the state (phys), nothing else.  No LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 2, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all or sparse not 0 or 1, cup_width outside [0.16, 0.4] or NaN,
 *   frame not 16-byte aligned, a float / int array not 4-byte aligned.
 * drq_vec_catch_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; phys is only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX,
 *   cup_width as for the step, frame not 16-byte aligned, phys not 4-byte aligned. */
int drq_vec_catch_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                       unsigned seed, int episode_length, int repeat, int reset_all, float cup_width, int sparse,
                       uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps, drq_stream_t stream);
int drq_vec_catch_render(const float* phys, long N, float cup_width, uint8_t* frame, drq_stream_t stream);

/* Walker.  A seventh task of the device environment, with entries of its own: a planar legged runner -- a torso with a
 * two-link leg at either end -- moves through an unbounded world by pushing on a ground with friction.  speed = 0 pays for
 * standing, speed > 0 for standing and moving forward at that speed -- in the image of the reference's walker_stand /
 * walker_walk / walker_run and cheetah_run (cfgs/task/, DMC's planar runners), not a port of them.  The one task here with
 * ground contact, four actuators, a reward on velocity and a camera that follows the body.  The body is particles and rods
 * under position-based dynamics, which needs no mass-matrix solve and no trigonometry.  These definitions are the
 * contract; they are exact to the bit.  Every float operation below is ONE correctly rounded IEEE float32 operation (+, -,
 * *, / or sqrt), in the written order (a + b * c + d * e is (a + b * c) + d * e), never fused.  The draws v_k and the
 * sanitising are those above.
 * World: the half plane y >= 0 above a ground, y upwards, gravity 10 along -y, dt = 0.01; periodic in x with period 4.
 * Body: six unit point masses, particle 0 the shoulder, 1 the hip, 2 the front knee, 3 the front foot, 4 the back knee, 5
 *   the back foot; forward is +x and the shoulder is in front.  Five rods (i, j, length): torso (0, 1, 0.4f); front thigh
 *   (0, 2, 0.25f); front shin (2, 3, 0.25f); back thigh (1, 4, 0.25f); back shin (4, 5, 0.25f).  Four muscles, each the
 *   distance across a joint, (i, j, mid, half, lo, hi): front hip (1, 2, 0.46f, 0.1f, 0.3f, 0.6f); front knee
 *   (0, 3, 0.34f, 0.06f, 0.25f, 0.43f); back hip (0, 4, 0.46f, 0.1f, 0.3f, 0.6f); back knee (1, 5, 0.34f, 0.06f, 0.25f,
 *   0.43f).  [lo, hi] is what a sweep projects the distance into; after a step every muscle distance is inside the joint's
 *   hard limits [lo - 0.005, hi + 0.005], which keep every joint away from straight and from folded.
 * State per environment e: phys f32 [N][24], phys[4 i .. 4 i + 3] = (x_i, y_i, vx_i, vy_i) of particle i; t i32 [N],
 *   episode u32 [N], over u8 [N] as above.  speed is a launch argument, 0 <= speed <= 2.
 *   A phys written from outside (a restored checkpoint) is trusted as the other tasks' state is: its coordinates must be
 *   finite and in the range the rule keeps them in, |x_i| <= 2.71 and 0 <= y_i <= 4; beyond it the frame's integers are
 *   not defined.
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; five draws v_0 .. v_4:
 *   tilt = v_0 * 0.05f;  n = sqrt(tilt * tilt + 1);  ux = 1 / n;  uy = tilt / n;
 *   d0 = 0.46f + v_1 * 0.025f;  d1 = 0.34f + v_2 * 0.015f;  d2 = 0.46f + v_3 * 0.025f;  d3 = 0.34f + v_4 * 0.015f;
 *   x_0 = ux * 0.2f;  y_0 = uy * 0.2f;  x_1 = -x_0;  y_1 = -y_0;  px = uy;  py = -ux;   (the torso's normal, downwards)
 *   knee(B, D, dist):  al = (0.0625f - dist * dist + 0.4f * 0.4f) / 0.8f;  h = sqrt(0.0625f - al * al);
 *     K.x = B.x + al * D.x + h * px;  K.y = B.y + al * D.y + h * py
 *   foot(B, K, dist):  wx = (K.x - B.x) / 0.25f;  wy = (K.y - B.y) / 0.25f;  dd = dist * dist;  al = dd / 0.5f;
 *     h = sqrt(dd - al * al);  F.x = B.x + al * wx + h * wy;  F.y = B.y + al * wy - h * wx
 *   P_2 = knee(P_0, (-ux, -uy), d0);  P_3 = foot(P_0, P_2, d1);  P_4 = knee(P_1, (ux, uy), d2);  P_5 = foot(P_1, P_4, d3);
 *   low = min(y_2, y_3, y_4, y_5);  every y_i = y_i - low  (the lowest knee or foot on the ground);  every velocity 0.
 *   Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The action is not read.
 * Sub-step, (a_0 .. a_3) the sanitised action (action[e][m] drives muscle m, front hip, front knee, back hip, back knee,
 *   each NaN to 0, then the clamp to [-1, 1]; columns 4 .. A-1 are not read), in this order:
 *   1. every particle i = 0 .. 5:  vx = vx * 0.9f;  vy = vy * 0.9f - 0.1f;  ox = x;  oy = y;  x = x + vx * 0.01f;
 *      y = y + vy * 0.01f                                                  (drag, gravity, the old position kept, the advance)
 *   2. the targets:  T_m = mid_m + a_m * half_m
 *   3. eight sweeps s = 0 .. 7, each: muscle 0, 1, 2, 3; the rods torso, front thigh, front shin, back thigh, back shin; the
 *      ground.  A constraint between i and j:  dx = x_j - x_i;  dy = y_j - y_i;  d2 = dx * dx + dy * dy;
 *        d2 == 0: d = 0, (nx, ny) = (0, 1)   (a fixed normal);  otherwise d = sqrt(d2);  nx = dx / d;  ny = dy / d
 *        and, for its correction c:  h = c * 0.5f;  hx = nx * h;  hy = ny * h;  x_i = x_i + hx;  y_i = y_i + hy;
 *        x_j = x_j - hx;  y_j = y_j - hy                                                 (split equally between its ends)
 *      muscle m:  c = 0;  s < 4: c = clamp((d - T_m) * 0.5f, -0.004f, 0.004f)    (soft; the clamp is the force limit; the
 *        last four sweeps only hold the limits);  q = d - c;  q < lo_m: c = d - lo_m;  else q > hi_m: c = d - hi_m
 *      rod:  c = d - length
 *      ground, every particle:  y < 0: y = 0
 *   4. every particle:  vx = (x - ox) * 100;  vy = (y - oy) * 100;  y == 0: vx = vx * 0.1f   (friction: the ground leaves a
 *      tenth of the horizontal velocity);  s2 = vx * vx + vy * vy;  s2 > 4: k = 2 / sqrt(s2);  vx = vx * k;  vy = vy * k
 *   5. the wrap:  mid = (x_0 + x_1) * 0.5f;  mid >= 2: every x_i = x_i - 4;  else mid < -2: every x_i = x_i + 4
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always: the task never ends an episode itself, and a fallen
 *   body lies there until the time limit.
 *   Reward r_i of the new state:  height = (y_0 + y_1) * 0.5f;  upright = (x_0 - x_1) * 2.5f;  clamp01(v) = clamp(v, 0, 1);
 *   stand = clamp01((height - 0.1f) * 10) * clamp01((upright - 0.5f) * 2.5f);  speed == 0: r_i = stand;  otherwise
 *   v = (vx_0 + vx_1) * 0.5f;  move = clamp01(v / speed);  r_i = stand * (1 + 5 * move) / 6.   The body stands at a height
 *   of 0.25; walker_walk is speed 0.3, about what a scripted open-loop gait reaches, walker_run speed 0.6.
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel; pixel (i, j) has its centre at
 *   (16 j + 8, 16 i + 8).  672 units (42 pixels) are one unit of length, y points up and the ground line y = 0 is at 1008.
 *   The camera's x is the torso's middle, as an integer:  C = (int)floorf((x_0 + x_1) * 0.5f * 672);
 *   X_i = (int)floorf(x_i * 672 + 0.5f) - C + 672;  Y_i = (int)floorf(1008.5f - y_i * 672).  Everything after that is
 *   integer arithmetic.  Every particle is within 0.2 + 0.5 of the camera up to the rods' 1 %, so inside the frame's half
 *   width 1; |x_i| <= 2 + 0.71 by the wrap, so every integer is below 2^12 in magnitude whatever the episode's length.
 *   Per pixel, with P = (16 j + 8, 16 i + 8), later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels, fixed to the frame;
 *   the ground, P.y > 1008: with w = P.x - 672 + C the world's coordinate and m = w mod 336 in 0 .. 335 (the floor modulo,
 *     also of a negative w), m < 168 in (64, 255, 64), otherwise (64, 64, 255): stripes of 0.25 fixed to the world;
 *   the back thigh P_1 -- P_4 and the back shin P_4 -- P_5 in (255, 64, 255);  the torso P_0 -- P_1 in (255, 64, 64);  the
 *   front thigh P_0 -- P_2 and the front shin P_2 -- P_3 in (64, 255, 255): capsules of radius 18 (the cartpole's capsule:
 *   the cross product squared in int64; a segment of length 0 is a disc).
 *   No velocity is in a frame: it shows in how the ground scrolls between stacked frames.  A shape pixel holds 64 and 255
 *   only and never three equal channels.
 *
 * drq_vec_walker_step: one launch, N workgroups of 256 threads with the shape of drq_vec_cartpole_step.  Writes every byte
 *   of frame, reward, discount, first, substeps and the state (phys), nothing else.  No LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 4, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all not 0 or 1, speed outside [0, 2] or NaN, frame not 16-byte
 *   aligned, a float / int array not 4-byte aligned.
 * drq_vec_walker_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; phys is only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or > INT32_MAX,
 *   frame not 16-byte aligned, phys not 4-byte aligned. */
int drq_vec_walker_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                        unsigned seed, int episode_length, int repeat, int reset_all, float speed, uint8_t* frame,
                        float* reward, float* discount, uint8_t* first, int* substeps, drq_stream_t stream);
int drq_vec_walker_render(const float* phys, long N, uint8_t* frame, drq_stream_t stream);

/* Finger.  An eighth task of the device environment, with entries of its own: the reacher's arm of two links above a rod
 * that turns freely on a hinge.  The agent drives the finger and is paid for the motion of the rod (the spinner), which it
 * can only influence through contact -- in the image of the reference's finger_spin / finger_turn_easy /
 * finger_turn_hard (cfgs/task/, DMC's finger), not a port of them.  The one task here of manipulation.  These definitions
 * are the contract; they are exact to the bit.  Every float operation below is ONE correctly rounded IEEE float32
 * operation (+, -, *, / or sqrt), in the written order (a + b * c + d * e is (a + b * c) + d * e), never fused.  The draws
 * v_k, the sanitising, normalise() and direction() are those above ("Cartpole", "Reacher").
 * World: [-1, 1]^2, y upwards, no gravity, dt = 0.01.  The finger: links of 0.4 and 0.3 with unit point masses at the elbow
 *   and the tip, rooted at (0, 0.2); the fingertip is a disc of radius 0.06.  The spinner: a rod of length 0.3 and radius
 *   0.05 on a hinge at (0, -0.2), inertia 0.05.  Touching is a distance of 0.11 between the fingertip's centre and the
 *   rod's axis (the segment from the hinge to the rod's tip).  Only the fingertip collides, and only with the rod: the
 *   finger's two links pass over the rod, the hinge and each other.  Skin: after a sub-step the fingertip's centre is no
 *   closer to the axis than 0.11 - 0.011.
 * State per environment e: phys f32 [N][9] = (c1, s1, w1, c2, s2, w2, cs, ss, ws) -- the shoulder's unit vector and angular
 *   velocity, the elbow's (relative to the upper link), the rod's; target f32 [N][2], the unit vector (gx, gy) of the
 *   target's angle, drawn in both modes; t i32 [N], episode u32 [N], over u8 [N] as above.  mode (0 spin, 1 turn),
 *   target_radius and sparse are launch arguments.
 * Geometry of a state (what the reset, the impulse and the separation read):
 *   c12 = c1 * c2 - s1 * s2;  s12 = s1 * c2 + c1 * s2;  fx = 0.3f * c12;  fy = 0.3f * s12        (the forearm)
 *   tx = 0.4f * c1 + fx;  ty = 0.4f * s1 + fy                                   (the fingertip's centre from the root)
 *   qx = tx;  qy = ty + 0.4f                                                    (... from the hinge)
 *   proj = qx * cs + qy * ss;  u = clamp(proj, 0, 0.3f);  rx = cs * u;  ry = ss * u     (the closest point of the axis)
 *   dx = qx - rx;  dy = qy - ry;  e2 = dx * dx + dy * dy
 *   normal:  e2 == 0: e = 0, (nx, ny) = (0, 1)   (a fixed normal);  otherwise e = sqrt(e2);  nx = dx / e;  ny = dy / e
 *   levers:  j1 = ny * tx - nx * ty;  j2 = ny * fx - nx * fy;  js = rx * ny - ry * nx
 *   rotate(c, s, k):  k == 0: (c, s) stay as they are;  otherwise c' = c - s * k;  s' = s + c * k;  (c, s) = normalise(c', s')
 * Reset of e (reset_all = 1, or over[e] == 1): episode += 1 (mod 2^32), t = 0, over = 0; four draws v_0 .. v_3:
 *   (c1, s1) = direction(v_0);  (c2, s2) = direction(v_1);  (cs, ss) = direction(v_2);  w1 = w2 = ws = 0;
 *   the geometry;  e2 < 0.0169f  (closer than 0.13):  qx * qx + qy * qy >= 0.0169f: (cs, ss) = normalise(-qx, -qy)  (the rod
 *   points away from the fingertip);  otherwise (c1, s1, c2, s2) = (0, 1, 1, 0)  (the finger straight up).  So no episode
 *   starts in penetration.  v = v_3;  v < 0: v = v * 0.75f - 0.225f;  otherwise v = v * 0.75f + 0.225f;  (ax, ay) =
 *   direction(v);  (gx, gy) = normalise(cs * ax - ss * ay, ss * ax + cs * ay): the rod's direction turned by 45 degrees or more.
 *   Outputs first = 1, reward = 0, discount = 1, substeps = 0, the frame of the new state.  The action is not read.
 * Sub-step, (a1, a2) the sanitised action (action[e][0] the shoulder's torque, action[e][1] the elbow's, each NaN to 0,
 *   then the clamp to [-1, 1]; columns 2 .. A-1 are not read), in this order:
 *   1. the drive (the reacher's, with these links; torque 2 per unit of action, damping 0.5):
 *      M11 = 0.41f + 0.24f * c2;  M12 = 0.09f + 0.12f * c2;  h = 0.12f * s2                             (M22 = 0.09)
 *      cor = (2 * w1) * w2 + w2 * w2;  tau1 = (a1 * 2 - 0.5f * w1) + h * cor;  tau2 = (a2 * 2 - 0.5f * w2) - h * (w1 * w1)
 *      det = M11 * 0.09f - M12 * M12                                     (= 0.0288 - 0.0144 c2^2 >= 0.0144: never near 0)
 *      al1 = (0.09f * tau1 - M12 * tau2) / det;  al2 = (M11 * tau2 - M12 * tau1) / det
 *      w1 = clamp(w1 + al1 * 0.01f, -6, 6);  w2 = clamp(w2 + al2 * 0.01f, -6, 6);  ws = ws * 0.97f
 *   2. the impulse, at the positions as they are: the geometry;  e2 < 0.0441f  (within 0.21): the normal and the levers;
 *      gap = e - 0.11f;  lim = -(max(gap, 0) * 100);  vn = (j1 * w1 + j2 * w2) - js * ws
 *      u1 = (0.09f * j1 - M12 * j2) / det;  u2 = (M11 * j2 - M12 * j1) / det;  den = (j1 * u1 + j2 * u2) + (js * js) * 20
 *      vn < lim and den > 0:  lam = (lim - vn) / den;  w1 = w1 + u1 * lam;  w2 = w2 + u2 * lam;  ws = ws - (js * 20) * lam
 *      One impulse along the normal, shared by effective mass (the arm's n^T J M^-1 J^T n, the rod's js^2 / I), leaves
 *      the two no more approaching speed than closes the gap in this step; touching, it removes all of it (restitution
 *      0).  At the hinge end js = 0: the finger alone is stopped, by the same formula.  It never adds kinetic energy.
 *   3. the clamps:  w1 = clamp(w1, -6, 6);  w2 = clamp(w2, -6, 6);  ws = clamp(ws, -10, 10)
 *   4. the advance:  rotate(c1, s1, w1 * 0.01f);  rotate(c2, s2, w2 * 0.01f);  rotate(cs, ss, ws * 0.01f)
 *      (a body at rest keeps its vector to the bit)
 *   5. the separation, at the new positions: the geometry;  e2 < 0.0121f: the normal and the levers;
 *      den = (j1 * j1) * 2.5f + (js * js) * 20;  den >= 0.01f:  mu = (0.11f - e) / den;  rotate(c1, s1, (j1 * 2.5f) * mu);
 *      rotate(cs, ss, -((js * 20) * mu)).   The shoulder and the rod turn until the two touch again; the elbow does not,
 *      so the mass matrix and the kinetic energy stay as they are.  Without a lever (den < 0.01f) nothing is turned.
 *   t += 1;  over = 1 only when t == episode_length;  d_i = 1 always: the task never ends an episode itself.
 *   Reward r_i of the new state.  mode 0 (spin):  sparse: r_i = ws >= 2 ? 1 : 0;  dense: r_i = clamp(ws / 2, 0, 1).
 *   mode 1 (turn):  dx = 0.3f * cs - 0.3f * gx;  dy = 0.3f * ss - 0.3f * gy;  d2 = dx * dx + dy * dy  (the rod's tip from the
 *   target's centre G = hinge + 0.3 (gx, gy));  sparse: r_i = d2 <= target_radius * target_radius ? 1 : 0;  dense:
 *   r_i = 1 / (1 + 4 * d2).   finger_turn_easy is target_radius 0.1, finger_turn_hard 0.04.
 * Macro step: the one of "Tasks and action repeat" with every d_i = 1; in the sparse forms the reward is an exact small
 *   integer, 0 .. repeat.
 * Frame of a state, u8 [3][84][84].  Coordinates are integers in 1/16 pixel; pixel (i, j) has its centre at
 *   (16 j + 8, 16 i + 8).  672 units (42 pixels) are one unit of length, y points up, the world's origin is at (672, 672):
 *   the root at (672, 538), the hinge at (672, 806).  The finger (0.2 + 0.7 + 0.06), the rod (0.2 + 0.3 + 0.05) and the
 *   target's disc (0.2 + 0.3 + 0.2) stay inside the frame.  Each coordinate is rounded once:
 *   ax = c1 * 268.8f;  ay = s1 * 268.8f;  EX = (int)floorf(ax + 672.5f);  EY = (int)floorf(672.5f - (ay + 134.4f))     (the elbow)
 *   TX = (int)floorf((ax + c12 * 201.6f) + 672.5f);  TY = (int)floorf(672.5f - ((ay + s12 * 201.6f) + 134.4f))      (the fingertip)
 *   SX = (int)floorf(cs * 201.6f + 672.5f);  SY = (int)floorf(672.5f - (ss * 201.6f - 134.4f))                     (the rod's tip)
 *   GX = (int)floorf(gx * 201.6f + 672.5f);  GY = (int)floorf(672.5f - (gy * 201.6f - 134.4f))                     (the target)
 *   GR = (int)floorf(target_radius * 672 + 0.5f)
 *   Everything after that is integer arithmetic.  Per pixel, with P = (16 j + 8, 16 i + 8), later rules drawn over earlier:
 *   background 32 + ((i + j) >> 2) in all three channels;
 *   the target, mode 1 only, |P - G|^2 <= GR * GR, in (64, 255, 64);
 *   the hinge, |P - (672, 806)|^2 <= 44 * 44, in (64, 64, 255);
 *   the rod, the capsule of radius 34 around the segment hinge -- S, in (255, 64, 255);
 *   the rod's tip, |P - S|^2 <= 34 * 34, in (64, 64, 255);
 *   the upper link, the capsule of radius 20 around the segment root -- E, in (255, 64, 64);
 *   the forearm, the capsule of radius 20 around the segment E -- T, in (64, 255, 255);
 *   the fingertip, |P - T|^2 <= 40 * 40, in (255, 255, 64).
 *   A capsule is the cartpole's (the cross product squared in int64; a segment of length 0 is a disc).
 *   No velocity is in a frame.  A shape pixel holds 64 and 255 only and never three equal channels.
 *
 * drq_vec_finger_step: one launch, N workgroups of 256 threads with the shape of drq_vec_cartpole_step.  Writes every byte
 *   of frame, reward, discount, first, substeps and the state (phys and target), nothing else.  No LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null pointer (action only without reset_all), N < 1 or > INT32_MAX, A < 2, repeat < 1
 *   or > DRQ_TASK_MAX_REPEAT, episode_length < 1, reset_all, mode or sparse not 0 or 1, target_radius outside [0.02, 0.2]
 *   or NaN, frame not 16-byte aligned, a float / int array not 4-byte aligned.
 * drq_vec_finger_render: the frames of the states as they are, by the frame rule above (the same device function): every
 *   byte of frame, nothing else; phys and target are only read.  DRQ_EARG, nothing launched: a null pointer, N < 1 or
 *   > INT32_MAX, mode and target_radius as for the step, frame not 16-byte aligned, phys or target not 4-byte aligned. */
int drq_vec_finger_step(float* phys, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                        const float* action, unsigned seed, int episode_length, int repeat, int reset_all, int mode,
                        float target_radius, int sparse, uint8_t* frame, float* reward, float* discount, uint8_t* first,
                        int* substeps, drq_stream_t stream);
int drq_vec_finger_render(const float* phys, const float* target, long N, int mode, float target_radius, uint8_t* frame,
                          drq_stream_t stream);

/* ---- exploration bonus.  New functionality: the reference explores by the noise of its policy alone (drqv2.py:164-175)
 * and every reward its replay sees is the environment's.  This is the count-based bonus of "#Exploration" (Tang et al.
 * 2017) -- a SimHash of the frame, a table of visit counts, bonus = beta / sqrt(count) -- on the frames of N lockstep
 * environments as "device environment" writes them and "single-frame step-major replay" stores them, where they are:
 * no download, no host wait.  These definitions are the contract; everything up to the count is integer arithmetic
 * and exact, the bonus is exact to the bit.
 * Input: frame u8 [N][3][84][84].  Per environment n:
 *   cells       the frame is cut into a 21 x 21 grid of 4 x 4 blocks; s[gy][gx] = the int32 sum over the 3 channels and the
 *               16 pixels (rows 4 gy .. 4 gy + 3, columns 4 gx .. 4 gx + 3) of block (gy, gx), at most 48 x 255 = 12,240.
 *               D = 441 cells, i = gy * 21 + gx.
 *   centring    v_i = 441 * s_i - sum_j s_j: exact in int32 (|v_i| <= 441 * 12,240), and sum_i v_i = 0
 *   projection  for bit j = 0 .. bits-1:  p_j = sum_i a(j, i) * v_i, accumulated in int64, with
 *               a(j, i) = +1 if fmix32(seed ^ (j * 441 + i) * 0x9E3779B9) & 1, else -1, in uint32 arithmetic; fmix32 is the
 *               murmur3 finaliser of "device environment".  The signs are computed, no matrix is stored.
 *               (With k signs +1, |p_j| <= 12,240 k (882 - 2 k) <= 12,240 * 220 * 442 = 1,190,217,600: the frame that is 255
 *               on the +1 cells and 0 elsewhere.  The sum is exact in any order; int64 leaves the bound no role.)
 *   code        code = sum_j (p_j > 0) << j: a projection of exactly zero gives bit 0, so a uniform frame has code 0.
 *               1 <= bits <= DRQ_SIMHASH_MAX_BITS (24).  Adding a constant to every pixel changes no v_i and no code.
 *   table       count: i32 [2^bits], zeroed by the caller before the first step
 *   update = 1  FIRST every environment adds 1 to count[code_n], THEN every environment reads c_n = count[code_n]: two
 *               environments with one code in one step both see the count after both increments, and the result does
 *               not depend on the order of the workgroups
 *   update = 0  the step only reads: c_n may be 0
 *   bonus       bonus_n = beta / sqrt((float)c_n) in float32, the conversion, the square root and the division each
 *               correctly rounded (numpy: np.float32(beta) / np.sqrt(np.float32(c))); bonus_n = beta for c_n = 0
 *   reward      with reward and reward_out (f32 [N], both or neither): reward_out_n = reward_n + bonus_n, one float32 add
 * drq_explore_simhash_step: two launches on the stream, whose boundary is the order between incrementing and reading (no
 *   cooperative launch, no spin).  Hash and count: N workgroups of 256 threads, one per environment; a lane owns a cell
 *   and loads each of its 12 pixel rows as one aligned dword (a frame row is 21 dwords), so the 21,168 bytes are read
 *   once; s and v pass through LDS; bit j is a strided sum over the 441 cells by wave j % 4, reduced inside the wave;
 *   one lane stores code_out[n] and under update does one atomic add of 1 on count[code_n].  Bonus: one thread per
 *   environment.  Writes every element of code_out, count_out (i32 [N]: c_n), bonus_out (f32 [N]) and, when given,
 *   reward_out; count only by the increments; nothing else.  reward_out may be reward itself.
 *   DRQ_EARG, nothing launched: a null frame, count, code_out, count_out or bonus_out, reward without reward_out or
 *   reward_out without reward, N < 1 or > INT32_MAX, bits < 1 or > 24, update not 0 or 1, a pointer not 4-byte aligned. */
#define DRQ_SIMHASH_MAX_BITS 24
int drq_explore_simhash_step(const uint8_t* frame, long N, int bits, unsigned seed, float beta, int update, int* count,
                             int* code_out, int* count_out, float* bonus_out, const float* reward, float* reward_out,
                             drq_stream_t stream);

/* ---- k-NN bonus.  New functionality: a novelty measure in feature space beside the count of "exploration bonus".  RE3
 * (Seo et al., ICML 2021) pays log(1 + ||y - y_kNN||), y the features of a fixed random encoder, the neighbours looked
 * up among the rows of the replay when a batch is drawn.  This is the hot part: for B drawn rows of a feature table, the
 * distance to the k-th nearest other row, without the B x M matrix of distances ever existing.  These definitions are the
 * contract; the result is exact to the bit.
 * Inputs: table f32 [S][d], row-major, 1 <= d <= DRQ_KNN_MAX_DIM (64); live, 0 <= live <= S: only rows < live exist;
 *   slots int64 [B]; k, 1 <= k <= DRQ_KNN_MAX_K (8); stride >= 1 and 0 <= offset < stride.  Output: dist f32 [B].
 *   candidates  the rows c = offset + j * stride with c < live, for j = 0, 1, ...
 *   query       for b with s = slots[b]:  s < 0 or s >= live:  dist[b] = 0 and no row is read for it.  Otherwise q = table[s].
 *   distance    for every candidate c != s:  D(c): acc = 0;  for i = 0 .. d-1 in that order:  t = q[i] - x[i];  acc = acc + t * t
 *               with x = table[c].  Every -, * and + is one float32 operation, rounded on its own; nothing is fused or
 *               reassociated.  A D that is NaN counts as +infinity.
 *   result      fewer than k candidates other than s:  dist[b] = 0.  Otherwise dist[b] = sqrtf(the k-th smallest D),
 *               correctly rounded (+infinity where that D is).  Ties need no rule: a value is returned, not an index.
 *   No row >= live is ever read, whatever it holds.  The row itself is excluded by its index, not by its distance: a
 *   duplicate of the query elsewhere in the table is a neighbour at distance 0.
 * drq_explore_knn: two launches on the stream.  Partial lists: a grid of G x ceil(B / 256) workgroups of 256 threads; a lane
 *   owns a query (its row in registers) and the sorted list of its 8 smallest D; the candidates are dealt in chunks of
 *   DRQ_KNN_CHUNK (128) rows, chunk ch to workgroup ch mod G, and staged in LDS once per 256 queries, where every lane of
 *   a wave reads the same address; G = min(chunks, max(1, 512 / ceil(B / 256))).  Each lane writes its list to
 *   ws [B][G][8].  Merge: one wave per query folds the G lists into one and stores the result.  D is exact, min and max
 *   are exact, so the bits do not depend on G, on the dealing or on the order of anything; no atomics.  Writes every
 *   element of dist and the first B G 8 floats of ws, nothing else.  With no candidate at all only the merge is launched.
 *   drq_explore_knn_ws_bytes(B, live, stride): the bytes of ws that serve every offset (0 for arguments the entry refuses,
 *   and for live = 0).
 *   DRQ_EARG, nothing launched: a null table, slots or dist; S < 1; d < 1 or > 64; live < 0 or > S; B < 1 or
 *   > DRQ_KNN_MAX_QUERIES (2^20); k < 1 or > 8; stride < 1; offset < 0 or >= stride; table or dist not 4-byte aligned,
 *   slots not 8-byte aligned, ws not 16-byte aligned.  DRQ_EWS, nothing launched: candidates exist and ws is null or
 *   ws_bytes < B G 32. */
#define DRQ_KNN_MAX_DIM 64
#define DRQ_KNN_MAX_K 8
#define DRQ_KNN_CHUNK 128
#define DRQ_KNN_MAX_QUERIES 1048576
size_t drq_explore_knn_ws_bytes(long B, long live, long stride);
int drq_explore_knn(const float* table, long S, int d, long live, const int64_t* slots, long B, int k, long stride,
                    long offset, float* dist, float* ws, size_t ws_bytes, drq_stream_t stream);

/* ---- distractions. New functionality: the reference trains and evaluates on the clean frames of dm_control.  The
 * Distracting Control Suite (Stone et al. 2021) and DMControl-GB (Hansen & Wang 2021) ask whether a pixel agent still
 * works when the image changes in ways that do not matter, and perturb exactly three things: the background, the colours
 * and the camera.  This applies the three to the frames of N lockstep environments as "device environment" writes them,
 * where they are: one launch per step, no download, no host wait.  These definitions are the contract; they are exact to
 * the bit.  All arithmetic is integer: uint32 where it says so, int32 otherwise.
 * Inputs: frame_in u8 [N][3][84][84]; first u8 [N] or NULL = no flag set; key u8 [3][84][84] or NULL (the clean background
 *   of the renderer); bank u8 [M][F][3][84][84] or NULL (M clips of F background frames).  State per environment e, read
 *   and written: episode u32 [N], t u32 [N], both 0 before the first call.  Scalars: seed; reset_all, hold, dynamic (0 / 1);
 *   camera P, 0 .. DRQ_DISTRACT_MAX_CAMERA (8); camera_period >= 1; color C, 0 .. DRQ_DISTRACT_MAX_COLOR (128); bg_mode
 *   0 (none), 1 (noise), 2 (bank); bg_alpha a, 0 .. 256; M and F, 1 .. DRQ_DISTRACT_MAX_BANK (65,536), read in mode 2 only.
 *   Output: frame_out u8 [N][3][84][84], which overlaps frame_in nowhere.
 * State step of e, before anything is drawn (skipped with hold = 1, see below):
 *   reset_all = 1 or first[e] != 0:  episode += 1 (mod 2^32), t = 0;   otherwise t += 1 (mod 2^32).
 *   tau = dynamic ? (t & 0xFFFFF) : 0.
 * Draws: draw(k) = fmix32(seed ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ (256 + k) * 0xC2B2AE35) in uint32 arithmetic,
 *   episode the new count, fmix32 the murmur3 finaliser of "device environment".  The offset 256 keeps these draws apart
 *   from an environment's own draws k = 0, 1, ... under the same seed.
 * Fold: tri(v, m) for v >= 0:  0 when m == 0;  otherwise r = v mod 2m and tri = r <= m ? r : 2m - r   (0 .. m and back).
 * Camera: ox = tri(draw(0) % (2P + 1) + (draw(2) % 3) * (tau / camera_period), 2P) - P, and oy likewise from draw(1) and
 *   draw(3): an offset in [-P, P] per axis that starts anywhere and sweeps at 0, 1 or 2 pixels per camera_period steps.
 *   The source pixel of output pixel (i, j) = (row, column) is si = clamp(i + oy, 0, 83), sj = clamp(j + ox, 0, 83) (edge
 *   replication), and s_c = frame_in[e][c][si][sj].
 * Keying: the pixel is BACKGROUND iff key != NULL and s_c == key[c][si][sj] for all three channels c -- the comparison is
 *   made at the source pixel, so the foreground moves with the camera.  With key == NULL every pixel is foreground, and
 *   bg_mode must be 0.
 * Foreground colour, per channel c:  gain_c = 256 - C + draw(4 + c) % (2C + 1);  off_c = (int)(draw(7 + c) % (C + 1)) - (C >> 1);
 *   f_c = clamp(((s_c * gain_c + 128) >> 8) + off_c, 0, 255).
 * Background value n_c at output pixel (i, j):
 *   mode 0:  n_c = s_c.
 *   mode 1:  value noise on a lattice of 12 pixels that drifts with tau.  vx = (int)(draw(11) % 5) - 2;  vy = (int)(draw(12) % 5) - 2;
 *     X = j + tau * vx;  Y = i + tau * vy;  gx = floor(X / 12), fx = X - 12 gx, and gy, fy likewise from Y (X and Y can be
 *     negative: the division rounds toward minus infinity, 0 <= fx, fy <= 11).
 *     L(c, gy, gx) = fmix32(draw(10) ^ c * 0x9E3779B9 ^ (uint32)gy * 0x85EBCA6B ^ (uint32)gx * 0xC2B2AE35) >> 24
 *     top = L(c, gy, gx) * (12 - fx) + L(c, gy, gx + 1) * fx;  bot = the same at gy + 1;
 *     n_c = (top * (12 - fy) + bot * fy + 72) / 144      (at most (255 * 144 + 72) / 144 = 255)
 *   mode 2:  the clip m = draw(10) % M, its frame f = tri(draw(11) % F + tau, F - 1) -- the clip is played forward and
 *     backward in turn (ping-pong) from a drawn start;  n_c = bank[m][f][c][i][j].
 * Blend: b_c = (a * n_c + (256 - a) * s_c + 128) >> 8.     Output: frame_out[e][c][i][j] = background ? b_c : f_c.
 * Identity: camera = 0, color = 0, bg_mode = 0 writes frame_in back bit for bit (gain 256, offset 0, n_c = s_c), for any key
 *   and any bg_alpha; so does bg_alpha = 0 in any mode with camera = 0 and color = 0.  The state words still step.
 * hold = 1 draws the frame of the state AS IT IS: the state step is skipped, episode and t are read and not written, first
 *   is not read, reset_all must be 0.  After a call that stepped, a hold call on the same frame_in writes the same
 *   frame_out; it is what a restored environment shows before its next step (a checkpoint holds episode and t).
 *
 * drq_vec_distract: one launch, N workgroups of 256 threads, one per environment.  The state words and the flag are read
 *   wave-uniformly, so the state step, the draws and every scalar derived from them are computed once per wave on the
 *   scalar unit; the frame and the key test are staged in LDS as one dword per pixel (three aligned 16-byte loads of the
 *   frame and three of the key per 16 pixels; pixel p at dword p + (p >> 4), which spreads a wave over all banks) beside
 *   the 9 x 9 x 3 lattice values the window can touch in mode 1 (they are hashed once, not per pixel); a workgroup barrier;
 *   one lane stores the state, all store the frame as 16-byte pieces, 16 pixels of all three channel planes per lane and
 *   round.  No atomics, nothing crosses workgroups.  Writes every byte of frame_out and, without hold, episode[e] and t[e]
 *   of every environment; nothing else.  The caller orders the launches on one stream.
 *   DRQ_EARG, nothing launched: a null frame_in, frame_out, episode or t; N < 1 or > INT32_MAX; reset_all, hold or dynamic
 *   not 0 or 1; hold with reset_all; camera, color or bg_alpha outside its range; camera_period < 1; bg_mode not 0, 1 or 2;
 *   bg_mode != 0 without a key; bg_mode 2 without a bank or with M or F outside 1 .. 65,536; frame_out overlapping frame_in
 *   (frame_out == frame_in included); frame_in, frame_out, key or (mode 2) bank not 16-byte aligned; episode or t not
 *   4-byte aligned. */
#define DRQ_DISTRACT_MAX_CAMERA 8
#define DRQ_DISTRACT_MAX_COLOR 128
#define DRQ_DISTRACT_MAX_BANK 65536
int drq_vec_distract(const uint8_t* frame_in, const uint8_t* first, const uint8_t* key, const uint8_t* bank,
                     unsigned* episode, unsigned* t, long N, unsigned seed, int reset_all, int hold, int camera,
                     int camera_period, int color, int bg_mode, int bg_alpha, int dynamic, int M, int F,
                     uint8_t* frame_out, drq_stream_t stream);

/* ---- strong augmentation.  New functionality: the reference's only augmentation is its random shift (drqv2.py:19-45).
 * These are the two augmentations the methods of DMControl-GB (SVEA, SODA, "DrQ + aug"; Hansen & Wang 2021) are built
 * from, on a batch of uint8 frame stacks: random_overlay blends the observation with an unrelated image, random_conv
 * passes every frame through a random 3 x 3 convolution.  These definitions are the contract; both are exact to the bit.
 * obs and out are u8 [B][C][84][84] with C in {3, 6, 9, 12}: a stack of C / 3 RGB frames, oldest first; frame g of sample b
 * is channels 3g .. 3g + 2.  Each entry is one launch on the stream.
 *
 * drq_aug_overlay: bank u8 [M][3][84][84], idx i32 [B], alpha_q8 an int in 0 .. 256.  For sample b, frame g, colour channel c
 *   and pixel p, with y = bank[clamp(idx[b], 0, M - 1)][c][p] and x = obs[b][3g + c][p]:
 *     out[b][3g + c][p] = (x * (256 - alpha_q8) + y * alpha_q8 + 128) >> 8
 *   in integer arithmetic.  alpha_q8 = 0 returns obs exactly, 256 the bank image exactly; the same bank image goes over
 *   every frame of a stack, as DMControl-GB repeats it.  The clamp exists so that no value of idx can read outside the bank
 *   (the index lives on the device and cannot be checked on the host without a wait).  out may be obs itself (in place).
 *   A grid-stride walk over B x 3 x 441 pieces of 16 pixels; the bank piece is loaded once and reused over the C / 3 frames.
 *   Writes every byte of out, nothing else.
 *   DRQ_EARG, nothing launched: a null pointer; obs, out or bank not 16-byte aligned; idx not 4-byte aligned; B < 1;
 *   B C 7,056 > INT32_MAX; C outside {3, 6, 9, 12}; M < 1; alpha_q8 outside 0 .. 256; out overlapping obs without being obs;
 *   out overlapping the bank.
 * drq_aug_random_conv: w f32 [B][3][3][3][3] = (sample, c_out, c_in, ky, kx): one filter bank per sample, applied to each of
 *   its C / 3 frames with replicate padding.  For output channel co of frame g at (i, j) = (row, column):
 *     acc = 0.0f;  for ci = 0 .. 2, ky = 0 .. 2, kx = 0 .. 2, in that order:  acc = acc + w[b][co][ci][ky][kx] * p,
 *       p = (float)obs[b][3g + ci][clamp(i + ky - 1, 0, 83)][clamp(j + kx - 1, 0, 83)] * 0.003921568859368563f
 *       (every * and + one float32 operation, nothing fused; the constant is 1 / 255 rounded to float32)
 *     q = acc / (1.0f + fabsf(acc)), the division correctly rounded;  q = 0 if q != q
 *     v = (0.5f + 0.5f * q) * 255.0f;   out[b][3g + co][i][j] = (uint8_t)(int)(v + 0.5f)
 *   The squash is the rational sigmoid, in place of a transcendental, so that numpy reproduces it to the bit: this is in
 *   the image of DMControl-GB's sigmoid(conv2d(x / 255)), not a port of it.  All-zero weights give 128 everywhere; an
 *   infinite or NaN sum gives 128 as well (inf / inf is NaN).  One workgroup of 256 threads per (sample, frame): the three
 *   input planes and the 81 weights are staged in LDS, a lane computes 16 consecutive pixels of all three output channels
 *   and stores them as three 16-byte pieces.  Writes every byte of out, nothing else.
 *   DRQ_EARG, nothing launched: a null pointer; obs or out not 16-byte aligned; w not 4-byte aligned; B < 1;
 *   B C 7,056 > INT32_MAX; C outside {3, 6, 9, 12}; out overlapping obs (out == obs included: neighbours are read). */
int drq_aug_overlay(const uint8_t* obs, const uint8_t* bank, const int* idx, uint8_t* out, long B, int C, int M,
                    int alpha_q8, drq_stream_t stream);
int drq_aug_random_conv(const uint8_t* obs, const float* w, uint8_t* out, long B, int C, drq_stream_t stream);

/* ---- evaluation. New functionality: the reference evaluates its one environment on the host -- the 9-channel
 * observation comes out of a FrameStackWrapper (dmc.py:87-109), the episodes are recorded by video.py (train.py:98-122).
 * For N lockstep environments whose frames are device tensors ("device environment") both are one launch each, and
 * neither needs a ring of "single-frame step-major replay".  These definitions are the contract; everything is integer
 * arithmetic and exact to the bit.  A frame is u8 [3][84][84] = 21,168 bytes = 1,323 pieces of 16 bytes; a stack is three
 * frames along the channel axis, u8 [9][84][84] = 63,504 bytes = 3,969 pieces, oldest frame first.
 *
 * drq_vec_stack_push: the FrameStackWrapper rule for N environments.  prev, next u8 [N][9][84][84], frame u8
 *   [N][3][84][84], first u8 [N] or NULL = no flags.  For every environment e:
 *     reset_all or first[e] != 0:  next[e] = (frame[e], frame[e], frame[e])           (dmc.py:98-103)
 *     otherwise:                   next[e][0:6] = prev[e][3:9], next[e][6:9] = frame[e]   (:105-109)
 *   prev[e] is not read for a reset environment; with reset_all = 1 prev may be NULL.  Every byte of next is written,
 *   nothing else.  N x 4 workgroups of 256 threads, 16-byte pieces: a piece never crosses a frame, so every source and
 *   destination piece is whole and 16-byte aligned.  No LDS, no atomics; the caller orders the launches on one stream.
 *   DRQ_EARG, nothing launched: a null next or frame, a null prev without reset_all, N < 1 or > INT32_MAX, reset_all not
 *   0 or 1, prev / next / frame not 16-byte aligned, prev or frame overlapping next.
 * drq_vec_video_record: one mosaic image of the newest frames.  out u8 [GH S][GW S][3], S = 84 k, k = 1 .. 4, channels
 *   last.  Tile m < GH GW sits at tile row gy = m / GW, tile column gx = m % GW.  A tile with m < M shows environment
 *   e = envs[m] (envs: i32 [M] on the device, every entry in [0, N): the caller checks that once; the entry reads nothing
 *   for an e outside and leaves that tile zero): the byte at tile-local (y, x, c) is frame[e][c][y / k][x / k] -- every
 *   pixel k x k times, fused with the transposition.  Dimming: if done != NULL (i32 [N], the `done` of "episode
 *   statistics") and limit > 0 and done[e] >= limit, the tile shows an episode that no longer counts and the byte is that
 *   value >> 2.  Tiles m >= M are zero.  Every byte of out is written by every call, nothing else.
 *   The image is walked as one flat array of GH GW 21,168 k^2 bytes, a multiple of 16 for every k, in pieces of 16 bytes
 *   when out is 16-byte aligned, of 4 when it is 4-byte aligned, else of 1: a tile row is 252 k bytes, a multiple of 16
 *   only for k = 4, so a piece may run from one tile into the next or into the next image row, and the store width
 *   follows from the address of out alone.  ceil(pieces / 1,024) workgroups of 256 threads (at most 65,536, then they
 *   stride), no LDS, no atomics.
 *   DRQ_EARG, nothing launched: a null frame, envs or out, k outside 1 .. 4, M < 1, M > GH GW, GH or GW < 1, GH GW > 2^20,
 *   N < 1 or > INT32_MAX, limit < 0, envs or done not 4-byte aligned. */
int drq_vec_stack_push(const uint8_t* prev, uint8_t* next, const uint8_t* frame, const uint8_t* first, long N,
                       int reset_all, drq_stream_t stream);
int drq_vec_video_record(const uint8_t* frame, const int* envs, int M, const int* done, int limit, uint8_t* out, int GH,
                         int GW, int k, long N, drq_stream_t stream);

/* ---- episode files for the step-major ring.  New functionality: the bulk movements between the ring of "step-major
 * replay" / "single-frame step-major replay" and episode-major staging (an episode file of the reference,
 * replay_buffer.py:22-34, is arrays [len + 1][...] whose index 0 is the dummy reset transition).  The host plans
 * (drqv2_amd/episodes.py), these launches copy; these definitions are the contract.
 *
 * drq_vec_export_rows: one launch gathers M steps.  table is int32 [M][3] on the device, entry m = (t, e, t0): absolute row
 *   t of environment e in the episode whose reset row is t0 <= t.  stack = 1: a slot holds the whole observation, obs u8
 *   [M][frame_bytes] receives slot (t, e).  stack = 3: a slot holds one frame, obs u8 [M][3 frame_bytes] receives the
 *   frames of rows max(t-2, t0), max(t-1, t0), t of environment e, oldest first -- the reference's FrameStackWrapper
 *   (dmc.py:87-109) inside that episode, and what drq_vec_stack_gather gives for slot (t, e) when the flags of rows
 *   t0 .. t say the same (first only on t0).  No flag is read.  act_out f32 [M][A], rew_out f32 [M], disc_out f32 [M]
 *   receive the ring's action, reward and discount of (t, e), and for t == t0 the canonical dummies 0, 0, 1 whatever the
 *   ring holds.  An entry with e outside [0, N), t0 < 0 or t < t0 leaves its output rows as they were; no other entry
 *   can address anything outside the ring (rows are taken modulo R).  That the rows are still live is the caller's.
 *   DRQ_EARG, nothing launched: a null pointer, R, N, A, M <= 0, frame_bytes <= 0 or % 16 != 0, stack not 1 or 3, frames
 *   or obs not 16-byte aligned, another pointer not 4-byte aligned.
 * drq_vec_fill: one launch writes the n consecutive rows T .. T+n-1 for all N environments from step-major sources:
 *   src_frames u8 [n][N][frame_bytes] (16-byte aligned), src_action f32 [n][N][A], src_reward, src_discount f32 [n][N],
 *   src_first u8 [n][N].  The effect is exactly that of drq_vec_add(t = T + i, the sources of row i) for i = 0 .. n-1:
 *   row 0 stores first = 1 for every environment whatever src_first says, and rows past the ring's end continue at ring
 *   row 0 within the one launch.  n <= R, so no two rows share a ring row.  That is the entry's only limit on n: a
 *   caller that keeps a priority tree and lets it follow row by row afterwards (drq_vec_per_advance reads the flags of
 *   the row nstep - 1 behind the one it counts) chooses n <= R - nstep itself, so that no row of the launch has
 *   overwritten those flags.
 *   DRQ_EARG, nothing launched: a null pointer (src_first too), R, N, A, n <= 0, n > R, T < 0, frame_bytes <= 0 or
 *   % 16 != 0, frames / src_frames not 16-byte aligned, a float pointer not 4-byte aligned. */
int drq_vec_export_rows(const uint8_t* frames, const float* action, const float* reward, const float* discount, long R,
                        long N, int A, long frame_bytes, int stack, const int* table, int M, uint8_t* obs, float* act_out,
                        float* rew_out, float* disc_out, drq_stream_t stream);
int drq_vec_fill(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R, long N, int A,
                 long frame_bytes, long T, int n, const uint8_t* src_frames, const float* src_action,
                 const float* src_reward, const float* src_discount, const uint8_t* src_first, drq_stream_t stream);

/* ---- the four random draws of one update in one launch, bit-identical to the ATen launches of the reference's calls
 * (torch.randint(0, range, (B,1,1,2), dtype=float32) x2 from drqv2.py:34,241-242; torch.empty((B,A)).normal_() x2 from
 * utils.py:135 via drqv2.py:183,211): Philox4x32-10, key = seed, subsequence = element index, offsets offset + 0, 4, 8,
 * 12.  (seed, offset) = torch's CUDA generator state before the draws; the caller advances its offset by 16.
 * n_shift = 2*B, n_noise = B*A, each <= 65536 (else DRQ_EARG: ATen's launch geometry differs there).  n_noise = 0: the
 * two shift draws only (offsets + 0, 4; the caller advances by 8 and draws the noises itself). */
int drq_rng_draws(unsigned long long seed, unsigned long long offset, int n_shift, int n_noise, int range,
                  float* shift_obs, float* shift_next, float* noise_critic, float* noise_actor, drq_stream_t stream);

/* ---- autograd of the modules (drqv2_amd/autograd.py: Encoder / Actor / Critic / RandomShiftsAug forwards as
 * differentiable ops for user losses; update() does not use these).  Deterministic gather forms, no atomics.
 * drq_relu_mask_pad: out [planes][h+2pad][h+2pad] = dy [planes][h][h] where mask > 0 (mask NULL: everywhere), zero
 *   elsewhere and on the border -- the encoder output's gradient in the padded layout the conv gradients read.
 * drq_conv1_dgrad: input gradient of the first encoder layer Conv2d(9,32,3,stride 2) (drqv2.py:55): dy_pad
 *   [nb][32][45][45] = the pre-activation gradient [41][41] with a zero border of 2, w [32][9][3][3], dx [nb][9][84][84]
 *   (8-byte aligned); row and column 83 receive no tap and are 0.
 * drq_aug_bwd_f32: input gradient of drq_aug_fwd_f32 (RandomShiftsAug on a float frame): dy [n][c][hw][hw] -> dx, the
 *   adjoint of the forward's bilinear taps with the forward's own fp32 weights; shift_xy / base_grid as there, shifts
 *   integers in [0, 2*pad], pad <= 5.
 * drq_tanh_bwd: dx = dy * (1 - y*y) for y = tanh(x) (the policy output, drqv2.py:89). */
int drq_relu_mask_pad(const float* dy, const float* mask, float* out, long planes, int h, int pad, drq_stream_t stream);
int drq_conv1_dgrad(const float* dy_pad, const float* w, float* dx, int nb, drq_stream_t stream);
int drq_aug_bwd_f32(const float* dy, const float* shift_xy, const float* base_grid, float* dx, int n, int c, int hw,
                    int pad, drq_stream_t stream);
int drq_tanh_bwd(const float* y, const float* dy, float* dx, long n, drq_stream_t stream);

/* ---- dormant ratio and perturbation: the two primitives DrM (Xu et al. 2024, "Mastering Visual RL through Dormant
 * Ratio Minimization") adds to the DrQ-v2 update.  New functionality, the reference has neither.  Deterministic: fixed
 * summation orders, no float atomics, the same bits on every run.
 * drq_dormant_scores: score[j] = (sum_b |act[b*ld + j]|) / rows for j < units: the mean absolute activation of a layer's
 *   units over a batch (Sokar et al. 2023).  rows, units >= 1, ld >= units (else DRQ_EARG).  Per column the rows are
 *   added in the two-stage order of drq_colsum (64 columns x 16 row groups below 1,024 rows, 16 x 64 from there on), then
 *   divided by rows.  A NaN activation makes its column's score NaN and no other.
 * drq_dormant_count: one workgroup.  m = (sum_j score[j]) / units with the sum in this order: chain t (t < 256) adds
 *   score[t], score[t + 256], ... in that order starting from 0, then chain t takes chain t + o for o = 128, 64, ..., 1.
 *   Unit j is dormant when score[j] <= tau * m (one fp32 product), and every unit is when m == 0.  ADDS the number of
 *   dormant units to count[0] and units to count[1] (int32; the caller zeroes the pair once, several layers then
 *   accumulate into it with no host read) and writes m to layer_mean[0] (may be NULL).  tau >= 0 and finite, units >= 1,
 *   else DRQ_EARG.  A NaN score makes m NaN and no unit of the layer dormant.
 * drq_lerp_flat: p[i] = fmaf(a, p[i], (1 - a) * p0[i]) for i < n -- 1 - a and its product with p0[i] each rounded to
 *   fp32, then ONE fused multiply-add; the pull of a parameter arena toward a fresh initialisation p0.  a in [0, 1] and
 *   n >= 0, else DRQ_EARG (a NaN too); pointers 4-byte aligned.  n == 0 and a == 1 launch nothing (a == 1: p keeps its
 *   bits); a == 0 stores p0[i] itself, whatever p[i] held.  16-byte loads where p and p0 are misaligned by the same
 *   amount, with a scalar head and tail. */
int drq_dormant_scores(const float* act, long ld, int rows, int units, float* score, drq_stream_t stream);
int drq_dormant_count(const float* score, int units, float tau, int* count, float* layer_mean, drq_stream_t stream);
int drq_lerp_flat(float* p, const float* p0, long n, float a, drq_stream_t stream);

/* ---- whole-step entry: DrQV2Agent.update (drqv2.py:230-262) ------------------------------------ */
typedef struct {
  int B, global_B, C, A, F, H;
  const uint8_t* obs;        /* [B][C][84][84] */
  const uint8_t* next_obs;
  const float* action;       /* [B][A] */
  const float* reward;       /* [B] */
  const float* discount;     /* [B] */
  const float* shift_obs;    /* [B][2] */
  const float* shift_next;
  const float* noise_critic; /* [B][A] */
  const float* noise_actor;
  const float* base_grid;    /* [84] */
  float* params;             /* arenas laid out by drq_param_layout */
  float* grads;
  float* adam_m;
  float* adam_v;
  float* ws;                 /* drq_step_ws_bytes(), zero-initialised once */
  size_t ws_bytes;
  float* sums;               /* [8] local partial sums of the metrics ([11] for drq_update_phase_bc) */
  double lr, tau;
  float std, clip;
  long step_critic, step_enc, step_actor; /* 1-based Adam step numbers of THIS update */
  float gscale;              /* multiplies every gradient inside Adam.  The loss kernels already scale local
                              * gradients by 1/global_B, so a SUM all-reduce needs gscale = 1 (what the host
                              * passes); 1/world_size is only for hosts that feed per-rank MEAN gradients. */
  drq_stream_t stream;
  float* sums_host;          /* optional (may be NULL): device-visible pinned host memory, 16 floats.  As soon as
                              * sums[0..7] are final (after the actor loss, BEFORE the actor backward / Adam /
                              * Polyak tail of the update) phase 1 writes them to sums_host[0..7], then stores the
                              * 32-bit value (uint32_t)step_actor in slot 8 with system-scope release.  The host
                              * reads the metrics (drqv2.py:191-198,218-223: the .item() calls) by polling slot 8
                              * instead of draining the stream.  Single-GPU only: with data parallelism the sums
                              * are partial until the host has all-reduced them. */
  int store_aug_next;        /* 0: only the obs view's augmented encoder input is kept in the AUG workspace buffer (rows
                              * [0,B); conv1's weight gradient reads it).  1 (verification): the next_obs view is
                              * stored as well (rows [B,2B)), 65 MB more traffic at B=256. */
  int bf16;                  /* 0: fp32 everywhere (the reference's arithmetic).  1 (BASELINE configs[4], new functionality):
                              * conv2..4 forward / dgrad / wgrad and the nn.Linear GEMMs of the update run on the bf16
                              * MFMA (operands rounded to bf16 when staged, fp32 accumulation) -- except two products of
                              * the trunk layer that are bound by memory, not arithmetic, and keep their faster fp32
                              * kernels: its input gradient (always) and its weight gradient below batch 512; conv1 (fused with
                              * the augmentation) multiplies on the bf16 MFMA too; storage, the augmentation arithmetic,
                              * conv1's weight gradient, LayerNorm, the output heads, losses, Adam and
                              * Polyak stay fp32.  act() always runs in fp32. */
  void* const* timing_events; /* optional (may be NULL): host array of timing_n hipEvent_t created with timing enabled.
                              * Instrumentation for bench.py's roofline: pairs recorded on `stream` right before / after
                              * [0],[1] the conv2 forward launch of phase 3; [2],[3] the conv3 input-gradient launch of
                              * phase 5; [4],[5] the launch(es) of the conv2..4 weight gradients; [6],[7] phase 4 (the
                              * heads of the critic update: trunks .. trunk input gradient); [8],[9] phases 6-7 without
                              * the critic's optimiser step (the heads of the actor update).  Pairs beyond timing_n
                              * are not recorded. */
  int timing_n;              /* entries of timing_events: 0, 4, 6, 8 or 10; other values are not supported */
  const int64_t* obs_index;      /* optional (both or neither): the batch is NOT materialised -- `obs` / `next_obs` are */
  const int64_t* next_obs_index; /* stores of frames (a device replay ring, [slots][C][84][84] u8) and row b of the batch
                              * is frame obs_index[b] of `obs` / next_obs_index[b] of `next_obs` (replay_buffer.py:152-153:
                              * idx-1 and idx+nstep-1).  The fused aug+conv1 launch gathers its source rows straight from
                              * the store. */
  int flags;                 /* schedule switches for A/B measurements and for tests that hold both forms to the oracle:
                              * DRQ_STEP_NO_ROW_FUSION (1): LayerNorm / policy output layer / first MLP layers as separate
                              * launches (the round-2 schedule) instead of csrc/rowblock.hip's fused ones;
                              * DRQ_STEP_NO_GEMM3 (2): hidden-layer gradients on the round-2 kernels instead of
                              * csrc/gemm3.hip;
                              * DRQ_STEP_BF16_FP32_ACTS (4, bf16 only): the outputs of conv1..conv3 stay fp32 NCHW between
                              * the layers (round 2's storage) instead of bf16 [frame][y][x][32] -- the same update bit
                              * for bit, more memory traffic;
                              * DRQ_STEP_BF16_FP32_GRADS (8, bf16 only): the gradients handed from one encoder input
                              * gradient to the next (of conv3's and conv2's outputs) stay fp32 instead of bf16 in that
                              * layout -- the same weight gradients bit for bit; the two bias gradients they feed then
                              * sum unrounded values.  A workspace must be zeroed when these two bits change between
                              * updates (the zero borders of the padded buffers move).
                              * DRQ_STEP_OVERLAP_ACTOR (16, fp32, DRQ_PHASE_ALL of drq_update_phase_overlap only, which
                              * brings the second stream): the critic's optimiser step and the actor update (phases
                              * 6-7) are issued on that stream beside the encoder backward (phase 5), whose three
                              * Winograd input gradients then leave a part of the chip's workgroup slots free.  The same
                              * launches on the same operands: the update is the serial one bit for bit.  Ignored (the
                              * serial schedule runs) with timing_events, bf16, and in every other phase id or entry.
                              * DRQ_STEP_BUDGET(n) (bits 8-13, A/B measurements): with the bit above, the slots the
                              * input gradients hold, n in 1..32 thirty-seconds of the chip's two slots per CU (n x 16 workgroups
                              * on 256 CUs); 0 = the library's choice. */
} DrqStep;
#define DRQ_STEP_NO_ROW_FUSION 1
#define DRQ_STEP_NO_GEMM3 2
#define DRQ_STEP_BF16_FP32_ACTS 4
#define DRQ_STEP_BF16_FP32_GRADS 8
#define DRQ_STEP_OVERLAP_ACTOR 16
#define DRQ_STEP_BUDGET(n) (((n) & 63) << 8)

/* Parameter arena: tensors in parameters() order of encoder, critic, actor, critic_target, each start
 * aligned to 64 floats, each network's segment padded to a multiple of 512 floats (a segment is one optimiser
 * launch and one data-parallel exchange bucket: it splits into 2/4/8 equal slices of whole lines).  out[] receives, in this order: encoder 8 offsets, critic 16, actor 10,
 * critic_target 16, then [enc_beg, enc_end, critic_beg, critic_end, actor_beg, actor_end, target_beg,
 * target_end], then total.  Returns the number of longs written (59) or <0. */
int drq_param_layout(int C, int A, int F, int H, long* out, int cap);
#define DRQ_PARAM_LAYOUT_LEN 59

size_t drq_step_ws_bytes(int B, int C, int A, int F, int H);
/* offsets (in floats) of named buffers inside ws, for tests and tools; ids below. */
long drq_step_ws_offset(int B, int C, int A, int F, int H, int buffer_id);
enum {
  DRQ_WS_AUG = 0, DRQ_WS_ACT1, DRQ_WS_ACT2, DRQ_WS_ACT3, DRQ_WS_FEAT, DRQ_WS_Z_NEXT, DRQ_WS_Z_OBS,
  DRQ_WS_HA_T, DRQ_WS_HA_C, DRQ_WS_H_AN, DRQ_WS_H_AO, DRQ_WS_Q, DRQ_WS_TQ, DRQ_WS_DQ, DRQ_WS_MU_O,
  DRQ_WS_DY4, DRQ_WS_DY3, DRQ_WS_DY2, DRQ_WS_DY1, DRQ_WS_DZ_C, DRQ_WS_DZ_A, DRQ_WS_HA_C2,
  DRQ_WS_P1, DRQ_WS_P2,   /* policy hidden activations (post-ReLU), [2B][H]: rows [0,B) obs, [B,2B) next_obs */
  DRQ_WS_C1, DRQ_WS_C2,   /* critic Q hidden activations (post-ReLU) of the critic loss, [2 heads][B][H] */
  /* the head section's other buffers, for the per-launch audit (tests/test_hip_head_audit.py).  The ids are appended:
   * the ones above keep their values; the workspace layout does not depend on the order of the ids. */
  DRQ_WS_XHAT_C, DRQ_WS_RSTD_C, DRQ_WS_XHAT_A, DRQ_WS_RSTD_A,   /* LayerNorm's normalised rows [B][F] and 1/sigma [B] */
  DRQ_WS_Z_C2,            /* the stepped critic's trunk output of the actor loss [B][F] (when no split-K records) */
  DRQ_WS_HROWS,           /* actor trunk output after LayerNorm+tanh, [2B][F]: rows [0,B) obs, [B,2B) next_obs */
  DRQ_WS_P3,              /* policy output before the tanh, [2B][A] */
  DRQ_WS_Z4,              /* the four trunk outputs of phase 4, [4][B][F] (when no split-K records) */
  DRQ_WS_T1, DRQ_WS_T2,   /* target Q hidden activations [2][B][H]; phase 6 reuses them for the stepped critic */
  DRQ_WS_DC2, DRQ_WS_DC1, /* gradients of the Q hidden layers [2][B][H] */
  DRQ_WS_DHA,             /* gradient of the critic's [h, action] input per head, [2][B][F+A] (when no records) */
  DRQ_WS_DLN,             /* gradient of LayerNorm's output [B][F] */
  DRQ_WS_DPRE,            /* gradient of the policy output before the tanh [B][A] (unfused output-layer backward) */
  DRQ_WS_DP2, DRQ_WS_DP1, /* gradients of the policy hidden layers [B][H] */
  DRQ_WS_DH_A,            /* gradient of the actor trunk output [B][F] (when no records) */
  DRQ_WS_DA,              /* gradient of the action per Q head, [2][B][A] (when no records) */
  DRQ_WS_NBUF_PUBLIC
};

/* One update = phases 3..9 in this order (phase -1, DRQ_PHASE_ALL, runs them all: single GPU):
 *   3  ENCODE          aug + encoder forward (drqv2.py:241-246)         reads the encoder weights only
 *   4  CRITIC_HEADS    trunks, policy, Q heads, TD loss, backward down to the encoder output (:180-200)
 *                      leaves ALL critic gradients and sums[0..4]; first reader of the actor weights
 *   5  CONV_BACKWARD   encoder backward                                  leaves the encoder gradients
 *   6  ACTOR_FORWARD   Adam(critic) + Polyak (:201,:259-260), actor loss through the updated critic (:210-216)
 *                      leaves sums[5..6]; publishes sums to sums_host when that is set
 *   7  ACTOR_BACKWARD  actor backward (:218-220)                         leaves the actor gradients
 *   8  ENCODER_OPT     Adam(encoder) (:202)   commutes to here: phases 6/7 work on features encoded before it (:255)
 *   9  ACTOR_OPT       Adam(actor) (:221)
 * Composite ids kept for callers that exchange at coarser points: 0 (CRITIC) = 3,4,5; 1 (ACTOR) = 6,7; 2 (OPT) = 8,9
 * in one launch.
 * For hosts that follow the reference's METHOD boundaries (DrQV2Agent.update_critic / update_actor, drqv2.py:177-228)
 * phase 6 is also available in pieces: 10 (CRITIC_OPT) = Adam(critic) alone (no Polyak), 11 (ACTOR_LOSS) = the actor
 * loss of phase 6 without the optimiser step, 12 (POLYAK) = Polyak alone (utils.soft_update_params), 13 (REDRAW) =
 * re-draw the actor update's action from the policy output stored by phase 4 with s->noise_actor (update_critic does
 * not know that draw yet).  update_critic = 4, 5, 10, 8; update_actor = 13, 11, 7, 9; results equal phase -1 bit for
 * bit (tests/test_hip_step.py).
 * A data-parallel host SUM-all-reduces the critic gradients while 5 runs, the encoder gradients while 6/7 run,
 * the metric sums after 6 and the actor gradients after 7; 8 may be deferred until the next update's phase 3
 * and 9 until its phase 4 (or drq_act_forward), so both exchanges overlap compute. */
enum {
  DRQ_PHASE_ALL = -1, DRQ_PHASE_CRITIC = 0, DRQ_PHASE_ACTOR = 1, DRQ_PHASE_OPT = 2,
  DRQ_PHASE_ENCODE = 3, DRQ_PHASE_CRITIC_HEADS = 4, DRQ_PHASE_CONV_BACKWARD = 5, DRQ_PHASE_ACTOR_FORWARD = 6,
  DRQ_PHASE_ACTOR_BACKWARD = 7, DRQ_PHASE_ENCODER_OPT = 8, DRQ_PHASE_ACTOR_OPT = 9,
  DRQ_PHASE_CRITIC_OPT = 10, DRQ_PHASE_ACTOR_LOSS = 11, DRQ_PHASE_POLYAK = 12, DRQ_PHASE_REDRAW = 13
};
int drq_update_phase(const DrqStep* s, int phase);
/* drq_update_phase with a second stream of the same device (side_stream, not NULL; if it is s->stream itself the
 * serial schedule runs).  With
 * DRQ_STEP_OVERLAP_ACTOR set in s->flags and phase = DRQ_PHASE_ALL the overlapped schedule runs (see the flag); every
 * other call is drq_update_phase(s, phase).  The library orders side_stream after s->stream and joins it back into
 * s->stream before the update's last launches with two events of its own (one pair per device, created on first use,
 * no timing, no system-scope fence): when the call returns, everything it issued is ordered before whatever the
 * caller puts on s->stream next, as in the serial schedule.  Nothing else may run on side_stream meanwhile. */
int drq_update_phase_overlap(const DrqStep* s, drq_stream_t side_stream, int phase);
/* The same update with the DrQ+BC actor loss (see the BC entries above), alpha finite and > 0: the critic step is
 * unchanged bit for bit; phases 6 / 11 and 7 issue the BC forms of the loss and of the policy output backward in place
 * of the plain ones, launch for launch.  a_beh is s->action as phase 4 consumed it (the copy phase 4 left in the
 * workspace is read, so the caller's tensor need not outlive phase 4).  s->sums must hold 11 floats (slots 9 and 10, see
 * above); with s->sums_host set those two are published in slots 9 and 10 before the sequence word.  Single GPU only:
 * global_B != B is DRQ_EARG.  The descriptor is unchanged, so callers of the plain entry are not affected. */
int drq_update_phase_bc(const DrqStep* s, int phase, float bc_alpha);
/* The same update with the critic loss weighted per row (prioritized replay; drq_td_mse_w's definitions): is_weight is
 * float [B] on the device, td_abs float [B] receives the per-sample error in phase 4.  Same phases as drq_update_phase,
 * the launches are those of the plain update one for one: the weighted loss is a compile-time form of the same two
 * loss launches (fused into the Q output backward, or drq_td_mse_w in front of it).  sums[4] is the weighted sum; the
 * other sums and the actor step are the plain update's; weights of 1.0f give the plain update bit for bit.
 * DRQ_EARG: null is_weight / td_abs, or global_B != B (single GPU only).  The descriptor is unchanged. */
int drq_update_phase_per(const DrqStep* s, int phase, const float* is_weight, float* td_abs);

/* The indexed update on a single-frame ring ("single-frame step-major replay"): s->obs == s->next_obs = the ring's
 * frames u8 [R N][3][84][84], s->obs_index / s->next_obs_index = the newest-frame slots of the two stacks of every row,
 * first u8 [R N] the ring's flags.  is_weight and td_abs: both NULL = the plain loss, both given =
 * drq_update_phase_per's weighted loss.  The launches are the indexed update's one for one (the fused aug+conv1 launch
 * gathers the stacks); the result is, bit for bit, the update on the stacks drq_vec_stack_gather produces.
 * DRQ_EARG: null first, R, N <= 0, missing indices, s->obs != s->next_obs, global_B != B (single GPU only), one of
 * is_weight / td_abs without the other.  The descriptor is unchanged. */
int drq_update_phase_frames(const DrqStep* s, int phase, const uint8_t* first, long R, long N, const float* is_weight,
                            float* td_abs);

/* sums[0..7] -> sums_host[0..7], then seq -> slot 8 with system-scope release (see DrqStep.sums_host); for hosts
 * that reduce the sums themselves before publishing them. */
int drq_publish_sums(const float* sums, float* sums_host, unsigned seq, drq_stream_t stream);

/* Encoder+actor forward for DrQV2Agent.act (drqv2.py:164-175): obs u8 [n][C][84][84] -> mu [n][A]
 * (n <= 2*B; uses s->params, s->ws, s->stream only; must not run between the phases of an update). */
int drq_act_forward(const DrqStep* s, const uint8_t* obs, int n, float* mu_out);

/* ---- batched policy inference on launches of its own (csrc/act.hip): the body of DrQV2Agent.act (drqv2.py:164-175)
 * for n frame stacks at once, without unsqueeze(0) / [0].  obs u8 [n][C][84][84] -> obs/255 - 0.5 (:64) -> the four
 * Conv2d+ReLU (:55-59) -> flatten (:66) -> actor trunk Linear + LayerNorm + tanh (:74-75) -> policy MLP (:77-81) ->
 * tanh = mu [n][A] (:88-89); action_out [n][A] = mu (noise == NULL: dist.mean, :169) or clamp(mu + noise*std,
 * +-(1 - 1e-6)) with noise [n][A] the caller's standard-normal draw (dist.sample(clip=None), :171, utils.py:112-126).
 * The :173-174 uniform_ override stays with the caller.  fp32 throughout; six kernel launches for any n; the weights
 * are read from `params` (the arena of drq_param_layout) as they are when the launches run, nothing is cached between
 * calls.  Domain: C = 9, 1 <= n <= 256, 0 < F <= 256, any A, H >= 1; anything else is DRQ_EARG before any launch.
 * ws: drq_act_ws_bytes(n_max, ...) bytes (0 = unsupported dimensions) serve every n <= n_max; a ws_bytes smaller than
 * drq_act_ws_bytes(n, ...) is DRQ_EWS.  It is scratch only: no counter or state lives in it, and it is never the step
 * workspace, so a call may sit between the phases of an update.  mu_out may be NULL. */
size_t drq_act_ws_bytes(int n_max, int C, int A, int F, int H);
int drq_act_batch(const float* params, int C, int A, int F, int H, const uint8_t* obs, int n, const float* noise,
                  float std, float* mu_out, float* action_out, void* ws, size_t ws_bytes, drq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
