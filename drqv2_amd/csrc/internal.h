// Launchers called across the library's .hip files that are not part of the C ABI (include/drqv2_hip.h).
// Every function here has C++ linkage and hidden visibility: the mangled name carries the signature, so a definition
// that drifts from its declaration fails to compile in the defining file (which includes this header) or to link
// (-z defs).  Grouped by defining file.
#pragma once
#include "common.h"
#include "conv_plan.h"
#include "gemm_plan.h"

// ---- layernorm.hip
// LayerNorm+tanh of n problems; problem i may also copy tail_n (<= 64) columns of tail[i] behind its F outputs, and
// part != NULL sums the split-K partials of drq_gemm_batched_partial instead of reading z
int drq_ln_tanh_fwd_multi_part(int n, const float* const* z, int ldz, const float* const* gamma,
                               const float* const* beta, float* const* out, const int* ldo, float* const* xhat,
                               float* const* rstd, int rows, int F, const float* const* tail, const int* tail_ld,
                               int tail_n, const float* part, const float* const* bias, int splitk, hipStream_t st);
int drq_ln_tanh_bwd_part(const float* dh0, int ld0, const float* dh1, int ld1, const float* h, int ldh,
                         const float* xhat, const float* rstd, const float* gamma, float* dz, float* dln,
                         float* dgamma, float* dbeta, int rows, int F, const float* part, int splitk, int nprob,
                         int ldp, hipStream_t st);
int drq_ln_param_grad(const float* dln, const float* xhat, float* dgamma, float* dbeta, int rows, int F,
                      hipStream_t st);

// ---- losses.hip: the actor loss that also publishes to the host mirror (the C entries pass no mirror).
// a_beh != NULL: the DrQ+BC loss; NULL: the plain loss, ldb and alpha unused
int drq_actor_loss_ex(const float* q1, const float* q2, const float* a, long lda, const float* a_beh, long ldb,
                      const float* mu, float std, float alpha, float* dq1, float* dq2, float* sums, int B, int A,
                      float inv_global_B, float* sums_host, unsigned seq, hipStream_t st);

// ---- qout.hip: the twin-Q output layer backward with a loss computed inside it
// the TD loss; is_weight and td_abs [B] both given: weighted per row (prioritized replay, drq_td_mse_w's arithmetic),
// both NULL: the plain loss
int drq_qout_bwd_td(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
                    const float* discount, const float* is_weight, float inv_global_B, float* sums, float* td_abs,
                    const float* const* h, const float* const* w, float* const* dh, float* const* dw, float* const* db,
                    int B, int H, hipStream_t st);
// the actor loss, published to the host mirror when one is given; a_beh as for drq_actor_loss_ex
int drq_qout_bwd_actor(const float* q1, const float* q2, const float* act, long lda, const float* a_beh, long ldb,
                       const float* mu, float std, float alpha, int A, float inv_global_B, float* sums,
                       float* sums_host, unsigned seq, const float* const* h, const float* const* w, float* const* dh,
                       int B, int H, hipStream_t st);

// ---- policy_out.hip
int drq_policy_out_fwd(const float* h2, const float* w, const float* b, float* p3, int rows, int H, int A,
                       const float* noise, float std, float clip, int use_clip, int srow0, float* mu_out,
                       float* a_out, long lda_out, const float* noise0, float* mu_out0, float* a_out0, long lda_out0,
                       hipStream_t st);
// a_beh != NULL: the DrQ+BC pull in dmu (act, lda, ldb, bc_scale); NULL: the plain backward
int drq_policy_out_bwd(const float* da1, const float* da2, long ld, int col0, const float* mu, const float* act,
                       long lda, const float* a_beh, long ldb, float bc_scale, const float* p2, const float* w,
                       float* dp2, float* dw, float* db, int B, int H, int A, const float* part, int splitk,
                       hipStream_t st);

// ---- optim.hip: Adam over two independent segments in one launch
int drq_adam_flat2(float* p0, const float* g0, float* m0, float* v0, long n0, long step0, float* p1, const float* g1,
                   float* m1, float* v1, long n1, long step1, double lr, float gscale, hipStream_t st);

// ---- the GEMM family (gemm.hip, gemm2.hip, gemm3.hip, skinny.hip).  gemm_plan.h chooses the kernel: an entry completes
// the call's GemmShape, asks the planner and hands call and plan to drq_gemm_launch, the one switch over the launchers.
// the LayerNorm parameter gradients that may ride in the trunk weight gradient's launch (rows = 0: none)
struct LnRider {
  const float *dln = nullptr, *xhat = nullptr;
  float *dgamma = nullptr, *dbeta = nullptr;
  int rows = 0, F = 0;
};
// One call: nbatch problems of one shape, C_b = epilogue(A_b B_b).  The caller sets the shape's first block and these;
// the optional arrays may be null and so may their elements
struct GemmCall : GemmShape {
  const float *const *A = nullptr, *const *B = nullptr, *const *bias_p = nullptr, *const *aux_p = nullptr;
  float *const *C = nullptr, *const *rowsum_p = nullptr;   // rowsum: bias gradient of a weight-gradient GEMM
  const float* const* qw = nullptr;   // ring forward: weight row and partial dots of a following Linear(N, 1)
  float* const* qpart = nullptr;
  bool leave_partials = false;        // a split-K result stays in ws as records, the caller sums them
  LnRider ln;                         // rides where the plan is the trunk weight gradient's kernel, else its own launch
  float* ws = nullptr;
  hipStream_t st = nullptr;
};
// argument block shared by the kernels of gemm2.hip and gemm3.hip
struct MlpArgs {
  const float *A[kGemmMaxBatch], *B[kGemmMaxBatch], *bias[kGemmMaxBatch];
  const float* qw[kGemmMaxBatch];            // ring forward: weight row [N] of a following Linear(N, 1) or null
  float* qpart[kGemmMaxBatch];               // its partial dots [M][N / BN] (column tile j: the sum over its columns)
  const float* aux[kGemmMaxBatch];           // ReLU mask source [M][ldaux] or null
  float *C[kGemmMaxBatch], *rowsum[kGemmMaxBatch];   // rowsum (weight-gradient form): [M] row sums of A or null
  long lda, ldb, ldc;
  int ldaux, M, N, K, relu;
  unsigned a_bytes, b_bytes;
};
// row of element r of a lane's 32x32 MFMA accumulator (column = lane & 31, half = lane >> 5)
__device__ __forceinline__ int mfma32_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- gemm.hip.  drq_gemm_prepare derives the shape's second block from the pointers; false: an operand is missing
bool drq_gemm_prepare(GemmCall& c);
MlpArgs drq_gemm_fill(const GemmCall& c);
// GV_NONE -> DRQ_EARG, GV_EWS -> DRQ_EWS; w: the weight-gradient half of a pair plan (c is the input-gradient half)
int drq_gemm_launch(const GemmCall& c, const GemmPlan& p, const GemmCall* w = nullptr);
int drq_gemm_batched_any(GemmCall c);
// the forward form with the split-K sum left to the caller: *splitk_out records per problem in ws, 1 = result in C
int drq_gemm_batched_partial_any(GemmCall c, int* splitk_out);
// both gradients of one hidden layer (w: dW = dy^T x with db, d: dx = (dy W) masked): one launch where a pair kernel
// takes the shapes (the ring kernel's if ring_pair asks for it, else the LDS-free kernel's in fp32), else two calls
int drq_gemm_wgrad_dgrad(GemmCall w, GemmCall d, bool ring_pair);
// ---- skinny.hip, gemm2.hip, gemm3.hip: launchers of a planned call (w, d: the halves of a pair)
// what a launcher returns after its launch: 0 or the hipError_t
inline int drq_launched() { DRQ_LAUNCH_CHECK(); return DRQ_OK; }
int drq_skinny_dgrad(const GemmCall& c);
int drq_trunk_wgrad(const GemmCall& c, const GemmPlan& p);
int drq_trunk_fwd_partial(const GemmCall& c, const GemmPlan& p);
int drq_gemm2(const GemmCall& c, const GemmPlan& p);
int drq_gemm2_wgrad_dgrad(const GemmCall& w, const GemmCall& d, const GemmPlan& p);
int drq_gemm3(const GemmCall& c, const GemmPlan& p);
int drq_gemm3_wgrad_dgrad(const GemmCall& w, const GemmCall& d, const GemmPlan& p);

// ---- rowblock.hip: LayerNorm+tanh fused with the first MLP layers; policy output layer + sample fused with the
// target critic's first layers (DRQ_EARG = shape not eligible)
int drq_lnl1_fwd(int njobs, const float* const* part, const float* const* z, const float* const* bias,
                 const float* const* gamma, const float* const* beta, float* const* out, const int* ldo,
                 float* const* xhat, float* const* rstd, const float* const* tail, const int* tail_ld, const int* tail_n,
                 const int* rows, const int* nheads, const float* const* w, const float* const* b, float* const* y, int F,
                 int H, int splitk, long slab, hipStream_t st);
int drq_polout_l1_fwd(const float* p2, const float* w3, const float* b3, float* p3, int rows, int srow0, int H, int A,
                      int F, float std, float clip, int use_clip, const float* noise_hi, float* mu_hi, float* ha_hi,
                      long lda_hi, const float* noise_lo, float* mu_lo, float* ha_lo, long lda_lo, int nheads,
                      const float* const* w, const float* const* b, float* const* y, hipStream_t st);

// ---- the convolution family (conv.hip, conv_wino.hip, conv_wino_wgrad.hip, conv_bf16.hip, conv1aug.hip).  conv_plan.h
// holds the launch arithmetic: an entry checks its pointers, builds the ConvView of its strided operand, asks the planner
// and hands the kernel's arguments and the plan to a launcher that only launches.
static_assert(kConvOk == DRQ_OK && kConvEarg == DRQ_EARG && kConvEws == DRQ_EWS, "ConvPlan::rc is the entry's result");
// conv1aug.hip: bf_mma selects the bf16-MFMA form of the layer's products; ring_first != NULL: obs == obs1 is a
// ring of single frames (R rows x N environments), fidx0 / fidx1 the newest-frame slots of the stacks
int drq_conv1_aug_fwd_any(int bf_mma, const uint8_t* obs, const float* shift, const uint8_t* obs1, const float* shift1,
                          const float* base_grid, const float* w, const float* bias, float* xaug, float* y, int n,
                          int n_store, hipStream_t st, const float* const* wino_w, float* wino_u, const long* fidx0,
                          const long* fidx1, const uint8_t* ring_first, long ring_R, long ring_N);
// conv_wino.hip: the Winograd kernels with the layer's U image prepared by conv1_aug_kernel's rider
int drq_conv3x3_fwd_wino_pre(const float* x, const float* w, const float* u_image, const float* bias, float* y, int nb,
                             int hin, int relu, ConvView yv, hipStream_t st);
int drq_conv3x3_dgrad_wino_pre(const float* dy_pad, const float* w, const float* u_image, const float* mask, float* dx,
                               int nb, int hout, ConvView dxv, hipStream_t st, int budget = 0);
// conv_bf16.hip: the bf16 launches with activations in bf16 [frame][y][x][32] where the flags say so
int drq_conv3x3_fwd_bf16_lay(const void* x, const float* w, const float* bias, void* y, int nb, int hin, int relu,
                             ConvView yv, int lay, hipStream_t st);
int drq_conv3x3_dgrad_bf16_lay(const void* dy_pad, const float* w, const void* mask, void* dx, int nb, int hout,
                               ConvView dxv, int lay, hipStream_t st);
int drq_conv3x3_wgrad_partial_bf16_lay(const void* x, const void* dy, int nb, int hin, ConvView dyv, float* part,
                                       size_t part_bytes, int* nblocks, int lay, hipStream_t st);
// conv.hip: per-layer partial records; fixed-order reduction of the records of up to four layers; the tail of the public
// weight-gradient entries: rc of their partial launch, then the reduction of its one job
int drq_conv3x3_wgrad_partial(const float* x, const float* dy, int nb, int cin, int hin, int stride, ConvView dyv,
                              float* part, size_t part_bytes, int* nblocks, hipStream_t st);
int drq_conv3x3_wgrad_reduce_multi(int n, const float* const* part, const int* nblocks, const int* cin,
                                   float* const* dw, float* const* db, hipStream_t st);
int drq_conv3x3_wgrad_reduce_one(int rc, const float* part, int nblocks, int cin, float* dw, float* db, hipStream_t st);
// conv_wino_wgrad.hip: the 32->32 layers' records in Winograd form (same format, same reduction); wino3: conv2..4 in one
// launch where plan_ww3 merges them (DRQ_EARG where it does not)
int drq_conv3x3_wgrad_partial_wino(const float* x, const float* dy, int nb, int hin, ConvView dyv, float* part,
                                   size_t part_bytes, int* nblocks, hipStream_t st);
int drq_conv3x3_wgrad_partial_wino3(const float* const* x, const float* const* dy, int nb, const ConvView* dyv,
                                    float* const* part, size_t part_bytes, int* nblocks, hipStream_t st);

// ---- act.hip: batched policy inference on launches of its own (drq_act_batch; the C entry lives in step.hip beside
// the parameter layout).  ws holds drq_act_batch_ws_floats(n, F, H) floats; no state, no counter.
constexpr int kActMaxRows = 256;
struct ActWeights {
  const float *enc_w[4], *enc_b[4];
  const float *trunk_w, *trunk_b, *ln_g, *ln_b;
  const float *w[3], *b[3];   // policy MLP
};
bool drq_act_batch_supported(int n, int C, int A, int F, int H);
long drq_act_batch_ws_floats(int n, int F, int H);
int drq_act_batch_launch(const ActWeights& p, int A, int F, int H, const uint8_t* obs, int n, const float* noise,
                         float std, float* mu_out, float* action_out, float* ws, hipStream_t st);

// ---- vecstats.hip: the 64-byte header of the episode statistics (include/drqv2_hip.h, "episode statistics"), as the
// device state and the host mirror hold it
struct VecStatsHeader {
  long rows, episodes, length_sum;
  double return_sum;
  float min_return, max_return;
  int reserved[6];
};
static_assert(sizeof(VecStatsHeader) == 64, "the header is 64 bytes");
