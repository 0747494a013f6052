// Optimiser steps and flat maps: Adam (torch/optim/adam.py) with optional fused Polyak (utils.py:42-45), its two-segment
// and sharded forms, the rank-ordered slice sum, Polyak alone, fill and tanh.
#include "common.h"
#include "internal.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults) over a flat arena, rounding sequence of torch's CPU kernels
// (oracle/drq_oracle.py:adam_step), optional fused Polyak update of a target arena.
// ------------------------------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n, float neg_step_size, float sqrt_bc2, float gscale,
                            float* __restrict__ tgt, float tau, float one_minus_tau) {
  // one rounding per operation, in torch's order (oracle/drq_oracle.py:adam_step); sqrtf and / are the
  // IEEE-correct forms (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is NOT.
#pragma clang fp contract(off)
  const float w1 = (float)(1.0 - 0.9), b2 = 0.999f, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (gscale != 1.0f) gi *= gscale;
    const float mi = __fmaf_rn(w1, __fsub_rn(gi, m[i]), m[i]);
    const float vi = __fmaf_rn(__fmul_rn(gi, w2), gi, __fmul_rn(v[i], b2));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(vi), sqrt_bc2), eps);
    const float pi = __fadd_rn(p[i], __fdiv_rn(__fmul_rn(neg_step_size, mi), denom));
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (tgt) tgt[i] = __fadd_rn(__fmul_rn(tau, pi), __fmul_rn(one_minus_tau, tgt[i]));
  }
}

struct AdamSeg2 {
  float* p[2];
  const float* g[2];
  float* m[2];
  float* v[2];
  long n[2];
  float neg_step_size[2], sqrt_bc2[2];
  float gscale;
};

__global__ void adam2_kernel(AdamSeg2 a) {
#pragma clang fp contract(off)
  const int z = blockIdx.y;
  float* __restrict__ p = a.p[z];
  const float* __restrict__ g = a.g[z];
  float* __restrict__ m = a.m[z];
  float* __restrict__ v = a.v[z];
  const long n = a.n[z];
  const float neg_step_size = a.neg_step_size[z], sqrt_bc2 = a.sqrt_bc2[z];
  const float w1 = (float)(1.0 - 0.9), b2 = 0.999f, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (a.gscale != 1.0f) gi *= a.gscale;
    const float mi = __fmaf_rn(w1, __fsub_rn(gi, m[i]), m[i]);
    const float vi = __fmaf_rn(__fmul_rn(gi, w2), gi, __fmul_rn(v[i], b2));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(vi), sqrt_bc2), eps);
    const float pi = __fadd_rn(p[i], __fdiv_rn(__fmul_rn(neg_step_size, mi), denom));
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// Data parallel, sharded optimiser (ZeRO-1): this rank owns n parameters of a segment; recv holds the `world` ranks'
// copies of its gradient slice (recv[r*stride + i], the result of an all-to-all) -- summed here in RANK ORDER (the same
// order on every rank and in drq_sum_slices: bit-identical to the replicated path) and fed straight into the Adam
// arithmetic of adam_kernel; the gradient sum never goes back to memory.
__global__ void adam_reduce_kernel(float* __restrict__ p, const float* __restrict__ recv, long stride, int world,
                                   float* __restrict__ m, float* __restrict__ v, long n, float neg_step_size,
                                   float sqrt_bc2, float gscale) {
#pragma clang fp contract(off)
  const float w1 = (float)(1.0 - 0.9), b2 = 0.999f, w2 = (float)(1.0 - 0.999), eps = 1e-8f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = recv[i];
    for (int r = 1; r < world; ++r) gi = __fadd_rn(gi, recv[(long)r * stride + i]);
    if (gscale != 1.0f) gi *= gscale;
    const float mi = __fmaf_rn(w1, __fsub_rn(gi, m[i]), m[i]);
    const float vi = __fmaf_rn(__fmul_rn(gi, w2), gi, __fmul_rn(v[i], b2));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(vi), sqrt_bc2), eps);
    p[i] = __fadd_rn(p[i], __fdiv_rn(__fmul_rn(neg_step_size, mi), denom));
    m[i] = mi;
    v[i] = vi;
  }
}

// out[i] = ((in[i] + in[stride + i]) + in[2*stride + i]) + ... : the `world` copies of a gradient slice in rank order
__global__ void sum_slices_kernel(const float* __restrict__ in, long stride, int world, float* __restrict__ out, long n) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float s = in[i];
    for (int r = 1; r < world; ++r) s = __fadd_rn(s, in[(long)r * stride + i]);
    out[i] = s;
  }
}

__global__ void ema_kernel(const float* __restrict__ p, float* __restrict__ t, long n, float tau,
                           float one_minus_tau) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    t[i] = __fadd_rn(__fmul_rn(tau, p[i]), __fmul_rn(one_minus_tau, t[i]));
}

__global__ void fill_kernel(float* p, long n, float v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void tanh_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = tanhf(x[i]);
}

// step = 1-based Adam step count; the bias corrections are formed in double on the host exactly as
// torch/optim/adam.py does, and rounded to float last
struct AdamScalars {
  float neg_step_size, sqrt_bc2;
};
AdamScalars adam_scalars(double lr, long step) {
  const double bc1 = 1.0 - pow(0.9, (double)step);
  const double bc2 = 1.0 - pow(0.999, (double)step);
  return {(float)(-(lr / bc1)), (float)sqrt(bc2)};
}

}  // namespace

// two independent segments (encoder, actor) in one launch: same arithmetic per element as adam_kernel
int drq_adam_flat2(float* p0, const float* g0, float* m0, float* v0, long n0, long step0, float* p1, const float* g1,
                   float* m1, float* v1, long n1, long step1, double lr, float gscale, hipStream_t st) {
  if (!p0 || !g0 || !m0 || !v0 || !p1 || !g1 || !m1 || !v1 || n0 <= 0 || n1 <= 0 || step0 <= 0 || step1 <= 0)
    return DRQ_EARG;
  AdamSeg2 a{};
  const long steps[2] = {step0, step1};
  float* ps[2] = {p0, p1}; const float* gs[2] = {g0, g1}; float* ms[2] = {m0, m1}; float* vs[2] = {v0, v1};
  const long ns[2] = {n0, n1};
  for (int i = 0; i < 2; ++i) {
    const AdamScalars k = adam_scalars(lr, steps[i]);
    a.p[i] = ps[i]; a.g[i] = gs[i]; a.m[i] = ms[i]; a.v[i] = vs[i]; a.n[i] = ns[i];
    a.neg_step_size[i] = k.neg_step_size;
    a.sqrt_bc2[i] = k.sqrt_bc2;
  }
  a.gscale = gscale;
  const long nmax = n0 > n1 ? n0 : n1;
  hipLaunchKernelGGL(adam2_kernel, dim3(drq_grid_for(nmax), 2), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// tgt != null fuses  tgt <- tau*p_new + (1-tau)*tgt
DRQ_API int drq_adam_flat(float* p, const float* g, float* m, float* v, long n, double lr, long step, float gscale,
                  float* tgt, double tau, hipStream_t st) {
  if (!p || !g || !m || !v || n <= 0 || step <= 0) return DRQ_EARG;
  const AdamScalars k = adam_scalars(lr, step);
  hipLaunchKernelGGL(adam_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, p, g, m, v, n, k.neg_step_size, k.sqrt_bc2,
                     gscale, tgt, (float)tau, (float)(1.0 - tau));
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_adam_reduce_flat(float* p, const float* recv, long stride, int world, float* m, float* v, long n, double lr,
                                 long step, float gscale, hipStream_t st) {
  if (!p || !recv || !m || !v || n <= 0 || step <= 0 || world < 1 || stride < n) return DRQ_EARG;
  const AdamScalars k = adam_scalars(lr, step);
  hipLaunchKernelGGL(adam_reduce_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, p, recv, stride, world, m, v, n,
                     k.neg_step_size, k.sqrt_bc2, gscale);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_sum_slices(const float* in, long stride, int world, float* out, long n, hipStream_t st) {
  if (!in || !out || n <= 0 || world < 1 || stride < n) return DRQ_EARG;
  hipLaunchKernelGGL(sum_slices_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, in, stride, world, out, n);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_ema_flat(const float* p, float* t, long n, double tau, hipStream_t st) {
  if (!p || !t || n <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(ema_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, p, t, n, (float)tau, (float)(1.0 - tau));
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_tanh(const float* x, float* y, long n, hipStream_t st) {
  if (!x || !y || n <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(tanh_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, x, y, n);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_fill(float* p, long n, float v, hipStream_t st) {
  if (!p || n <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(fill_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, p, n, v);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
