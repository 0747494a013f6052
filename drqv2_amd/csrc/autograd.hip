// Backward kernels that only the autograd path of the modules needs (drqv2_amd/autograd.py): the update() step
// never differentiates with respect to its inputs, so it has no use for them.
//   relu_mask_pad: the encoder output's gradient, masked by conv4's ReLU, into the zero-padded conv-gradient layout;
//   conv1_dgrad:   input gradient of Conv2d(9,32,3,stride 2) (drqv2.py:55) in gather form;
//   aug_bwd_f32:   input gradient of RandomShiftsAug on a float frame (drqv2.py:19-45) in gather form;
//   tanh_bwd:      dy * (1 - y^2) of the policy's output tanh (drqv2.py:89).
// Every output element is written by one thread with a fixed summation order: no atomics, run-to-run bit-stable.
#include "common.h"

namespace {

__global__ void relu_mask_pad_kernel(const float* __restrict__ dy, const float* __restrict__ mask,
                                     float* __restrict__ out, long total, int h, int pad) {
  const unsigned hp = h + 2 * pad;
  const unsigned plane = hp * hp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const unsigned p = (unsigned)i / plane;            // total < 2^32 (checked by the launcher)
    const unsigned r = (unsigned)i - p * plane;
    const int y = (int)(r / hp) - pad, x = (int)(r - (r / hp) * hp) - pad;
    float v = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < h) {
      const long s = ((long)p * h + y) * h + x;
      // threshold_backward: the gradient passes where the ReLU's output is > 0 (a select, not a product)
      v = (mask == nullptr || mask[s] > 0.f) ? dy[s] : 0.f;
    }
    out[i] = v;
  }
}

// dx[b][ci][iy][ix] = sum over (co, ky, kx) with iy = 2 oy + ky, ix = 2 ox + kx of dy[b][co][oy][ox] w[co][ci][ky][kx].
// An even input row takes ky = 0 (oy = iy/2) and ky = 2 (oy = iy/2 - 1), an odd one ky = 1 only; columns alike.  One
// thread owns the 2x2 input block (2n..2n+1, 2m..2m+1) of all nine channels: it reads dy at (n, m), (n, m-1),
// (n-1, m), (n-1, m-1) and every lane runs the same nine taps per output channel (no divergence); the weight indices
// are wave-uniform.  Out-of-range oy / ox (-1 and 41) fall on the zero border of dy_pad, so row and column 83 are 0.
constexpr int kC1Hp = 45, kC1Hi = 84, kC1N = 42, kC1Ci = 9;

__global__ __launch_bounds__(256) void conv1_dgrad_kernel(const float* __restrict__ dyp, const float* __restrict__ w,
                                                          float* __restrict__ dx, int nb) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nb * kC1N * kC1N) return;
  const int b = t / (kC1N * kC1N);
  const int r = t - b * kC1N * kC1N;
  const int n = r / kC1N, m = r - n * kC1N;
  float acc[kC1Ci][4];
#pragma unroll
  for (int ci = 0; ci < kC1Ci; ++ci) acc[ci][0] = acc[ci][1] = acc[ci][2] = acc[ci][3] = 0.f;
  const float* d = dyp + (long)b * kCout * kC1Hp * kC1Hp + (n + 2) * kC1Hp + (m + 2);
  for (int co = 0; co < kCout; ++co) {
    const float* dc = d + co * kC1Hp * kC1Hp;
    const float v00 = dc[0];              // dy[n][m]
    const float v01 = dc[-1];             // dy[n][m-1]
    const float v10 = dc[-kC1Hp];         // dy[n-1][m]
    const float v11 = dc[-kC1Hp - 1];     // dy[n-1][m-1]
    const float* wc = w + co * kC1Ci * 9;
#pragma unroll
    for (int ci = 0; ci < kC1Ci; ++ci) {
      const float* k = wc + ci * 9;
      acc[ci][0] += v00 * k[0] + v01 * k[2] + v10 * k[6] + v11 * k[8];   // (2n,   2m)
      acc[ci][1] += v00 * k[1] + v10 * k[7];                             // (2n,   2m+1)
      acc[ci][2] += v00 * k[3] + v01 * k[5];                             // (2n+1, 2m)
      acc[ci][3] += v00 * k[4];                                          // (2n+1, 2m+1)
    }
  }
  float* o = dx + (long)b * kC1Ci * kC1Hi * kC1Hi + (2 * n) * kC1Hi + 2 * m;
#pragma unroll
  for (int ci = 0; ci < kC1Ci; ++ci) {
    float* oc = o + ci * kC1Hi * kC1Hi;
    *reinterpret_cast<float2*>(oc) = make_float2(acc[ci][0], acc[ci][1]);
    *reinterpret_cast<float2*>(oc + kC1Hi) = make_float2(acc[ci][2], acc[ci][3]);
  }
}

// RandomShiftsAug backward.  The forward (aug.hip aug_kernel) samples output (i, j) from the four taps
// (x0 + {0,1}, y0 + {0,1}) of the replicate-padded frame with weights wx_t * wy_u that are 0 / 1 only up to fp32
// rounding of the grid coordinate (1e-5 off at the far end of the frame).  Its exact adjoint: source pixel (sy, sx)
// collects dy[i][j] * wy(i) * wx(j), where wx(j) sums the x weights of the taps of column j that land on sx after the
// replicate clamp (both do at the border).  The weights are recomputed with the forward's own statements.
constexpr int kAugCand = 8;   // output columns that can reach one source column: 4 inside, pad + 3 at a border

__device__ __forceinline__ float aug_axis_weight(int o, int s, float sh, const float* __restrict__ base, int h, int pad) {
#pragma clang fp contract(off)
  const int S = h + 2 * pad;
  const float sc = (float)(2.0 / (double)S);
  const float g = base[o] + sh * sc;
  const float ix = ((g + 1.f) * (float)S - 1.f) / 2.f;
  const float f = floorf(ix);
  const int x0 = (int)f;
  const float w1 = ix - f, w0 = (f + 1.f) - ix;
  float wt = 0.f;
  auto cl = [&](int v) { v -= pad; return v < 0 ? 0 : (v > h - 1 ? h - 1 : v); };
  if (x0 >= 0 && x0 < S && cl(x0) == s) wt = wt + w0;
  if (x0 + 1 >= 0 && x0 + 1 < S && cl(x0 + 1) == s) wt = wt + w1;
  return wt;
}

// candidate outputs [lo, lo + kAugCand) of source coordinate s under shift sh (a tap position is within 2 of o + sh)
__device__ __forceinline__ int aug_axis_lo(int s, float sh, int h, int pad) {
  const int si = (int)floorf(sh);
  const int lo = s == 0 ? 0 : (s == h - 1 ? h - 3 + pad - si : s + pad - si - 2);
  return lo < 0 ? 0 : lo;
}
__device__ __forceinline__ int aug_axis_hi(int s, float sh, int h, int pad) {
  const int si = (int)floorf(sh);
  const int hi = s == h - 1 ? h - 1 : (s == 0 ? pad - si + 1 : s + pad - si + 1);
  return hi > h - 1 ? h - 1 : hi;
}

__global__ __launch_bounds__(256) void aug_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ shift,
                                                      const float* __restrict__ base, float* __restrict__ dx, int n, int c,
                                                      int h, int pad) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int hw = h * h;
  if (idx >= (long)n * hw) return;
  const int b = (int)(idx / hw);
  const int r = (int)(idx - (long)b * hw);
  const int sy = r / h, sx = r - sy * h;
  const float shx = shift[2 * b + 0], shy = shift[2 * b + 1];
  const int lx = aug_axis_lo(sx, shx, h, pad), hx = aug_axis_hi(sx, shx, h, pad);
  const int ly = aug_axis_lo(sy, shy, h, pad), hy = aug_axis_hi(sy, shy, h, pad);
  float wx[kAugCand], wy[kAugCand];
#pragma unroll
  for (int k = 0; k < kAugCand; ++k) {
    wx[k] = lx + k <= hx ? aug_axis_weight(lx + k, sx, shx, base, h, pad) : 0.f;
    wy[k] = ly + k <= hy ? aug_axis_weight(ly + k, sy, shy, base, h, pad) : 0.f;
  }
  const float* src = dy + (long)b * c * hw;
  float* dst = dx + (long)b * c * hw + r;
  for (int ch = 0; ch < c; ++ch) {
    const float* p = src + (long)ch * hw;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < kAugCand; ++ky) {
      if (wy[ky] == 0.f) continue;
      const float* row = p + (long)(ly + ky) * h + lx;
      float racc = 0.f;
#pragma unroll
      for (int kx = 0; kx < kAugCand; ++kx)
        if (wx[kx] != 0.f) racc += wx[kx] * row[kx];
      acc += wy[ky] * racc;
    }
    dst[(long)ch * hw] = acc;
  }
}

__global__ void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float t = y[i];
    dx[i] = dy[i] * (1.f - t * t);
  }
}

inline unsigned grid_cap(long n) {
  long g = (n + 255) / 256;
  const long cap = 8L * drq_num_cus();
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

DRQ_API int drq_relu_mask_pad(const float* dy, const float* mask, float* out, long planes, int h, int pad,
                              hipStream_t st) {
  if (!dy || !out || planes <= 0 || h <= 0 || pad < 0) return DRQ_EARG;
  const long total = planes * (long)(h + 2 * pad) * (h + 2 * pad);
  if (total >= (1L << 32)) return DRQ_EARG;
  hipLaunchKernelGGL(relu_mask_pad_kernel, dim3(grid_cap(total)), dim3(256), 0, st, dy, mask, out, total, h, pad);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_conv1_dgrad(const float* dy_pad, const float* w, float* dx, int nb, hipStream_t st) {
  if (!dy_pad || !w || !dx || nb <= 0 || (long)nb * kC1N * kC1N >= (1L << 31)) return DRQ_EARG;
  if (reinterpret_cast<uintptr_t>(dx) % 8) return DRQ_EARG;   // float2 stores
  const long threads = (long)nb * kC1N * kC1N;
  hipLaunchKernelGGL(conv1_dgrad_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, dy_pad, w, dx, nb);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_aug_bwd_f32(const float* dy, const float* shift_xy, const float* base_grid, float* dx, int n, int c,
                            int hw, int pad, hipStream_t st) {
  // pad + 3 candidate columns per border source column must fit kAugCand
  if (!dy || !shift_xy || !base_grid || !dx || n <= 0 || c <= 0 || hw <= 0 || pad < 0 || pad + 3 > kAugCand)
    return DRQ_EARG;
  const long total = (long)n * hw * hw;
  hipLaunchKernelGGL(aug_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dy, shift_xy, base_grid,
                     dx, n, c, hw, pad);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_tanh_bwd(const float* y, const float* dy, float* dx, long n, hipStream_t st) {
  if (!y || !dy || !dx || n <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(grid_cap(n)), dim3(256), 0, st, y, dy, dx, n);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
