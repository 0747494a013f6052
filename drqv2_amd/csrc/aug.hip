// RandomShiftsAug (drqv2.py:19-45) fused with the encoder's /255-0.5 (drqv2.py:64), and that conversion alone.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// RandomShiftsAug: replicate-pad by `pad`, bilinear grid_sample (zeros, align_corners=False) at
// base[j] + shift*2/S.  One thread per output pixel, looping over channels (coordinates and the
// four tap weights are per (sample,y,x)).  Arithmetic follows ATen's GridSampler scalar formulas.
// ------------------------------------------------------------------------------------------------
// obs1/shift1 (optional): a second set of n frames handled by blockIdx.y == 1, written behind the first n frames of
// out (the update augments obs and next_obs with independent shifts: one launch for both)
// v / 255 correctly rounded (v >= 0, normal range) in three instructions instead of the IEEE division sequence:
// q = v*r, e = v - 255 q (exact), q' = q + e*r with r = RN(1/255).  tools/check_div255.py checks every float32
// mantissa against the exactly rounded quotient (the identity is scale invariant).
__device__ __forceinline__ float div255(float v) {
  const float r = 1.0f / 255.0f;
  const float q = __fmul_rn(v, r);
  const float e = __fmaf_rn(-q, 255.0f, v);
  return __fmaf_rn(e, r, q);
}

template <typename T>
__global__ void aug_kernel(const T* __restrict__ obs, const float* __restrict__ shift,
                           const float* __restrict__ base, float* __restrict__ out, int n, int c, int h,
                           int pad, int fuse_norm, const T* __restrict__ obs1 = nullptr,
                           const float* __restrict__ shift1 = nullptr) {
  // one rounding per operation, in the order of the CPU restatement (oracle/drq_oracle.py
  // random_shifts_aug): the tap weights are differences of nearly equal numbers, so a fused
  // multiply-add anywhere in the coordinate chain changes them by O(1) relative.
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int hw = h * h;
  if (idx >= (long)n * hw) return;
  if (blockIdx.y == 1) {
    obs = obs1;
    shift = shift1;
    out += (long)n * c * hw;
  }
  const int b = (int)(idx / hw);
  const int r = (int)(idx - (long)b * hw);
  const int i = r / h, j = r - i * h;
  const int S = h + 2 * pad;
  const float sc = (float)(2.0 / (double)S);
  const float gx = base[j] + shift[2 * b + 0] * sc;
  const float gy = base[i] + shift[2 * b + 1] * sc;
  const float ix = ((gx + 1.f) * (float)S - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)S - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix;
  const float wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
  const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;   // nw, ne, sw, se
  const bool okx0 = x0 >= 0 && x0 < S, okx1 = x0 + 1 >= 0 && x0 + 1 < S;
  const bool oky0 = y0 >= 0 && y0 < S, oky1 = y0 + 1 >= 0 && y0 + 1 < S;
  auto cl = [&](int v) { v -= pad; return v < 0 ? 0 : (v > h - 1 ? h - 1 : v); };
  const int sx0 = cl(x0), sx1 = cl(x0 + 1), sy0 = cl(y0), sy1 = cl(y0 + 1);
  const T* src = obs + (long)b * c * hw;
  float* dst = out + (long)b * c * hw + r;
  const int o00 = sy0 * h + sx0, o01 = sy0 * h + sx1, o10 = sy1 * h + sx0, o11 = sy1 * h + sx1;
  const bool k00 = okx0 && oky0, k01 = okx1 && oky0, k10 = okx0 && oky1, k11 = okx1 && oky1;
  auto blend = [&](float t00, float t01, float t10, float t11) {
    // each product is rounded on its own (torch's grid_sample does not fuse them): the empty asm keeps hipcc from
    // contracting a product into the following add, which the contract(off) pragma does not prevent in a lambda
    float p0 = t00 * w00, p1 = t01 * w01, p2 = t10 * w10, p3 = t11 * w11;
    asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
    float v = 0.f;
    if (k00) v = v + p0;
    if (k01) v = v + p1;
    if (k10) v = v + p2;
    if (k11) v = v + p3;
    if (fuse_norm) v = __fsub_rn(div255(v), 0.5f);
    return v;
  };
  if (c == 9) {          // frame_stack 3 (cfgs/config.yaml:7): all 36 tap loads in flight together
    T t[9][4];
#pragma unroll
    for (int ch = 0; ch < 9; ++ch) {
      const T* s = src + (long)ch * hw;
      t[ch][0] = s[o00]; t[ch][1] = s[o01]; t[ch][2] = s[o10]; t[ch][3] = s[o11];
    }
#pragma unroll
    for (int ch = 0; ch < 9; ++ch)
      dst[(long)ch * hw] = blend((float)t[ch][0], (float)t[ch][1], (float)t[ch][2], (float)t[ch][3]);
  } else {
    for (int ch = 0; ch < c; ++ch) {
      const T* s = src + (long)ch * hw;
      dst[(long)ch * hw] = blend((float)s[o00], (float)s[o01], (float)s[o10], (float)s[o11]);
    }
  }
}

// The same augmentation for uint8 frames with the source rows staged through LDS.  aug_kernel issues 4 byte
// loads per channel and pixel (36 global load instructions per thread, 64 bytes each per wave): at 9x84x84 it is
// bound by the texture addresser, not by memory (63 us for 163 MB).  Here a workgroup owns R output rows of one
// sample: it copies the source rows those touch (all channels, usually R+1 rows of h bytes) into LDS with dword
// loads, and the four taps become LDS byte reads.  Coordinates, weights, tap selection and the blend are the
// statements of aug_kernel, so results are bit-identical; a row range that does not fit NR rows (not expected:
// the grid is monotone with unit steps) reads its taps from global memory like aug_kernel.
__global__ __launch_bounds__(256) void aug_rows_kernel(const uint8_t* __restrict__ obs, const float* __restrict__ shift,
                                                       const float* __restrict__ base, float* __restrict__ out,
                                                       int n, int c, int h, int pad, int fuse_norm,
                                                       const uint8_t* __restrict__ obs1,
                                                       const float* __restrict__ shift1, int R, int NR) {
#pragma clang fp contract(off)
  extern __shared__ unsigned aug_lds[];           // [c][NR][h/4] dwords
  const int hw = h * h, hq = h >> 2;
  const int b = blockIdx.y;
  if (blockIdx.z == 1) {
    obs = obs1;
    shift = shift1;
    out += (long)n * c * hw;
  }
  const int S = h + 2 * pad;
  const float sc = (float)(2.0 / (double)S);
  auto cl = [&](int v) { v -= pad; return v < 0 ? 0 : (v > h - 1 ? h - 1 : v); };
  const float shx = shift[2 * b + 0] * sc, shy = shift[2 * b + 1] * sc;
  auto coord = [&](int k, float sh, float& f) {   // unnormalised sample coordinate of grid index k
    const float g = base[k] + sh;
    const float v = ((g + 1.f) * (float)S - 1.f) / 2.f;
    f = floorf(v);
    return v;
  };
  const int i0 = blockIdx.x * R;
  const int ilast = i0 + R - 1 < h - 1 ? i0 + R - 1 : h - 1;
  float fa, fb;
  coord(i0, shy, fa);
  coord(ilast, shy, fb);
  const int sy_lo = cl((int)fa), sy_hi = cl((int)fb + 1);       // the grid is increasing: rows in between lie inside
  const int nrows = sy_hi - sy_lo + 1;
  const bool staged = nrows >= 1 && nrows <= NR;
  const uint8_t* src = obs + (long)b * c * hw;
  if (staged) {
    // thread -> (row slot, dword of the row); row slots walk the (channel, row) pairs without a division per step
    const int rs = threadIdx.x / hq, q = threadIdx.x - rs * hq;
    const int nslots = 256 / hq;
    if (rs < nslots) {
      const int step_ch = nslots / nrows, step_r = nslots - step_ch * nrows;
      int ch = rs / nrows, r = rs - ch * nrows;
      while (ch < c) {
        aug_lds[(ch * NR + r) * hq + q] =
            reinterpret_cast<const unsigned*>(src + (long)ch * hw + (long)(sy_lo + r) * h)[q];
        r += step_r;
        ch += step_ch;
        if (r >= nrows) {
          r -= nrows;
          ++ch;
        }
      }
    }
  }
  __syncthreads();
  const int il = threadIdx.x / h, j = threadIdx.x - il * h;
  const int i = i0 + il;
  if (il >= R || i >= h) return;
  float fx, fy;
  const float ix = coord(j, shx, fx), iy = coord(i, shy, fy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix;
  const float wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
  const bool okx0 = x0 >= 0 && x0 < S, okx1 = x0 + 1 >= 0 && x0 + 1 < S;
  const bool oky0 = y0 >= 0 && y0 < S, oky1 = y0 + 1 >= 0 && y0 + 1 < S;
  const int sx0 = cl(x0), sx1 = cl(x0 + 1), sy0 = cl(y0), sy1 = cl(y0 + 1);
  // a tap outside the padded frame is skipped by aug_kernel; here it gets weight +0 (t >= 0, so the sum is
  // unchanged bit for bit), and the first add of aug_kernel is 0 + x = x: no selects and one add less per channel
  const float w00 = okx0 && oky0 ? wx0 * wy0 : 0.f, w01 = okx1 && oky0 ? wx1 * wy0 : 0.f;     // nw, ne
  const float w10 = okx0 && oky1 ? wx0 * wy1 : 0.f, w11 = okx1 && oky1 ? wx1 * wy1 : 0.f;     // sw, se
  auto blend = [&](float t00, float t01, float t10, float t11) {
    // each product is rounded on its own: the empty asm keeps hipcc from contracting it into the following add
    // (the contract(off) pragma is not honoured inside this lambda once the selects around the adds are gone)
    float p0 = t00 * w00, p1 = t01 * w01, p2 = t10 * w10, p3 = t11 * w11;
    asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
    float v = p0 + p1;
    v = v + p2;
    v = v + p3;
    if (fuse_norm) v = __fsub_rn(div255(v), 0.5f);
    return v;
  };
  float* dst = out + (long)b * c * hw + i * h + j;
  if (staged) {
    const uint8_t* l = reinterpret_cast<const uint8_t*>(aug_lds);
    const int o00 = (sy0 - sy_lo) * h + sx0, o01 = (sy0 - sy_lo) * h + sx1;
    const int o10 = (sy1 - sy_lo) * h + sx0, o11 = (sy1 - sy_lo) * h + sx1;
    for (int ch = 0; ch < c; ++ch) {
      const uint8_t* s = l + ch * NR * h;
      dst[(long)ch * hw] = blend((float)s[o00], (float)s[o01], (float)s[o10], (float)s[o11]);
    }
  } else {
    const int o00 = sy0 * h + sx0, o01 = sy0 * h + sx1, o10 = sy1 * h + sx0, o11 = sy1 * h + sx1;
    for (int ch = 0; ch < c; ++ch) {
      const uint8_t* s = src + (long)ch * hw;
      dst[(long)ch * hw] = blend((float)s[o00], (float)s[o01], (float)s[o10], (float)s[o11]);
    }
  }
}

// rows-in-LDS launch when the frame layout allows it (dword rows); returns false when it does not
bool launch_aug_rows(const uint8_t* obs, const float* shift, const uint8_t* obs1, const float* shift1,
                     const float* base, float* out, int n, int c, int h, int pad, int fuse_norm, hipStream_t st) {
  if (h % 4 != 0 || h > 256 || n > 65535 || ((uintptr_t)obs & 3) || (obs1 && ((uintptr_t)obs1 & 3))) return false;
  const int R = 256 / h, NR = R + 2;
  const size_t lds = (size_t)c * NR * h;
  if (R < 1 || lds > 64 * 1024) return false;
  hipLaunchKernelGGL(aug_rows_kernel, dim3((unsigned)((h + R - 1) / R), (unsigned)n, obs1 ? 2 : 1), dim3(256), lds, st,
                     obs, shift, base, out, n, c, h, pad, fuse_norm, obs1, shift1, R, NR);
  return true;
}

__global__ void u8_normalize_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (float)x[i] / 255.0f - 0.5f;
}

}  // namespace

DRQ_API int drq_aug_fwd(const uint8_t* obs, const float* shift_xy, const float* base_grid, float* out, int n, int c,
                int hw, int pad, int fuse_norm, hipStream_t st) {
  if (!obs || !shift_xy || !base_grid || !out || n <= 0 || c <= 0 || hw <= 0 || pad < 0) return DRQ_EARG;
  if (launch_aug_rows(obs, shift_xy, nullptr, nullptr, base_grid, out, n, c, hw, pad, fuse_norm, st)) {
    DRQ_LAUNCH_CHECK();
    return DRQ_OK;
  }
  const long total = (long)n * hw * hw;
  hipLaunchKernelGGL(aug_kernel<uint8_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, obs, shift_xy,
                     base_grid, out, n, c, hw, pad, fuse_norm);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// same op on a float frame (RandomShiftsAug.forward is handed obs.float(), drqv2.py:241)
DRQ_API int drq_aug_fwd_f32(const float* x, const float* shift_xy, const float* base_grid, float* out, int n, int c, int hw,
                    int pad, hipStream_t st) {
  if (!x || !shift_xy || !base_grid || !out || n <= 0 || c <= 0 || hw <= 0 || pad < 0) return DRQ_EARG;
  const long total = (long)n * hw * hw;
  hipLaunchKernelGGL(aug_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, shift_xy, base_grid,
                     out, n, c, hw, pad, 0);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// Encoder input conversion without augmentation (drqv2.py:64 on a uint8 frame, as act() does)
DRQ_API int drq_u8_normalize(const uint8_t* x, float* y, long n, hipStream_t st) {
  if (!x || !y || n <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(u8_normalize_kernel, dim3(drq_grid_for(n)), dim3(256), 0, st, x, y, n);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
