// Batched policy inference for DrQV2Agent.act_batch (drqv2.py:164-175 of the reference applied to n frame stacks):
// an inference path of its own for 1..kActMaxRows frames, fp32 throughout, six launches, no cross-workgroup hand-off
// inside a launch (every seam is a launch boundary, so nothing waits on the device and no counter is kept):
//   1  act_conv_pair<conv1, conv2>   uint8 frames -> /255 - 0.5 -> conv1+ReLU -> conv2+ReLU        [n][32][39][39]
//   2  act_conv_pair<conv3, conv4>   -> conv3+ReLU -> conv4+ReLU = the flattened features          [n][39200]
//   3  act_trunk_partial             split-K records of Linear(39200 -> F): ONE pass over the weights for all rows
//   4  act_ln_l1                     sum of the records + bias, LayerNorm, tanh, Linear(F -> H)+ReLU
//   5  act_dense<false>              Linear(H -> H)+ReLU, one wave per output column: the weights are streamed once
//   6  act_dense<true>               Linear(H -> A), tanh = mu, action = clamp(mu + noise*std) (utils.py:112-126)
// The conv launches compute a 6x6 output tile of the second layer from an 8x8 tile of the first one kept in LDS (halo
// recompute): 49 resp. 36 workgroups per frame, so that one frame already spreads over the chip.  Every weight is read
// from the parameter arena inside the launches: nothing is cached between calls.
#include "common.h"
#include "internal.h"

namespace {

constexpr int kR = 32 * 35 * 35;      // repr_dim
constexpr int kTile = 6;              // output tile of the second layer of a pair
constexpr int kMid = kTile + 2;       // tile of the first layer: 8 x 8 = one wave of positions
constexpr int kCoW = 4;               // output channels per wave of a conv workgroup
constexpr int kConvThreads = 32 / kCoW * 64;   // 8 waves: the scalar weight loads of one hide behind the others
constexpr int kKC = 160;              // trunk: columns of the 39200-long reduction per workgroup
constexpr int kChunks = kR / kKC;     // 245 records
constexpr int kTrunkRows = 16;        // trunk / dense: rows per workgroup
static_assert(kChunks * kKC == kR, "the trunk chunks tile the reduction exactly");

__device__ __forceinline__ float act_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// kCoW output channels [co0, co0+kCoW) at one position: acc[j] += sum over a 3x3 window `win` of input channel c.
// co0 is wave-uniform, so the weights come through the scalar path.
template <int CIN>
__device__ __forceinline__ void conv_taps(float (&acc)[kCoW], const float (&win)[9], const float* __restrict__ w, int co0,
                                          int c) {
#pragma unroll
  for (int j = 0; j < kCoW; ++j) {
    const float* wp = w + ((long)(co0 + j) * CIN + c) * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j] = fmaf(win[t], wp[t], acc[j]);
  }
}

// Two encoder layers in one launch.  Layer A: Conv2d(CIN, 32, 3, stride S)+ReLU on an input of HIN x HIN (uint8 frames
// normalised on load when U8, else fp32 NCHW); layer B: Conv2d(32, 32, 3)+ReLU.  Workgroup = (tile, frame); wave w
// computes output channels [4w, 4w+4); a lane is one position of the tile.  out: fp32 NCHW [n][32][HOUT][HOUT] (for the
// last pair that IS the flattened feature row, index c*1225 + y*35 + x).
template <int CIN, int S, int HIN, bool U8>
__global__ __launch_bounds__(kConvThreads) void act_conv_pair_kernel(const void* __restrict__ in, const float* __restrict__ wa,
                                                            const float* __restrict__ ba, const float* __restrict__ wb,
                                                            const float* __restrict__ bb, float* __restrict__ out) {
  constexpr int HMID = (HIN - 3) / S + 1, HOUT = HMID - 2;
  constexpr int TILES = (HOUT + kTile - 1) / kTile;
  constexpr int P = (kMid - 1) * S + 3;          // input patch edge: 17 (stride 2) or 10
  __shared__ float s_in[CIN * P * P];
  __shared__ float s_mid[32 * kMid * kMid];
  const int tid = threadIdx.x, lane = tid & 63;
  const int co0 = __builtin_amdgcn_readfirstlane(tid >> 6) * kCoW;
  const int ty = blockIdx.x / TILES, tx = blockIdx.x - ty * TILES;
  const long frame = blockIdx.y;
  const int iy0 = ty * kTile * S, ix0 = tx * kTile * S;
  // the patch, coordinates clamped to the frame: positions beyond it feed only outputs that are not stored
  for (int i = tid; i < CIN * P * P; i += kConvThreads) {
    const int c = i / (P * P), rem = i - c * (P * P);
    const int py = rem / P, px = rem - py * P;
    const int gy = min(iy0 + py, HIN - 1), gx = min(ix0 + px, HIN - 1);
    const long src = ((frame * CIN + c) * HIN + gy) * HIN + gx;
    if (U8)
      s_in[i] = (float)static_cast<const uint8_t*>(in)[src] / 255.0f - 0.5f;   // drqv2.py:64
    else
      s_in[i] = static_cast<const float*>(in)[src];
  }
  __syncthreads();
  {
    const int my = lane >> 3, mx = lane & 7;
    float acc[kCoW];
#pragma unroll
    for (int j = 0; j < kCoW; ++j) acc[j] = ba[co0 + j];
#pragma unroll 2
    for (int c = 0; c < CIN; ++c) {
      float win[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) win[t] = s_in[c * P * P + (my * S + t / 3) * P + mx * S + t % 3];
      conv_taps<CIN>(acc, win, wa, co0, c);
    }
#pragma unroll
    for (int j = 0; j < kCoW; ++j) s_mid[(co0 + j) * 64 + lane] = fmaxf(acc[j], 0.f);
  }
  __syncthreads();
  {
    const int l = min(lane, kTile * kTile - 1);
    const int py = l / kTile, px = l - py * kTile;
    float acc[kCoW];
#pragma unroll
    for (int j = 0; j < kCoW; ++j) acc[j] = bb[co0 + j];
#pragma unroll 2
    for (int c = 0; c < 32; ++c) {
      float win[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) win[t] = s_mid[c * 64 + (py + t / 3) * kMid + px + t % 3];
      conv_taps<32>(acc, win, wb, co0, c);
    }
    const int oy = ty * kTile + py, ox = tx * kTile + px;
    if (lane < kTile * kTile && oy < HOUT && ox < HOUT) {
#pragma unroll
      for (int j = 0; j < kCoW; ++j)
        out[((frame * 32 + co0 + j) * HOUT + oy) * HOUT + ox] = fmaxf(acc[j], 0.f);
    }
  }
}

// Split-K records of the trunk Linear(39200 -> F): workgroup (chunk, row block) multiplies columns [chunk*160, +160) of
// up to 16 feature rows (LDS) with the same columns of every weight row (registers, each read once per row block).
// Eight lanes share one output: 20 products each, then a three-step tree.  part[chunk][row][f], without bias.
__global__ __launch_bounds__(256) void act_trunk_partial_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ w, float* __restrict__ part,
                                                                int n, int F) {
  __shared__ f32x4 s_x[kTrunkRows][kKC / 4];
  const int tid = threadIdx.x;
  const long k0 = (long)blockIdx.x * kKC;
  const int r0 = blockIdx.y * kTrunkRows;
  const int nr = min(kTrunkRows, n - r0);
  for (int i = tid; i < nr * (kKC / 4); i += 256) {
    const int r = i / (kKC / 4), q = i - r * (kKC / 4);
    s_x[r][q] = reinterpret_cast<const f32x4*>(feat + (long)(r0 + r) * kR + k0)[q];
  }
  __syncthreads();
  const int s = tid & 7, fl = tid >> 3;
  for (int f0 = 0; f0 < F; f0 += 32) {
    const int f = f0 + fl;
    const f32x4* wp = reinterpret_cast<const f32x4*>(w + (long)min(f, F - 1) * kR + k0);
    f32x4 wv[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) wv[i] = wp[s + 8 * i];
    for (int r = 0; r < nr; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const f32x4 x = s_x[r][s + 8 * i];
        acc = fmaf(wv[i].x, x.x, acc);
        acc = fmaf(wv[i].y, x.y, acc);
        acc = fmaf(wv[i].z, x.z, acc);
        acc = fmaf(wv[i].w, x.w, acc);
      }
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 4);
      if (s == 0 && f < F) part[((long)blockIdx.x * n + r0 + r) * F + f] = acc;
    }
  }
}

// Workgroup (row, block of 256 columns): z = sum of the row's trunk records + bias (four interleaved chains, then a
// tree), h = tanh(LayerNorm(z)) (eps 1e-5, affine), p1[row][j] = relu(h . w1[j] + b1[j]) for the block's columns j.
__global__ __launch_bounds__(256) void act_ln_l1_kernel(const float* __restrict__ part, const float* __restrict__ tb,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        float* __restrict__ p1, int n, int F, int H) {
  __shared__ float s_red[4][256];
  __shared__ float s_h[256];
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  const int row = blockIdx.x;
  for (int f = lane; f < F; f += 64) {
    float acc = 0.f;
#pragma unroll 8
    for (int s = grp; s < kChunks; s += 4) acc += part[((long)s * n + row) * F + f];
    s_red[grp][f] = acc;
  }
  __syncthreads();
  if (grp == 0) {
    float v[4];
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = lane + 64 * q;
      v[q] = f < F ? ((s_red[0][f] + s_red[1][f]) + (s_red[2][f] + s_red[3][f])) + tb[f] : 0.f;
      sum += v[q];
    }
    const float mean = act_wave_sum(sum) / (float)F;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = lane + 64 * q < F ? v[q] - mean : 0.f;
      ss += d * d;
    }
    const float rstd = 1.0f / sqrtf(act_wave_sum(ss) / (float)F + 1e-5f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = lane + 64 * q;
      if (f < F) s_h[f] = tanhf((v[q] - mean) * rstd * gamma[f] + beta[f]);
    }
  }
  __syncthreads();
  const int j = blockIdx.y * 256 + tid;
  if (j >= H) return;
  const float* wr = w1 + (long)j * F;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int f = 0;
  for (; f + 4 <= F; f += 4) {
    a0 = fmaf(s_h[f], wr[f], a0);
    a1 = fmaf(s_h[f + 1], wr[f + 1], a1);
    a2 = fmaf(s_h[f + 2], wr[f + 2], a2);
    a3 = fmaf(s_h[f + 3], wr[f + 3], a3);
  }
  for (; f < F; ++f) a0 = fmaf(s_h[f], wr[f], a0);
  p1[(long)row * H + j] = fmaxf(((a0 + a1) + (a2 + a3)) + b1[j], 0.f);
}

// y[r][j] = x[r] . w[j] + b[j] for up to 16 rows, one WAVE per output column j (the lanes split the reduction, a six-step
// tree joins them), so that N columns spread over N/4 workgroups and every weight row is read by one wave.
// FINAL = false: ReLU (the hidden layer).  FINAL = true (the output layer): mu = tanh(y); action = mu, or with a noise
// tensor clamp(mu + noise*std, +-(1 - 1e-6)): TruncatedNormal.sample(clip=None).
template <bool FINAL>
__global__ __launch_bounds__(256) void act_dense_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ y, int n,
                                                        int K, int N, const float* __restrict__ noise, float std,
                                                        float* __restrict__ mu_out) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= N) return;                       // whole waves leave; the kernel has no barrier
  const int r0 = blockIdx.y * kTrunkRows, r1 = min(n, r0 + kTrunkRows);
  const float* wr = w + (long)j * K;
  const float bias = b[j];
  for (int r = r0; r < r1; r += 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xr[u] = x + (long)min(r + u, r1 - 1) * K;
    if ((K & 3) == 0) {
      for (int k = lane * 4; k < K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xr[u] + k);
          acc[u] = fmaf(wv.x, xv.x, acc[u]);
          acc[u] = fmaf(wv.y, xv.y, acc[u]);
          acc[u] = fmaf(wv.z, xv.z, acc[u]);
          acc[u] = fmaf(wv.w, xv.w, acc[u]);
        }
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        const float wv = wr[k];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fmaf(wv, xr[u][k], acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = act_wave_sum(acc[u]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (r + u >= r1) break;
        const long o = (long)(r + u) * N + j;
        const float v = acc[u] + bias;
        if (!FINAL) {
          y[o] = fmaxf(v, 0.f);
        } else {
          const float mu = tanhf(v);
          if (mu_out) mu_out[o] = mu;
          const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
          y[o] = noise ? fminf(fmaxf(mu + noise[o] * std, lo), hi) : mu;
        }
      }
    }
  }
}

inline long al64(long x) { return (x + 63) & ~63L; }

struct ActWs {
  long act2, feat, part, p1, p2, total;   // offsets in floats
};
ActWs act_ws_layout(int n, int F, int H) {
  ActWs w{};
  long off = 0;
  auto take = [&](long cnt) {
    const long o = off;
    off = al64(off + cnt);
    return o;
  };
  w.act2 = take((long)n * 32 * 39 * 39);
  w.feat = take((long)n * kR);
  w.part = take((long)kChunks * n * F);
  w.p1 = take((long)n * H);
  w.p2 = take((long)n * H);
  w.total = off;
  return w;
}

}  // namespace

bool drq_act_batch_supported(int n, int C, int A, int F, int H) {
  return C == 9 && n >= 1 && n <= kActMaxRows && A >= 1 && F >= 1 && F <= 256 && H >= 1;
}

long drq_act_batch_ws_floats(int n, int F, int H) { return act_ws_layout(n, F, H).total; }

int drq_act_batch_launch(const ActWeights& p, int A, int F, int H, const uint8_t* obs, int n, const float* noise,
                         float std, float* mu_out, float* action_out, float* ws, hipStream_t st) {
  const ActWs W = act_ws_layout(n, F, H);
  float *act2 = ws + W.act2, *feat = ws + W.feat, *part = ws + W.part, *p1 = ws + W.p1, *p2 = ws + W.p2;
  const int rb = (n + kTrunkRows - 1) / kTrunkRows;
  hipLaunchKernelGGL((act_conv_pair_kernel<9, 2, 84, true>), dim3(7 * 7, n), dim3(kConvThreads), 0, st, obs, p.enc_w[0],
                     p.enc_b[0], p.enc_w[1], p.enc_b[1], act2);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL((act_conv_pair_kernel<32, 1, 39, false>), dim3(6 * 6, n), dim3(kConvThreads), 0, st, act2, p.enc_w[2],
                     p.enc_b[2], p.enc_w[3], p.enc_b[3], feat);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(act_trunk_partial_kernel, dim3(kChunks, rb), dim3(256), 0, st, feat, p.trunk_w, part, n, F);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(act_ln_l1_kernel, dim3(n, (H + 255) / 256), dim3(256), 0, st, part, p.trunk_b, p.ln_g, p.ln_b,
                     p.w[0], p.b[0], p1, n, F, H);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(act_dense_kernel<false>, dim3((H + 3) / 4, rb), dim3(256), 0, st, p1, p.w[1], p.b[1], p2, n, H, H,
                     nullptr, 0.f, nullptr);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(act_dense_kernel<true>, dim3((A + 3) / 4, rb), dim3(256), 0, st, p2, p.w[2], p.b[2], action_out, n,
                     H, A, noise, std, mu_out);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
