// Weight gradient of the encoder's 32->32 layers in Winograd F(2x2,3x3) form on the f32 matrix cores.
//
// Reference op: the autograd weight / bias gradient of nn.Conv2d(32,32,3,1) (drqv2.py:56-58).  With
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A   per 2x2 output tile (conv_wino.hip),
// the gradient of the loss with respect to g is
//   dg = G^T [ sum over samples and tiles of (A dY A^T) .* (B^T d B) ] G      per (cout, cin):
// 16 positions x a 32x32 (cout x cin) matrix, reduced over all tiles -- 16 tile-GEMMs instead of the direct form's
// 9 pixel-GEMMs over four times as many pixels: 2.25x fewer matrix FLOPs.
//
// Mapping: v_mfma_f32_16x16x4_f32 with K = 4 tiles: D[cout 16][cin 16] += dM[cout][tile] * V[tile][cin].  Lane l holds
// channel l&15 (+16 for the second half) and tile 4s + (l>>4) of step s of a tile row -- in BOTH roles: it loads that
// channel's 2x2 dY patch (A operand, after A dY A^T) and that channel's 4x4 input patch (B operand, after B^T d B)
// straight from global memory (the patches of the four tiles of a step are 40 contiguous bytes of a row: L2 serves the
// re-touched lines).  A wave takes steps of four consecutive tiles round-robin and keeps all 16 positions x 2x2 channel-half quadrants x 4 registers =
// 256 accumulators (one wave per SIMD: the unified register file holds them as AGPRs).  At the end every wave maps its
// sums back to 3x3 taps (G^T . G), the four waves of a workgroup are added through LDS in wave order and the workgroup
// writes ONE partial record in the format of conv3x3_wgrad3_kernel (conv.hip): the same fixed-order reduction kernel
// finishes the job (deterministic, no float atomics).
#include "common.h"
#include "internal.h"

namespace {

struct WWArgs {
  const float* x;     // layer input  [NB][32][HIN][HIN]
  const float* dy;    // grad of the pre-activation, zero-padded by 2, addressed with strides; dy_off = element (0,0)
  int dy_bs, dy_cs, dy_rs, dy_off;
  float* part;        // [nblocks][9*1024 + 64]
  unsigned x_bytes, dy_bytes;
  int nb;
};

typedef unsigned u32x4q __attribute__((ext_vector_type(4)));
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));

// bx / nblk: the workgroup's index among the nblk workgroups that share this layer (a launch of its own: blockIdx.x /
// gridDim.x; the three-layer launch below gives every layer a range of its grid)
template <int HIN>
__device__ __forceinline__ void ww_body(const WWArgs& a, int bx, int nblk) {
#pragma clang fp contract(off)
  constexpr int HOUT = HIN - 2;
  constexpr int TH = (HOUT + 1) / 2;          // tiles per row / tile rows per sample
  constexpr int PLANE = HIN * HIN * 4;        // bytes of one input channel
  constexpr int PART = 9 * 1024 + 64;
  extern __shared__ __attribute__((aligned(16))) float red[];   // [4 waves][PART]
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = lane & 15, tq = lane >> 4;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dy_bytes, 0x00020000);
  constexpr int kDrop = (int)0x80000000u;     // beyond num_records: the load returns 0
  const int dcs4 = a.dy_cs * 4, drs4 = a.dy_rs * 4;

  // work: steps of 4 consecutive tiles of the flattened (sample, tile row, tile column) index, dealt round-robin to
  // the waves of the grid (a step may straddle two tile rows: every lane places its own tile)
  constexpr int TT = TH * TH;
  const int ntile = a.nb * TT;
  const int nstep = (ntile + 3) >> 2;
  const int nw = nblk * 4, gw = bx * 4 + wid;
  const int total = gw < nstep ? (nstep - 1 - gw) / nw + 1 : 0;

  // per-lane byte offsets of this wave's it-th step: the x patch and the dY patch
  auto item_off = [&](int it, int& xo, int& dyo) {
    const int t = 4 * (gw + it * nw) + tq;
    const int tc = t < ntile ? t : ntile - 1;
    const int b = tc / TT, rem = tc - b * TT;
    const int ty = rem / TH, tx = rem - ty * TH;
    xo = (((b * 32 + ch) * HIN + 2 * ty) * HIN + 2 * tx) * 4;
    dyo = t < ntile ? (a.dy_off + b * a.dy_bs + ch * a.dy_cs + 2 * ty * a.dy_rs + 2 * tx) * 4 : kDrop;
  };
  // two register sets of patches: the loads of step it+2 are issued while step it multiplies (one wave per SIMD has
  // nobody else to hide an HBM miss behind: one step = 64 MFMAs = 2048 matrix cycles is not always enough)
  auto load_item = [&](float (&Pdx)[2][16], float (&Pdy)[2][4], int xo, int dyo) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4q v = __builtin_amdgcn_raw_buffer_load_b128(xrs, xo, h * (16 * PLANE) + i * (HIN * 4), 0);
        const unsigned e0 = v[0], e1 = v[1], e2 = v[2], e3 = v[3];
        Pdx[h][i * 4 + 0] = __uint_as_float(e0);
        Pdx[h][i * 4 + 1] = __uint_as_float(e1);
        Pdx[h][i * 4 + 2] = __uint_as_float(e2);
        Pdx[h][i * 4 + 3] = __uint_as_float(e3);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const u32x2q v = __builtin_amdgcn_raw_buffer_load_b64(drs, dyo, h * 16 * dcs4 + i * drs4, 0);
        const unsigned e0 = v[0], e1 = v[1];
        Pdy[h][i * 2 + 0] = __uint_as_float(e0);
        Pdy[h][i * 2 + 1] = __uint_as_float(e1);
      }
    }
  };

  // the k-th of the twelve load instructions of an item: 0..7 = x rows (h = k>>2, i = k&3), 8..11 = dY rows
  auto load_one = [&](float (&Pdx)[2][16], float (&Pdy)[2][4], int xo, int dyo, int k) {
    if (k < 8) {
      const int h = k >> 2, i = k & 3;
      const u32x4q v = __builtin_amdgcn_raw_buffer_load_b128(xrs, xo, h * (16 * PLANE) + i * (HIN * 4), 0);
      const unsigned e0 = v[0], e1 = v[1], e2 = v[2], e3 = v[3];
      Pdx[h][i * 4 + 0] = __uint_as_float(e0);
      Pdx[h][i * 4 + 1] = __uint_as_float(e1);
      Pdx[h][i * 4 + 2] = __uint_as_float(e2);
      Pdx[h][i * 4 + 3] = __uint_as_float(e3);
    } else {
      const int h = (k - 8) >> 1, i = (k - 8) & 1;
      const u32x2q v = __builtin_amdgcn_raw_buffer_load_b64(drs, dyo, h * 16 * dcs4 + i * drs4, 0);
      const unsigned e0 = v[0], e1 = v[1];
      Pdy[h][i * 2 + 0] = __uint_as_float(e0);
      Pdy[h][i * 2 + 1] = __uint_as_float(e1);
    }
  };

  f32x4 acc[16][2][2];                        // [position][cout half][cin half]
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) acc[p][qa][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[2] = {0.f, 0.f};                 // bias gradient: sum of this lane's dY values per channel half

  // one step: transforms of the patches in P, then P is refilled with item `nit`, then the 64 MFMAs
  auto step = [&](float (&Pdx)[2][16], float (&Pdy)[2][4], int nit) {
    int nxo, ndyo;
    item_off(nit < total ? nit : total - 1, nxo, ndyo);
    float V[2][16], M[2][16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // V = B^T d B
      float t[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        t[0 * 4 + j] = Pdx[h][0 * 4 + j] - Pdx[h][2 * 4 + j];
        t[1 * 4 + j] = Pdx[h][1 * 4 + j] + Pdx[h][2 * 4 + j];
        t[2 * 4 + j] = Pdx[h][2 * 4 + j] - Pdx[h][1 * 4 + j];
        t[3 * 4 + j] = Pdx[h][1 * 4 + j] - Pdx[h][3 * 4 + j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        V[h][i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2];
        V[h][i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2];
        V[h][i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1];
        V[h][i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3];
      }
      // dM' = A' dY A'^T with A' = [[1,0],[1,1],[1,-1],[0,1]]: the last row of A = [0,-1] with its sign flipped (no
      // negations here); dM = S dM' S with S = diag(1,1,1,-1), and S moves into the final transform: dg = (SG)^T dU' (SG)
      const float y00 = Pdy[h][0], y01 = Pdy[h][1], y10 = Pdy[h][2], y11 = Pdy[h][3];
      bsum[h] += (y00 + y01) + (y10 + y11);
      const float r[4][2] = {{y00, y01}, {y00 + y10, y01 + y11}, {y00 - y10, y01 - y11}, {y10, y11}};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        M[h][i * 4 + 0] = r[i][0];
        M[h][i * 4 + 1] = r[i][0] + r[i][1];
        M[h][i * 4 + 2] = r[i][0] - r[i][1];
        M[h][i * 4 + 3] = r[i][1];
      }
    }
    // The refill's twelve loads are spread over the step's 64 MFMAs, three ahead of every sixteen: a wave issues in
    // order, so a burst of loads that backs up in the texture addresser's queue would hold its MFMAs too -- and this
    // kernel has one wave per SIMD.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
#pragma unroll
      for (int k = 3 * k4; k < 3 * k4 + 3; ++k) load_one(Pdx, Pdy, nxo, ndyo, k);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 4 * k4; p < 4 * k4 + 4; ++p)
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)
            acc[p][qa][qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(M[qa][p], V[qb][p], acc[p][qa][qb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  float dx0[2][16], dy0[2][4];
  if (total > 0) {
    int xo, dyo;
    item_off(0, xo, dyo);
    load_item(dx0, dy0, xo, dyo);
  }
  for (int it = 0; it < total; ++it) step(dx0, dy0, it + 1);

  // ---- dg = G^T dU G per (cout, cin) -> this wave's image of the partial record in LDS
  // D register r of lane l: cout = 16*qa + 4*(l>>4) + r, cin = 16*qb + (l&15)
  // record element of (cout, cin, tap): tap*1024 + rr*64 + half*32 + cin with cout = (rr&3) + 8*(rr>>2) + 4*half
  float* mine = red + wid * PART;
#pragma unroll
  for (int qa = 0; qa < 2; ++qa)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float u[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) u[i][j] = acc[i * 4 + j][qa][qb][r];
        float tm[3][4];                        // (SG)^T u: G with the sign of its last row flipped (see dM' above)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float hs = 0.5f * (u[1][j] + u[2][j]), hd = 0.5f * (u[1][j] - u[2][j]);
          tm[0][j] = u[0][j] + hs;
          tm[1][j] = hd;
          tm[2][j] = hs - u[3][j];
        }
        const int co = 16 * qa + 4 * tq + r, ci = 16 * qb + ch;
        const int half = (co >> 2) & 1, rr = (co & 3) + 4 * (co >> 3);
        float* dst = mine + rr * 64 + half * 32 + ci;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float hs = 0.5f * (tm[ky][1] + tm[ky][2]), hd = 0.5f * (tm[ky][1] - tm[ky][2]);
          dst[(ky * 3 + 0) * 1024] = tm[ky][0] + hs;
          dst[(ky * 3 + 1) * 1024] = hd;
          dst[(ky * 3 + 2) * 1024] = hs - tm[ky][3];
        }
      }
  // bias: lanes with the same channel (4 tile quarters) are added by the record reduction's two slots and here
  {
    float b0 = bsum[0], b1 = bsum[1];
    b0 += __shfl_xor(b0, 16); b0 += __shfl_xor(b0, 32);
    b1 += __shfl_xor(b1, 16); b1 += __shfl_xor(b1, 32);
    if (lane < 16) {
      mine[9 * 1024 + ch] = b0;
      mine[9 * 1024 + 16 + ch] = b1;
      mine[9 * 1024 + 32 + ch] = 0.f;
      mine[9 * 1024 + 48 + ch] = 0.f;
    }
  }
  __syncthreads();
  float4* out = reinterpret_cast<float4*>(a.part + (long)bx * PART);
  const float4* r4 = reinterpret_cast<const float4*>(red);
  for (int i = threadIdx.x; i < PART / 4; i += 256) {
    const float4 p = r4[i], q = r4[PART / 4 + i], v = r4[2 * (PART / 4) + i], w = r4[3 * (PART / 4) + i];
    out[i] = make_float4((p.x + q.x) + (v.x + w.x), (p.y + q.y) + (v.y + w.y), (p.z + q.z) + (v.z + w.z),
                         (p.w + q.w) + (v.w + w.w));
  }
}

template <int HIN>
__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_wino_kernel(WWArgs a) {
  const int G = (int)gridDim.x;   // XCD-aware order, see conv3x3_wgrad_wino3_kernel
  ww_body<HIN>(a, (G & 7) ? (int)blockIdx.x : ((int)blockIdx.x & 7) * (G >> 3) + ((int)blockIdx.x >> 3), G);
}

// The three 32->32 layers of the encoder backward in ONE launch: layer l owns workgroups [beg[l], beg[l+1]) of the
// grid (shares proportional to its steps), every wave still accumulates one layer only and every workgroup writes one
// record of its layer.  Two launches' worth of cold start, epilogue and tail less than three launches.
struct WW3Args {
  WWArgs l[3];        // HIN = 41, 39, 37 (conv2, conv3, conv4)
  int beg[4];
};
__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_wino3_kernel(WW3Args g) {
  // XCD-aware order (workgroups go to the eight XCDs round-robin by blockIdx; speed only): every XCD takes a contiguous
  // eighth of the grid, so that the workgroups which read neighbouring steps of a round -- 40 of 128 bytes of a line
  // horizontally, two of four input rows vertically -- share an L2 instead of pulling each line through the fabric once
  // per XCD
  const int G = (int)gridDim.x;
  const int b = (G & 7) ? (int)blockIdx.x : ((int)blockIdx.x & 7) * (G >> 3) + ((int)blockIdx.x >> 3);
  if (b < g.beg[1]) ww_body<41>(g.l[0], b, g.beg[1]);
  else if (b < g.beg[2]) ww_body<39>(g.l[1], b - g.beg[1], g.beg[2] - g.beg[1]);
  else ww_body<37>(g.l[2], b - g.beg[2], g.beg[3] - g.beg[2]);
}

constexpr int kWwLds = 4 * conv_part(false) * 4;   // bytes: the four waves' images of a record

template <int HIN>
int launch_ww(const WWArgs& a, const ConvPlan& p, hipStream_t st) {
  if (const int rc = drq_max_dynamic_lds<conv3x3_wgrad_wino_kernel<HIN>>(kWwLds)) return rc;
  hipLaunchKernelGGL((conv3x3_wgrad_wino_kernel<HIN>), dim3((unsigned)p.grid), dim3(256), kWwLds, st, a);
  return drq_launched();
}

// the kernel's arguments for one layer; false: an operand is missing or too large
bool ww_args(WWArgs& a, const float* x, const float* dy, int nb, int hin, const ConvView& v, float* part) {
  const size_t frame = 32 * (size_t)hin * hin;
  if (!x || !dy || !part || !conv_bytes_ok(nb, frame) || !view_ok(nb, v)) return false;
  a = WWArgs{x, dy, (int)v.bs, (int)v.cs, (int)v.rs, (int)v.off, part, conv_bytes(nb, frame), conv_bytes(nb, v.bs), nb};
  return true;
}

}  // namespace

// internal (step.hip): conv2, conv3, conv4 (hin 41, 39, 37) in one launch; x[l], dy[l], part[l] and the dY view per
// layer; nblocks[l] = records written for layer l.  The caller asks plan_ww3 first: a batch it does not merge is refused
int drq_conv3x3_wgrad_partial_wino3(const float* const* x, const float* const* dy, int nb, const ConvView* dyv,
                                    float* const* part, size_t part_bytes, int* nblocks, hipStream_t st) {
  if (!x || !dy || !dyv || !part || !nblocks || nb <= 0) return DRQ_EARG;
  WW3Args g{};
  for (int l = 0; l < 3; ++l)
    if (!ww_args(g.l[l], x[l], dy[l], nb, kEncH[l + 1], dyv[l], part[l]) || ((size_t)part[l] & 15)) return DRQ_EARG;
  const ConvPlan p = plan_ww3(drq_num_cus(), nb, part_bytes);
  if (p.rc) return p.rc;
  for (int l = 0; l < 3; ++l) {
    g.beg[l + 1] = p.beg[l + 1];
    nblocks[l] = p.records[l];
  }
  if (const int rc = drq_max_dynamic_lds<conv3x3_wgrad_wino3_kernel>(kWwLds)) return rc;
  hipLaunchKernelGGL(conv3x3_wgrad_wino3_kernel, dim3((unsigned)p.grid), dim3(256), kWwLds, st, g);
  return drq_launched();
}

// internal (step.hip, conv.hip's public entry): partial records of the 32->32 weight gradient in Winograd form, same
// record format and reduction as drq_conv3x3_wgrad_partial
int drq_conv3x3_wgrad_partial_wino(const float* x, const float* dy, int nb, int hin, ConvView dyv, float* part,
                                   size_t part_bytes, int* nblocks, hipStream_t st) {
  WWArgs a;
  if (!nblocks || nb <= 0 || !ww_args(a, x, dy, nb, hin, dyv, part)) return DRQ_EARG;
  const ConvPlan p = plan_ww(drq_num_cus(), nb, hin, dyv, part_bytes);
  if (p.rc) return p.rc;
  if (((size_t)part & 15) != 0) return DRQ_EARG;
  *nblocks = p.records[0];
  return drq_dispatch<41, 39, 37>(hin, [&](auto h) { return launch_ww<decltype(h)::value>(a, p, st); });
}
