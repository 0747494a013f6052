// The convolution family's host arithmetic as pure functions: the grid of every launch, the partial records a weight
// gradient leaves, its refusals and the workspace it needs.  Every grid cap and threshold of conv.hip, conv_wino.hip,
// conv_wino_wgrad.hip, conv_bf16.hip and conv1aug.hip is here and nowhere else.  Plain C++17, no HIP, no device query,
// no globals (the CU count is a parameter): tests/conv_plan_dump.cpp compiles this header alone.
#pragma once
#include <cstddef>

// Encoder geometry (drqv2.py:55-59): 84 -(k3,s2)-> 41 -> 39 -> 37 -> 35, 32 channels.
constexpr int kEncH[5] = {84, 41, 39, 37, 35};
constexpr int kConvOk = 0, kConvEarg = -1, kConvEws = -2;   // DRQ_OK, DRQ_EARG, DRQ_EWS (internal.h holds them equal)

// A strided view of [nb][32][h][h] fp32 data: element (b, c, y, x) at off + b*bs + c*cs + y*rs + x
struct ConvView {
  long bs, cs, rs, off;
  static constexpr ConvView contiguous(int h) { return {32L * h * h, (long)h * h, h, 0}; }
  // the interior of a buffer zero-padded by 2, as the update stores its gradients
  static constexpr ConvView padded(int h) { return {32L * (h + 4) * (h + 4), (long)(h + 4) * (h + 4), h + 4, 2L * (h + 4) + 2}; }
};
// the kernels address operands through 32-bit buffer offsets: nb frames of `frame` elements stay below 2 GiB
inline bool conv_bytes_ok(size_t nb, size_t frame, size_t elem_bytes = 4) { return nb * frame * elem_bytes < (1ull << 31); }
inline unsigned conv_bytes(size_t nb, size_t frame, size_t elem_bytes = 4) { return (unsigned)(nb * frame * elem_bytes); }
inline bool view_ok(int nb, const ConvView& v) { return v.off >= 0 && v.bs > 0 && conv_bytes_ok(nb, v.bs); }

// floats per partial record of a weight gradient: [taps or kernel rows][16 registers][64 lanes], then 64 bias pieces
constexpr int conv_part(bool small) { return (small ? 3 : 9) * 1024 + 64; }

// geometry the planners share with the kernels
constexpr int kConvBlk = 2, kConvTpw = 1;          // direct kernel: workgroups per CU it is tuned for, tiles per wave
constexpr int kConv1Bands = 5, kConv1MaxU = 64;    // fused aug+conv1: bands of output rows per frame, units per workgroup
constexpr int conv_bf_wgs(int lay) { return (lay & 1) ? 3 : 2; }                    // bf16 kernel: workgroups per CU
constexpr int conv_bf_npart(int lay, int hin) { return conv_bf_wgs(lay) == 3 && hin >= 43 ? 4 : 3; }   // parts per sample
constexpr bool conv_hin32_ok(int hin) { return hin == 41 || hin == 39 || hin == 37; }   // the 32->32 layers' inputs

struct ConvPlan {
  int rc = kConvOk;             // kConvEarg / kConvEws: the entry refuses with it
  int grid = 0, grid_y = 1;     // workgroups (riders included)
  int records[3] = {0, 0, 0};   // partial records left per layer
  int beg[4] = {0, 0, 0, 0};    // three-layer weight gradient: layer l owns workgroups [beg[l], beg[l + 1])
  bool merged = true;           // three-layer weight gradient: false = too small, the layers launch one by one
  bool small = false;           // direct weight gradient: conv1's form (columns = (cin, kx), two workgroups per CU)
  size_t ws_bytes = 0;          // workspace the launch needs (per layer)
};
inline ConvPlan conv_refuse(int rc) { ConvPlan p; p.rc = rc; p.merged = false; return p; }
inline int conv_grid(long want, long cap) { if (want > cap) want = cap; return (int)(want < 1 ? 1 : want); }
// room for n records per layer in `have` bytes, else DRQ_EWS
inline ConvPlan& conv_ws(ConvPlan& p, long n, size_t have) {
  p.ws_bytes = (size_t)n * conv_part(p.small) * sizeof(float);
  if (p.ws_bytes > have) p.rc = kConvEws;
  return p;
}

// conv3x3_kernel (direct forward / input gradient): 8 waves x kConvTpw tiles of 32 pixels per workgroup and round
inline ConvPlan plan_conv_direct(int cus, int nb, int hin, int stride) {
  ConvPlan p;
  const int hout = (hin - 3) / stride + 1;
  const long ntiles = ((long)nb * hout * hout + 31) / 32;
  p.grid = conv_grid((ntiles + 8 * kConvTpw - 1) / (8 * kConvTpw), (long)kConvBlk * cus);
  return p;
}

// conv3x3_wgrad_kernel (conv1) / conv3x3_wgrad3_kernel (32->32): a wave takes runs of (sample, output row) units
inline ConvPlan plan_wgrad_direct(int cus, int nb, int cin, int hin, int stride, size_t part_bytes) {
  if (!(cin == 9 && hin == 84 && stride == 2) && !(cin == 32 && stride == 1 && conv_hin32_ok(hin))) return conv_refuse(kConvEarg);
  ConvPlan p;
  // conv1 (small): 63 MFMAs per output row against 38 staging loads + LDS writes that the wave cannot overlap with
  // its own MFMAs; its tile is 15 KB per wave and it needs 180 VGPRs, so two workgroups share a CU and one's staging
  // runs under the other's MFMAs
  p.small = cin * 3 <= 32;
  const int hout = (hin - 3) / stride + 1;
  p.grid = p.records[0] = conv_grid(((long)nb * hout + 3) / 4, (p.small ? 2L : 1L) * cus);
  return conv_ws(p, p.grid, part_bytes);
}

// conv3x3_wino_kernel (Winograd forward / input gradient): a wave takes units of 16 2x2 tiles, two workgroups per CU
inline long wino_units(int nb, int hin) { return ((long)nb * ((hin - 1) / 2) * ((hin - 1) / 2) + 15) / 16; }
// budget: workgroup slots the launch may hold, 0 = all of them (two per CU: every caller but the overlapped update's
// input gradients, which leave the rest to the launches of a second stream).  A budget counts in sixteens -- the grids
// the kernel's XCD-aware order takes (wino_deal) -- and never enlarges a grid.
inline ConvPlan plan_wino(int cus, int nb, int hin, int budget = 0) {
  ConvPlan p;
  long cap = 2L * cus;
  if (budget > 0 && budget < cap) cap = budget < 16 ? 16 : budget & ~15;
  p.grid = conv_grid((wino_units(nb, hin) + 3) / 4, cap);
  return p;
}
// slots the three input gradients of the overlapped update hold on a chip of `cus` CUs (DESIGN.md section 3, round 4:
// chosen by the sweep of profiles/overlap_budget_sweep.txt); the budget is given in 512ths of the chip
constexpr int kWinoOverlapBudget512 = 224;
inline int wino_overlap_budget(int cus, int budget512 = kWinoOverlapBudget512) {
  return (int)(2L * cus * budget512 / 512);
}

// What wave `wid` of workgroup `block` does in a conv3x3_wino_kernel launch of `grid` workgroups over nunit units; the
// kernel and the host walk of the tests decode the same function.  Units are dealt round-robin: wave gw takes units
// gw, gw + nwave, ... of the first q rounds.  The r = nunit - q*nwave units left over are cut in HALF-units (16 tiles
// x one half of the output channels) wherever that lowers the busiest wave's load: with 2r <= nwave every left-over
// unit goes to two neighbouring waves as two halves; with 2r > nwave the first nf = 2r - nwave waves take a whole
// unit, every other wave a half.  Workgroup -> position in a round, XCD-aware (grids in sixteens): on each half of the
// grid every XCD (block & 7) takes a contiguous eighth of the half's positions.  The map is a bijection of [0, grid)
// for every such grid, so each unit and half-unit has exactly one owner whatever the grid; only the speed reasoning
// (blocks b and b + grid/2 share a CU) is exact at grid = two per CU alone.
#ifdef __HIPCC__
#define CONV_PLAN_HD __host__ __device__
#else
#define CONV_PLAN_HD
#endif
struct WinoDeal {
  int gw, nwave;        // this wave's position in a round, waves per round
  int nfull;            // whole units: gw + i*nwave, i < nfull
  bool has_half;        // ... then one half-unit:
  int half_unit, half_h;   // its unit, its half of the output channels
};
CONV_PLAN_HD inline WinoDeal wino_deal(int grid, int block, int wid, int nunit) {
  WinoDeal d;
  const int hg = grid >> 1;
  const int bh = block >= hg ? 1 : 0, bl = block - bh * hg;
  const int lb = (grid & 15) ? block : bh * hg + (bl & 7) * (hg >> 3) + (bl >> 3);
  d.gw = lb * 4 + wid;
  d.nwave = grid * 4;
  const int q = nunit / d.nwave, r = nunit - q * d.nwave;
  const int nf = 2 * r > d.nwave ? 2 * r - d.nwave : 0;
  d.nfull = q + (d.gw < nf ? 1 : 0);
  const int hk = d.gw - nf;                                   // index among the half-units
  d.has_half = hk >= 0 && hk < 2 * (r - nf);
  d.half_unit = q * d.nwave + nf + (hk >> 1);
  d.half_h = hk & 1;
  return d;
}

// steps of four 2x2 tiles of the Winograd weight gradient
inline long conv_ww_steps(int nb, int hin) { return ((long)nb * ((hin - 1) / 2) * ((hin - 1) / 2) + 3) / 4; }

// conv3x3_wgrad_wino_kernel (one 32->32 layer): one workgroup per CU, none without a step
inline ConvPlan plan_ww(int cus, int nb, int hin, const ConvView& dy, size_t part_bytes) {
  // The kernel reads row and column `hout` of every dy plane as the empty half of the last 2x2 tile: dy must be the
  // interior of a zero-padded buffer (one more zero row and column at least), as the update stores its gradients.  A
  // contiguous [nb][32][hout][hout] dy would silently wrap into the next row / plane: refused.
  const int hout = hin - 2;
  if (dy.rs < hout + 1 || dy.cs < (long)(hout + 1) * dy.rs) return conv_refuse(kConvEarg);
  ConvPlan p;
  p.grid = p.records[0] = conv_grid((conv_ww_steps(nb, hin) + 3) / 4, cus);
  return conv_ws(p, cus, part_bytes);   // room for one record per CU, whatever the grid
}

// conv3x3_wgrad_wino3_kernel: conv2, conv3, conv4 (hin 41, 39, 37) share one grid
inline ConvPlan plan_ww3(int cus, int nb, size_t part_bytes) {
  long steps[3], tot = 0;
  for (int l = 0; l < 3; ++l) tot += steps[l] = conv_ww_steps(nb, kEncH[l + 1]);
  if (cus < 3 || tot < 3L * 4) return conv_refuse(kConvEarg);   // tiny problems: the caller launches the layers one by one
  ConvPlan p;
  // workgroups per layer proportional to its steps (at least one each), all of them resident at once
  int used = 0;
  for (int l = 0; l < 3; ++l) {
    long n = (steps[l] * cus + tot / 2) / tot;
    if (n < 1) n = 1;
    if (n * 4 > steps[l]) n = (steps[l] + 3) / 4;
    used += p.records[l] = (int)n;
  }
  while (used > cus) {                                          // rounding overshoot: take from the largest share
    int m = 0;
    for (int l = 1; l < 3; ++l) if (p.records[l] > p.records[m]) m = l;
    --p.records[m]; --used;
  }
  int most = 0;
  for (int l = 0; l < 3; ++l) {
    p.beg[l + 1] = p.beg[l] + p.records[l];
    if (p.records[l] > most) most = p.records[l];
  }
  p.grid = p.beg[3];
  return conv_ws(p, most, part_bytes);
}

// conv3x3_bf16_kernel (bf16 forward / input gradient): a workgroup takes (sample, part of the output rows) units
inline ConvPlan plan_conv_bf16(int cus, int nb, int hin, int lay) {
  ConvPlan p;
  p.grid = conv_grid((long)nb * conv_bf_npart(lay, hin), (long)conv_bf_wgs(lay) * cus);
  return p;
}

// conv3x3_wgrad_bf16_kernel: one workgroup per CU, none without a (sample, output row) unit
inline ConvPlan plan_wgrad_bf16(int cus, int nb, int hin, size_t part_bytes) {
  if (!conv_hin32_ok(hin)) return conv_refuse(kConvEarg);
  ConvPlan p;
  p.grid = p.records[0] = conv_grid(((long)nb * (hin - 2) + 3) / 4, cus);
  return conv_ws(p, p.grid, part_bytes);
}

// conv1_aug_kernel: both views' (frame, band) units over two workgroups per CU; `riders` workgroups lead the grid
inline ConvPlan plan_conv1_aug(int cus, int n, int riders) {
  ConvPlan p;
  const long units = 2L * n * kConv1Bands;
  long blocks = units < 2L * cus ? units : 2L * cus;
  if (blocks * kConv1MaxU < units) blocks = (units + kConv1MaxU - 1) / kConv1MaxU;   // a workgroup's shift table holds kConv1MaxU units
  p.grid = (int)blocks + riders;
  return p;
}

// conv3x3_wgrad_reduce_multi_kernel: 64 record elements per workgroup, the largest record by the jobs
inline ConvPlan plan_reduce(int n, const int* cin) {
  ConvPlan p;
  for (int i = 0; i < n; ++i)
    if (conv_part(cin[i] * 3 <= 32) / 64 > p.grid) p.grid = conv_part(cin[i] * 3 <= 32) / 64;
  p.grid_y = n;
  return p;
}
