// The GEMM family's selection as a pure function: which kernel variant a call gets and the numbers its launch needs.
// Every eligibility rule and threshold of gemm.hip, gemm2.hip, gemm3.hip and skinny.hip is here and nowhere else.
// Plain C++17, no HIP, no device query, no globals: tests/gemm_plan_dump.cpp compiles this header alone.
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int kGemmMaxBatch = 8;   // problems per launch (same shape, independent pointers)

// What selection depends on.  A(m,k) = a_kc ? A[m*lda + k] : A[k*lda + m], B(k,n) = b_kc ? B[n*ldb + k] : B[k*ldb + n].
struct GemmShape {
  bool a_kc = true, b_kc = true;
  int nbatch = 1, M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0, ldc = 0;
  int ldaux = 0, scatter_hw = 0, tile = 0, splitk = 0;   // tile, splitk: the caller's requests, 0 = choose
  bool relu = false, bf16 = false;
  bool ring = false;                   // requested route: the ring kernel where it takes the shape (step.hip's policy)
  // derived from the call's pointers
  bool a_al16 = true, b_al16 = true;   // every A / B pointer is 16-byte aligned
  bool ws_al16 = false;                // there is a workspace and it is 16-byte aligned
  size_t ws_bytes = 0;
  bool bias = false, aux = false, rowsum = false;
  bool q_unpaired = false;             // ring forward: some problem has qw without qpart or the reverse
  int cus = 256;
};

// name = the one of tests/gemm_variants.py where it models the variant; NONE: no kernel takes this, the entry refuses
// (DRQ_EARG); EWS: the workspace is too small for the split-K records (DRQ_EWS); LDS, BF16, PAIR2: GemmPlan says which
#define GEMM_VARIANTS(X)                                                                                              \
  X(NONE, "EARG") X(EWS, "EWS") X(G3_FWD_64x64, "g3_fwd_64x64") X(G3_FWD_64x32, "g3_fwd_64x32")                       \
  X(G3_DGRAD_64x64, "g3_dgrad_64x64") X(G3_DGRAD_64x32, "g3_dgrad_64x32") X(G3_PAIR_D64, "g3_pair_d64")               \
  X(G3_PAIR_D32, "g3_pair_d32") X(G2_KS1, "g2_ks1") X(G2_KS4, "g2_ks4") X(SKINNY_DGRAD, "skinny_dgrad")               \
  X(TRUNK_WGRAD_4, "trunk_wgrad_4") X(TRUNK_WGRAD_8, "trunk_wgrad_8") X(TRUNK_WGRAD_16, "trunk_wgrad_16")             \
  X(TRUNK_FWD_TM1, "trunk_fwd_tm1") X(TRUNK_FWD_TM2, "trunk_fwd_tm2") X(TRUNK_FWD_WIDE, "trunk_fwd_wide")             \
  X(LDS, "lds") X(BF16, "bf16") X(PAIR2, "pair2")
#define GEMM_VARIANT_ENUM(id, name) GV_##id,
enum GemmVariant { GEMM_VARIANTS(GEMM_VARIANT_ENUM) };

struct GemmPlan {
  GemmVariant variant = GV_NONE;
  int splitk = 0, kchunk = 0;   // records per problem (0: the variant has no split count) and k per record
  int nq = 0, rows = 0;         // ring forward: partial-dot columns per row;  trunk forward: grid y (grid x = splitk)
  int tile = 0;                 // LDS: block tile 32x32 (1), 64x64 (2), 64x32 (3), 32x64 (4), 1 / 2 with a k-tile of 64 (5 / 6)
  bool v4 = false;              // LDS, BF16: 16-byte loads along k
  bool full = false;            // LDS: the variant without range masks;  BF16: the 128-column tile
  bool split_w = false, split_d = false;   // PAIR2: K split over the waves in the weight / input gradient half
  bool colsum_first = false;    // BF16 weight gradient: the bias gradient runs as its own drq_colsum pass first
};

inline const char* variant_name(const GemmPlan& p) {
#define GEMM_VARIANT_NAME(id, name) name,
  static const char* const names[] = {GEMM_VARIANTS(GEMM_VARIANT_NAME)};
  static const char* const lds[] = {"lds_tile1_v4_full", "lds_tile1_v4", "lds_tile1_scalar", "lds_tile2_v4",
                                    "lds_tile2_scalar",  "lds_tile3_v4", "lds_tile3_scalar", "lds_tile4_v4",
                                    "lds_tile4_scalar",  "lds_tile5_v4", "lds_tile5_scalar", "lds_tile6_v4",
                                    "lds_tile6_scalar"};
  return p.variant != GV_LDS ? names[p.variant] : lds[p.full ? 0 : 2 * p.tile - (p.v4 ? 1 : 0)];
}

inline GemmPlan& pick(GemmPlan& p, GemmVariant v) { p.variant = v; return p; }

// the kernels address operands through 32-bit buffer offsets: a [rows][ld] fp32 operand stays below 2 GiB
inline bool operand_bytes_ok(long rows, long ld) { return (size_t)rows * (size_t)ld * 4 < (1ull << 31); }
inline bool operand_bytes_ok(const GemmShape& s) {
  return operand_bytes_ok(s.a_kc ? s.M : s.K, s.lda) && operand_bytes_ok(s.b_kc ? s.N : s.K, s.ldb);
}
inline bool batch_ok(const GemmShape& s) { return s.nbatch > 0 && s.nbatch <= kGemmMaxBatch; }

// Split-K of the LDS-staged kernels in either precision: with no request, split when `tiles` output tiles leave the
// chip under-filled and K >= kmin, keeping kper of k (four k-tiles) per record.  False: the records do not fit ws.
inline bool plan_splitk(const GemmShape& s, int request, long tiles, int kmin, int kper, GemmPlan& p) {
  int sk = request;
  if (sk == 0) {
    sk = 1;
    if (tiles < 2L * s.cus && s.K >= kmin) {
      sk = (int)((3L * s.cus + tiles - 1) / tiles);
      if (sk > s.K / kper) sk = s.K / kper;
      if (sk < 1) sk = 1;
    }
  }
  p.kchunk = ((s.K + sk - 1) / sk + 63) / 64 * 64;
  p.splitk = (s.K + p.kchunk - 1) / p.kchunk;
  return p.splitk == 1 || (size_t)s.nbatch * p.splitk * s.M * s.N * sizeof(float) <= s.ws_bytes;
}

// gemm2.hip: split K over the four waves of a workgroup when the 32x32 tiles alone leave the chip under-filled
inline bool gemm2_split(const GemmShape& s) {
  return (long)(s.M / 32) * (s.N / 32) * s.nbatch < 4L * s.cus * 2 && s.K % 128 == 0 && s.K >= 512;
}

enum RingForm { RING_FWD, RING_DGRAD, RING_PAIR };

// one problem set of the ring kernel (gemm3.hip): whole 64-row / 32-column / 32-k tiles, 16-byte copies
inline bool ring_ok(const GemmShape& s) {
  return batch_ok(s) && s.M % 64 == 0 && s.N % 32 == 0 && s.K % 32 == 0 && s.M >= 64 && s.N >= 32 && s.K >= 64 &&
         s.lda % 4 == 0 && s.ldb % 4 == 0 && operand_bytes_ok(s) && s.a_al16 && s.b_al16;
}

// drq_mlp_fwd / drq_mlp_dgrad (and step.hip's ring route) / drq_mlp_wgrad_dgrad.  RING_PAIR: `s` is the input-gradient
// half (M = rows, N = Kin, K = Nout) and `w` the weight-gradient half (M = Nout, N = Kin, K = rows).
inline GemmPlan plan_ring(RingForm form, const GemmShape& s, const GemmShape* w = nullptr) {
  GemmPlan p;
  if (!ring_ok(s) || s.N % 64 || s.rowsum || s.scatter_hw || s.tile || s.splitk) return p;
  if (form == RING_PAIR) {
    if (!w || !ring_ok(*w) || s.K % 64) return p;
  } else if (form != (s.b_kc ? RING_FWD : RING_DGRAD) || !s.a_kc || s.q_unpaired) {
    return p;
  }
  // enough 64x64 tiles to give every CU one: one sub-tile per wave; else 64x32 tiles with the k-steps of a k-tile
  // split over two wave groups (twice the workgroups, half the MFMAs per wave).  The pair counts its input-gradient half
  const bool big = (long)(s.M / 64) * (s.N / 64) * s.nbatch >= s.cus;
  if (form == RING_FWD) p.nq = big ? s.N / 64 : s.N / 32;
  return pick(p, form == RING_FWD     ? (big ? GV_G3_FWD_64x64 : GV_G3_FWD_64x32)
                 : form == RING_DGRAD ? (big ? GV_G3_DGRAD_64x64 : GV_G3_DGRAD_64x32)
                                      : (big ? GV_G3_PAIR_D64 : GV_G3_PAIR_D32));
}

// drq_gemm2_wgrad_dgrad: the two gradients of one hidden layer on the LDS-free kernel, halves as for RING_PAIR
inline GemmPlan plan_pair2(const GemmShape& w, const GemmShape& d) {
  GemmPlan p;
  if (!batch_ok(d) || d.M % 32 || d.K % 32 || d.N % 32 || d.M < 64 || d.K < 64 || d.N < 32) return p;
  if (d.lda % 4 || !d.a_al16 || !operand_bytes_ok(w) || !operand_bytes_ok(d)) return p;
  p.split_w = gemm2_split(w);
  p.split_d = gemm2_split(d);
  return pick(p, GV_PAIR2);
}

// drq_gemm_batched_bf16 and the bf16 update: gemm_bf16_kernel for every shape
inline GemmPlan plan_bf16(const GemmShape& s) {
  GemmPlan p;
  if (!s.a_kc && s.b_kc) return p;
  const long tiles = (long)((s.M + 63) / 64) * ((s.N + 63) / 64) * s.nbatch;
  // a weight-gradient GEMM with few output tiles (the first layers: N = feature_dim (+ action_dim)) needs split-K to
  // fill the chip, and the fused bias gradient cannot be split: it gets its own pass (column sums of dy)
  p.colsum_first = s.rowsum && s.splitk == 0 && tiles < 2L * s.cus && s.K >= 512;
  if (!plan_splitk(s, s.rowsum && !p.colsum_first ? 1 : s.splitk, tiles, 512, 256, p)) return pick(p, GV_EWS);
  p.v4 = s.lda % 4 == 0 && s.ldb % 4 == 0 && s.a_al16 && s.b_al16;
  p.full = s.N > 64 && s.N <= 128 && s.K >= 4096;   // the trunk layer at feature_dim 100 (gemm_bf16_kernel, TN = 2)
  return pick(p, GV_BF16);
}

// drq_gemm_batched_f32 / drq_gemm_f32 / drq_gemm_batched_bf16 and the update's layers
inline GemmPlan plan_batched(const GemmShape& s) {
  GemmPlan p;
  if (s.M <= 0 || s.N <= 0 || s.K <= 0 || !batch_ok(s) || (s.rowsum && s.a_kc)) return p;
  if (s.bf16) return plan_bf16(s);
  if (s.ring && (p = plan_ring(RING_DGRAD, s)).variant != GV_NONE) return p;
  // an explicit tile / splitk request keeps the generic path (tests compare the two)
  const bool plain = s.nbatch == 1 && s.tile == 0 && s.splitk == 0 && !s.bias && !s.relu;
  // the skinny dgrad shape of the trunk layer (K = feature_dim, N = 39200)
  if (plain && s.a_kc && !s.b_kc && !s.rowsum && s.N >= 4096 && s.N % 32 == 0 && s.K <= 128 &&
      operand_bytes_ok(s.M, s.scatter_hw > 0 ? 32L * (s.scatter_hw + 4) * (s.scatter_hw + 4) : s.ldc) &&
      (!s.aux || operand_bytes_ok(s.M, s.ldaux)))
    return pick(p, GV_SKINNY_DGRAD);
  // the trunk layer's weight gradient (M = feature_dim, N = 39200, K = batch: dz^T stays in registers, K/32 steps)
  if (plain && !s.a_kc && !s.b_kc && !s.aux && s.scatter_hw == 0 && s.M <= 128 && s.N >= 4096 && s.N % 32 == 0 &&
      (s.K == 128 || s.K == 256 || s.K == 512) && operand_bytes_ok(s))
    return pick(p, s.K == 128 ? GV_TRUNK_WGRAD_4 : s.K == 256 ? GV_TRUNK_WGRAD_8 : GV_TRUNK_WGRAD_16);
  // hidden x hidden layers at multiple-of-32 shapes with a row-contiguous B: the LDS-free kernel (gemm2.hip).  In the
  // forward form every 16-byte lane load touches its own cache line and the LDS-staged kernel is faster
  if (s.tile == 0 && s.splitk == 0 && s.scatter_hw == 0 && !s.b_kc && s.M % 32 == 0 && s.N % 32 == 0 && s.K % 32 == 0 &&
      s.K >= 64 && s.M >= 32 && s.N >= 32 && operand_bytes_ok(s) && (!s.a_kc || (s.lda % 4 == 0 && s.a_al16)))
    return pick(p, gemm2_split(s) ? GV_G2_KS4 : GV_G2_KS1);
  // the LDS-staged kernel (block tiles: GemmPlan::tile)
  const long t_big = (long)((s.M + 63) / 64) * ((s.N + 63) / 64) * s.nbatch;
  const long t_small = (long)((s.M + 31) / 32) * ((s.N + 31) / 32) * s.nbatch;
  p.tile = s.tile == 0 ? (t_big >= 2L * s.cus ? 2 : 1) : s.tile;
  const long tiles = p.tile == 2 ? t_big : (p.tile >= 3 ? (t_big + t_small) / 2 : t_small);
  if (p.tile < 2 || p.tile > 6) p.tile = 1;
  if (!plan_splitk(s, s.rowsum ? 1 : s.splitk, tiles, 256, 128, p)) return pick(p, GV_EWS);
  if (!s.a_kc && s.b_kc) return p;
  // float4 loads along k for the k-contiguous operands (two row-contiguous operands: the scalar loaders)
  p.v4 = s.K % 4 == 0 && (s.a_kc || s.b_kc) && (!s.a_kc || (s.lda % 4 == 0 && s.a_al16)) &&
         (!s.b_kc || (s.ldb % 4 == 0 && s.b_al16));
  // the forward form of the hidden layers (all dimensions multiples of the tiles)
  p.full = p.tile == 1 && p.v4 && s.a_kc && s.b_kc && s.M % 32 == 0 && s.N % 32 == 0 && s.K % 32 == 0;
  return pick(p, GV_LDS);
}

// drq_gemm_batched_partial and the update's trunk: the forward form with the split-K sum left to the caller
inline GemmPlan plan_partial(const GemmShape& s) {
  GemmPlan p;
  // the fp32 trunk forward (k-contiguous operands, N <= 128, long K; gemm2.hip) writes records only
  if (!s.bf16 && s.a_kc && s.b_kc && s.N <= 128 && s.K >= 4096 && s.ldc == s.N && batch_ok(s) && s.M % 32 == 0 &&
      s.M >= 32 && s.N >= 1 && s.K % 32 == 0 && s.lda % 4 == 0 && s.ldb % 4 == 0 && s.ws_al16 && s.a_al16 && s.b_al16 &&
      operand_bytes_ok(s)) {
    // one workgroup per CU (one wave per SIMD): measured 51 us against 59 us with two and 66 us with four for the
    // four trunks of the critic update
    const int steps = s.K / 32;
    const bool wide = s.N > 64;               // four column tiles per wave, one row tile
    const bool tm2 = !wide && s.M % 64 == 0 && (long)s.nbatch * (s.M / 32) * 4 >= 64;
    p.rows = tm2 ? s.M / 64 : s.M / 32;
    p.splitk = (s.cus + s.nbatch * p.rows - 1) / (s.nbatch * p.rows);
    if (p.splitk * 4 > steps) p.splitk = steps / 4;
    // small batches (one or two row tiles): the consumer (LayerNorm) sums the split-K records row by row, and beyond
    // ~64 records per element that sum costs more than the extra workgroups save here
    if (p.splitk > 64) p.splitk = 64;
    if (p.splitk >= 2) {                      // a split count of 1 means "result in C" to the callers
      const bool fits = (size_t)s.nbatch * p.splitk * s.M * s.N * sizeof(float) <= s.ws_bytes;
      return pick(p, !fits ? GV_EWS : wide ? GV_TRUNK_FWD_WIDE : tm2 ? GV_TRUNK_FWD_TM2 : GV_TRUNK_FWD_TM1);
    }
  }
  GemmShape t = s;
  t.tile = s.bf16 ? 0 : 1;
  t.splitk = 0;
  return plan_batched(t);
}
