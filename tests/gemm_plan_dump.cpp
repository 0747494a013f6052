// What drqv2_amd/csrc/gemm_plan.h plans, one shape per input line, for tests/test_cpu_gemm_variants.py to hold against
// tests/gemm_variants.py.  Host only: the planner header is all it needs.  A line is
//   kind cus n M N K lda ldb ldc a_al16 b_al16 tile splitk bias relu aux rowsum qw qpart ldx scatter_hw ws_bytes
// with kind fwd / dgrad / wgrad (plan_batched in that layout), partial (plan_partial), mlp_fwd / mlp_dgrad / mlp_pair
// (plan_ring; the pair's M N K lda ldb are those of its input-gradient half, ldx is its weight-gradient half's ldb).
// The workspace is aligned; ws_bytes 0: there is none.  Output: the variant's name, "/s<split>" where it has one, and nq.
#include "../drqv2_amd/csrc/gemm_plan.h"

#include <cstdio>
#include <cstring>

int main() {
  char kind[16];
  int cus, n, M, N, K, a_al, b_al, tile, splitk, bias, relu, aux, rowsum, qw, qpart, scatter_hw;
  long lda, ldb, ldc, ldx, ws_bytes;
  while (std::scanf("%15s %d %d %d %d %d %ld %ld %ld %d %d %d %d %d %d %d %d %d %d %ld %d %ld", kind, &cus, &n, &M, &N, &K, &lda,
                    &ldb, &ldc, &a_al, &b_al, &tile, &splitk, &bias, &relu, &aux, &rowsum, &qw, &qpart, &ldx,
                    &scatter_hw, &ws_bytes) == 22) {
    const bool fwd = !std::strcmp(kind, "fwd") || !std::strcmp(kind, "partial") || !std::strcmp(kind, "mlp_fwd");
    GemmShape s;
    s.a_kc = std::strcmp(kind, "wgrad") != 0;
    s.b_kc = fwd;
    s.nbatch = n; s.M = M; s.N = N; s.K = K; s.lda = lda; s.ldb = ldb; s.ldc = ldc; s.ldaux = N;
    s.a_al16 = a_al != 0; s.b_al16 = b_al != 0; s.ws_al16 = ws_bytes > 0; s.ws_bytes = (size_t)ws_bytes;
    s.bias = bias != 0; s.relu = relu != 0; s.aux = aux != 0; s.rowsum = rowsum != 0; s.q_unpaired = qw != qpart;
    s.tile = tile; s.splitk = splitk; s.scatter_hw = scatter_hw; s.cus = cus;
    GemmPlan p;
    if (!std::strcmp(kind, "mlp_pair")) {
      GemmShape w = s;                  // dW [Nout][Kin] = dy^T x
      w.a_kc = false; w.M = K; w.N = N; w.K = M; w.ldb = ldx; w.ldc = N; w.aux = false; w.rowsum = true;
      p = plan_ring(RING_PAIR, s, &w);
    } else if (!std::strcmp(kind, "mlp_fwd") || !std::strcmp(kind, "mlp_dgrad")) {
      p = plan_ring(fwd ? RING_FWD : RING_DGRAD, s);
    } else {
      p = std::strcmp(kind, "partial") ? plan_batched(s) : plan_partial(s);
    }
    if (p.variant > GV_EWS && p.splitk > 0) std::printf("%s/s%d %d\n", variant_name(p), p.splitk, p.nq);
    else std::printf("%s %d\n", variant_name(p), p.nq);
  }
  return 0;
}
