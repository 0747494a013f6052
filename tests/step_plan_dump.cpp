// What the head section of the fused update decides for a shape, one shape per input line, for
// tests/test_cpu_head_audit.py to hold against tests/head_variants.py.  Host only: the two planner headers are all it
// needs.  A line is
//   cus B A F H bf16 flags
// and the answer
//   fuse_rows ln_rides qout_loss_fits_lds fused_head out_layer_kernel  sk_trunk4 sk_trunk1 sk_dha sk_da sk_dh
// the five predicates of drqv2_amd/csrc/step_plan.h, then the split-K record counts drq_gemm_batched_partial_any reports
// for the five products step.hip leaves to their consumer (<= 1: the product is in its own buffer, no records): the
// four trunks of phase 4, the one trunk of phase 6, the critic's layer-1 input gradient (both heads, F+A columns), its
// action columns alone (phase 7, asked for only when the output-layer backward is fused; 1 otherwise), and the policy's
// layer-1 input gradient.  The shapes are filled as Ctx::gemm / fwd_call do: 64 MiB of aligned workspace.
#include "../drqv2_amd/csrc/gemm_plan.h"
#include "../drqv2_amd/csrc/step_plan.h"

#include <cstdio>

static int records(int cus, int bf16, int n, int M, int N, int K, long lda, bool a_kc, long ldb, bool b_kc, long ldc,
                   bool bias, bool b_al16) {
  GemmShape s;
  s.bf16 = bf16 != 0; s.nbatch = n; s.M = M; s.N = N; s.K = K; s.lda = lda; s.a_kc = a_kc; s.ldb = ldb; s.b_kc = b_kc;
  s.ldc = ldc; s.bias = bias; s.a_al16 = true; s.b_al16 = b_al16; s.ws_al16 = true;
  s.ws_bytes = (size_t)16 * 1024 * 1024 * sizeof(float); s.cus = cus;
  const GemmPlan p = plan_partial(s);
  return p.variant <= GV_EWS ? -1 : p.splitk;
}

int main() {
  const int R = 32 * 35 * 35;
  int cus, B, A, F, H, bf16, flags;
  while (std::scanf("%d %d %d %d %d %d %d", &cus, &B, &A, &F, &H, &bf16, &flags) == 7) {
    const int FA = F + A;
    const bool fused_head = step_fused_head(B, A);
    std::printf("%d %d %d %d %d  %d %d %d %d %d\n", (int)step_fuse_rows(A, F, H, bf16, flags), (int)step_ln_rides(B, F, bf16),
                (int)step_qout_loss_fits_lds(B), (int)fused_head, (int)step_out_layer_kernel(A),
                records(cus, bf16, 4, B, F, R, R, true, R, true, F, true, true),
                records(cus, bf16, 1, B, F, R, R, true, R, true, F, true, true),
                records(cus, bf16, 2, B, FA, H, H, true, FA, false, FA, false, true),
                fused_head ? records(cus, bf16, 2, B, A, H, H, true, FA, false, A, false, F % 4 == 0) : 1,
                records(cus, bf16, 1, B, F, H, H, true, F, false, F, false, true));
  }
  return 0;
}
