// The head section's dispatch decisions of the fused update (step.hip), as free functions of the step's shape: which of
// two launch sequences a phase issues.  Host only, nothing but the public header: tests/step_plan_dump.cpp compiles it
// for the CPU and tests/test_cpu_head_audit.py holds the rows of the per-launch audit (tests/head_variants.py) to it.
#pragma once
#include <cstddef>

#include "../../include/drqv2_hip.h"

// row-local stages fused with the first MLP layers (rowblock.hip): fp32, shapes its kernels take
// measured (tools/ab_flags.py, same process, interleaved): cheetah_run B=256 1021.9 us fused against 1024.2, but
// humanoid_run (F+A = 121: odd, dword weight loads, 128-long padded reduction) 540 against 508 us at B=32 and 1220
// against 1203 at B=256 -- the fused kernels are chains of dependent memory round trips like the launches they
// replace, and only win where every weight row can be fetched with 8- or 16-byte loads into a 64-long reduction
// (taken only where the trunk forward also left split-K records, which is the GEMM planner's decision)
inline bool step_fuse_rows(int A, int F, int H, int bf16, int flags) {
  return !(flags & DRQ_STEP_NO_ROW_FUSION) && !bf16 && A <= 32 && F + A <= 64 && F % 2 == 0 && A % 2 == 0 &&
         H % 256 == 0;
}

// the LayerNorm parameter gradients ride in the trunk's weight-gradient launch (one extra workgroup) when the dedicated
// kernel takes the shape; the LayerNorm backward then leaves them out
inline bool step_ln_rides(int B, int F, int bf16) {
  return !bf16 && F <= 128 && (B == 128 || B == 256 || B == 512);
}

// B rows fit the LDS of the Q-output backward kernels that compute a loss as well (drq_qout_bwd_td / _actor)
inline bool step_qout_loss_fits_lds(int B) { return ((size_t)B + 5 * 1024 + 16) * 4 <= 60 * 1024; }

// policy output layer backward in one kernel (dpre, dW3, db3, dp2) when dpre fits its LDS
inline bool step_fused_head(int B, int A) { return A <= 32 && ((size_t)B * A + 4 * 1024) * 4 <= 60 * 1024; }

// the policy's output-layer kernel (output + tanh + sample in one launch) and the action tail riding in the LayerNorm
// launch take up to 64 action columns; beyond, the output layer is a GEMM, both draws are launches of their own and
// the action columns are copied
inline bool step_out_layer_kernel(int A) { return A <= 64; }
