"""The shapes of the per-launch audit of the update's head section (tests/test_hip_head_audit.py) and the decisions each
of them takes (a helper module: not collected, needs no GPU).

Which launches the head section issues depends on five predicates (drqv2_amd/csrc/step_plan.h) and on whether five of its
GEMMs leave split-K records in the workspace for their consumer (the planner, csrc/gemm_plan.h).  tests/step_plan_dump.cpp
prints all ten for a shape; tests/test_cpu_head_audit.py holds the `expect` of every row to it, requires every decision
to be taken on both sides by the rows, and holds the table of sides no batch can take to a sweep over every batch size.
"""
from collections import namedtuple

CUS = 256
MAX_BATCH = 4096                # StepEngine.MAX_BATCH

# the dump's columns, in its order; sk.* > 1 reads as "records are left"
PREDICATES = ("fuse_rows", "ln_rides", "qout_loss_fits_lds", "fused_head", "out_layer_kernel")
RECORDS = ("sk.trunk4", "sk.trunk1", "sk.dha", "sk.da", "sk.dh")
DECISIONS = PREDICATES + RECORDS

Row = namedtuple("Row", "B A F H mode updates expect reaches")


def _row(B, A, F, H, mode, expect, reaches, updates=1):
    """expect: the decisions that are TRUE for the row, space separated (every other one is false)"""
    return Row(B, A, F, H, mode, updates, frozenset(expect.split()), reaches)


# mode: fp32 / bf16 (compute dtype), bc (fp32, DrQ+BC with alpha BC_ALPHA), per (fp32, a loss weight per row)
BC_ALPHA = 2.5
AUDIT_ROWS = [
    _row(8, 6, 50, 256, "fp32", "fuse_rows qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "B < 32: the trunk kernels refuse the batch and the LDS-staged GEMM leaves 88 (phase 6: 205) records per trunk, "
         "which drq_lnl1_fwd sums.  No rider.  Fused output-layer backward reading records."),
    _row(32, 6, 50, 256, "fp32", "fuse_rows qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "Records of the trunk kernel.  drq_lnl1_fwd and drq_polout_l1_fwd (rows fused) in phases 4 and 6.  Second update "
         "from real Adam state, with different step counts for the encoder and the actor (drq_adam_flat2).", updates=2),
    _row(128, 6, 50, 1024, "fp32", "fuse_rows ln_rides qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "ln_rides: LayerNorm parameter gradients inside both trunk weight-gradient launches.  Ring pair kernels at the "
         "training width."),
    _row(32, 21, 100, 256, "fp32", "qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "Rows not fused (F+A > 64, odd A): drq_ln_tanh_fwd_multi_part with records, bias and tail.  Wide trunk forward."),
    _row(32, 1, 50, 256, "fp32", "qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh", "A = 1."),
    _row(8, 33, 50, 64, "fp32", "qout_loss_fits_lds out_layer_kernel sk.trunk4 sk.trunk1",
         "A > 32: drq_actor_dmu, then separate weight and input gradients of the output layer.  H = 64 < 256: no "
         "split-K in the three input-gradient GEMMs, DHA / DA / DH_A hold the products."),
    _row(8, 65, 20, 64, "fp32", "qout_loss_fits_lds sk.trunk4 sk.trunk1",
         "A > 64: drq_copy_cols.  Output layer as a GEMM.  Both draws by drq_trunc_normal_sample."),
    _row(1024, 12, 50, 256, "fp32", "fuse_rows qout_loss_fits_lds out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.dh",
         "B A > 11264 with A <= 32: unfused head.  The >= 1024-row shapes of the Q output backward and of drq_colsum."),
    _row(481, 6, 256, 256, "fp32", "qout_loss_fits_lds fused_head out_layer_kernel sk.trunk1 sk.dha sk.da sk.dh",
         "512 output tiles fill the chip: the four trunks of phase 4 leave NO records, drq_ln_tanh_fwd_multi_part reads Z4 "
         "plus the tail.  F = 256: four elements per lane in the LayerNorm kernels.  (No batch below 32 does this: the "
         "LDS-staged GEMM splits K whenever fewer than 512 tiles are left.)"),
    _row(2017, 6, 256, 64, "fp32", "qout_loss_fits_lds out_layer_kernel",
         "512 output tiles from ONE trunk: phase 6's product leaves no records either, drq_ln_tanh_fwd_multi_part reads "
         "Z_C2.  The smallest batch that does (B = 4065 at F = 100).  Random frames: the head does not care, and the "
         "smooth ones take longer to make than the row to run."),
    _row(32, 6, 50, 1024, "bf16", "qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "The head's GEMMs on the bf16 path."),
    _row(32, 6, 50, 256, "bc", "fuse_rows qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "actor_loss_bc inside drq_qout_bwd_actor.  BC form of drq_policy_out_bwd."),
    _row(8, 33, 50, 64, "bc", "qout_loss_fits_lds out_layer_kernel sk.trunk4 sk.trunk1", "drq_actor_dmu_bc."),
    _row(32, 6, 50, 256, "per", "fuse_rows qout_loss_fits_lds fused_head out_layer_kernel sk.trunk4 sk.trunk1 sk.dha sk.da sk.dh",
         "Weighted TD loss inside drq_qout_bwd_td, and td_abs."),
]

# sides no batch 1..MAX_BATCH takes, whatever A <= 256, F <= 256, H: decision -> (the side, why)
UNREACHABLE = {
    "qout_loss_fits_lds": (False, "(B + 5136) floats of LDS exceed 60 KiB from B = 10225 on; update() takes 4096 rows"),
}

def row_id(r):
    return "b%d-a%d-f%d-h%d-%s" % (r.B, r.A, r.F, r.H, r.mode)


def dump_line(r, cus=CUS, flags=0):
    return "%d %d %d %d %d %d %d\n" % (cus, r.B, r.A, r.F, r.H, int(r.mode == "bf16"), flags)


def decisions_of(values):
    """the dump's ten integers -> {decision: bool}"""
    assert len(values) == len(DECISIONS), values
    out = {k: bool(v) for k, v in zip(PREDICATES, values)}
    out.update({k: v > 1 for k, v in zip(RECORDS, values[len(PREDICATES):])})
    return out


def expected(r):
    return {k: k in r.expect for k in DECISIONS}
