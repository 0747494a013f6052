"""ctypes binding of libdrqv2_hip.so (include/drqv2_hip.h).  Loading fails loudly: there is no
CPU or PyTorch fallback for the update path."""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdrqv2_hip.so")

c_float_p = C.c_void_p   # device pointers travel as integers
c_u8_p = C.c_void_p
stream_t = C.c_void_p


class DrqStep(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("global_B", C.c_int), ("C", C.c_int), ("A", C.c_int), ("F", C.c_int), ("H", C.c_int),
        ("obs", c_u8_p), ("next_obs", c_u8_p),
        ("action", c_float_p), ("reward", c_float_p), ("discount", c_float_p),
        ("shift_obs", c_float_p), ("shift_next", c_float_p),
        ("noise_critic", c_float_p), ("noise_actor", c_float_p),
        ("base_grid", c_float_p),
        ("params", c_float_p), ("grads", c_float_p), ("adam_m", c_float_p), ("adam_v", c_float_p),
        ("ws", c_float_p), ("ws_bytes", C.c_size_t),
        ("sums", c_float_p),
        ("lr", C.c_double), ("tau", C.c_double),
        ("std", C.c_float), ("clip", C.c_float),
        ("step_critic", C.c_long), ("step_enc", C.c_long), ("step_actor", C.c_long),
        ("gscale", C.c_float),
        ("stream", stream_t),
        ("sums_host", c_float_p),
        ("store_aug_next", C.c_int),
        ("bf16", C.c_int),
        ("timing_events", C.POINTER(C.c_void_p)),
        ("timing_n", C.c_int),
        ("obs_index", C.c_void_p), ("next_obs_index", C.c_void_p),
        ("flags", C.c_int),
    ]


I, L, F, D, P, SZ = C.c_int, C.c_long, C.c_float, C.c_double, C.c_void_p, C.c_size_t

# name -> (restype, argtypes); mirrors include/drqv2_hip.h one to one
PROTOTYPES = {
    "drq_abi_version": (I, []),
    "drq_num_cus_in_effect": (I, []),
    "drq_set_num_cus": (I, [I]),
    "drq_aug_fwd": (I, [P, P, P, P, I, I, I, I, I, P]),
    "drq_aug_fwd_f32": (I, [P, P, P, P, I, I, I, I, P]),
    "drq_conv1_aug_fwd": (I, [P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv1_aug_fwd_bf16": (I, [P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv1_aug_fwd_bf16_nhwc": (I, [P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv1_aug_fwd_indexed": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv1_aug_fwd_frames": (I, [P, P, L, L, P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv1_aug_fwd_frames_bf16": (I, [P, P, L, L, P, P, P, P, P, P, P, P, P, I, I, P]),
    "drq_conv3x3_fwd": (I, [P, P, P, P, I, I, I, I, I, L, L, L, L, P]),
    "drq_conv3x3_dgrad": (I, [P, P, P, P, I, I, L, L, L, L, P]),
    "drq_conv3x3_fwd_wino": (I, [P, P, P, P, I, I, I, L, L, L, L, P]),
    "drq_conv3x3_dgrad_wino": (I, [P, P, P, P, I, I, L, L, L, L, P]),
    "drq_conv3x3_dgrad_wino_budget": (I, [P, P, P, P, I, I, L, L, L, L, I, P]),
    "drq_conv3x3_wgrad_wino": (I, [P, P, P, P, I, I, L, L, L, L, P, SZ, P]),
    "drq_conv3x3_wgrad": (I, [P, P, P, P, I, I, I, I, L, L, L, L, P, SZ, P]),
    "drq_conv3x3_wgrad_ws_bytes": (SZ, []),
    "drq_conv3x3_fwd_bf16": (I, [P, P, P, P, I, I, I, L, L, L, L, P]),
    "drq_conv3x3_dgrad_bf16": (I, [P, P, P, P, I, I, L, L, L, L, P]),
    "drq_conv3x3_wgrad_bf16": (I, [P, P, P, P, I, I, L, L, L, L, P, SZ, P]),
    "drq_conv3x3_fwd_bf16_nhwc": (I, [P, P, P, P, I, I, I, I, I, P]),
    "drq_conv3x3_dgrad_bf16_nhwc": (I, [P, P, P, P, I, I, I, I, L, L, L, L, P]),
    "drq_conv3x3_wgrad_bf16_nhwc": (I, [P, P, P, P, I, I, I, L, L, L, L, P, SZ, P]),
    "drq_gemm_f32": (I, [P, L, I, P, L, I, P, L, I, I, I, I, L, L, L, P, L, I, P, I, L, I, I, I, P, SZ, P]),
    "drq_gemm_batched_f32": (I, [I, P, L, I, P, L, I, P, L, I, I, I, P, I, P, I, P, I, I, I, P, SZ, P]),
    "drq_gemm_batched_bf16": (I, [I, P, L, I, P, L, I, P, L, I, I, I, P, I, P, I, P, I, I, P, SZ, P]),
    "drq_gemm_batched_partial": (I, [I, P, L, I, P, L, I, P, L, I, I, I, P, P, SZ, C.POINTER(I), P]),
    "drq_mlp_fwd": (I, [I, P, L, P, L, P, L, I, I, I, P, I, P, P, C.POINTER(I), P]),
    "drq_mlp_dgrad": (I, [I, P, L, P, L, P, L, I, I, I, P, I, P]),
    "drq_mlp_wgrad_dgrad": (I, [I, P, L, P, L, P, P, P, L, P, L, P, I, I, I, I, P]),
    "drq_ln_l1_fwd": (I, [I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, L, P]),
    "drq_policy_out_l1_fwd": (I, [P, P, P, P, I, I, I, I, I, F, F, I, P, P, P, L, P, P, P, L, I, P, P, P, P]),
    "drq_qout_fwd": (I, [I, P, P, P, P, I, I, P]),
    "drq_qout_bwd": (I, [I, P, P, P, P, P, P, I, I, P]),
    "drq_ln_tanh_fwd_multi": (I, [I, P, I, P, P, P, P, P, P, I, I, P]),
    "drq_ln_tanh_fwd": (I, [P, I, P, P, P, I, P, P, I, I, P]),
    "drq_ln_tanh_fwd2": (I, [P, P, I, P, P, P, P, P, I, P, I, P, P, P, P, I, I, P]),
    "drq_ln_tanh_bwd": (I, [P, I, P, I, P, I, P, P, P, P, P, P, P, I, I, P]),
    "drq_colsum": (I, [P, L, L, P, L, I, I, I, P]),
    "drq_trunc_normal_sample": (I, [P, P, F, F, I, P, P, L, I, I, P]),
    "drq_copy_cols": (I, [P, I, P, L, I, I, P]),
    "drq_td_mse": (I, [P, P, P, P, P, P, P, P, P, I, F, P]),
    "drq_td_mse_w": (I, [P, P, P, P, P, P, P, P, P, P, P, I, F, P]),
    "drq_actor_loss": (I, [P, P, P, L, P, F, P, P, P, I, I, F, P]),
    "drq_actor_dmu": (I, [P, P, L, I, P, P, I, I, P]),
    "drq_actor_loss_bc": (I, [P, P, P, L, P, L, P, F, F, P, P, P, I, I, F, P]),
    "drq_qout_bwd_actor_bc": (I, [P, P, P, L, P, L, P, F, F, I, F, P, P, P, P, I, I, P]),
    "drq_actor_dmu_bc": (I, [P, P, L, I, P, P, L, P, L, F, P, I, I, P]),
    "drq_policy_out_bwd_bc": (I, [P, P, L, I, P, P, L, P, L, F, P, P, P, P, P, I, I, I, P, I, P]),
    "drq_adam_flat": (I, [P, P, P, P, L, D, L, F, P, D, P]),
    "drq_ema_flat": (I, [P, P, L, D, P]),
    "drq_sum_slices": (I, [P, L, I, P, L, P]),
    "drq_adam_reduce_flat": (I, [P, P, L, I, P, P, L, D, L, F, P]),
    "drq_fill": (I, [P, L, F, P]),
    "drq_u8_normalize": (I, [P, P, L, P]),
    "drq_nstep_gather": (I, [P, P, P, P, P, I, I, L, I, F, P, P, P, P, P, P]),
    "drq_tanh": (I, [P, P, L, P]),
    "drq_per_fill": (I, [P, L, L, L, I, P]),
    "drq_per_sample": (I, [P, L, P, I, I, L, D, P, P, P]),
    "drq_per_update": (I, [P, L, P, P, I, D, D, P]),
    "drq_vec_add": (I, [P, P, P, P, P, L, L, I, L, L, P, P, P, P, P, P]),
    "drq_vec_sample": (I, [P, P, P, P, L, L, I, L, L, L, P, I, I, I, F, P, P, P, P, P, P, P, P, P]),
    "drq_vec_sample_mixed": (I, [P, P, P, P, L, L, L, I, L, L, L, L, P, I, I, I, I, F, P, P, P, P, P, P, P, P, P]),
    "drq_vec_per_advance": (I, [P, L, P, L, L, L, L, L, P]),
    "drq_vec_per_sample": (I, [P, L, P, P, P, P, L, L, I, L, L, L, P, I, I, F, D, P, P, P, P, P, P, P]),
    "drq_vec_per_update": (I, [P, L, P, L, L, L, L, L, P, P, I, D, D, P]),
    "drq_vec_stack_gather": (I, [P, P, L, L, L, P, L, I, P, P]),
    "drq_vec_add_render": (I, [P, P, P, P, P, L, L, I, L, P, I, I, P, P, P, P, P]),
    "drq_vec_stats_step": (I, [P, P, P, P, P, P, P, P, L, L, I, L, P, P, P]),
    "drq_vec_stats_publish": (I, [P, P, P, P, P, L, P, C.c_uint, P]),
    "drq_vec_stats_reset": (I, [P, P, P, P, P, P, P, P, L, L, P]),
    "drq_vec_reach_step": (I, [P, P, P, P, P, L, I, P, C.c_uint, I, I, P, P, P, P, P]),
    "drq_vec_task_step": (I, [I, P, P, P, P, P, P, L, I, P, C.c_uint, I, I, I, P, P, P, P, P, P]),
    "drq_vec_reach_render": (I, [P, P, L, P, P]),
    "drq_vec_reach_image": (I, [P, P, L, I, I, P]),
    "drq_vec_cartpole_step": (I, [P, P, P, P, L, I, P, C.c_uint, I, I, I, I, P, P, P, P, P, P]),
    "drq_vec_cartpole_render": (I, [P, L, P, P]),
    "drq_vec_reacher_step": (I, [P, P, P, P, P, L, I, P, C.c_uint, I, I, I, F, I, P, P, P, P, P, P]),
    "drq_vec_reacher_render": (I, [P, P, L, F, P, P]),
    "drq_vec_catch_step": (I, [P, P, P, P, L, I, P, C.c_uint, I, I, I, F, I, P, P, P, P, P, P]),
    "drq_vec_catch_render": (I, [P, L, F, P, P]),
    "drq_vec_walker_step": (I, [P, P, P, P, L, I, P, C.c_uint, I, I, I, F, P, P, P, P, P, P]),
    "drq_vec_walker_render": (I, [P, L, P, P]),
    "drq_vec_finger_step": (I, [P, P, P, P, P, L, I, P, C.c_uint, I, I, I, I, F, I, P, P, P, P, P, P]),
    "drq_vec_finger_render": (I, [P, P, L, I, F, P, P]),
    "drq_vec_maze_step": (I, [P, P, P, P, P, P, L, I, P, C.c_uint, I, I, I, I, I, I, C.c_uint, I, P, P, P, P, P, P]),
    "drq_vec_maze_render": (I, [P, P, P, L, I, P, P]),
    "drq_vec_maze_geodesic": (I, [P, P, P, L, I, P, P]),
    "drq_explore_simhash_step": (I, [P, L, I, C.c_uint, F, I, P, P, P, P, P, P, P]),
    "drq_explore_knn_ws_bytes": (SZ, [L, L, L]),
    "drq_explore_knn": (I, [P, L, I, L, P, L, I, L, L, P, P, SZ, P]),
    "drq_vec_distract": (I, [P, P, P, P, P, P, L, C.c_uint, I, I, I, I, I, I, I, I, I, I, P, P]),
    "drq_aug_overlay": (I, [P, P, P, P, L, I, I, I, P]),
    "drq_aug_random_conv": (I, [P, P, P, L, I, P]),
    "drq_vec_stack_push": (I, [P, P, P, P, L, I, P]),
    "drq_vec_video_record": (I, [P, P, I, P, I, P, I, I, I, L, P]),
    "drq_vec_export_rows": (I, [P, P, P, P, L, L, I, L, I, P, I, P, P, P, P, P]),
    "drq_vec_fill": (I, [P, P, P, P, P, L, L, I, L, L, I, P, P, P, P, P, P]),
    "drq_nstep_gather_frames": (I, [P, P, L, P, P, P, P, I, I, L, I, F, P, P, P, P, P, P]),
    "drq_relu_mask_pad": (I, [P, P, P, L, I, I, P]),
    "drq_conv1_dgrad": (I, [P, P, P, I, P]),
    "drq_aug_bwd_f32": (I, [P, P, P, P, I, I, I, I, P]),
    "drq_tanh_bwd": (I, [P, P, P, L, P]),
    "drq_dormant_scores": (I, [P, L, I, I, P, P]),
    "drq_dormant_count": (I, [P, I, F, P, P, P]),
    "drq_lerp_flat": (I, [P, P, L, F, P]),
    "drq_param_layout": (I, [I, I, I, I, C.POINTER(L), I]),
    "drq_step_ws_bytes": (SZ, [I, I, I, I, I]),
    "drq_step_ws_offset": (L, [I, I, I, I, I, I]),
    "drq_update_phase": (I, [C.POINTER(DrqStep), I]),
    "drq_update_phase_overlap": (I, [C.POINTER(DrqStep), P, I]),
    "drq_update_phase_bc": (I, [C.POINTER(DrqStep), I, F]),
    "drq_update_phase_per": (I, [C.POINTER(DrqStep), I, P, P]),
    "drq_update_phase_frames": (I, [C.POINTER(DrqStep), I, P, L, L, P, P]),
    "drq_act_forward": (I, [C.POINTER(DrqStep), P, I, P]),
    "drq_act_ws_bytes": (SZ, [I, I, I, I, I]),
    "drq_act_batch": (I, [P, I, I, I, I, P, I, P, F, P, P, P, SZ, P]),
    "drq_publish_sums": (I, [P, P, C.c_uint, P]),
    "drq_rng_draws": (I, [C.c_uint64, C.c_uint64, I, I, I, P, P, P, P, P]),
}

WS_IDS = ["AUG", "ACT1", "ACT2", "ACT3", "FEAT", "Z_NEXT", "Z_OBS", "HA_T", "HA_C", "H_AN", "H_AO", "Q", "TQ",
          "DQ", "MU_O", "DY4", "DY3", "DY2", "DY1", "DZ_C", "DZ_A", "HA_C2", "P1", "P2", "C1", "C2",
          "XHAT_C", "RSTD_C", "XHAT_A", "RSTD_A", "Z_C2", "HROWS", "P3", "Z4", "T1", "T2", "DC2", "DC1", "DHA", "DLN",
          "DPRE", "DP2", "DP1", "DH_A", "DA"]

# ids of drq_update_phase (the DRQ_PHASE_* enum of include/drqv2_hip.h, where each is described)
PHASE_ALL, PHASE_CRITIC, PHASE_ACTOR, PHASE_OPT = -1, 0, 1, 2
PHASE_ENCODE, PHASE_CRITIC_HEADS, PHASE_CONV_BACKWARD, PHASE_ACTOR_FORWARD, PHASE_ACTOR_BACKWARD = 3, 4, 5, 6, 7
PHASE_ENCODER_OPT, PHASE_ACTOR_OPT = 8, 9
PHASE_CRITIC_OPT, PHASE_ACTOR_LOSS, PHASE_POLYAK, PHASE_REDRAW = 10, 11, 12, 13

STEP_OVERLAP_ACTOR = 16   # DRQ_STEP_OVERLAP_ACTOR (DrqStep.flags)

PARAM_LAYOUT_LEN = 59   # DRQ_PARAM_LAYOUT_LEN: the offsets drq_param_layout writes

# the entries without a trailing drq_stream_t: they launch nothing, or their DrqStep carries the stream
NO_STREAM = frozenset({"drq_abi_version", "drq_num_cus_in_effect", "drq_set_num_cus", "drq_conv3x3_wgrad_ws_bytes", "drq_param_layout", "drq_step_ws_bytes",
                       "drq_step_ws_offset", "drq_update_phase", "drq_update_phase_overlap", "drq_update_phase_bc", "drq_update_phase_per",
                       "drq_update_phase_frames", "drq_act_forward", "drq_act_ws_bytes", "drq_explore_knn_ws_bytes"})

_lib = None


class DrqError(RuntimeError):
    pass


def load():
    """Returns the loaded library; raises if it has not been built (python -m drqv2_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DrqError(f"{LIB_PATH} is missing: build it with `python -m drqv2_amd.build` "
                       "(hipcc --offload-arch=gfx950).  The DrQ-v2 update path has no fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(lib, name):    # additive changes keep the ABI version: a library built before one lacks the entry
            raise DrqError(f"{LIB_PATH} does not export {name}: it was built from older sources; rebuild it with "
                           "`python -m drqv2_amd.build --force`")
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.drq_abi_version() != 7:
        raise DrqError("libdrqv2_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc == 0:
        return
    if rc == -1:
        raise DrqError(f"{what}: bad argument / unsupported shape (DRQ_EARG)")
    if rc == -2:
        raise DrqError(f"{what}: workspace too small (DRQ_EWS)")
    raise DrqError(f"{what}: HIP error {rc}")


def current_stream():
    """the current device's current stream as the library takes it (CPU tests replace this)"""
    return torch.cuda.current_stream().cuda_stream


def enqueue(name, *args, device=None):
    """Calls the stream entry `name` with args and the current stream of `device`, made current for the call (None:
    of the current device, as it stands); returns its status."""
    if name not in PROTOTYPES or name in NO_STREAM:
        raise DrqError(f"{name}: not an entry of the library that takes a stream")
    fn = getattr(load(), name)
    index = None if device is None else torch.device(device).index      # "cuda" without an index is the current one
    if index is None or index == torch.cuda.current_device():
        rc = fn(*args, current_stream())
    else:
        with torch.cuda.device(index):      # the library launches on the current HIP device
            rc = fn(*args, current_stream())
    return rc


def launch(name, *args, device=None):
    """enqueue() that raises DrqError, naming the entry, unless the status is DRQ_OK"""
    check(enqueue(name, *args, device=device), name)


def device_index(device):
    """`device` as tensors on it report theirs: "cuda" without an index is the current device"""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return d


def ptr(t):
    """data pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def param_layout(Cc, A, Fd, H):
    lib = load()
    buf = (L * PARAM_LAYOUT_LEN)()
    n = lib.drq_param_layout(Cc, A, Fd, H, buf, PARAM_LAYOUT_LEN)
    if n != PARAM_LAYOUT_LEN:
        raise DrqError("drq_param_layout failed")
    v = list(buf)
    return {"enc": v[0:8], "critic": v[8:24], "actor": v[24:34], "target": v[34:50],
            "seg": {"enc": (v[50], v[51]), "critic": (v[52], v[53]), "actor": (v[54], v[55]),
                    "target": (v[56], v[57])}, "total": v[58]}
