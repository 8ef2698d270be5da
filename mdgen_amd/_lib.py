"""ctypes binding of libmdgen_amd.so (include/mdgen_amd.h).  There is NO fallback: if the HIP
library is missing or fails to load, importing this module raises."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- must be imported first: provides the process-wide libamdhip64.so.7

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDGEN_AMD_LIB", os.path.join(_HERE, "libmdgen_amd.so"))   # override: debugging builds only

ABI_VERSION = 8   # include/mdgen_amd.h MDGEN_ABI_VERSION

EXPORTS = [
    "mdgen_last_error", "mdgen_abi_version", "mdgen_dev_build", "mdgen_ctx_create", "mdgen_ctx_destroy", "mdgen_ctx_set_weight",
    "mdgen_ctx_finalize", "mdgen_ctx_set_option", "mdgen_debug_view_plan", "mdgen_ctx_num_weights", "mdgen_ctx_weight_name", "mdgen_workspace_layout",
    "mdgen_denoiser_forward", "mdgen_sample_euler", "mdgen_rollout_euler", "mdgen_profile_enable", "mdgen_profile_report", "mdgen_profile_phase_trace", "mdgen_debug_dispatch_plan", "mdgen_debug_layout_maps", "mdgen_debug_mlp_stream_table", "mdgen_debug_train_linear", "mdgen_debug_train_dw", "mdgen_debug_train_attention", "mdgen_debug_train_plan",
    "mdgen_debug_ipa_attention", "mdgen_debug_ipa_slices",
    "mdgen_rigid_compose", "mdgen_rigid_invert",
    "mdgen_rigid_apply", "mdgen_quat_to_rot", "mdgen_rot_to_quat", "mdgen_prep_latents", "mdgen_prep_keyframes", "mdgen_upsample_euler",
    "mdgen_samples_to_atom14", "mdgen_atom14_to_cond", "mdgen_pdb_format", "mdgen_path_plan", "mdgen_masked_mse", "mdgen_from_3_points",
    "mdgen_grad_sumsq", "mdgen_adam_step", "mdgen_ema_update", "mdgen_train_workspace_bytes",
    "mdgen_train_forward_backward",
    "mdgen_train_num_milestones", "mdgen_train_bind_params",
    "mdgen_train_set_milestone_events",
    "mdgen_sample_dopri5", "mdgen_dopri5_workspace_bytes", "mdgen_debug_dopri5_controller",
    "mdgen_sample_rk", "mdgen_rk_workspace_bytes", "mdgen_debug_rk_plan", "mdgen_debug_rk_stage",
    "mdgen_rollout_rk", "mdgen_upsample_rk",
    "mdgen_sample_sde", "mdgen_sde_workspace_bytes", "mdgen_debug_sde_plan", "mdgen_debug_sde_dispatch_plan", "mdgen_debug_sde_stage",
    "mdgen_sample_sde_rng", "mdgen_debug_sde_noise", "mdgen_debug_sde_stage_rng", "mdgen_debug_philox", "mdgen_rollout_sde", "mdgen_upsample_sde", "mdgen_debug_graph_count",
    "mdgen_traj_dihedrals", "mdgen_traj_histograms", "mdgen_traj_acov", "mdgen_traj_acov_workspace_bytes",
    "mdgen_traj_lagged_moments", "mdgen_traj_lagged_moments_workspace_bytes", "mdgen_traj_project", "mdgen_traj_series_acov",
    "mdgen_traj_series_acov_workspace_bytes", "mdgen_traj_histograms_xy",
    "mdgen_traj_kmeans_assign", "mdgen_traj_kmeans_step", "mdgen_traj_kmeans_step_workspace_bytes", "mdgen_traj_kmeans_pp",
    "mdgen_traj_kmeans_pp_workspace_bytes", "mdgen_traj_count_matrix", "mdgen_tp_sample",
    "mdgen_ens_superpose", "mdgen_ens_moments", "mdgen_ens_moments_workspace_bytes", "mdgen_ens_pairwise_d2",
    "mdgen_ens_pairwise_d2_workspace_bytes", "mdgen_ens_contact_counts", "mdgen_ens_sasa_workspace_bytes", "mdgen_ens_sasa_counts",
]


class ModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "embed_dim", "mha_heads", "num_layers", "latent_dim", "ipa_heads", "ipa_head_dim", "ipa_qk", "ipa_v",
        "abs_pos_emb", "crop", "tps_condition")] + [("time_multiplier", C.c_float)]


class Shape(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("L", C.c_int32)]


class WsLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "total_bytes", "h", "qf", "kf", "vf", "obuf", "mod", "silu_t", "ipa_out", "h_ipa", "ipa_proj",
        "ipa_feat", "mask_bl", "rel7", "tgrid", "f32_scratch", "split", "fold", "embase")]


class ResidueTables(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "default_frames", "lit_positions", "atom14_group", "atom14_mask", "atom37_to_atom14", "atom37_mask",
        "chi_atom_indices", "chi_angles_mask")]

    @classmethod
    def from_dict(cls, tables):
        """From a dict of device tensors under the field names (geometry.residue_tables)."""
        return cls(*[tables[n].data_ptr() for n, _ in cls._fields_])


class Cond(C.Structure):
    """mdgen_cond: the conditioning pointers of a network evaluation.  Build it with `cond()`."""
    _fields_ = [(n, C.c_void_p) for n in (
        "mask", "start_rot", "start_trans", "end_rot", "end_trans", "rel7", "x_cond", "x_cond_mask", "aatype")]


class SdeOpts(C.Structure):
    """mdgen_sde_opts.  Build it with `sde_opts()`."""
    _fields_ = ([(n, C.c_int32) for n in ("method", "path", "diffusion_form", "last_step", "n_points")]
                + [(n, C.c_double) for n in ("diffusion_norm", "last_step_size", "sample_eps")])


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m mdgen_amd.build` (hipcc, gfx950). "
            "mdgen_amd has no CPU/PyTorch fallback path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    lib.mdgen_last_error.restype = C.c_char_p
    lib.mdgen_abi_version.restype = i32
    lib.mdgen_ctx_create.argtypes = [C.POINTER(vp), C.POINTER(ModelDesc)]
    lib.mdgen_ctx_destroy.argtypes = [vp]
    lib.mdgen_ctx_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32, vp]
    lib.mdgen_ctx_finalize.argtypes = [vp, vp]
    lib.mdgen_ctx_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.mdgen_debug_view_plan.argtypes = [C.POINTER(Shape), i32, C.POINTER(i32), C.POINTER(i32)]
    lib.mdgen_ctx_num_weights.argtypes = [vp]
    lib.mdgen_ctx_weight_name.argtypes = [vp, i32]
    lib.mdgen_ctx_weight_name.restype = C.c_char_p
    lib.mdgen_workspace_layout.argtypes = [vp, C.POINTER(Shape), i32, i32, C.POINTER(WsLayout)]
    ctx_shape, cond_p, ws_bytes = [vp, C.POINTER(Shape)], C.POINTER(Cond), [vp, sz]   # (ctx, shape) | mdgen_cond* | (workspace, bytes)
    lib.mdgen_denoiser_forward.argtypes = ctx_shape + [vp, vp, cond_p] + [vp, vp, vp] + ws_bytes + [vp]   # x, t | out, trace_h, trace_ipa
    lib.mdgen_sample_euler.argtypes = ctx_shape + [i32, vp, cond_p] + ws_bytes + [i32, vp]
    f64 = C.c_double
    lib.mdgen_sample_dopri5.argtypes = ctx_shape + [f64, f64, i32, vp, cond_p] + ws_bytes + [C.POINTER(i32), vp, vp]
    lib.mdgen_dopri5_workspace_bytes.argtypes = [vp, C.POINTER(Shape), C.POINTER(sz)]
    lib.mdgen_debug_dopri5_controller.argtypes = [vp, vp, i32, i32] + [vp] * 7
    lib.mdgen_sample_rk.argtypes = ctx_shape + [i32, i32, vp, cond_p] + ws_bytes + [i32, vp]
    lib.mdgen_rk_workspace_bytes.argtypes = [vp, C.POINTER(Shape), i32, i32, C.POINTER(sz)]
    lib.mdgen_debug_rk_plan.argtypes = [i32, i32, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)]
    lib.mdgen_debug_rk_stage.argtypes = [vp, C.POINTER(Shape), i32, i32, C.c_float] + [vp] * 10
    sde_p = C.POINTER(SdeOpts)
    lib.mdgen_sample_sde.argtypes = ctx_shape + [sde_p, vp, vp, i64, cond_p] + ws_bytes + [i32, vp]   # opts | x, noise, its step stride
    lib.mdgen_sde_workspace_bytes.argtypes = [vp, C.POINTER(Shape), sde_p, C.POINTER(sz)]
    lib.mdgen_debug_sde_plan.argtypes = [sde_p, vp, vp, i32, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(i32), vp]
    lib.mdgen_debug_sde_dispatch_plan.argtypes = [C.POINTER(Shape), sde_p, i32, i32, i32, i32, C.c_char_p, C.c_char_p, sz]
    lib.mdgen_debug_sde_stage.argtypes = [vp, C.POINTER(Shape), sde_p, i32, i32] + [vp] * 9
    lib.mdgen_sample_sde_rng.argtypes = ctx_shape + [sde_p, vp, vp, cond_p] + ws_bytes + [i32, vp]   # opts | x, rng words
    lib.mdgen_debug_sde_noise.argtypes = [C.POINTER(Shape), i32, vp, i32, i32, vp, vp]
    lib.mdgen_debug_sde_stage_rng.argtypes = [vp, C.POINTER(Shape), sde_p, i32, i32, i32] + [vp] * 9
    lib.mdgen_debug_philox.argtypes = [vp, vp, vp]
    lib.mdgen_debug_graph_count.argtypes = [vp, C.POINTER(i32)]
    tables_atom14 = [C.POINTER(ResidueTables), vp]
    lib.mdgen_rollout_euler.argtypes = (ctx_shape + [i32, i32] + [vp, vp] + [vp, vp, vp] + [vp] + [vp, vp]   # zs, mask | cond frame | seqres | x_cond, its mask
                                        + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_upsample_euler.argtypes = (ctx_shape + [i32, i32] + [vp, vp] + [vp, vp, vp] + [vp] + [vp, vp] + [vp, vp]   # ... | key frames | ... | start_rot, start_trans
                                         + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_rollout_rk.argtypes = (ctx_shape + [i32, i32, i32] + [vp, i64, vp] + [vp, vp, vp] + [vp] + [vp, vp]   # method, steps, blocks | zs, its block stride, mask | ...
                                     + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_upsample_rk.argtypes = (ctx_shape + [i32, i32, i32] + [vp, vp] + [vp, vp, vp] + [vp] + [vp, vp] + [vp, vp]   # as mdgen_upsample_euler after (method, steps, interval)
                                      + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_rollout_sde.argtypes = (ctx_shape + [sde_p, vp, i32] + [vp, i64, vp] + [vp, vp, vp] + [vp] + [vp, vp]   # as mdgen_rollout_rk after (opts, rng, blocks)
                                      + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_upsample_sde.argtypes = (ctx_shape + [sde_p, vp, i32] + [vp, vp] + [vp, vp, vp] + [vp] + [vp, vp] + [vp, vp]   # as mdgen_upsample_rk after (opts, rng, interval)
                                       + tables_atom14 + ws_bytes + [i32, vp])
    lib.mdgen_profile_enable.argtypes = [vp, i32]
    lib.mdgen_profile_phase_trace.argtypes = [vp, vp, i64]
    lib.mdgen_profile_report.argtypes = [vp, vp, C.c_char_p, sz]
    lib.mdgen_debug_dispatch_plan.argtypes = [C.POINTER(Shape), i32, i32, i32, i32, i32, i32, C.c_char_p, C.c_char_p, sz]
    lib.mdgen_debug_layout_maps.argtypes = [vp] * 5
    lib.mdgen_debug_mlp_stream_table.argtypes = [vp, i32]
    lib.mdgen_debug_train_linear.argtypes = [i32, vp, i32, vp, i32, vp, i64, i32, i32, vp, i32, vp, vp]
    lib.mdgen_debug_train_dw.argtypes = [i32, vp, i32, vp, i32, i64, i32, i32, vp, vp, vp, i64, vp]
    lib.mdgen_debug_train_attention.argtypes = [i32, vp, i64, i32, i32, i32, i32, i32, i32] + [vp] * 11
    lib.mdgen_debug_train_plan.argtypes = [C.POINTER(Shape), i32, i32, i32, i32, C.c_char_p, sz]
    lib.mdgen_debug_ipa_attention.argtypes = [vp] * 5 + [i32, i32, i32, vp, i64] + [vp] * 7 + [C.POINTER(i32), C.POINTER(i32), vp]
    lib.mdgen_debug_ipa_slices.argtypes = [i32, i32, i32, i64] + [C.POINTER(i32)] * 3
    lib.mdgen_rigid_compose.argtypes = [i64] + [vp] * 7
    lib.mdgen_rigid_invert.argtypes = [i64] + [vp] * 5
    lib.mdgen_rigid_apply.argtypes = [i64, i64, vp, vp, vp, vp, i32, vp]
    lib.mdgen_quat_to_rot.argtypes = [i64, vp, i32, vp, vp]
    lib.mdgen_rot_to_quat.argtypes = [i64, vp, vp, vp]
    lib.mdgen_prep_latents.argtypes = [C.POINTER(Shape), i32, i32] + [vp] * 7
    lib.mdgen_prep_keyframes.argtypes = [C.POINTER(Shape), i32] + [vp] * 8
    lib.mdgen_samples_to_atom14.argtypes = [C.POINTER(Shape), i32, i32] + [vp] * 10
    lib.mdgen_atom14_to_cond.argtypes = [i32, i32] + [vp] * 11
    lib.mdgen_pdb_format.argtypes = [i64, i32, i64] + [vp] * 8 + [i64, vp, vp]   # M, L, model_base | ... text, its capacity, status
    lib.mdgen_traj_dihedrals.argtypes = [i64, i32, i32, vp, vp, vp, vp]   # F, L, NF | atom14, quad (host), angles
    lib.mdgen_traj_histograms.argtypes = [i64, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]   # F, NF, angles | bins1, edges1 | P, pairs (host) | bins2, edges2 | ...
    lib.mdgen_traj_acov_workspace_bytes.argtypes = [i64, i32, i64, C.POINTER(sz)]
    lib.mdgen_traj_acov.argtypes = [i64, i32, i64, vp, vp, vp, vp, vp, sz, vp]   # n, NF, K | angles, acov, mean_sin, mean_cos | workspace, bytes
    lib.mdgen_traj_lagged_moments_workspace_bytes.argtypes = [i64, i32, i64, C.POINTER(sz)]
    lib.mdgen_traj_lagged_moments.argtypes = [i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]   # n, NF, lag | angles | sx, sy, cxx, cyy, cxy | workspace, bytes
    lib.mdgen_traj_project.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp]   # n, NF, d | angles, mean, W, out
    lib.mdgen_traj_series_acov_workspace_bytes.argtypes = [i64, i32, i64, C.POINTER(sz)]
    lib.mdgen_traj_series_acov.argtypes = [i64, i32, i64, vp, vp, vp, vp, sz, vp]   # n, NS, K | x, acov, mean | workspace, bytes
    lib.mdgen_traj_histograms_xy.argtypes = [i64, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]   # F, NC, values | P, pairs (host) | bins, edges_x, edges_y | hist2, dropped
    lib.mdgen_traj_kmeans_assign.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp]   # n, d, k | x, centers, assign, dist2 (or None)
    lib.mdgen_traj_kmeans_step_workspace_bytes.argtypes = [i64, i32, i32, C.POINTER(sz)]
    lib.mdgen_traj_kmeans_step.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, sz, vp]   # n, d, k | x, centers, assign | sums, counts, cost, state | tol | workspace, bytes
    lib.mdgen_traj_kmeans_pp_workspace_bytes.argtypes = [i64, i32, i32, C.POINTER(sz)]
    lib.mdgen_traj_kmeans_pp.argtypes = [i64, i32, i32, vp, vp, i32, i32, vp, vp, vp, sz, vp]   # n, d, k | x, u (host) | r0, r1 | chosen, mind2 | workspace, bytes
    lib.mdgen_traj_count_matrix.argtypes = [i64, i64, i32, vp, vp, vp, vp]   # n, lag, k | dtraj, counts, dropped
    u32, u64 = C.c_uint32, C.c_uint64
    lib.mdgen_tp_sample.argtypes = [i64, i32, i32, vp, vp, i32, i32, u64, u32, u64, i32, vp, vp, vp, vp, vp, vp]   # n_samples, N, k | Ta, Ba | start, end | seed, stream_id, sample_base | kb, Tb, Bb, phi (host) | paths, prob
    lib.mdgen_ens_superpose.argtypes = [i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]   # F, A | x, ref, w, exists (or None) | out, rot, rmsd (or None)
    lib.mdgen_ens_moments_workspace_bytes.argtypes = [i64, i32, C.POINTER(sz)]
    lib.mdgen_ens_moments.argtypes = [i64, i32, vp, vp, vp, vp, sz, vp]   # F, A | x, mean, cov | workspace, bytes
    lib.mdgen_ens_pairwise_d2_workspace_bytes.argtypes = [i64, i64, i32, C.POINTER(sz)]
    lib.mdgen_ens_pairwise_d2.argtypes = [i64, i64, i32, vp, vp, vp, vp, vp, sz, vp]   # Fa, Fb, A | xa, xb, d2 (or None), sums | workspace, bytes
    lib.mdgen_ens_contact_counts.argtypes = [i64, i32, vp, C.c_float, vp, vp]   # F, N | ca, cutoff2, counts
    lib.mdgen_ens_sasa_workspace_bytes.argtypes = [i32, i32, C.POINTER(sz)]
    lib.mdgen_ens_sasa_counts.argtypes = [i64, i32, i32, vp, vp, vp, C.c_float, vp, vp, sz, vp]   # F, A, P | x, radius (host), points (host), probe | counts | workspace, bytes
    lib.mdgen_from_3_points.argtypes = [i64] + [vp] * 6
    lib.mdgen_path_plan.argtypes = [i64, i64, i32] + [vp] * 6
    lib.mdgen_masked_mse.argtypes = [i64, i64] + [vp] * 5
    f32 = C.c_float
    lib.mdgen_grad_sumsq.argtypes = [i64, vp, f32, vp, i32, vp, vp]
    lib.mdgen_adam_step.argtypes = [i64, vp, vp, vp, vp, i32, f32, f32, f32, f32, f32, i32, f32, vp, f32, vp]
    lib.mdgen_ema_update.argtypes = [i64, vp, vp, f32, vp]
    lib.mdgen_train_workspace_bytes.argtypes = [vp, C.POINTER(Shape), C.POINTER(sz)]
    lib.mdgen_train_num_milestones.argtypes = [vp]
    lib.mdgen_train_bind_params.argtypes = [vp, vp, C.POINTER(i64)]
    lib.mdgen_train_set_milestone_events.argtypes = [vp, C.POINTER(vp), i32]
    lib.mdgen_train_forward_backward.argtypes = (ctx_shape + [vp, vp, cond_p] + [vp, vp] + [vp, vp] + [vp, vp]   # xt, t | target, loss_mask | loss, pred | grads, offsets
                                                 + ws_bytes + [vp, sz] + [vp])   # ... | tape, bytes | stream
    for n in EXPORTS:
        getattr(lib, n)
        if n not in ("mdgen_last_error", "mdgen_ctx_weight_name"):
            getattr(lib, n).restype = i32
    if lib.mdgen_dev_build() and "MDGEN_AMD_LIB" not in os.environ:
        raise ImportError(f"{LIB_PATH} is an experiment build (csrc/dev.h switches): rebuild with `python -m mdgen_amd.build --force`")
    got = lib.mdgen_abi_version()
    if got != ABI_VERSION:   # a stale .so would take struct writes / argument lists of another layout
        raise ImportError(f"{LIB_PATH} has ABI version {got}, this package expects {ABI_VERSION}: "
                          "rebuild it with `python -m mdgen_amd.build --force`")
    return lib


lib = _load()


class MdgenError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        raise MdgenError(f"libmdgen_amd error {rc}: {lib.mdgen_last_error().decode()}")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MdgenError("mdgen_amd runs on the GPU only (no CPU fallback): got a CPU tensor")


def ptr(t, dtype=None):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        raise MdgenError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MdgenError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def cond(mask, start_rot, start_trans, end_rot, end_trans, rel7, x_cond, x_cond_mask, aatype):
    """`Cond` of contiguous device tensors (None -> NULL); fp32, the last two int64.  Keep it alive across the call that takes it."""
    f32, i64 = torch.float32, torch.int64
    return Cond(*[ptr(t, dt) for t, dt in ((mask, f32), (start_rot, f32), (start_trans, f32), (end_rot, f32), (end_trans, f32),
                                           (rel7, f32), (x_cond, f32), (x_cond_mask, i64), (aatype, i64))])


def stream_ptr(device=None):
    """hipStream_t of torch's current stream on `device` (default: the current device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device_of(t):
    """Context manager making `t`'s device current: kernels are enqueued on THAT device's current stream
    (a launch on device 0's stream with device-1 pointers faults or loses its stream dependency)."""
    return torch.cuda.device(t.device)


def launch(fn, like, *args):
    """Call a stream-taking entry point `fn(*args, stream)` on `like`'s device: that device is made current for
    the call and the launch goes on ITS current stream (centralised device guard)."""
    with torch.cuda.device(like.device):
        check(fn(*args, stream_ptr()))


def train_plan(B, T, L_, tps=False, num_layers=1, train_precision=16, weight_misalign_bytes=0):
    """`mdgen_debug_train_plan` (host only): the kernel forms of one training step of this shape (include/mdgen_amd.h)."""
    import json
    buf = C.create_string_buffer(1 << 14)
    sh = Shape(B, T, L_)
    check(lib.mdgen_debug_train_plan(C.byref(sh), int(tps), num_layers, train_precision, weight_misalign_bytes, buf, len(buf)))
    return json.loads(buf.value.decode())


RK_METHODS = {"midpoint": 1, "heun3": 2, "rk4": 3}   # include/mdgen_amd.h mdgen_sample_rk `method`
RK_STAGES = {"midpoint": 2, "heun3": 3, "rk4": 4}    # network evaluations per step


def rk_plan(method, S):
    """`mdgen_debug_rk_plan` (host only): (time rows as a uint32 numpy array of fp32 bits, row index array [S][stages])."""
    import numpy as np
    code = RK_METHODS.get(method, method)
    S = int(S)
    cap = 4 * max(S, 1) + 1
    bits = np.zeros(cap, dtype=np.uint32)
    row_of = np.zeros(4 * max(S, 1), dtype=np.int32)
    n_rows, n_st = C.c_int32(), C.c_int32()
    check(lib.mdgen_debug_rk_plan(int(code), S, bits.ctypes.data, cap, C.byref(n_rows), row_of.ctypes.data, C.byref(n_st)))
    return bits[:n_rows.value].copy(), row_of[:S * n_st.value].reshape(S, n_st.value).copy()


# include/mdgen_amd.h mdgen_sde_opts: the reference's names (path.py:53-60 spells "inccreasing-decreasing") -> codes
SDE_METHODS = {"Euler": 1, "Heun": 2}
SDE_PATHS = {"Linear": 0, "GVP": 1}
SDE_FORMS = {"constant": 0, "SBDM": 1, "sigma": 2, "linear": 3, "decreasing": 4, "inccreasing-decreasing": 5}
SDE_LAST_STEPS = {None: 0, "Mean": 1, "Tweedie": 2, "Euler": 3}


def sde_opts(sampling_method="Euler", path_type="GVP", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
             num_steps=250, sample_eps=0.0):
    """`SdeOpts` from the reference's names (`num_steps`: grid points); an unknown name raises ValueError."""
    codes = []
    for what, table, name in (("sampling_method", SDE_METHODS, sampling_method), ("path_type", SDE_PATHS, path_type),
                              ("diffusion_form", SDE_FORMS, diffusion_form), ("last_step", SDE_LAST_STEPS, last_step)):
        if name not in table:
            raise ValueError(f"{what} must be one of {list(table)}, got {name!r}")
        codes.append(table[name])
    return SdeOpts(*codes, int(num_steps), float(diffusion_norm), float(last_step_size), float(sample_eps))


def sde_plan(opts):
    """`mdgen_debug_sde_plan` (host only) -> dict: "rows" (uint32 fp32 bits), "coef" (uint32 [rows][4]: R, iV, D, G), "row_of"
    [n_points - 1][stages], "last_row" (-1: no last step) and the scalars "dt", "q", "hdt", "h", "c0", "c1" as np.float32."""
    import numpy as np
    cap = 2 * max(opts.n_points, 2) + 1
    rows = np.zeros(cap, dtype=np.uint32)
    coef = np.zeros((cap, 4), dtype=np.uint32)
    row_of = np.zeros(2 * max(opts.n_points, 2), dtype=np.int32)
    sc = np.zeros(6, dtype=np.uint32)
    n_rows, n_st, last = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.mdgen_debug_sde_plan(C.byref(opts), rows.ctypes.data, coef.ctypes.data, cap, C.byref(n_rows), row_of.ctypes.data,
                                   C.byref(n_st), C.byref(last), sc.ctypes.data))
    S = opts.n_points - 1
    out = {"rows": rows[:n_rows.value].copy(), "coef": coef[:n_rows.value].copy(),
           "row_of": row_of[:S * n_st.value].reshape(S, n_st.value).copy(), "last_row": last.value}
    out.update(zip(("dt", "q", "hdt", "h", "c0", "c1"), sc.view(np.float32)))
    return out


def philox(ctr, key):
    """`mdgen_debug_philox` (host only): Philox4x32-10 of the four counter words under the two key words -> uint32[4]."""
    import numpy as np
    c, k, out = np.asarray(ctr, dtype=np.uint32).copy(), np.asarray(key, dtype=np.uint32).copy(), np.zeros(4, dtype=np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError("philox takes four counter words and two key words")
    check(lib.mdgen_debug_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data))
    return out


def rng_words(seed, sample_base=0, block_base=0):
    """The four words {seed, sample_base, block_base, 0} of mdgen_sample_sde_rng's `rng` as an int64 CPU tensor (bit patterns of the
    unsigned words: the seed mod 2^64, the bases mod 2^32); copy it into the call's device buffer on the call's stream."""
    def signed(v, bits):
        v = int(v) % (1 << bits)
        return v - (1 << 64) if v >= 1 << 63 else v
    return torch.tensor([signed(seed, 64), signed(sample_base, 32), signed(block_base, 32), 0], dtype=torch.int64)


def sde_noise(B, T, L_, D, rng, step, block=0):
    """`mdgen_debug_sde_noise`: the (B, T, L, D) noise of stochastic step `step` of block `block` under the device words `rng`."""
    out = torch.empty(B, T, L_, D, device=rng.device)
    sh = Shape(B, T, L_)
    launch(lib.mdgen_debug_sde_noise, rng, C.byref(sh), int(D), ptr(rng, torch.int64), int(step), int(block), ptr(out))
    return out


def sde_dispatch_plan(B, T, L_, opts, tps=False, num_layers=5, ncu=256, xcd_round_robin=True, options=None):
    """`mdgen_debug_sde_dispatch_plan` (host only): `dispatch_plan`'s dict for one step of sample_sde with `opts`."""
    import json
    buf = C.create_string_buffer(1 << 14)
    sh = Shape(B, T, L_)
    o = ",".join(f"{k}={int(v)}" for k, v in (options or {}).items()).encode()
    check(lib.mdgen_debug_sde_dispatch_plan(C.byref(sh), C.byref(opts), int(tps), num_layers, ncu, int(xcd_round_robin), o, buf, len(buf)))
    return json.loads(buf.value.decode())


def dispatch_plan(B, T, L_, n_steps=1, mode=0, tps=False, num_layers=5, ncu=256, xcd_round_robin=True, options=None):
    """`mdgen_debug_dispatch_plan` (host only): {"streams", "prepare": {kernel class: launches}, "views": [{"B", "classes"}]} of a call of this shape.
    mode 0: sample_euler (product path), 1: forward, 2: sample_euler under the profiler (one stream), 3: forward with trace_h,
    4: one attempted step of sample_dopri5, 5 / 6 / 7: one midpoint / heun3 / rk4 step of sample_rk (modes 4 .. 7 add "integrator":
    {kernel class: launches})."""
    import json
    buf = C.create_string_buffer(1 << 14)
    sh = Shape(B, T, L_)
    opts = ",".join(f"{k}={int(v)}" for k, v in (options or {}).items()).encode()
    check(lib.mdgen_debug_dispatch_plan(C.byref(sh), n_steps, mode, int(tps), num_layers, ncu, int(xcd_round_robin), opts, buf, len(buf)))
    return json.loads(buf.value.decode())
