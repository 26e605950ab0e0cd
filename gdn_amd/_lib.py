"""ctypes binding of libgdn_hip.so (C ABI declared in include/gdn_hip.h).

There is NO CPU fallback: if the shared library has not been built, or a tensor is not on
a HIP device, every op raises.  Build with `python -c "import __graft_entry__ as g; g.build()"`.
"""
from __future__ import annotations

import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GDN_HIP_LIB", os.path.join(_HERE, "libgdn_hip.so"))   # override: diagnostic builds
ABI_VERSION = 23

_c_int, _c_float, _p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

# name -> argtypes (restype is always int); mirrors include/gdn_hip.h one to one
SIGNATURES = {
    "gdn_abi_version": [],
    "gdn_nbr_pitch": [_c_int],
    "gdn_topk_graph": [_p, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p],
    "gdn_graph_from_topk": [_p, _c_int, _c_int, _p, _p, _p],
    "gdn_node_terms": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _p, _p],
    "gdn_bn_fold": [_p, _p, _p, _p, _c_float, _c_int, _p, _p],
    "gdn_project_fwd": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p],
    "gdn_project_fwd_series": [_p, _c_int, _c_int, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p],
    "gdn_tile_fits": [_c_int] * 4,
    "gdn_kernel_family": [_c_int] * 6,
    "gdn_tile_forward_form": [_c_int] * 5,
    "gdn_terms_pitch": [_c_int],
    "gdn_attn_aggregate_fwd": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_head_fwd": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_head_train_fwd": [_p] * 10 + [_c_float] + [_c_int] * 3 + [_c_float] * 4 + [_p] * 9,
    "gdn_head_train_workspace_bytes": [_c_int, _c_int],
    "gdn_head_train_stats_bytes": [_c_int],
    "gdn_exact_sum_workspace_bytes": [],
    "gdn_exact_sum": [_p, _c_int, _p, _p, _p],
    "gdn_head_train_bwd": [_p] * 10 + [_c_float, _p] + [_c_int] * 3 + [_c_float] * 2 + [_p] * 10,
    "gdn_head_train_fwd_rng": [_p] * 9 + [_c_float] + [_c_int] * 3 + [_c_float] * 4 + [_p] * 8 + [_c_int, _p],
    "gdn_head_train_bwd_rng": [_p] * 9 + [_c_float, _p] + [_c_int] * 3 + [_c_float] * 2 + [_p] * 9 + [_c_int, _p],
    "gdn_head_train_fwd_act": [_p] * 8 + [_c_float, _p, _c_float] + [_c_int] * 3 + [_c_float] * 4 + [_p] * 8 + [_c_int, _p],
    "gdn_head_train_bwd_act": [_p] * 9 + [_c_float, _p, _c_float, _p] + [_c_int] * 3 + [_c_float] * 2 + [_p] * 7 + [_c_int, _p],
    "gdn_mlp_train_saved_bytes": [_c_int] * 4,
    "gdn_mlp_train_workspace_bytes": [_c_int] * 4,
    "gdn_mlp_train_fwd": [_p] * 8 + [_c_int] * 4 + [_p] * 4,
    "gdn_mlp_train_bwd": [_p] * 4 + [_c_int] * 4 + [_p] * 7,
    "gdn_mlp_eval_workspace_bytes": [_c_int] * 4,
    "gdn_mlp_eval_fwd": [_p] * 6 + [_c_int] * 4 + [_p] * 3,
    "gdn_topk_graph_terms": [_p, _c_int, _c_int, _c_int] + [_p] * 8 + [_c_int, _p, _p],
    "gdn_forward_fused_plan_keys": [_p] * 4 + [_c_int] * 7 + [_p, _p],
    "gdn_forward_fused_series_plan_keys": [_p, _c_int, _c_int] + [_p] * 3 + [_c_int] * 6 + [_p, _p],
    "gdn_attn_aggregate_bwd_uses_reverse": [_c_int] * 3,
    "gdn_head_mse_workspace_bytes": [],
    "gdn_head_train_fwd_rng_mse": [_p] * 9 + [_c_float] + [_c_int] * 3 + [_c_float] * 4 + [_p] * 12 + [_c_int, _p],
    "gdn_project_bwd_partials": [_p] * 4 + [_c_int] * 4 + [_p, _p, _p],
    "gdn_train_finish": [_p, _p] + [_c_int] * 4 + [_p] * 8 + [_c_int, _c_int] + [_p] * 4,
    "gdn_adam_step": [_p] * 5 + [_c_int] + [ctypes.c_double] * 6 + [_c_int, _c_int, _p],
    "gdn_terms_bwd_acc": [_p] * 8 + [_c_int] * 3 + [_p] * 6 + [_c_int, _p],
    "gdn_mse_workspace_bytes": [],
    "gdn_mse_loss_grad": [_p, _p, ctypes.c_longlong, _p, _p, _p, _p],
    "gdn_forward_fused": [_p] * 11 + [_c_int] * 5 + [_p, _p],
    "gdn_forward_fused_series": [_p, _c_int, _c_int] + [_p] * 10 + [_c_int] * 5 + [_p, _p],
    "gdn_mlp_plan_bytes": [_c_int] * 3,
    "gdn_mlp_plan_layer": [_p] * 6 + [_c_float] + [_c_int] * 4 + [_p, _p],
    "gdn_mlp_plan_out": [_p, _p] + [_c_int] * 3 + [_p, _p],
    "gdn_mlp_fwd": [_p, _p] + [_c_int] * 4 + [_p, _p],
    "gdn_head_mlp_fwd": [_p] * 5 + [_c_int] * 5 + [_p, _p],
    "gdn_fused_plan_bytes": [_c_int] * 5,
    "gdn_fused_plan_build": [_p] * 10 + [_c_int] * 5 + [_p, _p],
    "gdn_forward_fused_plan": [_p, _p] + [_c_int] * 6 + [_p, _p, _p],
    "gdn_forward_fused_series_plan": [_p, _c_int, _c_int, _p] + [_c_int] * 5 + [_p, _p, _p],
    "gdn_fused_plan_limit_offset": [_c_int] * 5,
    "gdn_graph_bank_order": [_p, _c_int, _c_int, _p, _p],
    "gdn_forward_fused_gated": [_p] * 12 + [_c_int] * 5 + [_p, _p],
    "gdn_forward_fused_series_gated": [_p, _p, _c_int, _c_int] + [_p] * 10 + [_c_int] * 5 + [_p, _p],
    "gdn_project_fwd_wide": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p],
    "gdn_attn_aggregate_fwd_wide": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_attn_aggregate_bwd_wide": [_p] * 8 + [_c_int] * 4 + [_p] * 6,
    "gdn_project_fwd_bf16": [_p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p, _p],
    "gdn_attn_aggregate_fwd_bf16": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_head_fwd_bf16": [_p, _p, _p, _p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_forward_fused_bf16": [_p] * 11 + [_c_int] * 5 + [_p, _p],
    "gdn_attn_aggregate_bwd": [_p] * 8 + [_c_int] * 4 + [_p] * 6,
    "gdn_attn_aggregate_bwd_workspace_bytes": [_c_int] * 4,
    "gdn_train_supported": [_c_int] * 4,
    "gdn_rev_pitch": [_c_int],
    "gdn_graph_reverse": [_p, _p, _c_int, _c_int, _p, _p, _p],
    "gdn_project_bwd_workspace_bytes": [_c_int, _c_int, _c_int],
    "gdn_project_bwd": [_p] * 4 + [_c_int] * 4 + [_p] * 5,
    "gdn_terms_bwd": [_p] * 8 + [_c_int] * 3 + [_p] * 7,
    "gdn_score_workspace_bytes": [_c_int, _c_int],
    "gdn_score_select_workspace_bytes": [_c_int, _c_int, _c_int],
    "gdn_score_keys": [_p, _p, _c_int, _c_int, _c_int, _p, _p],
    "gdn_score_select": [_p, _c_int, _c_int, _c_int, ctypes.c_longlong, _p, _p, _p],
    "gdn_score_select_paths": [_p, _c_int, _c_int, _c_int, ctypes.c_longlong, _p, _p, _p, _p],
    "gdn_score_quantiles": [_p, _p, _c_int, _c_int, _p, _p, _p],
    "gdn_score_smooth_max": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p],
    "gdn_score_smooth_topm": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _c_int, _p, _p, _p],
    "gdn_series_fill_workspace_bytes": [_c_int, _c_int],
    "gdn_series_fill": [_p] + [_c_int] * 3 + [_p] * 7,
    "gdn_score_keys_keep": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p],
    "gdn_score_smooth_max_gaps": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _p, _p, _p, _p, _p],
    "gdn_score_smooth_topm_gaps": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p, _c_int, _p, _p, _p, _p, _p],
    "gdn_attention_workspace_bytes": [_c_int] * 4,
    "gdn_attention_mean": [_p, ctypes.c_longlong, ctypes.c_longlong] + [_p] * 4 + [_c_int] * 4 + [_p, _p, _p],
    "gdn_attention_at": [_p, ctypes.c_longlong, _p, _p, _c_int, _p, _p, _p] + [_c_int] * 3 + [_p, _p],
    "gdn_windows_gather": [_p, _c_int, ctypes.c_longlong, _p, ctypes.c_longlong, _p, ctypes.c_longlong, _c_int, _c_int,
                           _p, _p, _p],
    "gdn_epoch_advance": [_p, _p, _p, ctypes.c_longlong, _p],
    "gdn_mse_batch_means": [_p, _p, ctypes.c_longlong, _c_int, ctypes.c_longlong, _p, _p, _p, _p],
    "gdn_windows_gather_gaps": [_p, _c_int, ctypes.c_longlong, _p, ctypes.c_longlong, _p, ctypes.c_longlong, _c_int,
                                _c_int, _p, _p, _p, _p, _p, _p],
    "gdn_mse_batch_means_masked": [_p, _p, _p, ctypes.c_longlong, _c_int, ctypes.c_longlong, _p, _p, _p, _p, _p],
    "gdn_mse_loss_grad_masked": [_p, _p, _p, _p, _c_int, _c_int, _p, _p, _p, _p, _p],
    "gdn_stream_state_bytes": [_c_int, _c_int],
    "gdn_stream_init": [_p, _p, ctypes.c_longlong, _c_int, _c_int, _p],
    "gdn_stream_windows": [_p, _p, _c_int, _c_int, _c_int, _c_int, _p, _p],
    "gdn_stream_score": [_p] * 5 + [_c_int] * 4 + [_p] * 4,
    "gdn_stream_advance": [_p] * 6 + [_c_int] * 5 + [_p, _p, ctypes.c_longlong, _p],
    "gdn_stream_fill": [_p, _p] + [_c_int] * 4 + [_p] * 4,
    "gdn_stream_score_gaps": [_p] * 6 + [_c_int] * 4 + [_p] * 4,
    "gdn_stream_advance_gaps": [_p] * 8 + [_c_int] * 5 + [_p, _p, ctypes.c_longlong, _p, _p],
    "gdn_stream_calib_bytes": [_c_int, _c_int],
    "gdn_stream_calib_write": [_p] * 4 + [_c_int] * 5 + [_p] * 3,
    "gdn_stream_calib_write_gaps": [_p] * 5 + [_c_int] * 5 + [_p] * 3,
    "gdn_score_keys_valid": [_p, _p, _p, _c_int, _c_int, _c_int, _p, _p],
    "gdn_score_key_counts": [_p, _c_int, _c_int, _c_int, _p, _p],
    "gdn_score_select_counts": [_p, _c_int, _c_int, _c_int, _p, _c_int, _p, _p, _p, _p],
    "gdn_stream_calib_write_sensor": [_p] * 5 + [_c_int] * 5 + [_p] * 3,
    "gdn_prep_stats_workspace_bytes": [ctypes.c_longlong, _c_int],
    "gdn_prep_stats": [_p, ctypes.c_longlong, _c_int, _c_int, _p, _p, _p],
    "gdn_prep_series": [_p, ctypes.c_longlong, _c_int, _c_int, _p, _p, _c_int, _p, _p, _p, _p],
    "gdn_prep_ticks": [_p, _c_int, _c_int, _p, _c_int, _p, _c_int, _c_int, _p, _p, _c_int, _p],
    "gdn_episodes_workspace_bytes": [ctypes.c_longlong, ctypes.c_longlong],
    "gdn_episodes_scan": [_p, _p, ctypes.c_longlong, _c_int, ctypes.c_double, ctypes.c_double, _c_int, _c_int,
                          ctypes.c_longlong, ctypes.c_longlong] + [_p] * 10,
    "gdn_episodes_scan_grid": [_p, _p, ctypes.c_longlong, _c_int, ctypes.c_double, ctypes.c_double, _c_int, _c_int,
                               ctypes.c_longlong, ctypes.c_longlong] + [_p] * 9 + [_c_int, _p],
    "gdn_stream_events_bytes": [_c_int, ctypes.c_longlong],
    "gdn_stream_events": [_p] * 5 + [_c_int] * 5 + [ctypes.c_longlong, _p, _p],
    "gdn_alarm_sweep": [_p, _p, ctypes.c_longlong, _p, _p, _p, _p, ctypes.c_longlong, _p, _p],
    "gdn_fleet_state_bytes": [_c_int] * 3,
    "gdn_fleet_init": [_p, _p, ctypes.c_longlong, _c_int, _c_int, _c_int, _p],
    "gdn_fleet_windows": [_p] * 3 + [_c_int] * 4 + [_p, _p],
    "gdn_fleet_score": [_p] * 6 + [_c_int] * 5 + [_p] * 4,
    "gdn_fleet_advance": [_p] * 7 + [_c_int] * 5 + [_p, _p, ctypes.c_longlong, _p],
    "gdn_fleet_fill": [_p] * 3 + [_c_int] * 4 + [_p] * 4,
    "gdn_fleet_score_gaps": [_p] * 7 + [_c_int] * 5 + [_p] * 4,
    "gdn_fleet_advance_gaps": [_p] * 9 + [_c_int] * 5 + [_p, _p, ctypes.c_longlong, _p, _p],
    "gdn_fleet_events_bytes": [_c_int, _c_int, ctypes.c_longlong],
    "gdn_fleet_events": [_p] * 6 + [_c_int] * 7 + [ctypes.c_longlong, _p, _p],
    "gdn_fleet_calib_bytes": [_c_int] * 3,
    "gdn_fleet_calib_write": [_p] * 5 + [_c_int] * 6 + [_p] * 3,
    "gdn_fleet_calib_write_gaps": [_p] * 6 + [_c_int] * 6 + [_p] * 3,
    "gdn_fleet_calib_write_sensor": [_p] * 6 + [_c_int] * 6 + [_p] * 3,
    "gdn_fleet_ring_counts": [_p, _p, _c_int, _c_int, _c_int, _p, _p, _p],
    "gdn_fleet_ring_threshold_bytes": [_c_int, _c_int],
    "gdn_fleet_ring_threshold": [_p] * 5 + [_c_int] * 5 + [ctypes.c_double, _c_int] + [_p] * 8,
    "gdn_fleet_prep_bytes": [_c_int] * 3,
    "gdn_fleet_prep_ticks": [_p, _c_int, _c_int, _p, _p] + [_c_int] * 4 + [_p] * 4,
    "gdn_fleet_prep_ticks_units": [_p, _c_int, _c_int, _p, _p] + [_c_int] * 4 + [_p] * 4,
    "gdn_fleet_series_keys": [_p] * 4 + [_c_int] * 4 + [_p, _p],
    "gdn_fleet_series_smooth_max": [_p] * 3 + [_c_int] * 3 + [_p] * 3,
    "gdn_fleet_series_smooth_topm": [_p] * 3 + [_c_int] * 4 + [_p] * 3,
    "gdn_fleet_series_smooth_max_gaps": [_p] * 3 + [_c_int] * 3 + [_p] * 4,
    "gdn_fleet_series_smooth_topm_gaps": [_p] * 3 + [_c_int] * 4 + [_p] * 4,
}

# gdn_kernel_family's enums (include/gdn_hip.h "route table")
FAMILY_NONE, FAMILY_DENSE, FAMILY_TILE, FAMILY_LARGE, FAMILY_LONG, FAMILY_ANY = range(6)
STAGE_PROJECT, STAGE_AGGREGATE, STAGE_ATTN_BWD, STAGE_PROJECT_BWD, STAGE_TERMS, STAGE_HEAD, STAGE_FUSED = range(7)
ROUTE_WIDE, ROUTE_BF16, ROUTE_SERIES = 1, 2, 4


@functools.lru_cache(maxsize=None)      # a constant of the process per shape: eager callers ask on every launch
def family(stage: int, n: int, w: int, d: int, k: int, flags: int = 0) -> int:
    """The kernel family the library runs `stage` with at this shape (gdn_kernel_family, host only)."""
    return load().gdn_kernel_family(stage, n, w, d, k, flags) & 0xff


ERRORS = {-1: "GDN_ERR_ARG (null pointer or non-positive dimension)",
          -2: "GDN_ERR_LAUNCH (HIP launch failed)",
          -3: "GDN_ERR_UNSUPPORTED (shape outside the supported set, see include/gdn_hip.h)"}

_lib = None


class GdnHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the library once; raise loudly when it is missing or from another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GdnHipError(
            f"{LIB_PATH} not found: the HIP extension is not built and gdn_amd has no CPU "
            "fallback. Run `python -c \"import __graft_entry__ as g; g.build()\"` (needs hipcc).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = ctypes.c_longlong if name.endswith(("_bytes", "_offset")) else _c_int
    if lib.gdn_abi_version() != ABI_VERSION:
        raise GdnHipError(f"ABI mismatch: library {lib.gdn_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise GdnHipError(f"{name} failed: {ERRORS.get(rc, rc)}")
