"""ctypes binding of libxde_hip.so (C ABI: include/xde_hip.h).

The library is the product's only compute path.  There is NO CPU fallback: if the shared
object is missing, or a tensor is not on a ROCm device, the calls below raise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref

import torch

XDE_OK, XDE_EBADARG, XDE_EHIP, XDE_ETIMEOUT = 0, 1, 2, 3
XDE_MIRROR_SLOTS = 16
ABI_VERSION = 6
XDE_F32, XDE_F64 = 0, 1
XDE_MAX_K, XDE_MAX_SEG, XDE_MAX_STAGE = 14, 16, 13
XDE_MAX_PACK = 64
XDE_BP_MAX_X = XDE_MAX_K + 2  # operands of one xde_stage_cotangent launch
XDE_ROWS_MAX_K = 7  # operands of one xde_rows_* launch (include/xde_hip_rows.h)
XDE_P2P_MAX_RANKS, XDE_P2P_HANDLE_BYTES = 16, 64
COMBINE_RK, COMBINE_FUSE, COMBINE_WFUSE = 0, 1, 2
NORM_RMS, NORM_LINF = 0, 1
HISTORY_METHODS = {"cubic": 0, "linear": 1, "bez": 2}
STATUS_OK, STATUS_DT_UNDERFLOW, STATUS_NONFINITE, STATUS_MAX_STEPS = 0, 1, 2, 3
KID_NAMES = ("combine", "errnorm", "control", "dense", "scalednorm", "finalize", "commit", "combine_fuse", "combine_wfuse")

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libxde_hip.so")


class XdeCtrl(C.Structure):
    """xde_ctrl_t"""

    _fields_ = [
        ("t0", C.c_double),
        ("t1", C.c_double),
        ("dt", C.c_double),
        ("dt_last", C.c_double),
        ("t_plan", C.c_double),
        ("ratio_prev", C.c_double),
        ("ratio", C.c_double),
        ("ratio_seg", C.c_double * XDE_MAX_SEG),
        ("nonfinite", C.c_double),
        ("n_steps", C.c_int64),
        ("n_accept", C.c_int64),
        ("n_reject", C.c_int64),
        ("steps_in_interval", C.c_int64),
        ("accept", C.c_int32),
        ("sel_used", C.c_int32),
        ("status", C.c_int32),
        ("out_begin", C.c_int32),
        ("out_end", C.c_int32),
        ("next_out", C.c_int32),
        ("n_out", C.c_int32),
        ("done", C.c_int32),
        ("next_step_index", C.c_int32),
        ("on_step_t", C.c_int32),
        ("seq", C.c_int64),
        ("chk", C.c_uint64),
        ("reserved", C.c_int32 * 2),
    ]


class XdeCtrlParams(C.Structure):
    """xde_ctrl_params_t"""

    _fields_ = [
        ("struct_size", C.c_uint32),  # the binding's statement of the layout: checked by the library before anything else is read
        ("abi_version", C.c_uint32),
        ("rtol", C.c_double),
        ("atol", C.c_double),
        ("min_step", C.c_double),
        ("max_step", C.c_double),
        ("safety", C.c_double),
        ("ifactor", C.c_double),
        ("dfactor", C.c_double),
        ("order", C.c_double),
        ("max_num_steps", C.c_int64),
        ("time_dtype", C.c_int32),
        ("state_dtype", C.c_int32),
        ("direction", C.c_int32),
        ("norm_kind", C.c_int32),
        ("n_stage", C.c_int32),
        ("n_seg", C.c_int32),
        ("n_step_t", C.c_int32),
        ("pi_controller", C.c_int32),
        ("pi_beta", C.c_double),
        ("alpha", C.c_double * XDE_MAX_STAGE),
        ("seg_count", C.c_double * XDE_MAX_SEG),
        ("replay", C.c_void_p),
        ("n_replay", C.c_int64),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))
        self.abi_version = ABI_VERSION


class XdeSegments(C.Structure):
    """xde_segments_t"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_seg", C.c_int32),
        ("seg_start", C.c_int64 * XDE_MAX_SEG),
        ("seg_len", C.c_int64 * XDE_MAX_SEG),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))


class XdeError(RuntimeError):
    pass


_vp, _dp, _i32, _i64, _dbl = C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int64, C.c_double
_vpp, _params, _segs = C.POINTER(C.c_void_p), C.POINTER(XdeCtrlParams), C.POINTER(XdeSegments)

# header of include/ -> {symbol: (restype, argtypes)} of the entry points it declares; argtypes None: not declared (the zero-argument
# queries).  _bind declares the tables in this order, so a library that lacks a header's kernels is refused by that header's first
# symbol.  A new header is one more entry here and nothing else: tests/test_cabi_headers.py holds every table to its header.
HEADERS = {}
# the solvers' kernels, the control block and its host mirror, dense output, history, the peer-to-peer exchange, the profiler
HEADERS["xde_hip.h"] = {
    "xde_last_error": (C.c_char_p, []),
    "xde_abi_version": (_i32, None),
    "xde_sizeof_ctrl": (_i64, None),
    "xde_sizeof_ctrl_params": (_i64, None),
    "xde_sizeof_segments": (_i64, None),
    "xde_workspace_bytes": (_i64, None),
    "xde_stage_combine": (_i32, [_vp, _vp, _vp, _vpp, _vp, _dp, _i32, _i32, _dbl, _dbl, _vp, _i64, _i32, _vp, _dp, _dbl, C.c_uint32, _vp]),
    "xde_stage_combine_pre": (_i32, [_vp, _vp, _vp, _vp, _vpp, _dp, _i32, _dbl, _vp, _i64, _i32, C.c_uint32, _vp]),
    "xde_stage_combine_pre_weighted": (_i32, [_vp, _vp, _vp, _vpp, _dp, _i32, _dbl, _dbl, _vp, _i64, _i32, _dbl, _vp]),
    "xde_error_norm_partial": (_i32, [_vpp, _vp, _dp, _i32, _vp, _vp, _vp, _dbl, _dbl, _dbl, _vp, _segs, _i32, _i32, _vp, _vp, _vp]),
    "xde_error_norm_control": (_i32, [_vpp, _vp, _dp, _i32, _vp, _vp, _vp, _segs, _i32, _vp, _vp, _vp, _params, _vp, _vp, _vp, _vp, _vp]),
    "xde_error_ratio": (_i32, [_vp, _vpp, _vp, _dp, _i32, _vp, _vp, _vp, _dbl, _dbl, _dbl, _vp, _i64, _i32, _vp, _vp]),
    "xde_scaled_norm_partial": (_i32, [_vp, _vp, _vp, _dbl, _dbl, _segs, _i32, _i32, _vp, _i32, _vp]),
    "xde_norm_finalize": (_i32, [_vp, _i32, _vp, _vp]),
    "xde_norm_result": (_i32, [_vp, _dp, _i32, _i32, _i32, _vp, _vp]),
    "xde_rk_control": (_i32, [_vp, _params, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xde_ctrl_init": (_i32, [_vp, _params, _dbl, _dbl, C.c_int32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "xde_ctrl_retarget": (_i32, [_vp, _params, _vp, C.c_int32, _vp, _vp]),
    "xde_initial_step": (_i32, [_i32, _vp, _vp, _params, _dbl, _vp, _i32, _vp, _vp]),
    "xde_initial_step_fused": (_i32, [_i32, _vp, _vp, _vp, _segs, _i32, _vp, _params, _dbl, _vp, _i32, _vp, C.c_int32, _vp, _vp, _vp, _i64,
                                      _vp]),
    "xde_scaled_norm2_partial": (_i32, [_vp, _vp, _dbl, _dbl, _segs, _i32, _i32, _vp, _vp]),
    "xde_initial_step_tail": (_i32, [_i32, _vp, _vp, _params, _dbl, _vp, _i32, _vp, C.c_int32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "xde_ctrl_read": (_i32, [_vp, C.POINTER(XdeCtrl), _vp]),
    "xde_host_alloc": (_i32, [_i64, C.POINTER(C.c_void_p)]),
    "xde_host_free": (_i32, [_vp]),
    "xde_ctrl_wait": (_i32, [_vp, _i64, _dbl, C.POINTER(XdeCtrl)]),
    "xde_dense_eval": (_i32, [_vp, _vpp, _vp, _dp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i64, _vp]),
    "xde_commit": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "xde_pack_segments": (_i32, [_vp, _vpp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp, _i32, _i64, _i32, _vp]),
    "xde_dense_commit": (_i32, [_vp, _vpp, _dp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp]),
    "xde_hermite_gather": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "xde_history_gather": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "xde_lag_grad_workspace_bytes": (_i64, [_i32]),
    "xde_lag_grad": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "xde_scale_fanout": (_i32, [_vpp, _vp, _dp, _i32, _vp, _i64, _i32, _vp]),
    "xde_graph_replace_memsets": (_i32, [_vp, C.POINTER(C.c_int)]),
    "xde_p2p_mailbox_bytes": (_i64, None),
    "xde_p2p_alloc": (_i32, [C.POINTER(C.c_void_p)]),
    "xde_p2p_free": (_i32, [_vp]),
    "xde_p2p_export": (_i32, [_vp, _vp]),
    "xde_p2p_import": (_i32, [_vp, C.POINTER(C.c_void_p)]),
    "xde_p2p_close": (_i32, [_vp]),
    "xde_p2p_exchange": (_i32, [_vp, _vp, _vpp, _i32, _i32, _i32, _i64, _vp]),
    "xde_p2p_error": (_i32, [_vp, C.POINTER(C.c_int64), _vp]),
    "xde_p2p_error_info": (_i32, [_vp, C.POINTER(C.c_int64), _i32, _vp]),
    "xde_p2p_rk_control": (_i32, [_vp, _params, _vp, _vp, _vpp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp]),
    "xde_prof_enable": (_i32, [_i32]),
    "xde_prof_collect": (_i32, [C.POINTER(C.c_int64), _dp, _dp]),
}
# back-propagation through the accepted steps of an adaptive solve
HEADERS["xde_hip_backprop.h"] = {
    "xde_stage_cotangent": (_i32, [_vp, _vp, _vpp, _dp, _dp, _i32, _i64, _i32, _vp]),
    "xde_dense_cotangent": (_i32, [_vpp, _vp, _dp, _i32, C.c_uint32, _i64, _i32, _vp]),
}
# the fixed-step solvers' sub-stepping
HEADERS["xde_hip_grid.h"] = {
    "xde_interp_rows": (_i32, [_vpp, C.POINTER(C.c_int), _dp, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp]),
}
# sdeint's Euler-Maruyama, Milstein, SRK and reversible Heun steps
HEADERS["xde_hip_sde.h"] = {
    "xde_sde_em_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_em_backward": (_i32, [_vp, _vp, _vp, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_noise": (_i32, [_vp, _i64, C.c_uint64, _i64, _i32, _i32, _vp]),
    "xde_sde_milstein_support": (_i32, [_vp, _vp, _vp, _vp, _i64, _dbl, _dbl, _i32, _vp]),
    "xde_sde_milstein_support_backward": (_i32, [_vp, _vp, _vp, _i64, _dbl, _dbl, _i32, _vp]),
    "xde_sde_milstein_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_milstein_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_srk_stage1": (_i32, [_vp] * 6 + [_i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_srk_stage2": (_i32, [_vp] * 6 + [_i64, _dbl, _dbl, _i32, _vp]),
    "xde_sde_srk_step": (_i32, [_vp] * 8 + [_i64, _dbl, _dbl, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_srk_stage1_backward": (_i32, [_vp] * 6 + [_i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_srk_stage2_backward": (_i32, [_vp] * 5 + [_i64, _dbl, _dbl, _i32, _vp]),
    "xde_sde_srk_step_backward": (_i32, [_vp] * 7 + [_i64, _dbl, _dbl, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_noise_draw": (_i32, [_vp, _i64, C.c_uint64, _i64, _i32, _i32, _i32, _vp]),
    "xde_sde_rheun_predict": (_i32, [_vp] * 5 + [_i64, _dbl, _dbl, _i32, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_rheun_correct": (_i32, [_vp] * 6 + [_i64, _dbl, _dbl, _i32, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_rheun_adjoint_stage": (_i32, [_vp] * 5 + [_i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_rheun_adjoint_step": (_i32, [_vp] * 7 + [_i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
}


class XdeCdePlan(C.Structure):
    """Mirror of xde_cde_plan_t (include/xde_hip_cde.h)."""

    _fields_ = [(name, C.c_int32) for name in ("vec", "lds", "grouped", "R", "single", "S", "Hc", "Gb", "rows_per_pass", "nt")] + [
        ("items", C.c_int64), ("blocks", C.c_int64)]


# cdeint's control-derivative contraction and its cotangent
HEADERS["xde_hip_cde.h"] = {
    "xde_cde_contract": (_i32, [_vp] * 5 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_contract_backward": (_i32, [_vp] * 5 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_plan": (_i32, [_i32, _vp, _i64, _i32, _i32, _i32, C.POINTER(XdeCdePlan)]),
}


class XdeSeamPlan(C.Structure):
    """Mirror of xde_seam_plan_t (include/xde_hip_seam.h)."""

    _fields_ = [(name, C.c_int32) for name in ("blocks", "per_lane", "resident", "fits")]


# error norm + controller + next first stage combine as one resident launch
HEADERS["xde_hip_seam.h"] = {
    "xde_seam_state_bytes": (_i64, None),
    "xde_seam_plan": (_i32, [_i64, _i32, C.POINTER(XdeSeamPlan)]),
    "xde_seam_attempt": (_i32, [_vp, _dbl] + [_vp] * 7 + [_dbl, _i64, _i32, _vp, _vp, _vp, _params, _vp, _vp, _vp, _vp, _i64, _vp]),
    "xde_seam_expired": (_i32, [_vp, C.POINTER(C.c_int64), _vp]),
}
# the natural cubic spline control: coefficient build, gather, and the two contraction launches on it
HEADERS["xde_hip_spline.h"] = {
    "xde_spline_natural_coeffs": (_i32, [_vp] * 4 + [_i64, _i32, _i32, _i32, _vp]),
    "xde_spline_natural_gather": (_i32, [_vp] * 6 + [_i64, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_contract_natural": (_i32, [_vp] * 6 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_contract_natural_backward": (_i32, [_vp] * 6 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _vp]),
}


class XdeCdeGradPlan(C.Structure):
    """Mirror of xde_cdegrad_plan_t (include/xde_hip_cdegrad.h)."""

    _fields_ = [(name, C.c_int32) for name in ("vec", "P", "CL", "chunks", "rows", "strided")] + [("blocks", C.c_int64)]


# the gradient of cdeint with respect to its control path: the control's cotangent in the contraction, the transposes of the natural
# spline's coefficient build and gather
HEADERS["xde_hip_cdegrad.h"] = {
    "xde_cde_control_grad": (_i32, [_vp] * 5 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_control_grad_natural": (_i32, [_vp] * 6 + [_dbl, _i32, _i64, _i32, _i32, _i32, _i32, _vp]),
    "xde_cde_control_grad_plan": (_i32, [_vp, _i64, _i32, _i32, _i32, C.POINTER(XdeCdeGradPlan)]),
    "xde_spline_natural_coeffs_backward": (_i32, [_vp] * 6 + [_i64, _i32, _i32, _i32, _vp]),
    "xde_spline_natural_coeffs_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "xde_spline_natural_gather_backward": (_i32, [_vp] * 6 + [_i64, _i32, _i32, _i32, _i32, _vp]),
}
# the KL term of a latent SDE fused into the Euler-Maruyama step, and its cotangents
HEADERS["xde_hip_kl.h"] = {
    "xde_sde_kl_step": (_i32, [_vp] * 7 + [_i64, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_kl_backward": (_i32, [_vp] * 8 + [_i64, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
}
# per-sample output times of a joint adaptive solve: every row's own queries from the dense output of a step, and their cotangent
# (the newest table; it sits here because the order of the tables after it is pinned by their own tests)
HEADERS["xde_hip_teval.h"] = {
    "xde_teval_dense": (_i32, [_vp, _vp, _vp, _vpp, _dp, _i32, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _i32, _i32, _i64, _i64, _i64, _i32, _vp]),
    "xde_teval_cotangent": (_i32, [_vpp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _i32, _i32, C.c_uint32, _i64, _i64, _i64, _i32, _vp]),
}
# the Euler-Maruyama step with general or scalar noise, and its cotangents
HEADERS["xde_hip_gn.h"] = {
    "xde_sde_gn_step": (_i32, [_vp] * 4 + [_i64, _i64, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
    "xde_sde_gn_backward": (_i32, [_vp] * 3 + [_i64, _i64, _i64, _dbl, _dbl, C.c_uint64, _i64, _i32, _vp]),
}
# ddeint_steps: the delayed states of one stage from the Hermite tape of the solution, and the fan of their cotangent into its nodes
HEADERS["xde_hip_dde.h"] = {
    "xde_dde_tape_gather": (_i32, [_vp, _vp, _vpp, C.POINTER(C.c_int64), _dp, _dp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "xde_dde_tape_gather_backward": (_i32, [_vpp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _i32, _vp, _i64, _i64, _i32, _i32, _i32,
                                            _vp]),
}


class XdeRowsCtl(C.Structure):
    """Mirror of xde_rows_ctl_t (include/xde_hip_rows.h): the planes of the per-row control block."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(name, C.c_void_p) for name in (
        "t", "t_prev", "h", "h_used", "ratio", "nonfinite", "accept", "done", "status", "next_out", "n_accept", "n_reject",
        "steps_in_interval", "t_stage")]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))


_rows_ctl = C.POINTER(XdeRowsCtl)
# per-sample adaptive stepping: every row of the batch its own step
HEADERS["xde_hip_rows.h"] = {
    "xde_rows_stage_combine": (_i32, [_vp, _vp, _vp, _vpp, _dp, _dp, _i32, _rows_ctl, _i64, _i64, _i32, _vp]),
    "xde_rows_norm_control": (_i32, [_vpp, _dp, _i32, _vp, _vp, _vp, _rows_ctl, _params, _vp, C.c_int32, _i64, _i64, _i32, _vp]),
    "xde_rows_dense_commit": (_i32, [_vp, _vpp, _dp, _i32, _vp, _vp, _vp, _vp, _rows_ctl, _params, _vp, C.c_int32, _i64, _i64, _i32, _vp]),
    "xde_rows_scaled_norm": (_i32, [_vp, _vp, _vp, _vp, _dbl, _dbl, _i64, _i64, _i32, _vp]),
}
# logsignature windows: the depth-2 log-ODE control of cdeint, and its cotangent
HEADERS["xde_hip_logsig.h"] = {
    "xde_logsig_channels": (_i64, [_i64, _i32]),
    "xde_logsig_windows": (_i32, [_vp] * 2 + [_i64, _i64, _i64, _i64, _i32, _i32, _vp]),
    "xde_logsig_windows_backward": (_i32, [_vp] * 3 + [_i64, _i64, _i64, _i64, _i32, _i32, _vp]),
}
PROTOTYPES = {sym: proto for table in HEADERS.values() for sym, proto in table.items()}
XDE_INTERP_MAX_ROWS = 8
XDE_INTERP_LINEAR, XDE_INTERP_CUBIC = 0, 1
XDE_ROW_INTERP, XDE_ROW_COPY_A, XDE_ROW_COPY_B = 0, 1, 2
XDE_NOISE_NORMAL, XDE_NOISE_BITS = 0, 1
XDE_DDE_MAX_LAGS = 16  # delays of one xde_dde_tape_gather launch (include/xde_hip_dde.h)


class RowsCtl:
    """The per-row control block of a per-sample solve (xde_rows_ctl_t): two tensors of planes and the stage times, with the
    struct of their addresses the entry points take.  Allocated by torch on the state's device."""

    F64 = ("t", "t_prev", "h", "h_used", "ratio", "nonfinite")
    I32 = ("accept", "done", "status", "next_out", "n_accept", "n_reject", "steps_in_interval")

    def __init__(self, rows, n_stage, state_dtype, device):
        self.rows = int(rows)
        self.f64 = torch.zeros(len(self.F64), self.rows, dtype=torch.float64, device=device)
        self.i32 = torch.zeros(len(self.I32), self.rows, dtype=torch.int32, device=device)
        self.t_stage = torch.zeros(int(n_stage), self.rows, dtype=state_dtype, device=device)
        self.c = XdeRowsCtl()
        for i, name in enumerate(self.F64):
            setattr(self, name, self.f64[i])
            setattr(self.c, name, self.f64[i].data_ptr())
        for i, name in enumerate(self.I32):
            setattr(self, name, self.i32[i])
            setattr(self.c, name, self.i32[i].data_ptr())
        self.c.t_stage = self.t_stage.data_ptr()


class _Work:
    """The small per-solve device buffers of an adaptive solver."""

    __slots__ = ("key", "ctrl", "ws", "sums", "t_stage", "t_views")


# torch's C-level accessor of the current stream handle: ~0.3 us against ~4 us for torch.cuda.current_stream().cuda_stream
# (a Stream object is built each time); every launch needs the handle
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(device):
    """Raw hipStream_t of torch's current stream on the ROCm ``device`` (a key of the per-stream caches)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _raw_stream(idx) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream


_lib = None
_lib_lock = threading.Lock()


_REBUILD = "rebuild it with `python -m paddlexde_amd.csrc.build --force`"


def _declare(lib, sym):
    proto = PROTOTYPES[sym]
    try:
        fn = getattr(lib, sym)
    except AttributeError:
        raise XdeError("libxde_hip.so does not export {}: it is stale or not this project's build; {}".format(sym, _REBUILD)) from None
    fn.restype = proto[0]
    if proto[1] is not None:
        fn.argtypes = proto[1]
    return fn


def _bind(lib):
    """Declare every prototype on ``lib``: first that it is the ABI this binding speaks, then the struct layouts, then every entry
    point of HEADERS in table order."""
    _declare(lib, "xde_last_error")
    version = _declare(lib, "xde_abi_version")()
    if version != ABI_VERSION:
        raise XdeError("libxde_hip.so ABI version mismatch: the library is version {}, this binding is version {}; {}".format(
            version, ABI_VERSION, _REBUILD))
    if _declare(lib, "xde_sizeof_ctrl")() != C.sizeof(XdeCtrl):
        raise XdeError("xde_ctrl_t layout mismatch between header and ctypes mirror")
    if _declare(lib, "xde_sizeof_ctrl_params")() != C.sizeof(XdeCtrlParams):
        raise XdeError("xde_ctrl_params_t layout mismatch between header and ctypes mirror")
    if _declare(lib, "xde_sizeof_segments")() != C.sizeof(XdeSegments):
        raise XdeError("xde_segments_t layout mismatch between header and ctypes mirror")
    for sym in PROTOTYPES:
        _declare(lib, sym)


def load_library():
    """dlopen libxde_hip.so and declare prototypes.  Raises if it has not been built, or is not the library this binding speaks to."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise XdeError(
                "paddlexde_amd: {} is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python -m paddlexde_amd.csrc.build`. There is no CPU fallback.".format(LIB_PATH)
            )
        lib = C.CDLL(LIB_PATH)
        _bind(lib)
        _lib = lib
    return _lib


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return XDE_F32
    if dt == torch.float64:
        return XDE_F64
    raise TypeError("paddlexde_amd kernels support float32 and float64 states, got {}".format(dt))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _require_alike(who, what, like, tensors):
    """Refuse a tensor of ``tensors`` (``what`` they are, to ``who``) that is not contiguous or not of ``like``'s shape and dtype; None
    stands for a null pointer and is not checked."""
    for x in tensors:
        if x is not None and (not x.is_contiguous() or x.shape != like.shape or x.dtype != like.dtype):
            raise XdeError("{}: the {} must be contiguous tensors of one shape and dtype".format(who, what))


_LOGSIG_MAX_CHANNELS = 512


def logsig_channels(channels, depth):
    """K of include/xde_hip_logsig.h (what its channel query answers): ``channels`` at depth 1, ``channels + channels (channels - 1) / 2``
    at depth 2; the caps are refused here, before any launch."""
    channels, depth = int(channels), int(depth)
    if depth not in (1, 2):
        raise ValueError("logsignature depth {} is not built: depth 1 (increments) and depth 2 (increments and Levy areas) are".format(depth))
    if not 1 <= channels <= _LOGSIG_MAX_CHANNELS:
        raise ValueError("logsignature windows take 1 <= C <= {} channels, got {}".format(_LOGSIG_MAX_CHANNELS, channels))
    return channels if depth == 1 else channels + channels * (channels - 1) // 2


def _plan_dict(plan):
    """A launch plan (the mirror of one of the headers' ``xde_*_plan_t``) as a dict of its fields."""
    return {name: int(getattr(plan, name)) for name, _ in plan._fields_}


def _dbl_array(xs):
    if isinstance(xs, C.Array):  # pre-marshalled by the caller (per-stage coefficient rows never change)
        return xs
    return (C.c_double * len(xs))(*[float(x) for x in xs])


dbl_array = _dbl_array


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def make_segments(segs) -> XdeSegments:
    s = XdeSegments()
    s.n_seg = len(segs)
    for i, (start, length) in enumerate(segs):
        s.seg_start[i] = int(start)
        s.seg_len[i] = int(length)
    return s


class HipBackend:
    """The production backend: every method enqueues one kernel of libxde_hip.so on torch's current stream."""

    name = "hip"

    WAIT_TIMEOUT_MS = 600e3

    def __init__(self):
        self.lib = load_library()
        self._mirror_pool = []  # pinned host mirror rings, reused across solver instances
        self._mirrors = {}  # device ctrl pointer -> _Mirror
        self._work_pool = {}  # (device, state dtype, stream) -> free _Work sets
        self._seam_states = {}  # device ctrl pointer -> barrier state of xde_seam_attempt (zeroed once; tags only grow)
        self._lag_ws = {}  # (device, L, stream) -> workspace of xde_lag_grad (zeroed once; every launch leaves it re-armed)
        self._tls = threading.local()  # .capturing: this THREAD is recording a hipGraph (its launches do not execute)
        # (the init block can ride the mirror only under the checksummed publish protocol, XDE_CTRL_FLAGS bit 8 — the default)
        self._mirror_takes_init = (int(os.environ.get("XDE_CTRL_FLAGS", "15")) & 8) != 0

    # -- host mirror ring of the control block (see xde_rk_control / xde_ctrl_wait) -------------
    class _Mirror:
        __slots__ = ("ptr", "seq", "seq0", "peek", "init_published")

        def __init__(self, ptr):
            self.ptr, self.seq, self.seq0 = ptr, 0, 0
            self.init_published = False  # the block the solve started from is in slot seq0 of the ring (initial_step_tail)
            self.peek = None  # ctrl_peek_async's pool of idle (pinned buffer, event, device) triples

    def _acquire_mirror(self):
        if self._mirror_pool:
            m = self._mirror_pool.pop()
            m.seq0 = m.seq  # nothing published for the new owner yet: ctrl_read falls back to a device copy
            m.init_published = False
            return m
        ptr = C.c_void_p()
        self._check(self.lib.xde_host_alloc(XDE_MIRROR_SLOTS * C.sizeof(XdeCtrl), C.byref(ptr)), "xde_host_alloc")
        return HipBackend._Mirror(ptr.value)

    def _release_mirror(self, key):
        m = self._mirrors.pop(key, None)
        if m is not None:
            self._mirror_pool.append(m)

    # -- helpers -------------------------------------------------------------------------
    def _is_capturing(self):
        """True while THIS thread records a hipGraph through capture(): controller launches recorded there do not run, so
        they must not advance the host's sequence number; other threads' launches do run and are counted as usual."""
        return getattr(self._tls, "capturing", False)

    def _check(self, rc, who):
        if rc != XDE_OK:
            raise XdeError("{} failed (status {}): {}".format(who, rc, self.lib.xde_last_error().decode()))

    def require_device(self, *tensors):
        self._require_device(*tensors)

    @staticmethod
    def _require_device(*tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise XdeError(
                    "paddlexde_amd: tensors must live on a ROCm device (got device={}); there is no CPU path".format(t.device)
                )

    @staticmethod
    def _stream(t):
        """Raw hipStream_t of torch's current stream on the tensor's device (the launch stream of every kernel)."""
        if _raw_stream is not None:
            return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
        return torch.cuda.current_stream(t.device).cuda_stream

    # -- allocation (torch is the allocator; the library never allocates) -------------------
    def new_ctrl(self, device):
        t = torch.zeros(C.sizeof(XdeCtrl), dtype=torch.uint8, device=device)
        key = t.data_ptr()
        self._mirrors[key] = self._acquire_mirror()
        weakref.finalize(t, self._release_mirror, key)
        return t

    def new_workspace(self, device):
        return torch.zeros(int(self.lib.xde_workspace_bytes()), dtype=torch.uint8, device=device)

    # The small per-solve device buffers (control block + mirror, norm workspace, sums, stage times) are recycled between
    # solver instances on the same device and stream: odeint_adjoint's backward builds one solver per output interval, and
    # four allocations + fills each time are a measurable part of a launch-bound solve.  Reuse is stream-ordered.
    def acquire_work(self, device, state_dtype):
        key = (device.index, state_dtype, stream_of(device))
        pool = self._work_pool.setdefault(key, [])
        if pool:
            return pool.pop()
        w = _Work()
        w.key = key
        w.ctrl = self.new_ctrl(device)
        w.ws = self.new_workspace(device)
        w.sums = self.new_sums(device)
        w.t_stage = torch.zeros(XDE_MAX_STAGE, dtype=state_dtype, device=device)
        w.t_views = [w.t_stage[i] for i in range(XDE_MAX_STAGE)]  # the 0-dim stage times handed to func (made once per work set)
        return w

    def release_work(self, w):
        pool = self._work_pool.setdefault(w.key, [])
        if len(pool) < 8:
            pool.append(w)

    def new_sums(self, device):
        return torch.zeros(2 * XDE_MAX_SEG, dtype=torch.float64, device=device)

    # -- kernels ---------------------------------------------------------------------------
    def stage_combine(self, out, y0, ks, coef, mode, *, scale=1.0, dt_host=0.0, ctrl=None, y0_alt=None, k0_alt=None,
                      out2=None, coef2=None, damping=0.0, nt_mask=0):
        self._require_device(out, y0, out2, *ks)
        if out.numel() == 0:
            return
        rc = self.lib.xde_stage_combine(
            out.data_ptr(), y0.data_ptr(), _ptr(y0_alt), _ptr_array(ks), _ptr(k0_alt), _dbl_array(coef), len(ks),
            mode, float(scale), float(dt_host), _ptr(ctrl), out.numel(), dtype_code(out.dtype), _ptr(out2),
            _dbl_array(coef2) if coef2 is not None else None, float(damping), int(nt_mask) & 0xFFFFFFFF, self._stream(out),
        )
        self._check(rc, "xde_stage_combine")

    def stage_combine_pre(self, out, y0, pre, ks, coef, *, dt_host=0.0, ctrl=None, y0_alt=None, nt_mask=0):
        """out = y0 + ((pre + ks[0] coef[0] dt) + ...): a stage whose earlier operands the previous stage's launch has already summed
        into ``pre`` (its second output)."""
        self._require_device(out, y0, pre, y0_alt, *ks)
        if out.numel() == 0:
            return
        rc = self.lib.xde_stage_combine_pre(out.data_ptr(), y0.data_ptr(), _ptr(y0_alt), pre.data_ptr(), _ptr_array(ks), _dbl_array(coef),
                                            len(ks), float(dt_host), _ptr(ctrl), out.numel(), dtype_code(out.dtype),
                                            int(nt_mask) & 0xFFFFFFFF, self._stream(out))
        self._check(rc, "xde_stage_combine_pre")

    def stage_combine_pre_weighted(self, out, y0, pre, ks, coef, *, scale=1.0, dt_host=0.0, ctrl=None, damping=0.0):
        """out = ((pre + fuse(ks[0]) coef[0]) + ...) * scale: a fixed-step solver's final weighted sum whose leading terms the last
        stage-input launch (mode FUSE, ``out2`` / ``coef2``) has already summed into ``pre``."""
        self._require_device(out, y0, pre, *ks)
        if out.numel() == 0:
            return
        rc = self.lib.xde_stage_combine_pre_weighted(out.data_ptr(), y0.data_ptr(), pre.data_ptr(), _ptr_array(ks), _dbl_array(coef), len(ks),
                                                     float(scale), float(dt_host), _ptr(ctrl), out.numel(), dtype_code(out.dtype),
                                                     float(damping), self._stream(out))
        self._check(rc, "xde_stage_combine_pre_weighted")

    def error_norm_partial(self, ks, c_err, y0, y1, rtol, atol, segs, norm_kind, ws, *, dt_host=0.0, ctrl=None,
                           y0_alt=None, k0_alt=None, e_pre=None):
        self._require_device(y0, y1, ws, e_pre, *ks)
        rc = self.lib.xde_error_norm_partial(
            _ptr_array(ks), _ptr(k0_alt), _dbl_array(c_err), len(ks), y0.data_ptr(), _ptr(y0_alt), y1.data_ptr(),
            float(rtol), float(atol), float(dt_host), _ptr(ctrl), C.byref(segs), norm_kind, dtype_code(y0.dtype),
            ws.data_ptr(), _ptr(e_pre), self._stream(y0),
        )
        self._check(rc, "xde_error_norm_partial")

    def error_norm_control(self, ks, c_err, y0, y1, segs, ws, ctrl, params, t_span_dev, step_t_dev, t_stage, *, y0_alt=None,
                           k0_alt=None, e_pre=None):
        """Error norm + controller in one launch (single GPU, native norm)."""
        self._require_device(y0, y1, ws, ctrl, e_pre, *ks)
        m = self._mirrors.get(ctrl.data_ptr())
        rc = self.lib.xde_error_norm_control(
            _ptr_array(ks), _ptr(k0_alt), _dbl_array(c_err), len(ks), y0.data_ptr(), _ptr(y0_alt), y1.data_ptr(), C.byref(segs),
            dtype_code(y0.dtype), ws.data_ptr(), _ptr(e_pre), ctrl.data_ptr(), C.byref(params), t_span_dev.data_ptr(),
            _ptr(step_t_dev), t_stage.data_ptr(), m.ptr if m is not None else None, self._stream(y0),
        )
        self._check(rc, "xde_error_norm_control")
        if m is not None and not self._is_capturing():
            m.seq += 1

    def error_ratio(self, out, ks, c_err, y0, y1, rtol, atol, *, dt_host=0.0, ctrl=None, y0_alt=None, k0_alt=None, nonfinite_out=None):
        self._require_device(out, y0, y1, y0_alt, k0_alt, nonfinite_out, *ks)
        if out.numel() == 0:
            return
        rc = self.lib.xde_error_ratio(out.data_ptr(), _ptr_array(ks), _ptr(k0_alt), _dbl_array(c_err), len(ks), y0.data_ptr(),
                                      _ptr(y0_alt), y1.data_ptr(), float(rtol), float(atol), float(dt_host), _ptr(ctrl), out.numel(),
                                      dtype_code(out.dtype), _ptr(nonfinite_out), self._stream(out))
        self._check(rc, "xde_error_ratio")

    def scaled_norm_partial(self, a, b, y0, rtol, atol, segs, norm_kind, ws, slot):
        self._require_device(a, b, y0, ws)
        rc = self.lib.xde_scaled_norm_partial(
            a.data_ptr(), _ptr(b), y0.data_ptr(), float(rtol), float(atol), C.byref(segs), norm_kind,
            dtype_code(y0.dtype), ws.data_ptr(), slot, self._stream(y0),
        )
        self._check(rc, "xde_scaled_norm_partial")

    def norm_finalize(self, ws, slot, sums):
        self._require_device(ws, sums)
        self._check(self.lib.xde_norm_finalize(ws.data_ptr(), slot, sums.data_ptr(), self._stream(ws)), "xde_norm_finalize")

    def norm_result(self, sums, seg_count, norm_kind, state_dtype, result):
        self._require_device(sums, result)
        rc = self.lib.xde_norm_result(sums.data_ptr(), _dbl_array(seg_count), len(seg_count), norm_kind, state_dtype,
                                      result.data_ptr(), self._stream(sums))
        self._check(rc, "xde_norm_result")

    def rk_control(self, ctrl, params, ws, sums, t_span_dev, step_t_dev, t_stage):
        self._require_device(ctrl, t_span_dev, t_stage)
        m = self._mirrors.get(ctrl.data_ptr())
        rc = self.lib.xde_rk_control(ctrl.data_ptr(), C.byref(params), _ptr(ws), _ptr(sums), t_span_dev.data_ptr(),
                                     _ptr(step_t_dev), t_stage.data_ptr(), m.ptr if m is not None else None,
                                     self._stream(ctrl))
        self._check(rc, "xde_rk_control")
        if m is not None and not self._is_capturing():
            m.seq += 1

    def p2p_rk_control(self, ctrl, params, ws, exchange, t_span_dev, step_t_dev, t_stage):
        """finalize -> peer-to-peer exchange -> controller of a sharded attempt as ONE launch (``exchange``: a utils.PeerExchange)."""
        self._require_device(ctrl, ws, t_span_dev, t_stage)
        m = self._mirrors.get(ctrl.data_ptr())
        rc = self.lib.xde_p2p_rk_control(ctrl.data_ptr(), C.byref(params), ws.data_ptr(), exchange._local, exchange._peers,
                                         exchange.world, exchange.rank, exchange.SPIN_LIMIT, t_span_dev.data_ptr(), _ptr(step_t_dev),
                                         t_stage.data_ptr(), m.ptr if m is not None else None, self._stream(ctrl))
        self._check(rc, "xde_p2p_rk_control")
        if m is not None and not self._is_capturing():
            m.seq += 1

    def initial_step(self, phase, res, hs, params, t_start, t_probe, ctrl):
        """Scalar part of select_initial_step on the device (phase 0: h0; phase 1: the first step; phase 2: phase 0 with the start
        time in ``res[2]``)."""
        self._require_device(res, hs, ctrl, t_probe)
        rc = self.lib.xde_initial_step(int(phase), res.data_ptr(), hs.data_ptr(), C.byref(params), float(t_start), _ptr(t_probe),
                                       dtype_code(t_probe.dtype) if t_probe is not None else XDE_F32, ctrl.data_ptr(), self._stream(ctrl))
        self._check(rc, "xde_initial_step")

    def initial_step_fused(self, phase, a, b, y0, segs, hs, params, t_start, t_probe, ctrl, n_out=0, t_span_dev=None, step_t_dev=None,
                           t_stage=None, keep_seq=False):
        """The initial-step heuristic of a small state, one workgroup per phase (phase 1 also constructs the control block, like
        ctrl_init with the device-resident first step).  ``t_start = nan``: the start time is ``t_span_dev[0]``; ``keep_seq``: the
        block goes on counting its controller launches (a launch recorded in a graph and replayed per output interval)."""
        self._require_device(a, b, y0, hs, ctrl, t_probe, t_span_dev, t_stage)
        m = self._mirrors.get(ctrl.data_ptr()) if (phase == 1 and not keep_seq) else None
        seq0 = -1 if keep_seq else (m.seq if m is not None else 0)
        rc = self.lib.xde_initial_step_fused(int(phase), a.data_ptr(), _ptr(b), y0.data_ptr(), C.byref(segs), dtype_code(y0.dtype), hs.data_ptr(),
                                             C.byref(params), float(t_start), _ptr(t_probe),
                                             dtype_code(t_probe.dtype) if t_probe is not None else XDE_F32, ctrl.data_ptr(), int(n_out),
                                             _ptr(t_span_dev), _ptr(step_t_dev), _ptr(t_stage), seq0, self._stream(y0))
        self._check(rc, "xde_initial_step_fused")
        if m is not None:
            m.seq0 = seq0
            m.init_published = False

    def scaled_norm2_partial(self, f0, y0, rtol, atol, segs, norm_kind, ws):
        """Partials of norm(y0 / scale) (slot 0) and norm(f0 / scale) (slot 1) in one pass over (y0, f0)."""
        self._require_device(f0, y0, ws)
        rc = self.lib.xde_scaled_norm2_partial(f0.data_ptr(), y0.data_ptr(), float(rtol), float(atol), C.byref(segs), norm_kind,
                                               dtype_code(y0.dtype), ws.data_ptr(), self._stream(y0))
        self._check(rc, "xde_scaled_norm2_partial")

    def initial_step_tail(self, phase, ws, hs, params, t_start, t_probe, ctrl, n_out=0, t_span_dev=None, step_t_dev=None, t_stage=None,
                          keep_seq=False):
        """What followed a norm pass of the initial-step heuristic as launches of its own — finalize, result, the scalar phase, and in
        phase 1 the control block's construction — as ONE one-workgroup launch (states above initial_step_fused's reach).
        ``t_start = nan`` / ``keep_seq``: as initial_step_fused.  Phase 1 (not ``keep_seq``) also publishes the constructed block to the
        control block's host mirror: ``ctrl_peek_async(ctrl)`` then hands out that slot — where the first attempt lands, without
        a copy command on the stream (the publication takes a sequence number of its own: the slot it lands in may still
        hold the previous owner's last block under the old number)."""
        self._require_device(ws, hs, ctrl, t_probe, t_span_dev, t_stage)
        m = self._mirrors.get(ctrl.data_ptr()) if (phase == 1 and not keep_seq) else None
        publish = m is not None and not self._is_capturing() and self._mirror_takes_init
        if publish:
            m.seq += 1
        seq0 = -1 if keep_seq else (m.seq if m is not None else 0)
        rc = self.lib.xde_initial_step_tail(int(phase), ws.data_ptr(), hs.data_ptr(), C.byref(params), float(t_start), _ptr(t_probe),
                                            dtype_code(t_probe.dtype) if t_probe is not None else XDE_F32, ctrl.data_ptr(), int(n_out),
                                            _ptr(t_span_dev), _ptr(step_t_dev), _ptr(t_stage), seq0, m.ptr if publish else None,
                                            self._stream(ctrl))
        self._check(rc, "xde_initial_step_tail")
        if m is not None:
            m.seq0 = seq0
            m.init_published = publish

    def ctrl_init(self, ctrl, params, t_start, first_step, n_out, t_span_dev, step_t_dev, t_stage, first_step_dev=None, keep_seq=False):
        """``t_start = nan``: the start time is ``t_span_dev[0]``; ``keep_seq``: the block goes on counting its controller launches
        (both for a launch recorded in a graph and replayed per output interval)."""
        self._require_device(ctrl, t_span_dev, t_stage)
        m = None if keep_seq else self._mirrors.get(ctrl.data_ptr())
        seq0 = -1 if keep_seq else (m.seq if m is not None else 0)
        rc = self.lib.xde_ctrl_init(ctrl.data_ptr(), C.byref(params), float(t_start), float(first_step), int(n_out),
                                    t_span_dev.data_ptr(), _ptr(step_t_dev), t_stage.data_ptr(), seq0, _ptr(first_step_dev),
                                    self._stream(ctrl))
        self._check(rc, "xde_ctrl_init")
        if m is not None:
            m.seq0 = seq0
            m.init_published = False

    def ctrl_retarget(self, ctrl, params, t_span_dev, n_out):
        """New output list for a running solve (the device side of AdaptiveRKSolver.step(next_t))."""
        self._require_device(ctrl, t_span_dev)
        m = self._mirrors.get(ctrl.data_ptr())
        rc = self.lib.xde_ctrl_retarget(ctrl.data_ptr(), C.byref(params), t_span_dev.data_ptr(), int(n_out),
                                        m.ptr if m is not None else None, self._stream(ctrl))
        self._check(rc, "xde_ctrl_retarget")
        if m is not None and not self._is_capturing():
            m.seq += 1

    def ctrl_read(self, ctrl) -> XdeCtrl:
        """The newest control block.  With a host mirror: poll the pinned ring (no HIP call); else a blocking copy."""
        self._require_device(ctrl)
        m = self._mirrors.get(ctrl.data_ptr())
        if m is not None and m.seq > m.seq0:
            return self.ctrl_wait((m, m.seq))
        host = XdeCtrl()
        self._check(self.lib.xde_ctrl_read(ctrl.data_ptr(), C.byref(host), self._stream(ctrl)), "xde_ctrl_read")
        return host

    PEEK_POOL_MAX = 4  # idle (buffer, event) pairs kept per control block's mirror

    class _Peek:
        """One enqueued copy of a control block: OWNS its pinned buffer and its event until ``ctrl_peek_result`` has consumed it (or the
        handle is dropped); only then do they go back to the mirror's pool.  Any number of peeks may be pending on one block."""

        __slots__ = ("host", "ev", "device", "pool", "__weakref__")

        def __init__(self, host, ev, device, pool):
            self.host, self.ev, self.device, self.pool = host, ev, device, pool

        def _recycle(self):
            host, ev, pool = self.host, self.ev, self.pool
            self.host = self.ev = self.pool = None
            if host is None:
                return
            if pool is not None and len(pool) < HipBackend.PEEK_POOL_MAX:
                pool.append((host, ev, self.device))
            else:
                # not kept: releasing a pinned buffer records an event on the stream its copy ran on — which may be recording a
                # hipGraph right now (this runs from __del__, at any allocation): utils.graphed parks the pair until none is
                from .utils.graphed import release_when_idle

                release_when_idle((host, ev))

        def __del__(self):  # a handle nobody read (a solve that ended before its second attempt): the pair is reusable all the same —
            try:  # copies are stream-ordered, a later peek's copy and event land after this one's
                self._recycle()
            except Exception:  # interpreter shutdown
                pass

    def ctrl_peek_async(self, ctrl):
        """Enqueue a copy of the control block AS IT IS AT THIS POINT OF THE STREAM into pinned host memory (a freshly constructed block
        has no mirror slot); ``ctrl_peek_result(handle)`` waits for that copy only — not for anything enqueued after it.  Re-entrant:
        every handle has a buffer and an event of its own until it is consumed; they are pooled with the block's mirror (control
        blocks are recycled between solves), so a steady state of one peek per solve allocates nothing.  A block that the launch which
        constructed it has published to the host mirror (initial_step_tail), with no controller launch since, is read from there:
        nothing is enqueued."""
        self._require_device(ctrl)
        m = self._mirrors.get(ctrl.data_ptr())
        if m is not None and m.init_published and m.seq == m.seq0:
            return (m, m.seq0)
        pool = None
        if m is not None:
            if m.peek is None:
                m.peek = []
            pool = m.peek
        kept = None
        while pool:
            kept = pool.pop()
            if kept[2] == ctrl.device:
                break
            kept = None
        if kept is None:
            kept = (torch.empty(C.sizeof(XdeCtrl), dtype=torch.uint8).pin_memory(), torch.cuda.Event(), ctrl.device)
        host, ev = kept[0], kept[1]
        with torch.cuda.device(ctrl.device):
            host.copy_(ctrl, non_blocking=True)
            ev.record()
        return HipBackend._Peek(host, ev, ctrl.device, pool)

    def ctrl_peek_result(self, handle) -> XdeCtrl:
        if isinstance(handle, tuple):  # the block is in the mirror ring
            return self.ctrl_wait(handle)
        if handle.host is None:
            raise XdeError("ctrl_peek_result: this handle has been consumed already")
        handle.ev.synchronize()
        out = XdeCtrl.from_buffer_copy(handle.host.numpy().tobytes())
        handle._recycle()
        return out

    def ctrl_read_async(self, ctrl):
        """Handle for the control block of the newest controller launch; nothing is enqueued on the stream."""
        self._require_device(ctrl)
        m = self._mirrors.get(ctrl.data_ptr())
        if m is None or m.seq == m.seq0:
            raise XdeError("ctrl_read_async needs a control block from new_ctrl() with at least one controller launch")
        return (m, m.seq)

    def ctrl_wait(self, handle) -> XdeCtrl:
        m, seq = handle
        host = XdeCtrl()
        self._check(self.lib.xde_ctrl_wait(m.ptr, seq, self.WAIT_TIMEOUT_MS, C.byref(host)), "xde_ctrl_wait")
        return host

    def dense_eval(self, out_base, ks, mid, y0, y1, f1, ctrl, t_span_dev, time_dtype, *, y0_alt=None, k0_alt=None,
                   expect_step=-1):
        self._require_device(out_base, y0, y1, f1, ctrl, t_span_dev, *ks)
        if y0.numel() == 0:
            return
        rc = self.lib.xde_dense_eval(
            out_base.data_ptr(), _ptr_array(ks), _ptr(k0_alt), _dbl_array(mid), len(ks), y0.data_ptr(), _ptr(y0_alt),
            y1.data_ptr(), f1.data_ptr(), ctrl.data_ptr(), t_span_dev.data_ptr(), time_dtype, y0.numel(),
            dtype_code(y0.dtype), int(expect_step), self._stream(y0),
        )
        self._check(rc, "xde_dense_eval")

    def scale_fanout(self, outs, g, factors, dt_dev=None):
        self._require_device(g, *outs)
        if g.numel() == 0:
            return
        rc = self.lib.xde_scale_fanout(_ptr_array(outs), g.data_ptr(), _dbl_array(factors), len(outs), _ptr(dt_dev), g.numel(),
                                       dtype_code(g.dtype), self._stream(g))
        self._check(rc, "xde_scale_fanout")

    # -- back-propagation through the accepted steps (include/xde_hip_backprop.h) ------------------------------------------
    def stage_cotangent(self, out, xs, coef, *, out2=None, coef2=None):
        """out = sum_j xs[j] * coef[j]  [, out2 = sum_j xs[j] * coef2[j]]: one launch, every operand read once."""
        self._require_device(out, out2, *xs)
        rc = self.lib.xde_stage_cotangent(out.data_ptr(), _ptr(out2), _ptr_array(xs), _dbl_array(coef),
                                          _dbl_array(coef2) if coef2 is not None else None, len(xs), out.numel(),
                                          dtype_code(out.dtype), self._stream(out))
        self._check(rc, "xde_stage_cotangent")

    def dense_cotangent(self, outs, g_rows, weights, acc_mask=0):
        """outs = [y0, y1, y_mid, f0, f1] cotangents (None: not written) <- the [G, n] rows ``g_rows`` times the G x 5 ``weights``;
        bit k of ``acc_mask``: outs[k] accumulates."""
        self._require_device(g_rows, *[o for o in outs if o is not None])
        G = len(weights)
        n = g_rows.numel() // G if G else 0
        flat = [float(w) for row in weights for w in row]
        rc = self.lib.xde_dense_cotangent((C.c_void_p * 5)(*[_ptr(o) for o in outs]), g_rows.data_ptr(), _dbl_array(flat), G,
                                          int(acc_mask) & 0x1F, n, dtype_code(g_rows.dtype), self._stream(g_rows))
        self._check(rc, "xde_dense_cotangent")

    # -- sub-stepping of the fixed-step solvers (include/xde_hip_grid.h) ---------------------------------------------------
    def _interp_rows(self, dsts, kinds, weights, y_a, y_b, f_a=None, f_b=None):
        """Write the output rows of one grid step: ``dsts[r]`` <- row kind ``kinds[r]`` (XDE_ROW_*) at the four weights ``weights[r]``
        from the contiguous operands ``y_a, y_b`` (and ``f_a, f_b``: the cubic).  Every ``dsts[r]`` has ``y_a``'s shape and is either
        contiguous or a row block ``[..., L, D]`` of a contiguous ``[..., T*L, D]`` solution, all with the same strides.  Launches of
        XDE_INTERP_MAX_ROWS rows; each reads the operands once.

        Private on purpose: the public methods of this class are a frozen contract that tests/_cpu_double.py mirrors method for method
        (tests/test_cabi.py).  Folding this one into that contract, together with its numpy double, is a later maintainer edit; until
        then only FixedSolver's sub-stepping path calls it."""
        self._require_device(y_a, y_b, f_a, f_b, *dsts)
        cubic = f_a is not None
        outer, chunk, row_stride = _row_geometry(dsts[0], y_a)
        for d in dsts[1:]:
            if d.stride() != dsts[0].stride() or d.shape != dsts[0].shape:
                raise XdeError("_interp_rows: every destination row needs the same shape and strides")
        _require_alike("_interp_rows", "operands", y_a, (y_a, y_b, f_a, f_b))
        if y_a.numel() == 0:
            return
        dt = dtype_code(y_a.dtype)
        st = self._stream(y_a)
        M = XDE_INTERP_MAX_ROWS
        for r0 in range(0, len(dsts), M):
            part = dsts[r0 : r0 + M]
            G = len(part)
            flat = [float(w) for row in weights[r0 : r0 + M] for w in row]
            rc = self.lib.xde_interp_rows(_ptr_array(part), (C.c_int * G)(*[int(k) for k in kinds[r0 : r0 + M]]), _dbl_array(flat), G,
                                          y_a.data_ptr(), y_b.data_ptr(), _ptr(f_a), _ptr(f_b),
                                          XDE_INTERP_CUBIC if cubic else XDE_INTERP_LINEAR, outer, chunk, row_stride, dt, st)
            self._check(rc, "xde_interp_rows")

    # -- sdeint's Euler-Maruyama, Milstein and SRK steps (include/xde_hip_sde.h) ------------------------------------------------------------
    # Private for the reason _interp_rows is: the public methods are the contract tests/_cpu_double.py mirrors.  Only the fixed-step
    # solvers' SDE path (and its autograd node) call these.
    def _sde_call(self, who, outs, ins, *scalars):
        """One launch of the step entry point ``xde<who>(*outs, *ins, n, *scalars, dtype, stream)``: contiguous tensors of one shape and
        dtype on the device; an output given as None goes in as a null pointer (a skipped output of a backward), and so does an input
        (the zero cotangents of the reversible Heun sweep's first backward step)."""
        self._require_device(*outs, *ins)
        like = next(x for x in ins if x is not None)
        _require_alike(who, "operands", like, (*ins, *outs))
        rc = getattr(self.lib, "xde" + who)(*[_ptr(x) for x in (*outs, *ins)], like.numel(), *scalars, dtype_code(like.dtype),
                                            self._stream(like))
        self._check(rc, "xde" + who)

    def _sde_em_step(self, y1, y0, f, g, dt, s, seed, k):
        """``y1 = (y0 + f*dt) + g*(s*Z)`` with Z the normals of (``seed``, step ``k``); ``y1`` may be ``y0``.  One launch."""
        self._sde_call("_sde_em_step", (y1,), (y0, f, g), float(dt), float(s), int(seed), int(k))

    def _sde_em_backward(self, gf, gg, gy1, dt, s, seed, k):
        """``gf = gy1*dt`` and ``gg = gy1*(s*Z)`` (either may be None: skipped), one launch regenerating the forward's Z."""
        self._sde_call("_sde_em_backward", (gf, gg), (gy1,), float(dt), float(s), int(seed), int(k))

    def _sde_milstein_support(self, yb, y0, f, g, dt, s):
        """Milstein's support point ``yb = (y0 + f*dt) + g*s``.  One launch, no generator."""
        self._sde_call("_sde_milstein_support", (yb,), (y0, f, g), float(dt), float(s))

    def _sde_milstein_support_backward(self, gf, gg, gyb, dt, s):
        """``gf = gyb*dt`` and ``gg = gyb*s`` (either may be None: skipped), one launch."""
        self._sde_call("_sde_milstein_support_backward", (gf, gg), (gyb,), float(dt), float(s))

    def _sde_milstein_step(self, y1, y0, f, g, gb, dt, s, c, seed, k):
        """``y1 = ((y0 + f*dt) + g*w) + (gb - g)*q`` with ``w = s*Z``, ``q = c*(w*w - |dt|)`` and Z the normals of (``seed``, step
        ``k``); ``y1`` may be ``y0``.  One launch."""
        self._sde_call("_sde_milstein_step", (y1,), (y0, f, g, gb), float(dt), float(s), float(c), int(seed), int(k))

    def _sde_milstein_backward(self, gf, gg, ggb, gy1, dt, s, c, seed, k):
        """``gf = gy1*dt``, ``gg = gy1*(w - q)`` and ``ggb = gy1*q`` (any may be None: skipped), one launch regenerating the forward's Z."""
        self._sde_call("_sde_milstein_backward", (gf, gg, ggb), (gy1,), float(dt), float(s), float(c), int(seed), int(k))

    def _sde_srk_stage1(self, Y2, G2, G3, y0, a1, b1, dt, s, seed, k):
        """SRK's first three stage inputs: ``Y2 = (y0 + a1*(0.75*dt)) + b1*(1.5*p)``, ``G2 = (y0 + a1*(0.25*dt)) + b1*(0.5*s)`` and
        ``G3 = (y0 + a1*dt) - b1*s`` with ``p = 0.5*(s*Z + (s*V)/sqrt(3))``, Z and V the two draws of (``seed``, step ``k``).  One launch."""
        self._sde_call("_sde_srk_stage1", (Y2, G2, G3), (y0, a1, b1), float(dt), float(s), int(seed), int(k))

    def _sde_srk_stage2(self, G4, y0, a1, b1, b2, b3, dt, s):
        """SRK's last stage input ``G4 = (y0 + a1*(0.25*dt)) + ((b1*-5 + b2*3) + b3*0.5)*s``.  One launch, no generator."""
        self._sde_call("_sde_srk_stage2", (G4,), (y0, a1, b1, b2, b3), float(dt), float(s))

    def _sde_srk_step(self, y1, y0, a1, a2, b1, b2, b3, b4, dt, s, c, c3, seed, k):
        """``y1 = ((((y0 + (a1/3 + 2*a2/3)*dt) + b1*e1) + b2*e2) + b3*e3) + b4*e4`` with the weights e of include/xde_hip_sde.h on
        the two draws of (``seed``, step ``k``); ``y1`` may be ``y0``.  One launch."""
        self._sde_call("_sde_srk_step", (y1,), (y0, a1, a2, b1, b2, b3, b4), float(dt), float(s), float(c), float(c3), int(seed), int(k))

    def _sde_srk_stage1_backward(self, gy, ga1, gb1, gY2, gG2, gG3, dt, s, seed, k):
        """The cotangents of stage 1's ``y0``, ``a1`` and ``b1`` from those of its three outputs (any may be None: skipped), one
        launch regenerating the forward's draws."""
        self._sde_call("_sde_srk_stage1_backward", (gy, ga1, gb1), (gY2, gG2, gG3), float(dt), float(s), int(seed), int(k))

    def _sde_srk_stage2_backward(self, ga1, gb1, gb2, gb3, gG4, dt, s):
        """The cotangents of stage 2's ``a1`` and of its ``b1, b2, b3`` (the drift one, or the diffusion three together, may be None:
        skipped), one launch."""
        self._sde_call("_sde_srk_stage2_backward", (ga1, gb1, gb2, gb3), (gG4,), float(dt), float(s))

    def _sde_srk_step_backward(self, ga1, ga2, gb1, gb2, gb3, gb4, gy1, dt, s, c, c3, seed, k):
        """The cotangents of the step's ``a1, a2`` and of its ``b1 .. b4`` (the drift two together, or the diffusion four together, may
        be None: skipped), one launch regenerating the forward's draws."""
        self._sde_call("_sde_srk_step_backward", (ga1, ga2, gb1, gb2, gb3, gb4), (gy1,), float(dt), float(s), float(c), float(c3),
                       int(seed), int(k))

    def _sde_rheun_predict(self, yh1, y0, yh0, f0, g0, dt, s, direction, seed, k):
        """Reversible Heun's prediction ``yh1 = (((y0 + y0) - yh0) + f0*dt) + g0*w``, ``w = s*Z`` with Z the normals of (``seed``, step
        ``k``), ``dt`` and ``w`` times ``direction`` (+1, or -1: the reverse step); ``yh1`` may be ``yh0``.  One launch."""
        self._sde_call("_sde_rheun_predict", (yh1,), (y0, yh0, f0, g0), float(dt), float(s), int(direction), int(seed), int(k))

    def _sde_rheun_correct(self, y1, y0, f0, f1, g0, g1, dt, s, direction, seed, k):
        """Reversible Heun's correction ``y1 = (y0 + (f0 + f1)*(0.5*dt)) + (g0 + g1)*(0.5*w)``, ``dt`` and ``w`` times ``direction``;
        ``y1`` may be ``y0``.  One launch."""
        self._sde_call("_sde_rheun_correct", (y1,), (y0, f0, f1, g0, g1), float(dt), float(s), int(direction), int(seed), int(k))

    def _sde_rheun_adjoint_stage(self, bf, bg, af1, ag1, ay1, dt, s, seed, k):
        """The cotangents the sweep's vjp takes: ``bf = af1 + ay1*(0.5*dt)``, ``bg = ag1 + ay1*(0.5*w)``; ``af1`` and ``ag1`` None
        together: zero (the first backward step).  ``bf`` may be ``af1`` and ``bg`` may be ``ag1``.  One launch regenerating Z."""
        self._sde_call("_sde_rheun_adjoint_stage", (bf, bg), (af1, ag1, ay1), float(dt), float(s), int(seed), int(k))

    def _sde_rheun_adjoint_step(self, ay0, ayh0, af0, ag0, ay1, ayh1, v, dt, s, seed, k):
        """One backward step of the state cotangents: ``A = ayh1 + v``, ``ay0 = ay1 + (A + A)``, ``ayh0 = -A``,
        ``af0 = ay1*(0.5*dt) + A*dt``, ``ag0 = ay1*(0.5*w) + A*w``; ``ayh1`` None: zero.  ``ay0`` may be ``ay1`` and ``ayh0`` may be
        ``ayh1``.  One launch regenerating Z."""
        self._sde_call("_sde_rheun_adjoint_step", (ay0, ayh0, af0, ag0), (ay1, ayh1, v), float(dt), float(s), int(seed), int(k))

    def _sde_noise(self, out, seed, k, bits=False, draw=0):
        """The generator's output for (``seed``, step ``k``) into the contiguous ``out``: the normals Z (``out``'s dtype), or with
        ``bits`` the raw Philox words (``out`` int32 / uint32, one word per element).  ``draw=1``: the second draw, V."""
        self._require_device(out)
        if not out.is_contiguous():
            raise XdeError("_sde_noise: out must be contiguous")
        if bits:
            if out.element_size() != 4 or out.is_floating_point():
                raise XdeError("_sde_noise: the words go into a 32-bit integer tensor")
            mode, dt = XDE_NOISE_BITS, XDE_F32
        else:
            mode, dt = XDE_NOISE_NORMAL, dtype_code(out.dtype)
        if draw:
            rc = self.lib.xde_sde_noise_draw(out.data_ptr(), out.numel(), int(seed), int(k), int(draw), mode, dt, self._stream(out))
            self._check(rc, "xde_sde_noise_draw")
            return
        rc = self.lib.xde_sde_noise(out.data_ptr(), out.numel(), int(seed), int(k), mode, dt, self._stream(out))
        self._check(rc, "xde_sde_noise")

    # -- the KL term of a latent SDE fused into the Euler-Maruyama step (include/xde_hip_kl.h) ----------------------------------------
    # Private for the reason _sde_em_step is.  Only the fixed-step solvers' logqp path (and its autograd nodes) call these.
    def _kl_call(self, who, state, accs, like, *scalars):
        """The operand check the two KL entry points share; nothing is launched here.  ``state`` must be contiguous device tensors of
        ``like``'s shape and dtype and ``accs`` contiguous float64 device tensors with one element per row of ``like`` (a row is its
        last axis); None stands for a null pointer and is not checked.  Returns ``(rows, D, tail)``, ``tail`` being ``scalars`` followed
        by the dtype code and the stream: the arguments the caller's launch puts after its pointers."""
        self._require_device(*state, *accs)
        D = like.shape[-1]
        rows = like.numel() // D if D else 0
        _require_alike(who, "state operands", like, state)
        for x in accs:
            if x is not None and (not x.is_contiguous() or x.dtype != torch.float64 or x.numel() != rows):
                raise XdeError("{}: an accumulator is a contiguous float64 tensor with one element per row".format(who))
        return rows, D, scalars + (dtype_code(like.dtype), self._stream(like))

    def _sde_kl_step(self, y1, acc1, y0, f, g, h, acc0, dt, s, seed, k):
        """``y1 = (y0 + f*dt) + g*(s*Z)`` (xde_sde_em_step's bits) and, per row of the last axis, ``acc1 = acc0 + sum(((f - h)/g)**2) *
        (0.5*dt)`` in float64 — one launch.  ``acc0`` None: zero; ``acc1`` may be ``acc0`` and ``y1`` may be ``y0``; ``y1`` and ``y0``
        both None: only the accumulation (no generator)."""
        rows, D, tail = self._kl_call("_sde_kl_step", (y1, y0, f, g, h), (acc1, acc0), f, float(dt), float(s), int(seed), int(k))
        rc = self.lib.xde_sde_kl_step(_ptr(y1), _ptr(acc1), _ptr(y0), _ptr(f), _ptr(g), _ptr(h), _ptr(acc0), rows, D, *tail)
        self._check(rc, "xde_sde_kl_step")

    def _sde_kl_backward(self, gf, gg, gh, gy1, gacc, f, g, h, dt, s, seed, k):
        """The cotangents of ``f``, ``g`` and ``h`` (any may be None: skipped) from those of ``y1`` (``gy1``; None: the accumulate-only
        mode's backward) and of ``acc1`` (``gacc``, float64 per row), one launch regenerating the forward's Z."""
        rows, D, tail = self._kl_call("_sde_kl_backward", (gf, gg, gh, gy1, f, g, h), (gacc,), f, float(dt), float(s), int(seed), int(k))
        rc = self.lib.xde_sde_kl_backward(_ptr(gf), _ptr(gg), _ptr(gh), _ptr(gy1), _ptr(gacc), _ptr(f), _ptr(g), _ptr(h), rows, D, *tail)
        self._check(rc, "xde_sde_kl_backward")

    # -- the Euler-Maruyama step with general or scalar noise (include/xde_hip_gn.h) ---------------------------------------------------
    # Private for the reason _sde_em_step is.  Only FixedSolver._em_step under a non-diagonal BaseSDE (and its autograd node) call these.
    def _gn_call(self, who, state, mats, like, *scalars):
        """The operand check the two general-noise entry points share; nothing is launched here.  ``state`` must be contiguous device
        tensors of ``like``'s shape ``[.., D]`` and dtype and ``mats`` contiguous device tensors of shape ``[.., D, M]`` and that dtype,
        one M for all; None stands for a null pointer and is not checked (``like`` and one of ``mats`` are never None).  Returns
        ``(rows, D, M, tail)``, ``tail`` being ``scalars`` followed by the dtype code and the stream."""
        self._require_device(*state, *mats)
        if like.dim() < 1:
            raise XdeError("{}: the state needs a last axis".format(who))
        _require_alike(who, "state operands", like, state)
        M = None
        for x in mats:
            if x is None:
                continue
            if not x.is_contiguous() or x.dtype != like.dtype or x.shape[:-1] != like.shape or x.shape[-1] < 1:
                raise XdeError("{}: the diffusion operand must be a contiguous tensor of shape {} + (M,), M >= 1, and dtype {}, got {} {}".format(
                    who, tuple(like.shape), like.dtype, tuple(x.shape), x.dtype))
            M = x.shape[-1]
        D = like.shape[-1]
        rows = like.numel() // D if D else 0
        return rows, D, M, scalars + (dtype_code(like.dtype), self._stream(like))

    def _sde_gn_step(self, y1, y0, f, g, dt, s, seed, k):
        """``y1[.., d] = (y0[.., d] + f[.., d]*dt) + sum_m g[.., d, m]*(s*Z[.., m])``, the sum sequential in m, with Z the normals of
        (``seed``, step ``k``) over the flat ``[rows, M]`` array; ``g`` is ``[.., D, M]``; ``y1`` may be ``y0``.  One launch."""
        rows, D, M, tail = self._gn_call("_sde_gn_step", (y1, y0, f), (g,), y0, float(dt), float(s), int(seed), int(k))
        if rows == 0:
            return
        self._check(self.lib.xde_sde_gn_step(_ptr(y1), _ptr(y0), _ptr(f), _ptr(g), rows, D, M, *tail), "xde_sde_gn_step")

    def _sde_gn_backward(self, gf, gg, gy1, M, dt, s, seed, k):
        """``gf = gy1*dt`` (``[.., D]``) and ``gg[.., d, m] = gy1[.., d]*(s*Z[.., m])`` (``[.., D, M]``); either may be None: skipped.
        One launch regenerating the forward's Z."""
        rows, D, M_, tail = self._gn_call("_sde_gn_backward", (gf, gy1), (gg,), gy1, float(dt), float(s), int(seed), int(k))
        if M_ is not None and M_ != int(M):
            raise XdeError("_sde_gn_backward: gg's last axis is {}, M is {}".format(M_, int(M)))
        if rows == 0:
            return
        self._check(self.lib.xde_sde_gn_backward(_ptr(gf), _ptr(gg), _ptr(gy1), rows, D, int(M), *tail), "xde_sde_gn_backward")

    # -- the Hermite tape of ddeint_steps (include/xde_hip_dde.h) ---------------------------------------------------------------------
    # Private for the reason _interp_rows is.  Only xde/steps_dde.py's autograd node (solver/_autograd.py: DdeTapeGatherFn) calls these.
    def _dde_rows(self, who, x, rows, D, what):
        """The row stride (elements) of ``x``, a ``[rows, D]`` device tensor of unit element stride whose rows do not overlap."""
        if x.dim() != 2 or tuple(x.shape) != (rows, D) or (D > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < D):
            raise XdeError("{}: {} must be a [rows, D] = [{}, {}] tensor of unit element stride and a row stride >= D, got shape {} strides {}".format(
                who, what, rows, D, tuple(x.shape), x.stride()))
        return int(x.stride(0)) if rows > 1 else D

    def _dde_tape_gather(self, out, dtau, srcs, w, wd=None):
        """``out [rows, L, D]`` (and ``dtau``, unless None) <- the Hermite interpolant of every delay ``j < L`` of one stage:
        ``srcs[4j .. 4j + 3]`` are the ``[rows, D]`` end states and derivatives ``ya, fa, yb, fb`` of the delay's interval (tape nodes, or
        strided rows of a ``[rows, Th, D]`` history), ``w`` / ``wd`` the ``4L`` value / delay-derivative weights (host floats).  One
        launch per ``XDE_DDE_MAX_LAGS`` delays."""
        who = "_dde_tape_gather"
        self._require_device(out, dtau, *srcs)
        if out.dim() != 3 or not out.is_contiguous():
            raise XdeError("{}: out must be a contiguous [rows, L, D] tensor".format(who))
        rows, L, D = out.shape
        if (dtau is None) != (wd is None):
            raise XdeError("{}: dtau and wd are given together or not at all".format(who))
        _require_alike(who, "outputs", out, (dtau,))
        if L < 1 or len(srcs) != 4 * L or len(w) != 4 * L or (wd is not None and len(wd) != 4 * L):
            raise XdeError("{}: {} delays take {} operands and weights (got {} and {})".format(who, L, 4 * L, len(srcs), len(w)))
        if any(x.dtype != out.dtype for x in srcs):
            raise XdeError("{}: every operand must have the outputs' dtype {}".format(who, out.dtype))
        strides = [self._dde_rows(who, x, rows, D, "operand {}".format(i)) for i, x in enumerate(srcs)]
        if rows == 0 or D == 0:
            return
        code, stream = dtype_code(out.dtype), self._stream(out)
        for j0 in range(0, L, XDE_DDE_MAX_LAGS):
            n = min(XDE_DDE_MAX_LAGS, L - j0)
            sl = slice(4 * j0, 4 * (j0 + n))
            rc = self.lib.xde_dde_tape_gather(out.data_ptr(), _ptr(dtau), _ptr_array(srcs[sl]), (C.c_int64 * (4 * n))(*strides[sl]),
                                              _dbl_array(w[sl]), _dbl_array(wd[sl]) if wd is not None else None, rows, D, n, j0, L, code,
                                              stream)
            self._check(rc, "xde_dde_tape_gather")

    def _dde_tape_gather_backward(self, gouts, terms, g, j0=0):
        """``gouts[q]`` (contiguous ``[rows, D]``) <- the sum over ``terms[q] = [(lag, weight), ...]``, in that order, of
        ``g[:, j0 + lag, :] * weight``: the cotangents of the distinct node tensors the delays ``j0 + lag`` of a gather read, from
        ``g [rows, L, D]``, that of its ``out``.  One launch (at most ``4 XDE_DDE_MAX_LAGS`` outputs and terms)."""
        who = "_dde_tape_gather_backward"
        self._require_device(g, *gouts)
        if g.dim() != 3 or not g.is_contiguous():
            raise XdeError("{}: g must be a contiguous [rows, L, D] tensor".format(who))
        rows, L, D = g.shape
        nq = len(gouts)
        if nq < 1 or len(terms) != nq or any(len(ts) < 1 for ts in terms):
            raise XdeError("{}: every output takes a list of at least one (lag, weight) term".format(who))
        for o in gouts:
            if not o.is_contiguous() or tuple(o.shape) != (rows, D) or o.dtype != g.dtype:
                raise XdeError("{}: every output must be a contiguous [rows, D] tensor of g's dtype".format(who))
        if rows == 0 or D == 0:
            return
        first, lag, wt = [0], [], []
        for ts in terms:
            lag += [int(j) for j, _ in ts]
            wt += [float(x) for _, x in ts]
            first.append(len(lag))
        rc = self.lib.xde_dde_tape_gather_backward(_ptr_array(gouts), (C.c_int32 * (nq + 1))(*first), (C.c_int32 * len(lag))(*lag),
                                                   _dbl_array(wt), nq, g.data_ptr(), rows, D, int(j0), L, dtype_code(g.dtype), self._stream(g))
        self._check(rc, "xde_dde_tape_gather_backward")

    # -- logsignature windows (include/xde_hip_logsig.h) ------------------------------------------------------------------------------
    # Private for the reason _interp_rows is.  Only interpolation.logsig_windows (and its autograd node) call these.
    def _logsig_call(self, who, x, inc, grads, window_length, depth):
        """The operand check the two entry points share; nothing is launched here.  ``x [.., T, C]`` and ``inc [.., W, K]`` are contiguous
        device tensors of one floating dtype with the same leading axes, ``grads`` contiguous tensors of ``x``'s shape and dtype.
        Returns ``(B, T, C, L, depth, dtype code, stream)``, the arguments after the pointers."""
        self._require_device(x, inc, *grads)
        if x.dim() < 2:
            raise XdeError("{}: the series is [.., T, C]".format(who))
        _require_alike(who, "series operands", x, (x, *grads))
        T, Cn = x.shape[-2:]
        L, depth = int(window_length), int(depth)
        K = logsig_channels(Cn, depth)
        if L < 1 or T < 2:
            raise XdeError("{}: window_length >= 1 and T >= 2 (got {} and {})".format(who, L, T))
        W = -(-(T - 1) // L)
        if not inc.is_contiguous() or inc.dtype != x.dtype or tuple(inc.shape) != tuple(x.shape[:-2]) + (W, K):
            raise XdeError("{}: the windows are a contiguous tensor of shape {} and dtype {}, got {} {}".format(
                who, tuple(x.shape[:-2]) + (W, K), x.dtype, tuple(inc.shape), inc.dtype))
        return x.numel() // (T * Cn), T, Cn, L, depth, dtype_code(x.dtype), self._stream(x)

    def _logsig_windows(self, out, x, window_length, depth):
        """``out [.., W, K]`` <- the logsignatures of the windows of ``window_length`` steps of ``x [.., T, C]``.  One launch."""
        tail = self._logsig_call("_logsig_windows", x, out, (), window_length, depth)
        if tail[0] == 0:
            return
        self._check(self.lib.xde_logsig_windows(_ptr(out), _ptr(x), *tail), "xde_logsig_windows")

    def _logsig_windows_backward(self, gx, gout, x, window_length, depth):
        """``gx [.., T, C]`` <- the cotangent of ``x`` from ``gout [.., W, K]``, that of ``_logsig_windows``' output.  One launch."""
        tail = self._logsig_call("_logsig_windows_backward", x, gout, (gx,), window_length, depth)
        if tail[0] == 0:
            return
        self._check(self.lib.xde_logsig_windows_backward(_ptr(gx), _ptr(gout), _ptr(x), *tail), "xde_logsig_windows_backward")

    # -- per-sample adaptive stepping (include/xde_hip_rows.h) ------------------------------------------------------------------------
    # Private for the reason _interp_rows is.  Only solver/_rk_rows.py calls these.  ``ctl`` is a ``RowsCtl``.
    def _rows_call(self, who, ctl, like, *operands):
        """The operand check the four entry points share; nothing is launched here.  Returns ``(rows, D, dtype code, stream)``."""
        self._require_device(like, ctl.f64, ctl.i32, ctl.t_stage, *operands)
        if like.dim() < 2 or like.shape[0] != ctl.rows:
            raise XdeError("{}: the state is [rows, ...] with rows = {} (got {})".format(who, ctl.rows, tuple(like.shape)))
        _require_alike(who, "state operands", like, operands)
        return ctl.rows, like.numel() // ctl.rows, dtype_code(like.dtype), self._stream(like)

    def _rows_stage_combine(self, out, y0, ks, coef, ctl, *, out2=None, coef2=None):
        """``out[r] = y0[r] + sum_j ks[j][r] * (coef[j] * h[r])``, XDE_COMBINE_RK's op order row by row; done rows: ``out = y0``."""
        rows, D, code, st = self._rows_call("_rows_stage_combine", ctl, y0, out, out2, y0, *ks)
        rc = self.lib.xde_rows_stage_combine(_ptr(out), _ptr(out2), _ptr(y0), _ptr_array(ks), _dbl_array(coef),
                                             _dbl_array(coef2) if coef2 is not None else None, len(ks), C.byref(ctl.c), rows, D, code, st)
        self._check(rc, "xde_rows_stage_combine")

    def _rows_norm_control(self, ks, c_err, y0, y1, ctl, params, t_span_dev, *, e_pre=None):
        """Per row: the error ratio, the controller's verdict and next step, the next attempt's stage times.  One launch."""
        rows, D, code, st = self._rows_call("_rows_norm_control", ctl, y0, y0, y1, e_pre, *ks)
        self._require_device(t_span_dev)
        rc = self.lib.xde_rows_norm_control(_ptr_array(ks), _dbl_array(c_err), len(ks), _ptr(e_pre), _ptr(y0), _ptr(y1), C.byref(ctl.c),
                                            C.byref(params), _ptr(t_span_dev), t_span_dev.numel(), rows, D, code, st)
        self._check(rc, "xde_rows_norm_control")

    def _rows_dense_commit(self, out, ks, mid, y0, y1, f1, ctl, params, t_span_dev):
        """Per accepted row: its output times inside the step into ``out[j, r]``, then ``y0 <- y1``, ``ks[0] <- f1``, the cursor, done."""
        rows, D, code, st = self._rows_call("_rows_dense_commit", ctl, y0, y0, y1, f1, *ks)
        self._require_device(out, t_span_dev)
        if not out.is_contiguous() or out.dtype != y0.dtype or tuple(out.shape) != (t_span_dev.numel(),) + tuple(y0.shape):
            raise XdeError("_rows_dense_commit: the solution is a contiguous [T, *y0.shape] tensor of the state's dtype")
        rc = self.lib.xde_rows_dense_commit(_ptr(out), _ptr_array(ks), _dbl_array(mid), len(ks), _ptr(y0), _ptr(y1), _ptr(ks[0]), _ptr(f1),
                                            C.byref(ctl.c), C.byref(params), _ptr(t_span_dev), t_span_dev.numel(), rows, D, code, st)
        self._check(rc, "xde_rows_dense_commit")

    def _rows_scaled_norm(self, out, a, b, y0, rtol, atol):
        """``out[r] = rms((a[r] - b[r]) / (atol + |y0[r]| * rtol))`` (``b`` None: ``a[r]``), a float64 per row.  One launch."""
        self._require_device(out, a, b, y0)
        _require_alike("_rows_scaled_norm", "state operands", y0, (a, b))
        rows = y0.shape[0]
        if y0.dim() < 2 or not y0.is_contiguous() or out.dtype != torch.float64 or out.numel() != rows or not out.is_contiguous():
            raise XdeError("_rows_scaled_norm: the state is a contiguous [rows, ...] tensor and out a float64 [rows]")
        rc = self.lib.xde_rows_scaled_norm(_ptr(out), _ptr(a), _ptr(b), _ptr(y0), float(rtol), float(atol), rows, y0.numel() // rows,
                                           dtype_code(y0.dtype), self._stream(y0))
        self._check(rc, "xde_rows_scaled_norm")

    # -- per-sample output times of a joint solve (include/xde_hip_teval.h) --------------------------------------------------------------
    # Private for the reason _interp_rows is.  Only solver/_rk_teval.py calls these.  ``tq`` is float64 ``[rows, Q]`` (time-dtype values),
    # ``cnt`` int32 ``[rows]``; the step ``(t0, t1]`` and its ``dt`` are host floats.
    def _teval_call(self, who, big, tq, cnt, like, operands):
        """The operand check the two entry points share; nothing is launched here.  Returns ``(rows, D, Q, dtype code, stream)``."""
        self._require_device(big, tq, cnt, like, *operands)
        if like.dim() < 2 or not like.is_contiguous():
            raise XdeError("{}: the state is a contiguous [rows, ...] tensor (got {})".format(who, tuple(like.shape)))
        rows = like.shape[0]
        _require_alike(who, "state operands", like, operands)
        if tq.dim() != 2 or tq.shape[0] != rows or tq.dtype != torch.float64 or not tq.is_contiguous():
            raise XdeError("{}: tq is a contiguous float64 [rows, Q] tensor with rows = {}".format(who, rows))
        Q = tq.shape[1]
        if cnt.dtype != torch.int32 or tuple(cnt.shape) != (rows,) or not cnt.is_contiguous():
            raise XdeError("{}: cnt is a contiguous int32 [rows] tensor".format(who))
        if not big.is_contiguous() or big.dtype != like.dtype or tuple(big.shape) != (Q,) + tuple(like.shape):
            raise XdeError("{}: out / g is a contiguous [Q, *state.shape] tensor of the state's dtype".format(who))
        return rows, like.numel() // rows, Q, dtype_code(like.dtype), self._stream(like)

    def _teval_dense(self, out, tq, cnt, ks, mid, y0, y1, f0, f1, t0, t1, dt, direction, time_dtype):
        """``out[q, r]`` <- row r of the step's dense output at ``tq[r, q]``, for the queries of row r inside ``(t0, t1]``.  One launch."""
        rows, D, Q, code, st = self._teval_call("_teval_dense", out, tq, cnt, y0, [y1, f0, f1] + list(ks))
        rc = self.lib.xde_teval_dense(_ptr(out), _ptr(tq), _ptr(cnt), _ptr_array(ks), _dbl_array(mid), len(ks), _ptr(y0), _ptr(y1), _ptr(f0),
                                      _ptr(f1), float(t0), float(t1), float(dt), int(direction), int(time_dtype), rows, D, Q, code, st)
        self._check(rc, "xde_teval_dense")

    def _teval_cotangent(self, outs, g, tq, cnt, t0, t1, dt, direction, time_dtype, acc_mask=0):
        """outs = [y0, y1, y_mid, f0, f1] cotangents (None: not written) <- the cotangents ``g[q, r]`` of the queries inside ``(t0, t1]``;
        bit k of ``acc_mask``: outs[k] accumulates.  One launch."""
        like = next(o for o in outs if o is not None)
        rows, D, Q, code, st = self._teval_call("_teval_cotangent", g, tq, cnt, like, [o for o in outs if o is not None])
        rc = self.lib.xde_teval_cotangent((C.c_void_p * 5)(*[_ptr(o) for o in outs]), _ptr(g), _ptr(tq), _ptr(cnt), float(t0), float(t1),
                                          float(dt), int(direction), int(time_dtype), int(acc_mask) & 0x1F, rows, D, Q, code, st)
        self._check(rc, "xde_teval_cotangent")

    # -- the seam between two attempts as one resident launch (include/xde_hip_seam.h) ------------------------------------------------
    # Private for the reason _interp_rows is: the public methods are the contract tests/_cpu_double.py mirrors.  Only AdaptiveRKSolver
    # (options["seam"]) calls these.
    SEAM_SPIN_LIMIT = 4_000_000  # polls of the grid barrier before a workgroup gives up (seconds, not microseconds)

    def _seam_plan(self, n, dtype):
        """The launch plan of ``_seam_attempt`` for an ``n``-element state of ``dtype`` on the current device, as a dict of
        xde_seam_plan_t's fields.  Nothing is enqueued."""
        plan = XdeSeamPlan()
        self._check(self.lib.xde_seam_plan(int(n), dtype_code(dtype), C.byref(plan)), "xde_seam_plan")
        return _plan_dict(plan)

    def _seam_state(self, ctrl):
        key = ctrl.data_ptr()
        st = self._seam_states.get(key)
        if st is None:
            st = self._seam_states[key] = torch.zeros(int(self.lib.xde_seam_state_bytes()), dtype=torch.uint8, device=ctrl.device)
            weakref.finalize(ctrl, self._seam_states.pop, key, None)
        return st

    def _seam_attempt(self, k_last, c_last, e_pre, y0, f0, y1, out, a21, ws, ctrl, params, t_span_dev, step_t_dev, t_stage, *,
                      y0_alt=None, f0_alt=None):
        """Error norm of the attempt (e_pre form) + controller + ``out = y0' + f0' (a21 dt')``, the next attempt's first stage input, in
        ONE launch; (y0', f0') = (y1, k_last) when the controller accepts, the attempt's own (y0, f0) otherwise."""
        self._require_device(k_last, e_pre, y0, f0, y1, out, ws, ctrl, t_span_dev, t_stage, y0_alt, f0_alt)
        m = self._mirrors.get(ctrl.data_ptr())
        rc = self.lib.xde_seam_attempt(k_last.data_ptr(), float(c_last), e_pre.data_ptr(), y0.data_ptr(), _ptr(y0_alt), f0.data_ptr(),
                                       _ptr(f0_alt), y1.data_ptr(), out.data_ptr(), float(a21), y0.numel(), dtype_code(y0.dtype),
                                       ws.data_ptr(), self._seam_state(ctrl).data_ptr(), ctrl.data_ptr(), C.byref(params),
                                       t_span_dev.data_ptr(), _ptr(step_t_dev), t_stage.data_ptr(), m.ptr if m is not None else None,
                                       self.SEAM_SPIN_LIMIT, self._stream(y0))
        self._check(rc, "xde_seam_attempt")
        if m is not None and not self._is_capturing():
            m.seq += 1

    def _seam_expired(self, ctrl):
        """Tag (controller launch number) of the first seam launch on ``ctrl`` whose grid barrier expired, 0 = none.  Blocking."""
        st = self._seam_states.get(ctrl.data_ptr())
        if st is None:
            return 0
        tag = C.c_int64(0)
        self._check(self.lib.xde_seam_expired(st.data_ptr(), C.byref(tag), self._stream(ctrl)), "xde_seam_expired")
        return int(tag.value)

    # -- cdeint's vector field (include/xde_hip_cde.h) ----------------------------------------------------------------------------------
    # Private for the reason _interp_rows is: the public methods are the contract tests/_cpu_double.py mirrors.  Only CdeContractFn
    # (xde/base_cde.py) calls these.
    def _launch_time(self, who, t, like):
        """``t`` as a launch takes it, ``(t_dev, t_host, time_dtype)``: ONE float32 / float64 element on ``like``'s device (read by the
        kernel: no host synchronisation, and a captured launch replays with its current value) or a Python number."""
        if not torch.is_tensor(t):
            return None, float(t), XDE_F64
        self._require_device(t)
        if t.numel() != 1 or t.dtype not in (torch.float32, torch.float64) or t.device != like.device:
            raise XdeError("{}: t must be ONE float32 / float64 element on the series' device (got shape {}, {}, {})".format(
                who, tuple(t.shape), t.dtype, t.device))
        return t.data_ptr(), 0.0, dtype_code(t.dtype)

    def _cde_launch(self, who, out, src, series, coef, knots, t, method):
        """One launch of ``xde<who>``: the control's rows ``[B, Tn, C]`` — ``series`` of the ``method`` spline, or ``series, coef`` = ``Y,
        M`` of the natural control (``method`` None) — ``knots [Tn]``, the big operand ``[B, H, C]`` (``out`` of a ``_backward``, else
        ``src``) and the small one ``[B, H]`` contiguous on one device in one dtype; ``t`` as ``_launch_time`` takes it."""
        natural = coef is not None
        big, small = (out, src) if who.endswith("_backward") else (src, out)
        if natural:
            self._spline_operands(who, out, src, series, coef, knots)
        else:
            self._spline_operands(who, out, src, series, knots)
        if series.dim() != 3 or big.dim() != 3 or small.dim() != 2:
            raise XdeError("{}: expected {} [B, Tn, C], F [B, H, C] and out [B, H]".format(who, "Y, M" if natural else "series"))
        B, Tn, C_ = series.shape
        H = big.shape[1]
        agree = tuple(big.shape) == (B, H, C_) and tuple(small.shape) == (B, H) and tuple(knots.shape) == (Tn,)
        if not agree or (natural and coef.shape != series.shape):
            rows = "Y {}, M {}".format(tuple(series.shape), tuple(coef.shape)) if natural else "series {}".format(tuple(series.shape))
            raise XdeError("{}: shapes do not agree: {}, knots {}, F {}, out {}".format(
                who, rows, tuple(knots.shape), tuple(big.shape), tuple(small.shape)))
        t_dev, t_host, tt = self._launch_time(who, t, series)
        sym = "xde" + who
        fn, dt, st = getattr(self.lib, sym), dtype_code(series.dtype), self._stream(series)
        if natural:
            rc = fn(out.data_ptr(), src.data_ptr(), series.data_ptr(), coef.data_ptr(), knots.data_ptr(), t_dev, t_host, tt, B, H, C_, Tn,
                    dt, st)
        else:
            rc = fn(out.data_ptr(), src.data_ptr(), series.data_ptr(), knots.data_ptr(), t_dev, t_host, tt, B, H, C_, Tn,
                    HISTORY_METHODS[method], dt, st)
        self._check(rc, sym)

    def _cde_contract(self, out, F, series, knots, t, method):
        """``out[b, h] = sum_c F[b, h, c] * dX[b, c]`` with ``dX`` the derivative at ``t`` of the ``method`` ("linear" | "cubic") spline
        through ``series`` over ``knots``, in the summation order of include/xde_hip_cde.h.  One launch; dX is never written."""
        self._cde_launch("_cde_contract", out, F, series, None, knots, t, method)

    def _cde_contract_backward(self, gF, gout, series, knots, t, method):
        """``gF[b, h, c] = gout[b, h] * dX[b, c]``: the cotangent of ``_cde_contract``'s F.  One launch."""
        self._cde_launch("_cde_contract_backward", gF, gout, series, None, knots, t, method)

    def _cde_plan(self, backward, big, B, H, channels):
        """The launch plan of ``_cde_contract`` (``backward`` false: ``big`` is F) or ``_cde_contract_backward`` (``big`` is gF) for
        ``[B, H, channels]``, ``big``'s dtype and its alignment, as a dict of xde_cde_plan_t's fields.  Nothing is enqueued."""
        plan = XdeCdePlan()
        rc = self.lib.xde_cde_plan(int(bool(backward)), big.data_ptr(), int(B), int(H), int(channels), dtype_code(big.dtype), C.byref(plan))
        self._check(rc, "xde_cde_plan")
        return _plan_dict(plan)

    # -- the natural cubic spline control (include/xde_hip_spline.h) -------------------------------------------------------------------
    # Private for the reason the _cde_* methods are.  NaturalCubicSpline (interpolation) and CdeContractFn (xde/base_cde.py) call these.
    def _spline_operands(self, who, *tensors):
        self._require_device(*tensors)
        first = tensors[0]
        for x in tensors:
            if not x.is_contiguous() or x.dtype != first.dtype or x.device != first.device:
                raise XdeError("{}: the operands must be contiguous tensors of one dtype on one device".format(who))

    def _spline_natural_coeffs(self, Y, M, series, knots):
        """``Y, M [B, Tn, C]`` of the natural cubic spline through the observed (non-NaN) entries of ``series [B, Tn, C]`` over
        ``knots [Tn]``: the end rule, the Thomas solve and the fill of include/xde_hip_spline.h.  One launch."""
        who = "_spline_natural_coeffs"
        self._spline_operands(who, Y, M, series, knots)
        if series.dim() != 3 or Y.shape != series.shape or M.shape != series.shape or tuple(knots.shape) != (series.shape[1],):
            raise XdeError("{}: expected series, Y, M [B, Tn, C] and knots [Tn], got {}, {}, {}, {}".format(
                who, tuple(series.shape), tuple(Y.shape), tuple(M.shape), tuple(knots.shape)))
        B, Tn, C_ = series.shape
        rc = self.lib.xde_spline_natural_coeffs(Y.data_ptr(), M.data_ptr(), series.data_ptr(), knots.data_ptr(), B, Tn, C_,
                                                dtype_code(series.dtype), self._stream(series))
        self._check(rc, "xde_spline_natural_coeffs")

    def _spline_natural_gather(self, val, der, Y, M, knots, tq):
        """``val, der [..., L, D]`` of the path ``(Y, M [..., Tn, D], knots [Tn])`` at the query times ``tq [L]`` (``der`` may be
        None): history_gather's layout, the bits the contraction builds dX from."""
        who = "_spline_natural_gather"
        self._spline_operands(who, *[x for x in (val, der, Y, M, knots, tq) if x is not None])
        if val.numel() == 0:
            return
        Tn, D = Y.shape[-2], Y.shape[-1]
        if M.shape != Y.shape or tuple(knots.shape) != (Tn,) or tuple(val.shape) != tuple(Y.shape[:-2]) + (tq.numel(), D) or (
                der is not None and der.shape != val.shape):
            raise XdeError("{}: shapes do not agree: Y {}, M {}, knots {}, tq {}, val {}".format(
                who, tuple(Y.shape), tuple(M.shape), tuple(knots.shape), tuple(tq.shape), tuple(val.shape)))
        rc = self.lib.xde_spline_natural_gather(val.data_ptr(), _ptr(der), Y.data_ptr(), M.data_ptr(), knots.data_ptr(), tq.data_ptr(),
                                                Y.numel() // (Tn * D), Tn, tq.numel(), D, dtype_code(Y.dtype), self._stream(Y))
        self._check(rc, "xde_spline_natural_gather")

    def _cde_contract_natural(self, out, F, Y, M, knots, t):
        """``_cde_contract`` with ``dX`` the derivative at ``t`` of the natural cubic spline ``(Y, M, knots)``.  One launch."""
        self._cde_launch("_cde_contract_natural", out, F, Y, M, knots, t, None)

    def _cde_contract_natural_backward(self, gF, gout, Y, M, knots, t):
        """``gF[b, h, c] = gout[b, h] * dX[b, c]``: the cotangent of ``_cde_contract_natural``'s F.  One launch."""
        self._cde_launch("_cde_contract_natural_backward", gF, gout, Y, M, knots, t, None)

    # -- the gradient with respect to the control path (include/xde_hip_cdegrad.h) -----------------------------------------------------
    # Private for the reason the _cde_* methods are.  CdeControlContractFn (xde/base_cde.py) and the differentiable splines
    # (interpolation) call these.
    def _cde_grad_launch(self, who, outs, gout, F, knots, t, method):
        """One launch of ``xde<who>``: the control's cotangents ``outs`` (each ``[B, Tn, C]``), ``gout [B, H]``, ``F [B, H, C]`` and ``knots
        [Tn]`` contiguous on one device in one dtype; ``t`` as ``_launch_time`` takes it; ``method`` None for the natural control."""
        self._spline_operands(who, *outs, gout, F, knots)
        Tn = outs[0].shape[1] if outs[0].dim() == 3 else -1
        if F.dim() != 3 or gout.dim() != 2 or tuple(gout.shape) != tuple(F.shape[:2]) or tuple(knots.shape) != (Tn,):
            raise XdeError("{}: expected gout [B, H], F [B, H, C] and knots [Tn], got {}, {}, {}".format(
                who, tuple(gout.shape), tuple(F.shape), tuple(knots.shape)))
        B, H, C_ = F.shape
        for o in outs:
            if tuple(o.shape) != (B, Tn, C_):
                raise XdeError("{}: the control's cotangent must be [B, Tn, C] = {}, got {}".format(who, (B, Tn, C_), tuple(o.shape)))
        t_dev, t_host, tt = self._launch_time(who, t, F)
        tail = (dtype_code(F.dtype), self._stream(F))
        if method is not None:
            tail = (HISTORY_METHODS[method],) + tail
        rc = getattr(self.lib, "xde" + who)(*[o.data_ptr() for o in outs], gout.data_ptr(), F.data_ptr(), knots.data_ptr(), t_dev, t_host,
                                            tt, B, H, C_, Tn, *tail)
        self._check(rc, "xde" + who)

    def _cde_control_grad(self, gSeries, gout, F, knots, t, method):
        """``gSeries[b, k, c]``: the cotangent of the ``method`` ("linear" | "cubic") control's series in ``_cde_contract``, from ``gout
        [B, H]`` and ``F [B, H, C]`` — ``gdX = sum_h gout * F`` scattered to the rows ``X'(t)`` read, ``+0`` elsewhere.  One launch that
        writes every element of ``gSeries`` once."""
        self._cde_grad_launch("_cde_control_grad", (gSeries,), gout, F, knots, t, method)

    def _cde_control_grad_natural(self, gY, gM, gout, F, knots, t):
        """``gY, gM [B, Tn, C]``: the cotangents of the natural control's ``Y`` and ``M`` in ``_cde_contract_natural``.  One launch."""
        self._cde_grad_launch("_cde_control_grad_natural", (gY, gM), gout, F, knots, t, None)

    def _cde_control_grad_plan(self, F, B, H, channels):
        """The launch plan of ``_cde_control_grad`` / ``_natural`` for ``[B, H, channels]``, ``F``'s dtype and its alignment, as a dict
        of xde_cdegrad_plan_t's fields.  Nothing is enqueued."""
        plan = XdeCdeGradPlan()
        rc = self.lib.xde_cde_control_grad_plan(F.data_ptr(), int(B), int(H), int(channels), dtype_code(F.dtype), C.byref(plan))
        self._check(rc, "xde_cde_control_grad_plan")
        return _plan_dict(plan)

    def _spline_natural_coeffs_backward(self, gSeries, gY, gM, series, knots):
        """``gSeries [B, Tn, C]`` from the cotangents ``gY, gM`` of ``_spline_natural_coeffs``'s outputs: its transpose.  ``series`` is
        read for its NaN pattern; an unobserved entry gets ``+0``.  One launch (its workspace comes from torch's allocator)."""
        who = "_spline_natural_coeffs_backward"
        self._spline_operands(who, gSeries, gY, gM, series, knots)
        if series.dim() != 3 or not (gSeries.shape == gY.shape == gM.shape == series.shape) or tuple(knots.shape) != (series.shape[1],):
            raise XdeError("{}: expected gSeries, gY, gM, series [B, Tn, C] and knots [Tn], got {}, {}, {}, {}, {}".format(
                who, tuple(gSeries.shape), tuple(gY.shape), tuple(gM.shape), tuple(series.shape), tuple(knots.shape)))
        B, Tn, C_ = series.shape
        need = self.lib.xde_spline_natural_coeffs_backward_workspace_bytes(B, Tn, C_, dtype_code(series.dtype))
        ws = torch.empty(need // series.element_size(), dtype=series.dtype, device=series.device)
        rc = self.lib.xde_spline_natural_coeffs_backward(gSeries.data_ptr(), gY.data_ptr(), gM.data_ptr(), series.data_ptr(),
                                                         knots.data_ptr(), ws.data_ptr(), B, Tn, C_, dtype_code(series.dtype),
                                                         self._stream(series))
        self._check(rc, "xde_spline_natural_coeffs_backward")

    def _spline_natural_gather_backward(self, gY, gM, gval, gder, knots, tq):
        """``gY, gM [..., Tn, D]`` from the cotangents ``gval`` and / or ``gder [..., L, D]`` (either may be None) of
        ``_spline_natural_gather`` at ``tq [L]``: its transpose.  One launch, one owner per column."""
        who = "_spline_natural_gather_backward"
        self._spline_operands(who, *[x for x in (gY, gM, gval, gder, knots, tq) if x is not None])
        g = gval if gval is not None else gder
        if g is None:
            raise XdeError("{}: needs gval or gder".format(who))
        Tn, D = gY.shape[-2], gY.shape[-1]
        if gM.shape != gY.shape or tuple(knots.shape) != (Tn,) or tuple(g.shape) != tuple(gY.shape[:-2]) + (tq.numel(), D) or (
                gval is not None and gder is not None and gval.shape != gder.shape):
            raise XdeError("{}: shapes do not agree: gY {}, gM {}, knots {}, tq {}, cotangent {}".format(
                who, tuple(gY.shape), tuple(gM.shape), tuple(knots.shape), tuple(tq.shape), tuple(g.shape)))
        if gY.numel() == 0:
            return
        rc = self.lib.xde_spline_natural_gather_backward(gY.data_ptr(), gM.data_ptr(), _ptr(gval), _ptr(gder), knots.data_ptr(),
                                                         tq.data_ptr(), gY.numel() // (Tn * D), Tn, tq.numel(), D, dtype_code(gY.dtype),
                                                         self._stream(gY))
        self._check(rc, "xde_spline_natural_gather_backward")

    def hermite_gather(self, val, der, his, his_t, lags):
        """his [..., T, D] (contiguous), his_t [T], lags [L]  ->  val, der [..., L, D]."""
        self._require_device(val, der, his, his_t, lags)
        if val.numel() == 0:  # (an empty batch or no lags: nothing to write, and empty tensors have no storage to point at)
            return
        T, D = his.shape[-2], his.shape[-1]
        outer = his.numel() // (T * D) if T * D else 0
        rc = self.lib.xde_hermite_gather(val.data_ptr(), der.data_ptr(), his.data_ptr(), his_t.data_ptr(), lags.data_ptr(), outer,
                                         T, D, lags.numel(), dtype_code(his.dtype), self._stream(his))
        self._check(rc, "xde_hermite_gather")

    def history_gather(self, val, der, his, his_t, lags, method):
        """his [..., T, D] (contiguous), his_t [T], lags [L]  ->  val, der [..., L, D] of the history spline `method`
        ("cubic" | "linear" | "bez")."""
        self._require_device(val, der, his, his_t, lags)
        if val.numel() == 0:
            return
        T, D = his.shape[-2], his.shape[-1]
        outer = his.numel() // (T * D) if T * D else 0
        rc = self.lib.xde_history_gather(val.data_ptr(), der.data_ptr(), his.data_ptr(), his_t.data_ptr(), lags.data_ptr(), outer, T, D,
                                         lags.numel(), dtype_code(his.dtype), HISTORY_METHODS[method], self._stream(his))
        self._check(rc, "xde_history_gather")

    def lag_grad(self, grad_y, der):
        """sum over every axis but the lag axis of grad_y * der ([..., L, D] both, contiguous) -> [L], one launch."""
        self._require_device(grad_y, der)
        L, D = der.shape[-2], der.shape[-1]
        outer = der.numel() // (L * D) if L * D else 0
        if L == 0 or outer == 0:
            return torch.zeros(L, dtype=der.dtype, device=der.device)
        out = torch.empty(L, dtype=der.dtype, device=der.device)
        # per STREAM: the workspace holds the arrival counters and the partials of a launch in flight — two launches of the same L on
        # different streams (autograd on a side stream, two models) must not meet on them; same-stream launches are ordered
        key = (der.device.index, L, self._stream(der))
        ws = self._lag_ws.get(key)
        if ws is None:
            ws = self._lag_ws[key] = torch.zeros(int(self.lib.xde_lag_grad_workspace_bytes(L)), dtype=torch.uint8, device=der.device)
        rc = self.lib.xde_lag_grad(out.data_ptr(), grad_y.data_ptr(), der.data_ptr(), outer, D, L, dtype_code(der.dtype), ws.data_ptr(),
                                   self._stream(der))
        self._check(rc, "xde_lag_grad")
        return out

    def pack_segments(self, flat, tensors, segs, scales=None):
        """``flat`` (16-byte-aligned segments, pads zero) <- the contiguous device tensors ``tensors`` at ``segs`` = [(start, len)], one
        launch.  Returns False (nothing done) when the call does not fit the kernel: the caller packs with framework ops then."""
        n = len(tensors)
        if n < 1 or n > XDE_MAX_PACK or not flat.is_cuda or flat.dtype not in (torch.float32, torch.float64):
            return False
        if len(segs) != n:
            return False
        for x, (_, length) in zip(tensors, segs):
            # (a member whose element count is not its segment's — a func that returned a wrong-shaped or broadcastable member —
            # must not reach the kernel, which reads `length` elements from it: the framework-op pack raises, or broadcasts, as before)
            if x.dtype != flat.dtype or x.device != flat.device or not x.is_contiguous() or x.numel() != int(length):
                return False
        srcs = (C.c_void_p * n)(*[x.data_ptr() if x.numel() else None for x in tensors])
        starts = (C.c_int64 * n)(*[int(s) for s, _ in segs])
        lens = (C.c_int64 * n)(*[int(l) for _, l in segs])
        sc = _dbl_array(scales) if scales is not None else None
        rc = self.lib.xde_pack_segments(flat.data_ptr(), srcs, starts, lens, sc, n, flat.numel(), dtype_code(flat.dtype), self._stream(flat))
        self._check(rc, "xde_pack_segments")
        return True

    def dense_commit(self, out_base, ks, mid, y0, y1, f1, ctrl, t_span_dev, time_dtype):
        """dense_eval + commit in one launch (graph pipeline): rows of the last accepted step, then (y0, ks[0]) <- (y1, f1)."""
        self._require_device(out_base, y0, y1, f1, ctrl, t_span_dev, *ks)
        if y0.numel() == 0:
            return
        rc = self.lib.xde_dense_commit(out_base.data_ptr(), _ptr_array(ks), _dbl_array(mid), len(ks), y0.data_ptr(), y1.data_ptr(),
                                       ks[0].data_ptr(), f1.data_ptr(), ctrl.data_ptr(), t_span_dev.data_ptr(), time_dtype,
                                       y0.numel(), dtype_code(y0.dtype), self._stream(y0))
        self._check(rc, "xde_dense_commit")

    def commit(self, ctrl, y0_dst, y1_src, f0_dst, f1_src):
        self._require_device(ctrl, y0_dst, y1_src, f0_dst, f1_src)
        if y0_dst.numel() == 0:
            return
        rc = self.lib.xde_commit(ctrl.data_ptr(), y0_dst.data_ptr(), y1_src.data_ptr(), f0_dst.data_ptr(), f1_src.data_ptr(),
                                 y0_dst.numel(), dtype_code(y0_dst.dtype), self._stream(y0_dst))
        self._check(rc, "xde_commit")

    # -- hipGraph capture of one attempted step ---------------------------------------------------
    class _Graph:
        def __init__(self, backend, graph, ctrl, launches=1):
            self.backend, self.graph, self.ctrl, self.launches = backend, graph, ctrl, int(launches)

        def replay(self):
            """Launch the graph; returns one read handle per controller launch it holds, in order."""
            self.graph.replay()
            m = self.backend._mirrors.get(self.ctrl.data_ptr())
            if m is None:
                return []
            first = m.seq + 1
            m.seq += self.launches
            return [(m, first + i) for i in range(self.launches)]

    def capture(self, body, ctrl, launches=1):
        """Record ``body()`` (kernels of this library + the framework ops of the user's func) into a hipGraph; ``launches`` =
        controller launches ``body`` makes (attempted steps per replay)."""
        from .utils.graphed import CapturedGraph

        g = CapturedGraph()  # (replays of a graph that holds memset nodes are synchronised: see its docstring)
        self._tls.capturing = True
        try:
            with g.capture(capture_error_mode="thread_local"):  # other host threads may keep using the device meanwhile
                body()
        finally:
            self._tls.capturing = False
        g.finish()
        return HipBackend._Graph(self, g, ctrl, launches)

    # -- profiling ---------------------------------------------------------------------------
    def prof_enable(self, period=1):
        """0/False: off; p >= 1: time every p-th launch of each kernel with dispatch-stamped HIP events."""
        self._check(self.lib.xde_prof_enable(int(period)), "xde_prof_enable")

    def prof_collect(self):
        n = len(KID_NAMES)
        counts = (C.c_int64 * n)()
        ms = (C.c_double * n)()
        by = (C.c_double * n)()
        self._check(self.lib.xde_prof_collect(counts, ms, by), "xde_prof_collect")
        return {KID_NAMES[i]: {"launches": int(counts[i]), "ms": float(ms[i]), "bytes": float(by[i])} for i in range(n)}


def _row_geometry(dst, like):
    """(outer, chunk, row_stride) of a destination row block with ``like``'s shape: contiguous, or ``[..., L, D]`` cut from a contiguous
    ``[..., T*L, D]`` (lead dimensions that collapse into one stride)."""
    if dst.shape != like.shape or dst.dtype != like.dtype:
        raise XdeError("_interp_rows: a destination row has another shape or dtype than the operands")
    n = like.numel()
    if dst.is_contiguous():
        return 1, n, n
    if dst.dim() < 3 or dst.stride(-1) != 1 or dst.stride(-2) != dst.shape[-1]:
        raise XdeError("_interp_rows: a destination row must be a [..., L, D] block of a contiguous [..., T*L, D] solution")
    chunk = dst.shape[-1] * dst.shape[-2]
    row_stride = dst.stride(-3)
    for i in range(dst.dim() - 4, -1, -1):
        if dst.shape[i] > 1 and dst.stride(i) != dst.stride(i + 1) * dst.shape[i + 1]:
            raise XdeError("_interp_rows: the lead dimensions of a destination row do not collapse into one stride")
    if row_stride < chunk:
        raise XdeError("_interp_rows: destination rows overlap")
    return n // chunk if chunk else 0, chunk, row_stride


_backend = None


def get_backend():
    """The HIP backend (created on first use).  Raises loudly when the library is not built."""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    return _backend


def _set_backend_for_testing(backend):
    """TEST HOOK ONLY (tests/ inject a CPU double to exercise host logic without a GPU).

    Product code never calls this; passing None restores the HIP backend.
    """
    global _backend
    _backend = backend
