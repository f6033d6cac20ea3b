/*
 * xde_hip_seam.h — entry points of libxde_hip.so for the seam between two attempted steps of an embedded FSAL pair (Dopri5): the error
 * norm of attempt n, the step controller, and the FIRST stage combine of attempt n + 1 as ONE launch whose workgroups stay resident
 * across a grid barrier (host side: paddlexde_amd/solver/base_adaptive_solver_rk.py, options["seam"]).
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*, XDE_F32 /
 * XDE_F64).  Arguments are validated on the host before anything is enqueued: a refused call writes nothing.
 *
 * WHAT IT REPLACES.  xde_error_norm_partial(e_pre form: k = {k_last}, one segment) -> xde_rk_control(ws) -> xde_stage_combine(out,
 * y0', {f0'}, {a21}, XDE_COMBINE_RK) with (y0', f0') = (y1, k_last) when the controller accepted and the attempt's own (y0, f0)
 * otherwise — three dependent launches, the third of which reads y1 and k_last a second time.  Here a lane keeps the y1 and k_last
 * vectors it reduced in registers across the barrier and writes `out` from them.
 *
 * SAME BITS.  The launch runs the grid xde_error_norm_partial takes for the segment (one 256-lane workgroup per partial record), every
 * lane visits the elements that launch's lane visits, in its order (fp32 per lane -> fp64 -> shuffle tree -> LDS), and the records land
 * in the same slots of `ws`.  After the barrier EVERY workgroup reduces the records in xde_rk_control's fixed order and runs its
 * controller (the device code is shared); workgroup 0 alone writes the control block, the host mirror and `t_stage_out`.
 * out = y0' + f0' * (T(a21) * dt') is xde_stage_combine's arithmetic with the dt' the controller has just planned.
 *
 * RESIDENCY.  A plain launch.  Every workgroup must be resident at once: the grid is checked against (blocks per CU from the
 * occupancy query, at most 2) x (CUs of the device), proven once per device and kernel variant and cached, and a lane carries at most
 * XDE_SEAM_CAP 16-byte vectors per array; a state that does not fit is refused (xde_seam_plan says so without launching).
 *
 * THE BARRIER.  Records are stored write-through and drained, then the workgroup takes a ticket of the two-level arrival counter in
 * `ws` (16 first-level shards, blocks b and b + 16 share one); the last arriver re-arms the counter and stores the launch's tag
 * (ctrl->seq + 1: device-resident and strictly increasing, so a replayed launch tags itself) into the 16 generation words of `state`;
 * every other workgroup's first lane polls its shard's word with relaxed loads and s_sleep, at most `spin_limit` times.  On expiry —
 * or when an earlier launch on this `state` expired — the workgroup adds one to the non-finite count its controller sees, so the solve
 * stops with XDE_STATUS_NONFINITE, and records the tag in `state` (sticky; xde_seam_expired reads it: the host names the barrier, not
 * the state).  No wait is unbounded.
 *   state: xde_seam_state_bytes() bytes of device memory, zero before the first use, one per control block.
 */
#ifndef XDE_HIP_SEAM_H
#define XDE_HIP_SEAM_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_SEAM_CAP 16 /* 16-byte vectors of y1 (and of k_last) one lane carries across the barrier */

typedef struct xde_seam_plan {
  int32_t blocks;    /* workgroups = partial records (xde_error_norm_partial's grid for the segment) */
  int32_t per_lane;  /* 16-byte vectors per array the busiest lane carries */
  int32_t resident;  /* workgroups of this kernel the device holds at once (0: no device to ask) */
  int32_t fits;      /* blocks <= resident and per_lane <= XDE_SEAM_CAP */
} xde_seam_plan_t;

int64_t xde_seam_state_bytes(void);

/* The launch plan for an n-element state of `dtype`.  Nothing is enqueued; without a device `resident` and `fits` are 0. */
int xde_seam_plan(int64_t n, int dtype, xde_seam_plan_t* plan_out);

/*
 * k_last / c_last: the FSAL derivative f1 and its error coefficient; e_pre: the partial error sum the last stage's combine wrote;
 * y0 / f0 (and y0_alt / f0_alt, both or neither: the speculative pipeline's candidates, picked by ctrl->accept as the launch finds it):
 * the state the attempt started from; y1: its proposal.  out: n elements, may alias e_pre.  a21: the tableau's beta[0][0].
 * rtol / atol / norm kind / dtypes come from params (n_seg must be 1).  Everything else as xde_rk_control.
 */
int xde_seam_attempt(const void* k_last, double c_last, const void* e_pre, const void* y0, const void* y0_alt, const void* f0,
                     const void* f0_alt, const void* y1, void* out, double a21, int64_t n, int dtype, void* ws, void* state,
                     xde_ctrl_t* ctrl, const xde_ctrl_params_t* params, const double* t_span_dev, const double* step_t_dev,
                     void* t_stage_out, xde_ctrl_t* host_mirror, int64_t spin_limit, void* stream);

/* *tag_out = tag of the first launch on `state` whose barrier expired, 0 = none.  Blocking (copy + stream synchronise). */
int xde_seam_expired(const void* state, int64_t* tag_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XDE_HIP_SEAM_H */
