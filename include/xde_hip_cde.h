/*
 * xde_hip_cde.h — entry points of libxde_hip.so for cdeint: the vector field of a neural controlled differential equation
 * dz = F(t, z) dX(t), the batched contraction of the user's F[B, H, C] with the time derivative dX[B, C] of the control spline X
 * through a series[B, Tn, C] — and its cotangent (host side: paddlexde_amd/functional/cdeint.py, paddlexde_amd/xde/base_cde.py).
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64, XDE_HISTORY_*).  Arguments are validated on the host before anything is enqueued: a refused call writes nothing.
 * All arrays are contiguous, in the state dtype `dtype`; `knots[Tn]` are the series' times.
 *
 * THE TIME.  `t_dev`, when not null, points at ONE element of `time_dtype` (XDE_F32 or XDE_F64) in device memory, and the kernel reads
 * it: no host synchronisation, and a captured launch replays with whatever the element holds then.  With `t_dev` null the time is
 * `t_host` (`time_dtype` is still checked).  Either way tau = (state dtype)(t) — the time is converted to the series dtype first, as
 * InterpolationBase._gather does.
 *
 * dX[b, c] is, op for op, the `der` that xde_history_gather writes for outer = B, L = 1, lags = {tau}, D = C with the same method (the
 * same device functions): index = clip(bucketize(tau) - 1, 0, Tn - 1), the reference's scale conventions as written.
 * XDE_HISTORY_LINEAR and XDE_HISTORY_CUBIC are served; XDE_HISTORY_BEZIER is refused (its sliding four-row window is not a path
 * through the data).  dX is never written to memory.
 *
 * ARITHMETIC.  Products and sums in the state dtype, rounded op by op (the library is built with -ffp-contract=off).  THE SUMMATION
 * ORDER over c depends on C and the dtype only — not on B, H, the grid or pointer alignment.  With W = 4 (fp32) or 2 (fp64) elements
 * per 16 bytes, NV = ceil(C / W) vectors per row and R = min(64, the least power of two >= NV) lanes per (b, h) row:
 *
 *   lane j (0 <= j < R):  v_j = +0;  for each vector index q = j, j + R, j + 2R, ... < NV, for each c = q W, ..., min(q W + W, C) - 1
 *                         in ascending order:  v_j = v_j + F[b, h, c] * dX[b, c]
 *   then for off = R/2, R/4, ..., 1:  v_j = v_j + v_{j + off}  for every j < off      (a shuffle tree)
 *   out[b, h] = v_0
 *
 * Aligned operands with C % W == 0 are read as 16-byte vectors; anything else takes scalar loads with the same element-to-lane map
 * and the same bits.  No atomics.
 */
#ifndef XDE_HIP_CDE_H
#define XDE_HIP_CDE_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[b, h] = sum_c F[b, h, c] * dX[b, c] in the order above.  One launch; F is read once.  No overlap between out and the inputs.
 * Refused (XDE_EBADARG): a null out / F / series / knots, B < 1, H < 1, C < 1, Tn < 2, a dtype or time_dtype that is not XDE_F32 /
 * XDE_F64, a method that is not XDE_HISTORY_LINEAR / XDE_HISTORY_CUBIC, a pointer not aligned to its element type. */
int xde_cde_contract(void* out, const void* F, const void* series, const void* knots, const void* t_dev, double t_host, int time_dtype,
                     int64_t B, int H, int C, int Tn, int method, int dtype, void* stream);

/* gF[b, h, c] = gout[b, h] * dX[b, c]: the cotangent of F, one product per element, one launch.  (The contraction is linear in F; the
 * series, the knots and the time get no cotangent.)  Same checks. */
int xde_cde_contract_backward(void* gF, const void* gout, const void* series, const void* knots, const void* t_dev, double t_host,
                              int time_dtype, int64_t B, int H, int C, int Tn, int method, int dtype, void* stream);

/* THE LAUNCH PLAN.  What the host decides about a launch of either entry point from (B, H, C, dtype) and the 16-byte alignment of the
 * big operand: which kernel instantiation runs and how its rows are dealt to workgroups.  The bits of the result never depend on it;
 * it is reported so that a test can state which code a shape runs, whatever the tuning constants are. */
typedef struct xde_cde_plan {
  int32_t vec;           /* 16-byte vector loads / stores of the big operand (C % W == 0 and it is 16-byte aligned), else scalar */
  int32_t lds;           /* dX rows are kept in LDS (else recomputed per use: C is beyond the on-chip table) */
  int32_t grouped;       /* Gb > 1: consecutive batch rows share a work item */
  int32_t R;             /* forward: lanes per (b, h) row team; backward: 1 */
  int32_t single;        /* forward: a lane holds at most one vector of a row (else it strides along the row); backward: 0 */
  int32_t S, Hc;         /* slices of H per batch row, rows per slice (the last slice may be shorter) */
  int32_t Gb;            /* batch rows per work item (the last item may hold fewer) */
  int32_t rows_per_pass; /* rows of the big operand one workgroup covers before it walks on along its work item */
  int32_t nt;            /* forward: F is read with the streaming policy; backward: 0 */
  int64_t items;         /* work items: B * S, or ceil(B / Gb) */
  int64_t blocks;        /* workgroups launched: min(items, the grid cap); a workgroup takes items blocks apart */
} xde_cde_plan_t;

/* The plan of xde_cde_contract (backward == 0: `big` is F) or xde_cde_contract_backward (backward != 0: `big` is gF) into *plan, by
 * the function the launch itself uses.  Enqueues nothing and needs no device; `big` is used for its alignment only and never
 * dereferenced.  Refused (XDE_EBADARG): a null plan, B < 1, H < 1, C < 1, a dtype that is not XDE_F32 / XDE_F64, a `big` not aligned
 * to its element type. */
int xde_cde_plan(int backward, const void* big, int64_t B, int H, int C, int dtype, xde_cde_plan_t* plan);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_CDE_H */
