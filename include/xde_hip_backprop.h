/*
 * xde_hip_backprop.h — entry points of libxde_hip.so for back-propagation through the accepted steps of an adaptive solve
 * (odeint(..., options={"backprop": "steps"}); host side: paddlexde_amd/solver/_rk_backprop.py).
 *
 * The reference trains its adaptive solvers by back-propagating through the eager step ops
 * (solver/base_adaptive_solver_rk.py:150-170 keeps every stage in the graph; utils/ode_utils.py:85 keeps the controller out of
 * it).  Per accepted step, with lambda = dL/dy_{n+1} and nu_m = J_m^T mu_m the cotangent of stage input m:
 *     mu_i     = dt (b_i lambda + sum_{m>i} a_mi nu_m) + (dense-output terms) + [i = S] mu_0 of step n+1
 *     dL/dy_n  = lambda + sum_m nu_m + (dense-output terms)
 * Both are linear combinations of state-sized arrays: xde_stage_cotangent forms one (two from the same reads), and
 * xde_dense_cotangent turns the solution rows' cotangents of one step into the cotangents of the quartic's five operands.
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64 contiguous arrays of `n` elements; 16-byte-aligned pointers take the vector path, others a scalar path
 * with the same results).  Arguments are validated on the host before anything is enqueued.
 */
#ifndef XDE_HIP_BACKPROP_H
#define XDE_HIP_BACKPROP_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_BP_MAX_X (XDE_MAX_K + 2) /* operands of one xde_stage_cotangent: lambda, the nu_m, the dense terms */
#define XDE_BP_DENSE_OUTS 5          /* xde_dense_cotangent's outputs: y0, y1, y_mid, f0, f1 (in this order) */

/*
 * out[e]  = sum_j x[j][e] * coef[j]        (j = 0 .. nx-1, left to right, in the state dtype)
 * out2[e] = sum_j x[j][e] * coef2[j]       (only if out2 != NULL; coef2 required then)
 * The step size is folded into the coefficients by the caller.  `out` / `out2` may not alias an operand.
 */
int xde_stage_cotangent(void* out, void* out2, const void* const* x, const double* coef, const double* coef2, int nx, int64_t n,
                        int dtype, void* stream);

/*
 * Backward of the dense output of one accepted step (csrc/xde_dense.hip: quartic_) at its G output rows.
 * g_rows: the G cotangent rows, contiguous [G, n].  w: G x 5 weights, row-major: w[r*5 + k] is output k's weight of row r
 * (the quartic's weight of y0, y1, y_mid, f0, f1 at that row's x; the caller folds dt into the f0 / f1 weights).
 *     outs[k][e] = (acc_mask bit k ? outs[k][e] : 0) + sum_r g_rows[r][e] * w[r*5 + k]
 * A NULL outs[k] is not written.  Any G >= 1 (one launch per four rows; later launches accumulate).
 */
int xde_dense_cotangent(void* const* outs, const void* g_rows, const double* w, int G, uint32_t acc_mask, int64_t n, int dtype,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_BACKPROP_H */
