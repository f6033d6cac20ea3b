/*
 * xde_hip_spline.h — entry points of libxde_hip.so for the natural cubic spline as a control path of cdeint: irregular knots, partly
 * observed series (host side: paddlexde_amd/interpolation NaturalCubicSpline, paddlexde_amd/xde/base_cde.py).
 *
 * Same conventions as xde_hip.h and xde_hip_cde.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as
 * void*, XDE_F32 / XDE_F64).  Arguments are validated on the host before anything is enqueued: a refused call writes nothing, and
 * xde_last_error names the entry point.  All arrays are contiguous, in the one dtype `dtype`.
 *
 * THE PATH.  Per column (b, c) of series[B, Tn, C] over strictly increasing knots[Tn] (any spacing, Tn >= 2), all arithmetic in the
 * series dtype T, rounded op by op (the library is built with -ffp-contract=off; division is IEEE).  y_k = series[b, k, c],
 * t_k = knots[k].
 *
 *   OBSERVED means "not NaN".
 *   END RULE.  A NaN y_0 becomes the first observed value of the column, a NaN y_{Tn-1} the last observed one: the first and the last
 *     knot are always NODES, and so is every observed k in between.  A column with no observed value gives all-NaN rows of Y and M
 *     (the entry point cannot see device data; the Python class refuses such a series).
 *   SECOND DERIVATIVES M at the nodes.  Natural ends: M = 0 at the first and the last node.  Thomas algorithm over consecutive nodes
 *     a < i < b, ascending, with cp = dp = 0 at the first node:
 *         hl = t_i - t_a                      hr = t_b - t_i
 *         sl = (y_i - y_a) / hl               sr = (y_b - y_i) / hr
 *         rhs = 6 * (sr - sl)                 den = 2 * (hl + hr) - hl * cp_a
 *         cp_i = hr / den                     dp_i = (rhs - hl * dp_a) / den
 *     then descending over the interior nodes, b the node above i:   M_i = dp_i - cp_i * M_b.
 *   FILL.  Y and M are dense on the knot grid and describe the same piecewise cubic: at a node Y_k = y_k (after the end rule); at a
 *     missing j between consecutive nodes a < j < b, with h = t_b - t_a and s = t_j - t_a,
 *         M_j = M_a + (s / h) * (M_b - M_a)         Y_j = `val` below on the rows (a, b) with this h and s.
 *   EVALUATION at tau:
 *         i = clip(#{k : t_k <= tau} - 1, 0, Tn - 2)       h = t_{i+1} - t_i        s = tau - t_i
 *         sl = (Y_{i+1} - Y_i) / h
 *         d0 = sl - (h / 6) * (2 * M_i + M_{i+1})
 *         e  = (M_{i+1} - M_i) / h
 *         val = Y_i + s * (d0 + s * (M_i / 2 + (s / 6) * e))
 *         der = d0 + s * (M_i + (s / 2) * e)
 *     Outside the knots the first / last interval's cubic is continued (i is clipped); cdeint refuses such times.
 */
#ifndef XDE_HIP_SPLINE_H
#define XDE_HIP_SPLINE_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Y[B, Tn, C] and M[B, Tn, C] of series[B, Tn, C] over knots[Tn] as defined above.  One launch, one lane per column, no scratch (the
 * sweeps keep cp in Y and dp in M until they are replaced): Y and M must not overlap series or each other.
 * Refused (XDE_EBADARG): a null pointer, B < 1, C < 1, Tn < 2, a dtype that is not XDE_F32 / XDE_F64, a pointer not aligned to its
 * element type. */
int xde_spline_natural_coeffs(void* Y, void* M, const void* series, const void* knots, int64_t B, int Tn, int C, int dtype, void* stream);

/* val[outer, L, D] and der[outer, L, D] (`val` and `der` above) of the path (Y[outer, Tn, D], M[outer, Tn, D], knots[Tn]) at the L
 * query times tq[L], which are of the series dtype: the layout of xde_history_gather.  `der` may be null (it is then not written).
 * Refused (XDE_EBADARG): a null val / Y / M / knots / tq, outer < 1, L < 1, D < 1, Tn < 2, a bad dtype, a misaligned pointer. */
int xde_spline_natural_gather(void* val, void* der, const void* Y, const void* M, const void* knots, const void* tq, int64_t outer, int Tn,
                              int L, int D, int dtype, void* stream);

/* xde_cde_contract (include/xde_hip_cde.h) with dX[b, c] = the `der` above at tau = (series dtype)(t), built on chip from the rows i
 * and i + 1 of Y and M — the bits xde_spline_natural_gather writes.  In every other respect the contract of xde_cde_contract: the time
 * in device memory (`t_dev`, one element of `time_dtype`) or on the host (`t_host`), the summation order over c, 16-byte vectors for
 * aligned operands with C % W == 0 and scalar loads with the same bits otherwise, no atomics, one launch, the plan of xde_cde_plan.
 * Refused (XDE_EBADARG): a null out / F / Y / M / knots, B < 1, H < 1, C < 1, Tn < 2, a dtype or time_dtype that is not XDE_F32 /
 * XDE_F64, a pointer not aligned to its element type. */
int xde_cde_contract_natural(void* out, const void* F, const void* Y, const void* M, const void* knots, const void* t_dev, double t_host,
                             int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream);

/* gF[b, h, c] = gout[b, h] * dX[b, c] with that dX: xde_cde_contract_backward for the natural control.  Same checks. */
int xde_cde_contract_natural_backward(void* gF, const void* gout, const void* Y, const void* M, const void* knots, const void* t_dev,
                                      double t_host, int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_SPLINE_H */
