/*
 * xde_hip_teval.h — entry points of libxde_hip.so for PER-SAMPLE OUTPUT TIMES of a joint adaptive solve
 * (odeint(..., options={"t_eval": tq}); host side: paddlexde_amd/solver/_rk_teval.py).  The batch keeps one step sequence; every row
 * of the batch has its own list of times, and an accepted step writes, for every row, only the queries of that row it holds.
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64, -ffp-contract=off: every result below is the written op order, rounded op by op).  T is the state dtype, TT the
 * time dtype (`time_dtype`).  Arguments are validated on the host before anything is enqueued.
 *
 * THE LAYOUT.  A state operand is a contiguous rows x D array of T: element o = r * D + d, row r being sample r.  `out` and `g` are
 * contiguous Q x rows x D arrays of T: query q of row r starts at (q * rows + r) * D.  `tq` is rows x Q doubles holding TT values,
 * row r's times monotone in the direction of integration (equal neighbours allowed) over its first cnt[r] entries; `cnt` is int32
 * [rows], 0 <= cnt[r] <= Q, the number of leading entries of the row that are observations (what follows them is never read).
 * Every pointer is aligned to its element type (16-byte alignment is not required: rows that start on a 16-byte boundary take
 * 16-byte loads and stores, the others single elements, with the same bits).
 *
 * THE CAPS.  1 <= rows, 1 <= D <= 2^31, rows * D <= 2^40, 1 <= Q <= 2^31 - 1, Q * rows * D <= 2^48.
 *
 * MEMBERSHIP.  The step (t0, t1] (doubles holding TT values, t1 - t0 of the sign of `direction` = +1 / -1) holds query q of row r iff
 *
 *   q < cnt[r]   and   dir * t0 < dir * TT(tq[r][q])   and   dir * TT(tq[r][q]) <= dir * t1          (compared in TT)
 *
 * The queries a step holds of a row are a range [b, e) of the row (b = the first q < cnt[r] later than t0, e = the first later than
 * t1): both kernels find it by binary search in the row.  Consecutive accepted steps share t1 = t0 bit for bit, so every query later
 * than the start of the solve lies in exactly one step.  The kernels keep no state: no cursor, nothing recorded for the backward.
 *
 * THE MAPPING (results never depend on it).  With W = 4 (fp32) or 2 (fp64) and C = ceil(D / W) chunks of W consecutive elements,
 * G = min(256, smallest power of two >= C) lanes work on a row and a workgroup of 256 lanes holds 256 / G rows; D beyond the
 * workgroup's stride (256 W elements) is a loop in that workgroup.  No atomics.  A row with an empty range costs its workgroup the
 * read of cnt[r] and O(log Q) reads of the row's times.
 */
#ifndef XDE_HIP_TEVAL_H
#define XDE_HIP_TEVAL_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_TEVAL_OUTS 5 /* the cotangent launch's outputs: y0, y1, y_mid, f0, f1 (in this order) */

/*
 * 1. DENSE OUTPUT AT EVERY ROW'S OWN TIMES, one launch per accepted step.  The quartic of the joint dense output
 * (csrc/xde_dense.hip: quartic_; utils/ode_utils.py: interp_fit + interp_evaluate), op for op.  With dtT = T(TT(dt)), for row r and
 * every q of its range [b, e), per element o = r * D + d:
 *
 *   ymid = y0[o] + (k[0][o] * (dtT * T(mid[0])) + k[1][o] * (dtT * T(mid[1])) + ...)          left to right; once per row
 *   x    = T((TT(tq[r][q]) - t0) / (t1 - t0))                                                  in TT
 *   ca   = T(2) * dtT * (f1 - f0) - T(8) * (y1 + y0) + T(16) * ymid
 *   cb   = dtT * (T(5) * f0 - T(3) * f1) + T(18) * y0 + T(14) * y1 - T(32) * ymid
 *   cc   = dtT * (f1 - T(4) * f0) - T(11) * y0 - T(5) * y1 + T(16) * ymid
 *   cd   = dtT * f0
 *   out[(q * rows + r) * D + d] = (((y0 + x * cd) + x^2 * cc) + x^3 * cb) + x^4 * ca          x^2 = x * x, x^3 = x^2 * x, x^4 = x^3 * x
 *
 * Nothing else of `out` is written.  A row with an empty range reads none of the state operands.  1 <= nk <= XDE_MAX_K; k[0] may be
 * f0 and k[nk - 1] may be f1 (they are then read once).  `out` may not overlap a state operand.
 */
int xde_teval_dense(void* out, const double* tq, const int32_t* cnt, const void* const* k, const double* mid, int nk, const void* y0,
                    const void* y1, const void* f0, const void* f1, double t0, double t1, double dt, int direction, int time_dtype,
                    int64_t rows, int64_t D, int64_t Q, int dtype, void* stream);

/*
 * 2. THE COTANGENT OF LAUNCH 1, one launch per accepted step that holds a query: the quartic is linear in (y0, y1, y_mid, f0, f1).
 * With x_q as above widened to double, dts = double(T(TT(dt))) and, in float64 in the written order
 * (solver/_rk_backprop.py: quartic_weights),
 *
 *   x2 = x * x;  x3 = x2 * x;  x4 = x3 * x
 *   p0 = 1 - 11 x2 + 18 x3 - 8 x4     p1 = -5 x2 + 14 x3 - 8 x4     pm = 16 x2 - 32 x3 + 16 x4
 *   q0 = dts * (x - 4 x2 + 5 x3 - 2 x4)     q1 = dts * (x2 - 3 x3 + 2 x4)
 *   w  = (p0 + pm, p1, pm, q0, q1)            (y_mid = y0 + ...: its cotangent reaches y0 as well)
 *
 * for row r with the range [b, e), per element o = r * D + d and output j:
 *
 *   s = g[(b * rows + r) * D + d] * T(w_j(x_b));   acc_mask bit j:  s = outs[j][o] + s
 *   s = s + g[(q * rows + r) * D + d] * T(w_j(x_q))          for q = b + 1 .. e - 1, in this order
 *   outs[j][o] = s
 *
 * A row with an empty range writes outs[j][o] = 0, or keeps its value under acc_mask bit j.  A NULL outs[j] is not written (at
 * least one is not NULL).  The outputs may not overlap `g` or each other.
 */
int xde_teval_cotangent(void* const* outs, const void* g, const double* tq, const int32_t* cnt, double t0, double t1, double dt,
                        int direction, int time_dtype, uint32_t acc_mask, int64_t rows, int64_t D, int64_t Q, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_TEVAL_H */
