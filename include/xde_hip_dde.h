/*
 * xde_hip_dde.h — entry points of libxde_hip.so for ddeint_steps, the delay solver whose delayed states are read from the solution
 * being computed: the cubic Hermite interpolant of a tape of (time, state, derivative) nodes evaluated at all delays of one stage in
 * one launch, and the fan of its cotangent back into the nodes (host side: paddlexde_amd/xde/steps_dde.py,
 * paddlexde_amd/solver/_autograd.py).
 *
 * Same conventions as the other headers of this directory (status codes, the thread's last error text, device pointers borrowed from
 * the caller, `stream` = hipStream_t as void*, XDE_F32 / XDE_F64, -ffp-contract=off: every result below is the written op order,
 * rounded op by op).  Arguments are validated on the host before anything is enqueued; a refused call writes nothing.
 *
 * THE INTERPOLANT.  A delay j of a stage falls into one interval [a, b] of the tape, h = b - a, at sigma = (theta_j - a) / h in
 * [0, 1].  The host computes, in float64, the value weights
 *
 *   a0 = 2 s3 - 3 s2 + 1,   a1 = h (s3 - 2 s2 + sigma),   a2 = -2 s3 + 3 s2,   a3 = h (s3 - s2)        (s2 = sigma sigma, s3 = s2 sigma)
 *
 * and the weights of the derivative of the value with respect to the delay, -H'(theta),
 *
 *   b0 = -(6 s2 - 6 sigma) / h,   b1 = -(3 s2 - 4 sigma + 1),   b2 = -b0,   b3 = -(3 s2 - 2 sigma)
 *
 * and the kernels round them to the state dtype T.  The four operands of a delay are the interval's end states and end derivatives
 * ya, fa, yb, fb.
 *
 * THE CAPS.  1 <= rows, 1 <= D <= 2^30, rows * Ltot * D <= 2^48, at most XDE_DDE_MAX_LAGS delays per launch.  Every pointer is
 * aligned to its element type (16-byte alignment is not required: a launch whose bases, strides and D allow it moves 16-byte
 * vectors, any other moves single elements).
 */
#ifndef XDE_HIP_DDE_H
#define XDE_HIP_DDE_H

#include "xde_hip.h"

#define XDE_DDE_MAX_LAGS 16 /* delays per launch: 4 pointers, 4 strides and 8 weights each, about 2 KiB of a launch's 4 KiB of arguments */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE GATHER, one launch, 4 L N elements read and L N (2 L N with dtau) written, N = rows * D.  src[4 j + s], s = 0 .. 3 for
 * ya, fa, yb, fb of delay j < L, is a device pointer to a rows x D operand whose row r starts at element r * stride[4 j + s] (a
 * tape node: D; row i of a [rows, Th, D] history: Th * D with the base at its element i * D).  w and wd hold 4 L doubles each,
 * (a0, a1, a2, a3) and (b0, b1, b2, b3) per delay; src, stride, w and wd are HOST arrays, copied into the launch's arguments.
 * Per r < rows, j < L, d < D, in T:
 *
 *   out [(r * Ltot + j0 + j) * D + d] = (ya a0 + fa a1) + (yb a2 + fb a3)
 *   dtau[(r * Ltot + j0 + j) * D + d] = (ya b0 + fa b1) + (yb b2 + fb b3)
 *
 * so that a caller with more than XDE_DDE_MAX_LAGS delays fills a [rows, Ltot, D] array in tiles of delays j0 .. j0 + L - 1, and a
 * delay's result does not depend on its tile.  dtau and wd are null together: dtau is then not computed.  1 <= L <=
 * XDE_DDE_MAX_LAGS, 0 <= j0, j0 + L <= Ltot, every stride >= D.  Operands are read-only and may coincide with one another; no
 * output may overlap an operand or the other output.
 */
int xde_dde_tape_gather(void* out, void* dtau, const void* const* src, const int64_t* stride, const double* w, const double* wd,
                        int64_t rows, int64_t D, int L, int j0, int Ltot, int dtype, void* stream);

/*
 * THE COTANGENT, one launch without atomics, at most L N elements read and nq N written.  Output q < nq, gsrc[q], a contiguous
 * rows x D array, is the cotangent of one distinct node tensor (a state or a derivative of the tape) from g, the cotangent of the
 * gather's `out` ([rows, Ltot, D]).  Its terms are e in [first[q], first[q + 1]), first[0] = 0: per r < rows, d < D, in T,
 *
 *   acc             = g[(r * Ltot + j0 + lag[first[q]]) * D + d] * wt[first[q]]
 *   acc             = acc + g[(r * Ltot + j0 + lag[e]) * D + d] * wt[e]          for e = first[q] + 1 .. first[q + 1] - 1, in this order
 *   gsrc[q][r D + d] = acc
 *
 * with wt[e] the value weight the node had in delay j0 + lag[e].  Two delays that fall into one interval are two terms of the same
 * output: the result is a function of the operands' bits.  gsrc, first (nq + 1 entries), lag and wt (first[nq] entries) are HOST
 * arrays.  1 <= nq <= 4 * XDE_DDE_MAX_LAGS, every output has at least one term, first[nq] <= 4 * XDE_DDE_MAX_LAGS, 0 <= lag[e],
 * 0 <= j0, j0 + lag[e] < Ltot.  No output may overlap g or another output.
 */
int xde_dde_tape_gather_backward(void* const* gsrc, const int32_t* first, const int32_t* lag, const double* wt, int nq, const void* g,
                                 int64_t rows, int64_t D, int j0, int Ltot, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_DDE_H */
