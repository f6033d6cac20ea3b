/*
 * xde_hip_rows.h — entry points of libxde_hip.so for PER-SAMPLE adaptive stepping (odeint(..., options={"per_sample": True})): every
 * row of the batch carries its own time, step size, error ratio, verdict, output cursor and counters (host side:
 * paddlexde_amd/solver/_rk_rows.py).
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64, -ffp-contract=off: every result below is the written op order, rounded op by op).  T is the state dtype, TT the
 * time dtype (params->time_dtype).  Arguments are validated on the host before anything is enqueued.
 *
 * THE LAYOUT.  A state operand is a contiguous rows x D array of T: element o = r * D + d, row r being sample r.  The solution is a
 * contiguous n_out x rows x D array of T.
 *
 * THE CONTROL BLOCK is a struct of arrays of length rows (xde_rows_ctl_t: device pointers, the struct itself is host memory read
 * during the call).  The double planes hold TT values, as xde_ctrl_t does:
 *
 *   t        time of the row's y0 / f0 AFTER the last verdict (t_prev + h_used if accepted, else t_prev)
 *   t_prev   time the last attempt started from
 *   h        step of the pending attempt, signed
 *   h_used   step the last attempt took
 *   ratio, nonfinite     error ratio of the last attempt; non-finite elements of its y0
 *   accept               verdict of the last attempt (0 for a row that was frozen when it was judged)
 *   done                 every output of the row has been written: the row is FROZEN (nothing of it changes any more)
 *   status               XDE_STATUS_* (sticky); a row whose status is not OK is judged no more
 *   next_out             the row's output cursor: the first output not yet written
 *   n_accept, n_reject, steps_in_interval     as xde_ctrl_t's
 *   t_stage              [n_stage][rows] of T: the stage times of the pending attempt, t_stage[s * rows + r]
 *
 * THE CAPS.  1 <= rows, 1 <= D, rows * D <= 2^40, 1 <= n_out <= 2^31 - 1 and n_out * rows * D <= 2^48; the three launches that own
 * rows (2, 3 and 4) also ask D <= 2^31 (a row's chunks are counted in 32 bits).  Every pointer is aligned to its element type (16-byte
 * alignment is not required).
 *
 * THE ROW SUM.  Kernels 2 and 4 sum the float64 squares q(d) of a row in an order that is a function of (D, dtype) only — never of
 * rows, the grid, or the workgroup that got the row.  With W = 4 (fp32) or 2 (fp64) and C = ceil(D / W) chunks of W consecutive
 * elements, G = min(256, smallest power of two >= C) lanes work on a row:
 *
 *   S_g   = the sum of q(d) over the chunks c = g, g + G, g + 2G, ... in increasing d, sequentially, starting from 0.0   (g < G)
 *   sum   = the pairwise tree over S_0 .. S_{G-1}: S <- (S_0 + S_1, S_2 + S_3, ...) until one value is left
 *
 * and norm = |round_T(sqrt(round_T(sum / D)))|, xde_norm_result's RMS.  Non-finite counts are summed as integers.
 *
 * THE MAPPING (of launches 2, 3 and 4; results never depend on it).  A workgroup of 256 lanes holds 256 / G rows at a time: several
 * rows per wave at small D, one row per workgroup from C > 128 on, with D beyond the workgroup's stride (256 W elements) as a loop
 * inside that workgroup, not a second launch.  Launches 3 and 4 use ceil(rows * G / 256) workgroups (up to the grid cap, then a loop).
 * Launch 2 runs its controllers one lane per row after a BATCH of rows' sums: the batch is those 256 / G rows, doubled up to 64 rows
 * only while the launch keeps at least 1024 workgroups — a batch of samples is never folded into fewer workgroups than fill the
 * device, and with fewer than 2048 * 256 / G rows the launch has ceil(rows * G / 256) workgroups like the other two: at large D a
 * workgroup per row.
 */
#ifndef XDE_HIP_ROWS_H
#define XDE_HIP_ROWS_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_ROWS_MAX_K 7 /* operands of one xde_rows_* launch (Dopri8's 13 stages are not served) */

typedef struct xde_rows_ctl_t {
  uint32_t struct_size; /* = sizeof(xde_rows_ctl_t): checked before anything else is read */
  uint32_t reserved;
  double* t;
  double* t_prev;
  double* h;
  double* h_used;
  double* ratio;
  double* nonfinite;
  int32_t* accept;
  int32_t* done;
  int32_t* status;
  int32_t* next_out;
  int32_t* n_accept;
  int32_t* n_reject;
  int32_t* steps_in_interval;
  void* t_stage;
} xde_rows_ctl_t;

/*
 * 1. THE STAGE COMBINE, one launch.  Per element o = r * D + d, with dt = T(h[r]) and c_j = T(coef[j]) * dt:
 *
 *   acc     = k[0][o] * c_0;  acc = acc + k[j][o] * c_j       for j = 1 .. nk - 1, in this order
 *   out[o]  = y0[o] + acc                                       (XDE_COMBINE_RK's op order)
 *   out[o]  = y0[o]                                             where done[r]
 *
 * Where all h[r] are equal (and no row is done) the result is xde_stage_combine's, bit for bit.  The optional second output
 * (out2 and coef2 both non-null), with c2_j = dt * T(coef2[j]):  out2[o] = k[0][o] * c2_0 + k[1][o] * c2_1 + ... (left to right;
 * written for every row, done or not).  1 <= nk <= XDE_ROWS_MAX_K.  Reads of ctl: h, done.  No output may overlap an operand.
 */
int xde_rows_stage_combine(void* out, void* out2, const void* y0, const void* const* k, const double* coef, const double* coef2, int nk,
                           const xde_rows_ctl_t* ctl, int64_t rows, int64_t D, int dtype, void* stream);

/*
 * 2. ERROR NORM + CONTROLLER, one launch.  A row that is done or whose status is not OK gets accept = 0 and nothing else.  Any other
 * row r, with dt = T(h[r]), c_j = dt * T(c_err[j]), rtol = T(params->rtol), atol = T(params->atol), per element:
 *
 *   e   = k[0][o] * c_0  (e_pre given: e_pre[o] + k[0][o] * c_0);  e = e + k[j][o] * c_j  for j = 1 .. nk - 1
 *   tol = atol + rtol * fmax(|y0[o]|, |y1[o]|);  q = e / tol  in T;  q(d) = double(q) * double(q)
 *
 * ratio = norm of THE ROW SUM over q(d); nonfinite = number of non-finite y0[o] of the row.  One lane then runs xde_rk_control's
 * controller (the I-controller; step_t, replay and the PI controller are not served) on
 *
 *   t0 = TT(t[r]), dt = TT(h[r]), t1 = t0 + dt, the cursor next_out[r] and n_out output times t_span[] (doubles holding TT values)
 *
 * and writes t_prev = t0, t = accept ? t1 : t0, h_used = dt, h = the next step, ratio, nonfinite, accept, status, n_accept, n_reject,
 * steps_in_interval (0 when the step reaches an output, as xde_rk_control), and the next attempt's stage times
 *
 *   t_stage[s][r] = alpha_s == 1 ? T(t + h) : T(t) + T(alpha_s) * T(h)     (t + h summed in TT; all stages T(t) when the row will be done)
 *
 * It does NOT move next_out or set done: kernel 3 does, from the same comparison.  e_pre takes nk == 1; 1 <= nk <= XDE_ROWS_MAX_K.
 */
int xde_rows_norm_control(const void* const* k, const double* c_err, int nk, const void* e_pre, const void* y0, const void* y1,
                          const xde_rows_ctl_t* ctl, const xde_ctrl_params_t* params, const double* t_span, int32_t n_out, int64_t rows,
                          int64_t D, int dtype, void* stream);

/*
 * 3. DENSE OUTPUT + COMMIT, one launch, after kernel 2.  Rows with accept == 0 are untouched.  A row with accept, with t0 = TT(t_prev[r]),
 * t1 = TT(t[r]), dt = T(TT(h_used[r])), dir = params->direction: for every j from next_out[r] on while j < n_out and
 * dir * TT(t_span[j]) <= dir * t1, per element (xde_dense_commit's arithmetic):
 *
 *   ymid = y0[o] + (k[0][o] * (dt * T(mid[0])) + k[1][o] * (dt * T(mid[1])) + ...)          left to right
 *   x    = T((TT(t_span[j]) - t0) / (t1 - t0))
 *   out[(j * rows + r) * D + d] = the quartic of interp_fit / interp_evaluate through (y0, ymid, y1, f0 = k[0], f1) at x
 *
 * then y0[o] <- y1[o] and f0[o] <- f1[o] in place (f0 must be k[0]), next_out[r] <- the first j not written, done[r] <- (that j == n_out).
 * A step that holds no output only commits.  1 <= nk <= XDE_ROWS_MAX_K.
 */
int xde_rows_dense_commit(void* out, const void* const* k, const double* mid, int nk, void* y0, const void* y1, void* f0, const void* f1,
                          const xde_rows_ctl_t* ctl, const xde_ctrl_params_t* params, const double* t_span, int32_t n_out, int64_t rows,
                          int64_t D, int dtype, void* stream);

/*
 * 4. THE SCALED NORMS of the initial-step heuristic, one launch.  Per row, with scale = T(atol) + |y0[o]| * T(rtol) and
 * q = (b ? a[o] - b[o] : a[o]) / scale in T:  out[r] = norm of THE ROW SUM over double(q) * double(q), a double per row.
 */
int xde_rows_scaled_norm(double* out, const void* a, const void* b, const void* y0, double rtol, double atol, int64_t rows, int64_t D,
                         int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_ROWS_H */
