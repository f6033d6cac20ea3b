/*
 * xde_hip_cdegrad.h — entry points of libxde_hip.so for the gradient of cdeint with respect to its CONTROL PATH: the cotangent of
 * X'(t) in the contraction out[b, h] = sum_c F[b, h, c] * dX[b, c] scattered to the rows dX was built from, the transpose of the natural
 * cubic spline's coefficient build, and the transpose of its gather (host side: paddlexde_amd/xde/base_cde.py CdeControlContractFn,
 * paddlexde_amd/interpolation with differentiable=True).
 *
 * Same conventions as xde_hip.h, xde_hip_cde.h and xde_hip_spline.h (status codes, device pointers borrowed from the caller, `stream` =
 * hipStream_t as void*, XDE_F32 / XDE_F64, XDE_HISTORY_*).  Arguments are validated on the host before anything is enqueued: a refused
 * call writes nothing, and xde_last_error names the entry point.  All arrays are contiguous, in the one dtype `dtype` = T.  Products,
 * sums and quotients in T, rounded op by op (the library is built with -ffp-contract=off; division is IEEE).  No atomics.
 *
 * THE TIME of xde_cde_control_grad / _natural is the time of xde_cde_contract: `t_dev` (one element of `time_dtype` in device memory,
 * read by the kernel) or, with `t_dev` null, `t_host`; tau = T(t).
 *
 * ---------------------------------------------------------------------------------------------------------------------------------
 * (a) THE COTANGENT OF THE CONTROL IN THE CONTRACTION.  One launch, two phases per batch row b.
 *
 * PHASE 1.  gdX[b, c] = sum_h gout[b, h] * F[b, h, c].  THE SUMMATION ORDER over h depends on H only — not on B, C, the dtype, the
 * grid or pointer alignment.  With P = min(32, the least power of two >= H) partial sums per channel:
 *
 *   partial p (0 <= p < P):  v_p = +0;  for h = p, p + P, p + 2P, ... < H in ascending order:  v_p = v_p + gout[b, h] * F[b, h, c]
 *   then for off = P/2, P/4, ..., 1:  v_p = v_p + v_{p + off}  for every p < off
 *   gdX[b, c] = v_0
 *
 * F is read once, in 16-byte vectors along c where F is 16-byte aligned and C % W == 0 (W = 4 for fp32, 2 for fp64), with scalar loads
 * and the same bits otherwise.  gdX is never written to memory.
 *
 * PHASE 2.  dX[b, c] is linear in the rows of the control it reads, so its transpose is a short list of ENTRIES (row_j, w_j), j <
 * n, that depend on tau and the knots alone (built once per workgroup).  Every element of an output is written exactly once:
 *
 *   o = +0;  for j = 0, ..., n - 1 in ascending order, if row_j == k:  o = o + w_j * gdX[b, c];   out[b, k, c] = o
 *
 * so a row dX did not read gets +0, and there is no separate memset.
 *
 * XDE_HISTORY_LINEAR (gSeries; knots t, T(1) = one):
 *     i = clip(#{k : t_k < tau} - 1, 0, Tn - 1);   scale1(j) = t_{jj+1} - t_jj with jj = min(j, Tn - 2)
 *     n = 2:   (i, T(-1) / scale1(i)),   (min(i + 1, Tn - 1), T(1) / scale1(max(i - 1, 0)))
 *   (the transpose of rows_eval<2>'s `der` = -1 * (x_0 / sc_0) + 1 * (x_1 / sc_1); the reference's scale conventions as written).
 * XDE_HISTORY_CUBIC (gSeries):
 *     i as above;  h(j) = scale1(j);  h1 = h(i), h2 = h(i - 1) (h(0) when i == 0), ha = h(i), hb = h(i + 1);  sx = (tau - t_i) / h1
 *     s2 = sx * sx;  g0 = 6 s2 - 6 sx;  g1 = -6 s2 + 6 sx;  g2 = (3 s2 - 4 sx) + 1;  g3 = 3 s2 - 2 sx     (hermite_eval's g0..g3)
 *     a0 = g0 / h1;  a1 = g1 / h2;  b0 = g2 / ha;  b1 = g3 / hb;   i1 = min(i + 1, Tn - 1)
 *     mode 0 (i <= Tn - 3):  n = 6:  (i, a0), (i1, a1), (i1, b0), (i, -b0), (i + 2, b1), (i1, -b1)
 *     mode 1 (i == Tn - 2):  n = 6:  (i, a0), (i1, a1), (i1, b0), (i, -b0), (i1, b1), (i, -b1)
 *     mode 2 (i == Tn - 1):  n = 6:  (i, a0), (i1, a1), (i, b0), (Tn - 2, -b0), (i, b1), (Tn - 2, -b1)
 * XDE_HISTORY_BEZIER is refused, as in xde_cde_contract.
 * THE NATURAL CONTROL (gY from the Y entries, gM from the M entries; i, h, s of xde_hip_spline.h EVALUATION):
 *     rh = T(1) / h;   q = (s * s) / (T(2) * h)
 *     Y entries, n = 2:   (i, -rh),  (i + 1, rh)
 *     M entries, n = 2:   (i, (s - h / T(3)) - q),  (i + 1, q - h / T(6))
 *
 * ---------------------------------------------------------------------------------------------------------------------------------
 * (b) THE TRANSPOSE OF xde_spline_natural_coeffs.  Per column (b, c), with the NODES of xde_hip_spline.h (the first knot, the last
 * knot and every observed k in between), y_k = series[b, k, c] (only its NaN pattern is read), t = knots:
 *
 *   FOLD.  GY_n = gY_n and GM_n = gM_n at every node n; then, for consecutive nodes a < b and every missing row a < j < b in
 *     ascending order, with h = t_b - t_a, s = t_j - t_a:
 *         r = s / h;  l = T(1) - r;  s2 = s * s;  s3 = s2 * s
 *         wa = (-(s * h) / T(3) + s2 / T(2)) - s3 / (T(6) * h);     wb = -(s * h) / T(6) + s3 / (T(6) * h)
 *         GY_a = GY_a + l * gY_j;            GY_b = GY_b + r * gY_j
 *         GM_a = (GM_a + wa * gY_j) + l * gM_j;    GM_b = (GM_b + wb * gY_j) + r * gM_j
 *     (a node first takes the rows below it, as b, then the rows above it, as a).
 *   SOLVE.  The system of the forward sweep is symmetric.  Ascending over the interior nodes i with neighbours a < i < b, cp = dl = 0
 *     at the first node:   hl = t_i - t_a;  hr = t_b - t_i;  den = T(2) * (hl + hr) - hl * cp_a;  cp_i = hr / den;
 *     dl_i = (GM_i - hl * dl_a) / den;   descending:  lam_i = dl_i - cp_i * lam_b;   lam = 0 at the first and the last node (their M is
 *     the constant 0: GM there is dropped).
 *   RIGHT-HAND SIDE.  For consecutive nodes p < q:  u_pq = (T(6) * (lam_p - lam_q)) / (t_q - t_p).
 *     G_n = GY_n;  with the node a below n:  G_n = G_n + u_an;  then with the node b above n:  G_n = G_n - u_nb.
 *   END RULE.  gSeries_k = G_k at an observed k, +0 at every unobserved one.  Then, if y_0 is NaN, with kf the first observed row:
 *     gSeries_kf = gSeries_kf + G_0;  then, if y_{Tn-1} is NaN, with kl the last observed row:  gSeries_kl = gSeries_kl + G_{Tn-1}.
 *     A column with no observed value gets +0 everywhere.
 *
 * (c) THE TRANSPOSE OF xde_spline_natural_gather.  Per column (o, d) and row k, over the queries l = 0, ..., L - 1 in ascending
 * order, with (i, h, s) of query l (EVALUATION), gv = gval[o, l, d], gd = gder[o, l, d], and the weights
 *         r = s / h;  l_ = T(1) - r;  wa, wb as in FOLD;   rh, q as in (a);   ma = (s - h / T(3)) - q;   mb = q - h / T(6):
 *     y = +0;  m = +0
 *     if i == k:      [gval]  y = y + l_ * gv;  m = m + wa * gv;     [gder]  y = y + (-rh) * gd;  m = m + ma * gd
 *     if i + 1 == k:  [gval]  y = y + r * gv;   m = m + wb * gv;     [gder]  y = y + rh * gd;     m = m + mb * gd
 *     gY[o, k, d] = y;   gM[o, k, d] = m
 *   ([gval] / [gder]: skipped when that cotangent is null).  One owner per column, no atomics.  The queries are served in tiles of
 *   128: every output element is written once when L <= 128, and once per tile otherwise (a later tile starts from the stored sums,
 *   so the order of the additions is the ascending one either way).
 */
#ifndef XDE_HIP_CDEGRAD_H
#define XDE_HIP_CDEGRAD_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (a) for XDE_HISTORY_LINEAR / XDE_HISTORY_CUBIC: gSeries[B, Tn, C] from gout[B, H], F[B, H, C], knots[Tn] and the time.  One launch.
 * gSeries must not overlap the inputs.  Refused (XDE_EBADARG): a null gSeries / gout / F / knots, B < 1, H < 1, C < 1, Tn < 2, a dtype
 * or time_dtype that is not XDE_F32 / XDE_F64, a method that is not XDE_HISTORY_LINEAR / XDE_HISTORY_CUBIC, a pointer not aligned to
 * its element type. */
int xde_cde_control_grad(void* gSeries, const void* gout, const void* F, const void* knots, const void* t_dev, double t_host,
                         int time_dtype, int64_t B, int H, int C, int Tn, int method, int dtype, void* stream);

/* (a) for the natural control: gY[B, Tn, C] and gM[B, Tn, C].  One launch.  Same checks (gY and gM both required). */
int xde_cde_control_grad_natural(void* gY, void* gM, const void* gout, const void* F, const void* knots, const void* t_dev, double t_host,
                                 int time_dtype, int64_t B, int H, int C, int Tn, int dtype, void* stream);

/* THE LAUNCH PLAN of (a), from (B, H, C, dtype) and the 16-byte alignment of F.  The bits of the result never depend on it; it is
 * reported so that a test can state which code a shape runs. */
typedef struct xde_cdegrad_plan {
  int32_t vec;     /* F is read in 16-byte vectors (C % W == 0 and F is 16-byte aligned), else with scalar loads; the outputs are
                      stored in 16-byte vectors when vec holds and they are 16-byte aligned too, else element by element */
  int32_t P;       /* partial sums over h per channel: min(32, pow2ceil(H)) */
  int32_t CL;      /* lanes along c of a workgroup: 256 / P; a lane holds W consecutive channels */
  int32_t chunks;  /* passes of a workgroup over a batch row: ceil(ceil(C / W) / CL) */
  int32_t rows;    /* rows of F a lane adds per pass: ceil(H / P) */
  int32_t strided; /* B exceeds the grid cap: a workgroup takes batch rows `blocks` apart */
  int64_t blocks;  /* workgroups launched: min(B, the grid cap); one batch row per workgroup at a time */
} xde_cdegrad_plan_t;

/* The plan of xde_cde_control_grad / _natural into *plan, by the function the launch itself uses.  Enqueues nothing and needs no
 * device; `F` is used for its alignment only.  Refused (XDE_EBADARG): a null plan, B < 1, H < 1, C < 1, a bad dtype, an `F` not
 * aligned to its element type. */
int xde_cde_control_grad_plan(const void* F, int64_t B, int H, int C, int dtype, xde_cdegrad_plan_t* plan);

/* (b): gSeries[B, Tn, C] from gY, gM, series [B, Tn, C] and knots[Tn].  One launch, one lane per column, serial sweeps; `workspace`
 * holds xde_spline_natural_coeffs_backward_workspace_bytes(B, Tn, C, dtype) bytes, 16-byte aligned (cp and GY per node; dl and lam
 * live in gSeries until they are replaced).  gSeries and the workspace must not overlap the inputs or each other.
 * Refused (XDE_EBADARG): a null pointer, B < 1, C < 1, Tn < 2, a bad dtype, a misaligned pointer. */
int xde_spline_natural_coeffs_backward(void* gSeries, const void* gY, const void* gM, const void* series, const void* knots,
                                       void* workspace, int64_t B, int Tn, int C, int dtype, void* stream);

/* Bytes of (b)'s workspace: two arrays [B, Tn, C] of the dtype; -1 for B < 1, C < 1, Tn < 2 or a bad dtype. */
int64_t xde_spline_natural_coeffs_backward_workspace_bytes(int64_t B, int Tn, int C, int dtype);

/* (c): gY[outer, Tn, D] and gM[outer, Tn, D] from gval and / or gder [outer, L, D] at tq[L]; either cotangent may be null, not both.
 * Refused (XDE_EBADARG): a null gY / gM / knots / tq, gval and gder both null, outer < 1, L < 1, D < 1, Tn < 2, a bad dtype, a
 * misaligned pointer. */
int xde_spline_natural_gather_backward(void* gY, void* gM, const void* gval, const void* gder, const void* knots, const void* tq,
                                       int64_t outer, int Tn, int L, int D, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_CDEGRAD_H */
