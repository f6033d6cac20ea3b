/*
 * xde_hip_sde.h — entry points of libxde_hip.so for sdeint: Ito Euler-Maruyama, Milstein and SRK steps and Stratonovich reversible Heun
 * steps (with the cotangent sweep of sdeint_adjoint) with diagonal noise whose Brownian increments are generated inside the kernel (host side: paddlexde_amd/solver/base_fixed_solver.py, paddlexde_amd/functional/sdeint.py).
 *
 * Same conventions as xde_hip.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64).  Arguments are validated on the host before anything is enqueued.
 *
 * THE NOISE.  Z[e], the standard normal of element e (flat index, 0 <= e < n) at grid step k (0-based) under the 64-bit seed, is
 *
 *   Philox4x32-10 (Salmon et al., SC'11; rounds M0 = 0xD2511F53, M1 = 0xCD9E8D57, key bumps W0 = 0x9E3779B9, W1 = 0xBB67AE85)
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (j & 0xffffffff, j >> 32, k, 0)          -> words w0, w1, w2, w3
 *
 *   fp32: j = e / 4;  u_i = ((w_i >> 8) + 1) * 2^-24                      i = 0..3, in (0, 1]
 *         (Z[4j], Z[4j+1]) = BM(u_0, u_1),  (Z[4j+2], Z[4j+3]) = BM(u_2, u_3)
 *   fp64: j = e / 2;  u_a = (((w1:w0) >> 11) + 1) * 2^-53,  u_b = (((w3:w2) >> 11) + 1) * 2^-53    (hi:lo = hi * 2^32 + lo)
 *         (Z[2j], Z[2j+1]) = BM(u_a, u_b)
 *
 *   BM(u1, u2) = (r * cos(2 pi u2), r * sin(2 pi u2)),  r = sqrt(-2 log(u1))
 *
 * computed in the state dtype with the precise math library (log, sqrt, sincospi(2 u2)).  The noise of an element depends on
 * (seed, k, e) only.  |Z| <= sqrt(48 ln 2) = 5.77 (fp32) and sqrt(106 ln 2) = 8.57 (fp64).
 *
 * THE SECOND DRAW.  V[e] is the same mapping at counter = (j & 0xffffffff, j >> 32, k, 1): the last counter word is the draw, 0 for Z
 * and 1 for V.  Only the SRK entry points take V; Z is the Z of every other entry point.
 *
 * k is a grid step, 0 <= k < 2^32.  Operands are contiguous arrays of n elements of the state dtype; dt is the step's size and
 * s = sqrt(|dt|) rounded to the state dtype by the caller (both converted to the state dtype in the kernel).  The library is built
 * with -ffp-contract=off: every result below is the written op order, rounded op by op.
 */
#ifndef XDE_HIP_SDE_H
#define XDE_HIP_SDE_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XDE_NOISE_NORMAL 0 /* xde_sde_noise writes Z[e], e < n, in the state dtype */
#define XDE_NOISE_BITS 1   /* xde_sde_noise writes the raw words as uint32: out[4j + i] = w_i of counter j, for 4j + i < n */

/* y1 = (y0 + f * dt) + g * (s * Z).  y1 may be y0 (an in-place step); no other overlap. */
int xde_sde_em_step(void* y1, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, uint64_t seed,
                    int64_t k, int dtype, void* stream);

/* gf = gy1 * dt and gg = gy1 * (s * Z) in one launch (the cotangents of f and g; that of y0 is gy1 itself).  A null gf or gg skips
 * that output; both null: nothing to do. */
int xde_sde_em_backward(void* gf, void* gg, const void* gy1, int64_t n, double dt, double s, uint64_t seed, int64_t k, int dtype,
                        void* stream);

/*
 * MILSTEIN (Kloeden & Platen's explicit strong order 1.0 scheme, Ito, diagonal noise: g_i depends on y_i only).  Besides dt and s the
 * caller passes c = 0.5 / sqrt(|dt|) rounded to the state dtype, and c = 0 when dt == 0 (a zero-length step returns y0); all three
 * are converted to the state dtype in the kernel, and a = |dt| is taken there in the state dtype.  Z is the Z of (seed, k) above.
 *
 * The support point yb = (y0 + f * dt) + g * s, where the caller evaluates gb = g(t0, yb).  No generator; yb may be y0. */
int xde_sde_milstein_support(void* yb, const void* y0, const void* f, const void* g, int64_t n, double dt, double s, int dtype,
                             void* stream);

/* gf = gyb * dt and gg = gyb * s (the cotangents of f and g at the support point; that of y0 is gyb itself).  A null gf or gg skips
 * that output; both null: nothing to do. */
int xde_sde_milstein_support_backward(void* gf, void* gg, const void* gyb, int64_t n, double dt, double s, int dtype, void* stream);

/* w = s * Z,  q = c * (w * w - a),  y1 = ((y0 + f * dt) + g * w) + (gb - g) * q.  One launch, 5 n elements moved.  y1 may be y0; no
 * other overlap.  The first three terms are xde_sde_em_step's expression: with gb == g the result is the EM step's, bit for bit. */
int xde_sde_milstein_step(void* y1, const void* y0, const void* f, const void* g, const void* gb, int64_t n, double dt, double s,
                          double c, uint64_t seed, int64_t k, int dtype, void* stream);

/* gf = gy1 * dt, gg = gy1 * (w - q) and ggb = gy1 * q in one launch that regenerates Z (w and q as above; the cotangent of y0 is gy1
 * itself).  A null output is skipped, and the generator runs only if gg or ggb is wanted; all three null: nothing to do. */
int xde_sde_milstein_backward(void* gf, void* gg, void* ggb, const void* gy1, int64_t n, double dt, double s, double c, uint64_t seed,
                              int64_t k, int dtype, void* stream);

/*
 * SRK (Roessler's SRI1W1, "Runge-Kutta methods for the strong approximation of solutions of stochastic differential equations", SIAM J.
 * Numer. Anal. 48 (2010): derivative-free, strong order 1.5, Ito, diagonal noise: g_i depends on y_i only).  Besides dt, s and
 * Milstein's c the caller passes c3 = 1 / (6 |dt|) rounded to the state dtype, and c = c3 = 0 when dt == 0 (a zero-length step returns
 * y0); a = |dt| is taken in the kernel in the state dtype.  Z and V are the two draws of (seed, k).  Per element, in this op order:
 *
 *   w = s * Z                                   (the Brownian increment, EM's and Milstein's)
 *   p = 0.5 * (w + (s * V) * r3)                (I10 / |dt|)
 *   q = c * (w * w - a)                         (I11 / sqrt|dt|, Milstein's q)
 *   u = c3 * ((w * w - 3 * a) * w)              (I111 / |dt|)
 *
 * r3 = 1 / sqrt(3) = 0.57735026918962576451, and 1/3 = 0.33333333333333333333, 2/3 = 0.66666666666666666667,
 * 4/3 = 1.3333333333333333333, 5/3 = 1.6666666666666666667 are literals rounded to the state dtype; the other constants are exact.
 * The caller evaluates a1 = drift(t0, y0), b1 = diffusion(t0, y0) before stage 1, a2 = drift(t0 + 3/4 dt, Y2),
 * b2 = diffusion(t0 + 1/4 dt, G2), b3 = diffusion(t0 + dt, G3) after it, and b4 = diffusion(t0 + 1/4 dt, G4) after stage 2.
 *
 * Stage 1, one launch, 6 n elements moved; no overlap between operands:
 *   Y2 = (y0 + a1 * (0.75 * dt)) + b1 * (1.5 * p)
 *   G2 = (y0 + a1 * (0.25 * dt)) + b1 * (0.5 * s)
 *   G3 = (y0 + a1 * dt) - b1 * s */
int xde_sde_srk_stage1(void* Y2, void* G2, void* G3, const void* y0, const void* a1, const void* b1, int64_t n, double dt, double s,
                       uint64_t seed, int64_t k, int dtype, void* stream);

/* Stage 2: G4 = (y0 + a1 * (0.25 * dt)) + ((b1 * -5 + b2 * 3) + b3 * 0.5) * s.  No generator; 6 n; no overlap. */
int xde_sde_srk_stage2(void* G4, const void* y0, const void* a1, const void* b1, const void* b2, const void* b3, int64_t n, double dt,
                       double s, int dtype, void* stream);

/* The step, one launch, 8 n:
 *   e1 = ((-w - q) + 2 * p) - 2 * u        e2 = 4/3 * ((w + q) - p) + 5/3 * u
 *   e3 = 2/3 * ((w - p) - u) - 1/3 * q     e4 = u
 *   y1 = ((((y0 + (1/3 * a1 + 2/3 * a2) * dt) + b1 * e1) + b2 * e2) + b3 * e3) + b4 * e4
 * y1 may be y0; no other overlap. */
int xde_sde_srk_step(void* y1, const void* y0, const void* a1, const void* a2, const void* b1, const void* b2, const void* b3,
                     const void* b4, int64_t n, double dt, double s, double c, double c3, uint64_t seed, int64_t k, int dtype,
                     void* stream);

/* THE BACKWARDS regenerate Z and V from (seed, k).  Outputs may be null by group and are then skipped: a group is given whole or not
 * at all (a group given in part is refused, right after the null-pointer check and before the n / dtype / k checks), and the generator runs only if a written output depends on it; every group null: nothing
 * to do.
 *
 * Stage 1 (the cotangents of Y2, G2, G3 in; groups: gy | ga1 | gb1):
 *   gy  = (gY2 + gG2) + gG3
 *   ga1 = (gY2 * (0.75 * dt) + gG2 * (0.25 * dt)) + gG3 * dt
 *   gb1 = (gY2 * (1.5 * p) + gG2 * (0.5 * s)) - gG3 * s */
int xde_sde_srk_stage1_backward(void* gy, void* ga1, void* gb1, const void* gY2, const void* gG2, const void* gG3, int64_t n, double dt,
                                double s, uint64_t seed, int64_t k, int dtype, void* stream);

/* Stage 2 (groups: ga1 | gb1, gb2, gb3; the cotangent of y0 is gG4 itself; no generator):
 *   ga1 = gG4 * (0.25 * dt),  gb1 = gG4 * (-5 * s),  gb2 = gG4 * (3 * s),  gb3 = gG4 * (0.5 * s) */
int xde_sde_srk_stage2_backward(void* ga1, void* gb1, void* gb2, void* gb3, const void* gG4, int64_t n, double dt, double s, int dtype,
                                void* stream);

/* The step (groups: ga1, ga2 | gb1, gb2, gb3, gb4; the cotangent of y0 is gy1 itself):
 *   ga1 = gy1 * (1/3 * dt),  ga2 = gy1 * (2/3 * dt),  gb_i = gy1 * e_i */
int xde_sde_srk_step_backward(void* ga1, void* ga2, void* gb1, void* gb2, void* gb3, void* gb4, const void* gy1, int64_t n, double dt,
                              double s, double c, double c3, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * REVERSIBLE HEUN (Kidger, Foster, Li, Lyons, "Efficient and Accurate Gradients for Neural SDEs", NeurIPS 2021: algebraically
 * reversible, Stratonovich, diagonal noise, one drift and one diffusion evaluation per step; strong order 1 where g_i depends on y_i
 * only).  The one Stratonovich scheme of this header: every entry point above is Ito.  The carried state is (y, yh, fh, gh) with
 * yh = y0, fh = drift(t0, y0), gh = diffusion(t0, y0) at the first grid step.  Z is the Z of (seed, k) above and w = s * Z; where
 * s == 0 the generator is skipped and w = s (a zero-length step: y1 = y0 exactly, yh1 = 2 y0 - yh0).  `direction` is +1 or -1
 * (anything else: XDE_EBADARG, checked first): dt and s are multiplied by it, exactly, before the formulas — the reverse step is the
 * forward step's two formulas at direction -1, applied to the state at t1.
 *
 * Predict, one launch, 5 n elements moved; yh1 may be yh0, no other overlap:
 *   yh1 = (((y0 + y0) - yh0) + f0 * dt) + g0 * w
 * The caller then evaluates f1 = drift(t1, yh1), g1 = diffusion(t1, yh1). */
int xde_sde_rheun_predict(void* yh1, const void* y0, const void* yh0, const void* f0, const void* g0, int64_t n, double dt, double s,
                          int direction, uint64_t seed, int64_t k, int dtype, void* stream);

/* Correct, one launch, 6 n; y1 may be y0, no other overlap:
 *   y1 = (y0 + (f0 + f1) * (0.5 * dt)) + (g0 + g1) * (0.5 * w)
 * The cotangents of predict and correct need no entry point of their own: xde_sde_em_backward at (dt, s) writes predict's gf0, gg0
 * (gy0 = gyh1 + gyh1, gyh0 = -gyh1), and at (0.5 * dt, 0.5 * s) correct's gf0 = gf1, gg0 = gg1 (gy0 = gy1), bit for bit: halving is
 * exact. */
int xde_sde_rheun_correct(void* y1, const void* y0, const void* f0, const void* f1, const void* g0, const void* g1, int64_t n, double dt,
                          double s, int direction, uint64_t seed, int64_t k, int dtype, void* stream);

/* THE COTANGENT SWEEP of the reversible Heun scheme (state cotangents ay, ayh, af, ag; dt, s and w the forward step's), two launches
 * per backward step around the vjp they feed.
 *
 * Stage, 5 n (3 n on the first backward step):
 *   bf = af1 + ay1 * (0.5 * dt)        bg = ag1 + ay1 * (0.5 * w)
 * af1 and ag1 may be null together and are then read as zero (the first backward step: bf = ay1 * (0.5 * dt),
 * bg = ay1 * (0.5 * w)); one of them null is refused.  bf may be af1 and bg may be ag1; no other overlap.  The caller then takes
 * v = the vjp of (f1, g1) at yh1 with (bf, bg). */
int xde_sde_rheun_adjoint_stage(void* bf, void* bg, const void* af1, const void* ag1, const void* ay1, int64_t n, double dt, double s,
                                uint64_t seed, int64_t k, int dtype, void* stream);

/* Step, one launch, 7 n (6 n on the first backward step):
 *   A    = ayh1 + v
 *   ay0  = ay1 + (A + A)                      ayh0 = -A
 *   af0  = ay1 * (0.5 * dt) + A * dt          ag0  = ay1 * (0.5 * w) + A * w
 * ayh1 may be null and is then read as zero (A = v).  ay0 may be ay1 and ayh0 may be ayh1; no other overlap. */
int xde_sde_rheun_adjoint_step(void* ay0, void* ayh0, void* af0, void* ag0, const void* ay1, const void* ayh1, const void* v, int64_t n,
                               double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/* The generator itself (tests, diagnostics): mode XDE_NOISE_NORMAL writes the Z the step kernels above use (the same device
 * function); XDE_NOISE_BITS writes Philox words (dtype is checked but does not change them). */
int xde_sde_noise(void* out, int64_t n, uint64_t seed, int64_t k, int mode, int dtype, void* stream);

/* The same at counter word 3 = draw: 0 writes what xde_sde_noise writes, bit for bit; 1 writes V (or its words). */
int xde_sde_noise_draw(void* out, int64_t n, uint64_t seed, int64_t k, int draw, int mode, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_SDE_H */
