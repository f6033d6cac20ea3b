/*
 * xde_hip_gn.h — entry points of libxde_hip.so for sdeint with GENERAL or SCALAR noise (sdeint(..., solver=Euler | Heun | GeneralReversibleHeun,
 * options={"noise_type": "general" | "scalar"})): the Ito Euler-Maruyama step whose diffusion is a matrix per row of the state and its
 * cotangents, the two launches of the Stratonovich Heun (trapezoidal) step on such a diffusion with theirs, and the reversible Heun step
 * with the launches of its constant-memory cotangent sweep (host side: paddlexde_amd/solver/base_fixed_solver.py,
 * paddlexde_amd/solver/_autograd.py, paddlexde_amd/functional/sdeint_adjoint.py).
 *
 * Same conventions as xde_hip_sde.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64, dt the step's size and s = sqrt(|dt|) rounded to the state dtype by the caller, both converted to the state dtype T
 * in the kernel, -ffp-contract=off: every result below is the written op order, rounded op by op).  Arguments are validated on the host
 * before anything is enqueued.
 *
 * THE LAYOUT.  The state operands (y1, y0, f and their cotangents) are contiguous rows x D arrays of T: output o = r * D + d, a row
 * being the last axis of the state.  The diffusion g (and its cotangent gg) is a contiguous rows x D x M array of T: g[r, d, m] at
 * o * M + m.  M is the dimension of the Brownian motion; M == 1 is scalar noise.
 *
 * THE NOISE.  The Brownian increment of row r is w[r, m] = s * Z[r * M + m], m < M, with Z the draw 0 of (seed, k) of xde_hip_sde.h
 * over a FLAT array of n = rows * M elements (Philox block j = e / W, W = 4 fp32, 2 fp64, also where M % W != 0 and a row starts
 * inside a block).  xde_sde_noise on a rows x M buffer therefore writes exactly the normals these kernels use, and with M == D the
 * noise is that of xde_sde_em_step on the state.
 *
 * THE CAPS.  1 <= rows, 1 <= D <= 2^30, 1 <= M <= 2^30 and rows * D * M <= 2^48; 0 <= k < 2^32.  Every pointer is aligned to its
 * element type (16-byte alignment is not required: the kernels find the aligned part of every span themselves).
 */
#ifndef XDE_HIP_GN_H
#define XDE_HIP_GN_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE STEP, one launch, (3 + M) N elements read and N written, N = rows * D.  Per output o = r * D + d, in T:
 *
 *   a     = g[o * M] * w[r, 0]
 *   a     = a + g[o * M + m] * w[r, m]          for m = 1 .. M - 1, in this order
 *   y1[o] = (y0[o] + f[o] * dt) + a
 *
 * The sum runs over m sequentially for every M, every dtype and every launch shape: the result is a function of the operands' bits.
 * With M == D and g[r, d, m] = (d == m ? b[r, d] : 0) it is xde_sde_em_step's y1 on the diffusion b wherever the products are finite.
 * y1 may be y0 (an in-place step); no other overlap.
 */
int xde_sde_gn_step(void* y1, const void* y0, const void* f, const void* g, int64_t rows, int64_t D, int64_t M, double dt, double s,
                    uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * THE COTANGENTS, one launch that regenerates w from (seed, k): N elements read and (1 + M) N written.  From gy1, the cotangent of
 * y1 (that of y0 is gy1 itself):
 *
 *   gf[o]         = gy1[o] * dt
 *   gg[o * M + m] = gy1[o] * w[r, m]
 *
 * A null gf or gg skips that output; with gg null no generator runs (s, seed are not read; k is still checked); both null: nothing
 * to do (after the checks).  No output may overlap another operand.
 */
int xde_sde_gn_backward(void* gf, void* gg, const void* gy1, int64_t rows, int64_t D, int64_t M, double dt, double s, uint64_t seed,
                        int64_t k, int dtype, void* stream);

/*
 * HEUN (the stochastic trapezoidal rule: Stratonovich, strong order 1/2 in general and 1 for commutative noise), two launches around
 * the evaluations f1 = drift(t1, yp), g1 = diffusion(t1, yp).  Composed from per-formula launches the step would stream g0 twice (for
 * the predictor and again for the corrector) and g1 once; here the predictor KEEPS its matrix-vector product: it writes a0 = g0 w next
 * to yp, and the corrector reads a0 (N elements) and streams only g1 — two streams of M N elements per step, not three.  Both use the w
 * of (seed, k) above, and every sum over m is the step's: sequential in m for every launch shape.
 *
 * PREDICT, one launch, (3 + M) N elements read and 2 N written.  Per output o = r * D + d, in T:
 *
 *   a     = g0[o * M] * w[r, 0]
 *   a     = a + g0[o * M + m] * w[r, m]         for m = 1 .. M - 1, in this order
 *   a0[o] = a
 *   yp[o] = (y0[o] + f0[o] * dt) + a
 *
 * yp has the bits of xde_sde_gn_step's y1 on the same operands.  No operand may overlap an output.
 */
int xde_sde_gn_heun_predict(void* yp, void* a0, const void* y0, const void* f0, const void* g0, int64_t rows, int64_t D, int64_t M,
                            double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * CORRECT, one launch, (4 + M) N elements read and N written:
 *
 *   b     = g1[o * M] * w[r, 0]
 *   b     = b + g1[o * M + m] * w[r, m]         for m = 1 .. M - 1, in this order
 *   y1[o] = (y0[o] + (f0[o] + f1[o]) * (0.5 * dt)) + (a0[o] + b) * 0.5
 *
 * y1 may be y0 (an in-place step); no other overlap of y1 with an operand.
 */
int xde_sde_gn_heun_correct(void* y1, const void* y0, const void* f0, const void* f1, const void* a0, const void* g1, int64_t rows,
                            int64_t D, int64_t M, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * THE COTANGENTS OF BOTH, one launch that regenerates w from (seed, k).  From gy, the cotangent of the launch's state output, and gc, a
 * second cotangent that reaches the matrix (null: none), with the scalars cf and ca converted to T:
 *
 *   h             = gy[o] * ca
 *   c             = h + gc[o]                   (gc null: c = h;  gy null: c = gc[o])
 *   gf[o]         = gy[o] * cf
 *   ga[o]         = h
 *   gg[o * M + m] = c * w[r, m]
 *
 * A null gf, ga or gg skips that output; all null: nothing to do (after the checks).  With gy null gc must be given, and gf and ga
 * must be null.  With gg null no generator runs (s, seed are not read; k is still checked).  No output may overlap another operand.
 *
 * The corrector's cotangents are this launch at (cf, ca) = (0.5 * dt, 0.5) with gy = gy1 and gc null: gf is the cotangent of f0 and
 * of f1, ga that of a0, gg that of g1 (the cotangent of y0 is gy1 itself; halving is exact, as for xde_sde_rheun_correct).  The
 * predictor's are this launch at (cf, ca) = (dt, 1) with gy = gyp, gc = ga0 (the cotangent of its second output) and ga null: gf is
 * the cotangent of f0 and gg[o * M + m] = (gyp[o] + ga0[o]) * w[r, m] that of g0 — both cotangents that reach g0 in one launch, so
 * no M N elements are accumulated outside it; the cotangent of y0 is gyp itself.
 */
int xde_sde_gn_heun_backward(void* gf, void* ga, void* gg, const void* gy, const void* gc, int64_t rows, int64_t D, int64_t M, double cf,
                             double ca, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * REVERSIBLE HEUN on such a diffusion (solver=GeneralReversibleHeun; Stratonovich, one drift and one diffusion evaluation per step, and
 * algebraically reversible: sdeint_adjoint sweeps it backwards in constant memory).  The step carries (yh, fh, gh) and a = gh w besides
 * the state, with the w of (seed, k) above; every sum over m is the step's, sequential in m.  Step k is a predictor launch, the
 * evaluations fh1 = drift(t1, yh1), gh1 = diffusion(t1, yh1), and xde_sde_gn_heun_correct at (f0, f1, a0, g1) = (fh0, fh1, a, gh1).  A
 * reverse step is the same launches with dt and s negated by the caller (a negative s is legal in every entry point here).
 *
 * PREDICT, one launch, (4 + M) N elements read and 2 N written, (M + 6) N in all.  Per output o = r * D + d, in T:
 *
 *   a[o]   = g[o * M] * w[r, 0]  (+ g[o * M + m] * w[r, m] for m = 1 .. M - 1, in this order)
 *   yh1[o] = (((y[o] + y[o]) - yh0[o]) + f[o] * dt) + a[o]
 *
 * No output may overlap another operand.
 */
int xde_sde_gn_rheun_predict(void* yh1, void* a, const void* y, const void* yh0, const void* f, const void* g, int64_t rows, int64_t D,
                             int64_t M, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * THE SEAM between two steps, one launch and ONE pass over g1 = gh1, which meets two increments: step k0's corrector takes g1 w_{k0}
 * and step k1's predictor g1 w_{k1}.  (6 + M) N elements read and 3 N written: (M + 9) N for what the two launches move in
 * (2 M + 11) N; without the re-read of y1 the pair would save, (M + 8) against (2 M + 11).  Both increment arrays of a tile's rows are
 * generated once per workgroup; each output keeps two sums, both sequential in m.
 *
 *   y1[o]  = (y0[o] + (f0[o] + f1[o]) * (0.5 * dt0)) + (a0[o] + b) * 0.5,      b = sum_m g1[o * M + m] * w_{k0}[r, m]
 *   a1[o]  = sum_m g1[o * M + m] * w_{k1}[r, m]
 *   yh2[o] = (((y1[o] + y1[o]) - yh1[o]) + f1[o] * dt1) + a1[o]
 *
 * y1 has the bits of xde_sde_gn_heun_correct at (dt0, s0, k0), and (yh2, a1) those of xde_sde_gn_rheun_predict at (dt1, s1, k1) on
 * y = y1, yh0 = yh1, f = f1, g = g1; y1 goes from the register into the predictor, not through memory.  w_{k0} = s0 Z(seed, k0) and
 * w_{k1} = s1 Z(seed, k1); 0 <= k0, k1 < 2^32.  y1 may be y0 (an in-place step); no other overlap, and yh2 may not be yh1.
 */
int xde_sde_gn_rheun_seam(void* y1, void* yh2, void* a1, const void* y0, const void* f0, const void* f1, const void* a0, const void* yh1,
                          const void* g1, int64_t rows, int64_t D, int64_t M, double dt0, double s0, int64_t k0, double dt1, double s1,
                          int64_t k1, uint64_t seed, int dtype, void* stream);

/*
 * THE COTANGENT SWEEP of the scheme.  At grid point k1 = k0 + 1 it carries ay (of the state), ayh (of yh), af (of fh) and ONE state-sized
 * vector c in the place of the cotangent of gh: what reaches gh1 is rank two per output, c1[o] w_{k1}[r, :] from the step after and
 * (ay1[o] / 2) w_{k0}[r, :] from step k0's corrector, so no M N elements are carried from step to step.
 *
 * THE STAGE, one launch that regenerates both increments: 3 N elements read and (1 + M) N written, bg with 16-byte stores.
 *
 *   bf[o]         = af1[o] + ay1[o] * (0.5 * dt)
 *   p             = ay1[o] * 0.5
 *   bg[o * M + m] = c1[o] * w_{k1}[r, m] + p * w_{k0}[r, m]
 *
 * af1 and c1 null together (the first backward step): bf[o] = ay1[o] * (0.5 * dt) and bg[o * M + m] = p * w_{k0}[r, m]; s1 and k1 are
 * then not used (k1 is still checked).  ay1 null (the sweep's tail, for the cotangent of the initial state): bg[o * M + m] =
 * c1[o] * w_{k1}[r, m], and bf and af1 must be null.  bg, and one of ay1 and c1, are required; with ay1 given so is bf.  bf may be af1;
 * no other overlap.  (bf, bg) are the cotangents the vjp of (drift, diffusion) at yh1 takes.
 */
int xde_sde_gn_rheun_adjoint_stage(void* bf, void* bg, const void* af1, const void* c1, const void* ay1, int64_t rows, int64_t D, int64_t M,
                                   double dt, double s0, int64_t k0, double s1, int64_t k1, uint64_t seed, int dtype, void* stream);

/*
 * THE STEP, from v, the cotangent of yh1 that vjp returned; no generator and no matrix, n = rows * D elements of T, 7 n moved:
 *
 *   A       = ayh1[e] + v[e]                     (ayh1 null, the first backward step: A = v[e])
 *   ay0[e]  = ay1[e] + (A + A)
 *   ayh0[e] = -A
 *   af0[e]  = ay1[e] * (0.5 * dt) + A * dt
 *   c0[e]   = ay1[e] * 0.5 + A
 *
 * ay0 may be ay1 and ayh0 may be ayh1 (in place); no other overlap.  n == 0: nothing to do (after the checks).
 */
int xde_sde_gn_rheun_adjoint_step(void* ay0, void* ayh0, void* af0, void* c0, const void* ay1, const void* ayh1, const void* v, int64_t n,
                                  double dt, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_GN_H */
