/*
 * xde_hip_kl.h — entry points of libxde_hip.so for the KL term of a latent SDE (sdeint(..., options={"logqp": True, "prior_drift": h})):
 * the Ito Euler-Maruyama step of xde_hip_sde.h fused with the row-wise accumulation of the Girsanov integrand, and its cotangents
 * (host side: paddlexde_amd/solver/base_fixed_solver.py, paddlexde_amd/solver/_autograd.py).
 *
 * Between the posterior dy = f dt + g dW and the prior dy = h dt + g dW (one diagonal diffusion g) the KL divergence over a step is
 * 1/2 |(f - h) / g|^2 dt, summed over the state's last axis.  The step launch has f and g in registers already; it reads h as well,
 * and keeps the running sum of a row in a double.
 *
 * Same conventions as xde_hip_sde.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64, Z[e] the normal of flat element e at grid step k under the 64-bit seed, dt the step's size and s = sqrt(|dt|)
 * rounded to the state dtype by the caller, both converted to the state dtype T in the kernel, -ffp-contract=off: every result below
 * is the written op order, rounded op by op).  Arguments are validated on the host before anything is enqueued.
 *
 * THE LAYOUT.  The state operands (y1, y0, f, g, h and their cotangents) are contiguous rows x D arrays of T: element e = r * D + d, a
 * row being the last axis of the state.  The accumulators (acc1, acc0, gacc) are double[rows], whatever T is.  rows >= 0, D >= 1.
 *
 * THE NOISE of element e is the Z[e] of xde_hip_sde.h: Philox block j = e / W (W = 4 fp32, 2 fp64) over the FLAT array, not over the
 * row, also where D % W != 0 and a row starts inside a block.
 *
 * g == 0 gives a non-finite u that flows into acc1: nothing checks it (a check would need a synchronisation).  The diffusion of a
 * latent SDE must be non-zero.
 */
#ifndef XDE_HIP_KL_H
#define XDE_HIP_KL_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * THE STEP, one launch, 5 rows D elements and two doubles per row moved.  Per element e = r * D + d, in T:
 *
 *   y1[e] = (y0[e] + f[e] * dt) + g[e] * (s * Z[e])          xde_sde_em_step's expression on the same Z: the same bits
 *   u = (f[e] - h[e]) / g[e],  t = u * u                     each rounded in T
 *
 * and per row, in double:
 *
 *   q[r]    = sum over d of double(t)                        in an order this header does not fix: it depends on (D, dtype, whether
 *                                                            every state pointer is 16-byte aligned and D % W == 0, and r * D mod W)
 *                                                            only, so a launch repeats its bits, and both modes below give the same
 *   acc1[r] = acc0[r] + q[r] * (0.5 * double(T(dt)))         the signed dt
 *
 * acc0 null is read as zero.  acc1 may be acc0 and y1 may be y0.  y1 and y0 BOTH null is the accumulate-only mode: only f, g, h are read
 * (3 rows D), no generator runs, and s, seed and k are ignored (Milstein's step keeps its own launches and adds this one).  One of y1 /
 * y0 null without the other is refused, and so is any other overlap between an output and another operand.
 */
int xde_sde_kl_step(void* y1, double* acc1, const void* y0, const void* f, const void* g, const void* h, const double* acc0,
                    int64_t rows, int64_t D, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

/*
 * THE COTANGENTS, one launch that regenerates Z.  From gy1 (the cotangent of y1) and gacc (that of acc1); the cotangent of y0 is gy1
 * itself and that of acc0 is gacc itself.  Per row a = T(gacc[r] * double(T(dt))), rounded to T once; per element, in T:
 *
 *   u  = (f - h) / g
 *   c  = a * (u / g)
 *   gf = gy1 * dt + c
 *   gh = -c
 *   gg = gy1 * (s * Z) - c * u
 *
 * gy1 null is the accumulate-only mode's backward: gf = c, gh = -c, gg = -(c * u), no generator runs, and s, seed and k are ignored.
 * Each of gf, gg, gh may be null and is then skipped; all three null: nothing to do.  gacc, f, g and h are required.  No output may
 * overlap another operand.
 */
int xde_sde_kl_backward(void* gf, void* gg, void* gh, const void* gy1, const double* gacc, const void* f, const void* g, const void* h,
                        int64_t rows, int64_t D, double dt, double s, uint64_t seed, int64_t k, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_KL_H */
