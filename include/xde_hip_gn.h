/*
 * xde_hip_gn.h — entry points of libxde_hip.so for sdeint with GENERAL or SCALAR noise (sdeint(..., solver=Euler,
 * options={"noise_type": "general" | "scalar"})): the Ito Euler-Maruyama step whose diffusion is a matrix per row of the state, and its
 * cotangents (host side: paddlexde_amd/solver/base_fixed_solver.py, paddlexde_amd/solver/_autograd.py).
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

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_GN_H */
