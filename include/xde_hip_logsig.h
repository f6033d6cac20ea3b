/*
 * xde_hip_logsig.h — entry points of libxde_hip.so for LOGSIGNATURE WINDOWS: the depth-2 log-ODE control of cdeint (Morrill et al.,
 * "Neural rough differential equations for long time series").  A series of T points is cut into windows of L steps; each window is
 * replaced by its logsignature — its increment and, at depth 2, its Levy areas — and the CDE is solved on the W = ceil((T - 1) / L)
 * windows instead of the T - 1 steps (host side: paddlexde_amd/interpolation/__init__.py, logsig_windows and logsig_path).
 *
 * Same conventions as xde_hip_gn.h (status codes, device pointers borrowed from the caller, `stream` = hipStream_t as void*,
 * XDE_F32 / XDE_F64 naming the state dtype T, -ffp-contract=off: every result below is the written op order, rounded op by op).
 * Arguments are validated on the host before anything is enqueued.
 *
 * THE LAYOUT.  x is a contiguous B x T x C array of T.  Window w < W covers the points p_0 .. p_n = x[b, w L .. min((w + 1) L, T - 1), :],
 * so 1 <= n <= L and only the last window may be shorter.  The output is a contiguous B x W x K array of T: K = C at depth 1 and
 * K = C + C (C - 1) / 2 at depth 2, level 1 first (channel c at index c), then the pairs (i, j), i < j, in lexicographic order:
 * pair(i, j) = C + i (2 C - i - 1) / 2 + (j - i - 1).
 *
 * NaN.  A NaN (or infinite) entry of x propagates into every output of the windows that hold it, and into no other window.  These
 * entry points know nothing of "not observed": the caller fills unobserved entries first.
 *
 * THE CAPS.  1 <= B, 2 <= T, 1 <= C <= 512, 1 <= L (an L beyond T - 1 is one window), depth 1 or 2 (deeper levels are not built:
 * XDE_EBADARG), B * T * C <= 2^48 and B * W * K <= 2^48.  Every pointer is aligned to its element type (16-byte alignment is not
 * required: the kernels find the aligned part of every span themselves).  No output may overlap another operand.
 */
#ifndef XDE_HIP_LOGSIG_H
#define XDE_HIP_LOGSIG_H

#include "xde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K of the layout above, or -1 (and a message) when C or depth is outside the caps.  Nothing is enqueued. */
int64_t xde_logsig_channels(int64_t C, int depth);

/*
 * THE WINDOWS, one launch, B T C elements read and B W K written.  Per (b, w), with u_k = p_k - p_0 and D_k = p_{k+1} - p_k, both
 * rounded in T:
 *
 *   out[c]          = p_n[c] - p_0[c]                                                   (level 1: one subtraction)
 *   acc             = 0                                                                 (float64)
 *   acc             = acc + (double(u_k[i]) * double(D_k[j]) - double(u_k[j]) * double(D_k[i]))   for k = 1 .. n - 1, in this order
 *   out[pair(i, j)] = T(0.5 * acc)                                                      (level 2: the Levy area of channels i < j)
 *
 * n == 1 gives exact zeros at level 2.  The sum runs over k sequentially for every shape, every dtype and every launch plan: the
 * result is a function of the operands' bits.
 */
int xde_logsig_windows(void* out, const void* x, int64_t B, int64_t T, int64_t C, int64_t L, int depth, int dtype, void* stream);

/*
 * THE COTANGENT of x from gout, the cotangent of out: one launch, no atomics, every element of gx written once; B T C + B W K
 * elements read and B T C written.  Let g1 be a window's level-1 cotangents and G the antisymmetric matrix of its level-2 cotangents:
 * G[i][j] = gout[pair(i, j)] for i < j, G[j][i] = -G[i][j], G[i][i] = 0 (at depth 1: G = 0).  The window's contribution to its point
 * p_m, channel c, in float64:
 *
 *   s = 0
 *   s = s + double(G[c][j]) * double(T(nxt[j] - prv[j]))        for j = 0 .. C - 1, j != c, in this order
 *   q = 0.5 * s
 *   q = q + double(g1[c])   if m == n;      q = q - double(g1[c])   if m == 0
 *
 * where nxt and prv are the neighbours of p_m in the window's closed polygon p_0 .. p_n: the predecessor of p_0 is p_n and the
 * successor of p_n is p_0 (with n == 1 both neighbours are the other point and the difference is zero).  A point of one window gets
 * gx = T(q).  A point shared by two windows (t % L == 0, 0 < t < T - 1) gets gx = T(q_earlier + q_later): the earlier window's
 * contribution first, one rounding to T.  x is the forward's operand.
 */
int xde_logsig_windows_backward(void* gx, const void* gout, const void* x, int64_t B, int64_t T, int64_t C, int64_t L, int depth,
                                int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* XDE_HIP_LOGSIG_H */
