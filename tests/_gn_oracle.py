"""Test-side restatement of include/xde_hip_gn.h in numpy, written from the header and not from the kernel: the Ito Euler-Maruyama
step with general (and scalar) noise, its cotangents, and the walk of ``sdeint(..., solver=Euler, options={"noise_type": ...})``.
The state is ``[..., D]`` in the state dtype ``T``, the diffusion ``[..., D, M]``, the normals ``[..., M]``: one per row of the state
(its last axis) and m, element ``r*M + m`` of the flat array the generator of tests/_sde_oracle.py fills.  Every op is rounded in
``T``; the sum over m is sequential."""
import numpy as np

from . import _sde_oracle as SO


def noise_shape(state_shape, M):
    """The shape of the normals of a state of ``state_shape`` under an M-dimensional Brownian motion: ``[..., M]``."""
    return tuple(state_shape[:-1]) + (int(M),)


def increments(z, s, dtype):
    """``w = s * Z`` in the state dtype."""
    T = np.dtype(dtype).type
    return (T(s) * np.asarray(z, dtype=T)).astype(T)


def matvec(g, w, dtype):
    """``a[.., d] = g[.., d, 0]*w[.., 0]``, then ``a = a + g[.., d, m]*w[.., m]`` for m = 1 .. M-1 in this order, each op rounded."""
    T = np.dtype(dtype).type
    g, w = np.asarray(g, dtype=T), np.asarray(w, dtype=T)
    a = (g[..., 0] * w[..., 0:1]).astype(T)
    for m in range(1, g.shape[-1]):
        a = (a + (g[..., m] * w[..., m : m + 1]).astype(T)).astype(T)
    return a


def gn_step(y0, f, g, dt, s, z, dtype):
    """``y1 = (y0 + f*dt) + a`` on the normals ``z`` ([..., M], state dtype)."""
    T = np.dtype(dtype).type
    y0, f = np.asarray(y0, dtype=T), np.asarray(f, dtype=T)
    base = (y0 + (f * T(dt)).astype(T)).astype(T)
    return (base + matvec(g, increments(z, s, T), T)).astype(T)


def gn_backward(gy1, dt, s, z, dtype):
    """``(gf, gg)``: ``gf = gy1*dt`` ([..., D]) and ``gg[.., d, m] = gy1[.., d]*w[.., m]`` ([..., D, M])."""
    T = np.dtype(dtype).type
    gy1 = np.asarray(gy1, dtype=T)
    w = increments(z, s, T)
    return (gy1 * T(dt)).astype(T), (gy1[..., :, None] * w[..., None, :]).astype(T)


def gn_walk(drift, diffusion, y0, grid, dtype, noise):
    """The states at every point of ``grid`` (time dtype), step k on the normals ``noise(k)`` ([..., M]): [len(grid), *y0.shape]."""
    y = np.asarray(y0, dtype=dtype)
    out = [y]
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        y = gn_step(y, drift(grid[k], y), diffusion(grid[k], y), dt, SO.s_of(dt, dtype), noise(k), dtype)
        out.append(y)
    return np.stack(out)
