"""Test-side restatement of sdeint's reversible Heun step and of sdeint_adjoint's sweep (include/xde_hip_sde.h, "REVERSIBLE HEUN"), in
numpy, written from the header and not from the kernel — per step k, with s = sqrt(|dt|) computed in float64 and rounded to the state
dtype, w = s*Z on the Z of tests/_sde_oracle.py (w = s where s == 0: the generator is skipped), dt and w times the direction:

    predict  yh1 = (((y0 + y0) - yh0) + f0*dt) + g0*w
    correct  y1  = (y0 + (f0 + f1)*(0.5*dt)) + (g0 + g1)*(0.5*w)
    stage    bf  = af1 + ay1*(0.5*dt)        bg = ag1 + ay1*(0.5*w)                  (af1, ag1 None: bf = ay1*(0.5*dt), bg = ay1*(0.5*w))
    step     A   = ayh1 + v                  ay0 = ay1 + (A + A)    ayh0 = -A        (ayh1 None: A = v)
             af0 = ay1*(0.5*dt) + A*dt       ag0 = ay1*(0.5*w) + A*w
"""
import numpy as np

from . import _sde_oracle as SO


def w_of(dt, z, dtype, direction=1):
    T = np.dtype(dtype).type
    s = T(direction) * SO.s_of(dt, dtype)
    return s * z if s != 0 else np.full_like(z, s)


def predict(y0, yh0, f0, g0, dt, z, dtype, direction=1):
    T = np.dtype(dtype).type
    return (((y0 + y0) - yh0) + f0 * (T(direction) * T(dt))) + g0 * w_of(dt, z, dtype, direction)


def correct(y0, f0, f1, g0, g1, dt, z, dtype, direction=1):
    T = np.dtype(dtype).type
    return (y0 + (f0 + f1) * (T(0.5) * (T(direction) * T(dt)))) + (g0 + g1) * (T(0.5) * w_of(dt, z, dtype, direction))


def adjoint_stage(af1, ag1, ay1, dt, z, dtype):
    """(bf, bg)."""
    T = np.dtype(dtype).type
    hf, hg = ay1 * (T(0.5) * T(dt)), ay1 * (T(0.5) * w_of(dt, z, dtype))
    return (hf, hg) if af1 is None else (af1 + hf, ag1 + hg)


def adjoint_step(ay1, ayh1, v, dt, z, dtype):
    """(ay0, ayh0, af0, ag0)."""
    T = np.dtype(dtype).type
    w = w_of(dt, z, dtype)
    A = v if ayh1 is None else ayh1 + v
    return ay1 + (A + A), -A, ay1 * (T(0.5) * T(dt)) + A * T(dt), ay1 * (T(0.5) * w) + A * w


def rheun_walk(drift, diffusion, y0, grid, seed, dtype, noise=None, carry=False):
    """The states at every point of ``grid`` (time dtype), step k on the Z of (seed, k) — ``noise(k)``, when given, supplies it
    instead (the GPU's own).  Returns [len(grid), *y0.shape] (``carry``: and the yh of every grid point)."""
    y = np.asarray(y0, dtype=dtype)
    yh, f, g = y, drift(grid[0], y), diffusion(grid[0], y)
    out, hats = [y], [yh]
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        z = noise(k) if noise is not None else SO.state_normals(y.shape, seed, k, dtype)
        yh1 = predict(y, yh, f, g, dt, z, dtype)
        f1, g1 = drift(grid[k + 1], yh1), diffusion(grid[k + 1], yh1)
        y = correct(y, f, f1, g, g1, dt, z, dtype)
        yh, f, g = yh1, f1, g1
        out.append(y)
        hats.append(yh)
    return (np.stack(out), np.stack(hats)) if carry else np.stack(out)


def adjoint_sweep(drift, diffusion, vjp, y_end, yh_end, grid, seed, dtype, cotangents, noise=None):
    """The sweep of the plain plan: ``cotangents[j]`` is the cotangent of the state at grid point j, ``vjp(t, yh, bf, bg)`` the
    cotangent of yh through ``(drift, diffusion)(t, yh)``.  Returns (grad_y0, the reconstructed y0, the reconstructed yh0)."""
    n = len(grid) - 1
    y, yh = np.asarray(y_end, dtype=dtype), np.asarray(yh_end, dtype=dtype)
    f, g = drift(grid[n], yh), diffusion(grid[n], yh)
    ay, ayh, af, ag = np.zeros_like(y), None, None, None
    for k in range(n - 1, -1, -1):
        dt = grid[k + 1] - grid[k]
        z = noise(k) if noise is not None else SO.state_normals(y.shape, seed, k, dtype)
        ay = ay + cotangents[k + 1]
        bf, bg = adjoint_stage(af, ag, ay, dt, z, dtype)
        v = vjp(grid[k + 1], yh, bf, bg)
        ay, ayh, af, ag = adjoint_step(ay, ayh, v, dt, z, dtype)
        yh0 = predict(y, yh, f, g, dt, z, dtype, -1)
        f0, g0 = drift(grid[k], yh0), diffusion(grid[k], yh0)
        y = correct(y, f, f0, g, g0, dt, z, dtype, -1)
        yh, f, g = yh0, f0, g0
    return ((ay + ayh) + vjp(grid[0], yh, af, ag)) + cotangents[0], y, yh
