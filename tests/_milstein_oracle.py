"""Test-side restatement of sdeint's Milstein step (include/xde_hip_sde.h), in numpy, on the normals of tests/_sde_oracle.py: Kloeden &
Platen's explicit strong order 1.0 scheme for Ito SDEs with diagonal noise, in the state dtype's op order —

    yb = (y0 + f*dt) + g*s            gb = diffusion(t0, yb)
    w  = s*Z    q = c*(w*w - a)       y1 = ((y0 + f*dt) + g*w) + (gb - g)*q

with s = sqrt(|dt|) and c = 0.5/sqrt(|dt|) computed in float64 and rounded to the state dtype (c = 0 when dt == 0), a = |dt| in the
state dtype."""
import numpy as np

from . import _sde_oracle as SO


def c_of(dt, dtype):
    """c = 0.5/sqrt(|dt|) in float64 of the time-dtype dt, rounded to the state dtype; 0 for a zero-length step."""
    T = np.dtype(dtype).type
    root = np.sqrt(abs(np.float64(dt)))
    return T(0.5 / root) if root > 0 else T(0.0)


def support(y, f, g, dt, dtype):
    T = np.dtype(dtype).type
    return (y + f * T(dt)) + g * SO.s_of(dt, dtype)


def correction(dt, z, dtype):
    """(w, q) of a step of size dt on the normals z."""
    T = np.dtype(dtype).type
    w = SO.s_of(dt, dtype) * z
    return w, c_of(dt, dtype) * (w * w - abs(T(dt)))


def milstein_step(y, f, g, gb, dt, z, dtype):
    T = np.dtype(dtype).type
    w, q = correction(dt, z, dtype)
    return ((y + f * T(dt)) + g * w) + (gb - g) * q


def milstein_walk(drift, diffusion, y0, grid, seed, dtype, noise=None):
    """The states at every point of ``grid`` (time dtype), step k on the noise of (seed, k) — ``noise(k)``, when given, supplies Z
    instead (the GPU's own).  Returns [len(grid), *y0.shape]."""
    y = np.asarray(y0, dtype=dtype)
    out = [y]
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        z = noise(k) if noise is not None else SO.state_normals(y.shape, seed, k, dtype)
        f, g = drift(grid[k], y), diffusion(grid[k], y)
        gb = diffusion(grid[k], support(y, f, g, dt, dtype))
        y = milstein_step(y, f, g, gb, dt, z, dtype)
        out.append(y)
    return np.stack(out)
