"""Test-side restatement of include/xde_hip_kl.h in numpy, written from the header and not from the kernel: the Euler-Maruyama step
fused with the KL accumulation of a latent SDE, its cotangents, and the walk of ``sdeint(..., options={"logqp": True, ...})``.  State
arrays are ``[..., D]`` in the state dtype ``T`` (a row is the last axis), accumulators float64 ``[...]``; every element-wise op is
rounded in ``T``, the row sum ``q`` is ``math.fsum`` of the terms as doubles (exactly rounded: the kernel's order is not fixed)."""
import math

import numpy as np

from . import _sde_oracle as SO


def terms(f, g, h, dtype):
    """``t = u*u`` with ``u = (f - h)/g``, both rounded in the state dtype; returns ``(u, t)``."""
    T = np.dtype(dtype).type
    f, g, h = (np.asarray(x, dtype=T) for x in (f, g, h))
    u = ((f - h) / g).astype(T)
    return u, (u * u).astype(T)


def row_sums(t):
    """``q[r] = sum_d double(t[r, d])``, exactly rounded (float64, the shape of t without its last axis)."""
    t = np.asarray(t)
    flat = t.reshape(-1, t.shape[-1]).astype(np.float64)
    return np.array([math.fsum(row) for row in flat], dtype=np.float64).reshape(t.shape[:-1])


def half_dt(dt, dtype):
    """``0.5 * double(T(dt))``: the signed dt, through the state dtype."""
    return 0.5 * np.float64(np.dtype(dtype).type(dt))


def accumulate(acc0, f, g, h, dt, dtype):
    """``acc1 = acc0 + q * (0.5 * double(T(dt)))`` and the increment itself; ``acc0`` None: zero.  Returns ``(acc1, q * half)``."""
    q = row_sums(terms(f, g, h, dtype)[1])
    inc = q * half_dt(dt, dtype)
    return (np.zeros_like(q) if acc0 is None else np.asarray(acc0, dtype=np.float64)) + inc, inc


def kl_step(y0, f, g, h, acc0, dt, z, dtype):
    """The fused step: ``(y1, acc1)`` with ``y1`` xde_sde_em_step's expression on the normals ``z`` (state dtype)."""
    return SO.em_step(y0, f, g, dt, z, dtype), accumulate(acc0, f, g, h, dt, dtype)[0]


def kl_backward(gy1, gacc, f, g, h, dt, s, z, dtype):
    """``(gf, gg, gh)`` in the header's op order; ``gy1`` None: the accumulate-only mode's (``z`` and ``s`` are then not read)."""
    T = np.dtype(dtype).type
    f, g, h = (np.asarray(x, dtype=T) for x in (f, g, h))
    a = (np.asarray(gacc, dtype=np.float64) * np.float64(T(dt))).astype(T)[..., None]
    u = (f - h) / g
    c = a * (u / g)
    if gy1 is None:
        return c, -(c * u), -c
    gy1 = np.asarray(gy1, dtype=T)
    return gy1 * T(dt) + c, gy1 * (T(s) * z) - c * u, -c


def kl_walk(drift, diffusion, prior, y0, grid, dtype, noise, milstein=None):
    """The Euler-Maruyama walk of a latent SDE over ``grid`` (time dtype) on the normals ``noise(k)``: the states at every grid point
    and the cumulative KL sums there (float64, [len(grid), *y0.shape[:-1]]), and per step the increment ``q * half`` and the sum it was
    added to (for error bounds).  ``milstein(y, f, g, dt, z)``, when given, makes the state's step instead of Euler-Maruyama's."""
    y = np.asarray(y0, dtype=dtype)
    acc = np.zeros(y.shape[:-1], dtype=np.float64)
    states, cums, incs = [y], [acc], []
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        f, g, h = drift(grid[k], y), diffusion(grid[k], y), prior(grid[k], y)
        acc1, inc = accumulate(acc, f, g, h, dt, dtype)
        incs.append((np.abs(acc), np.abs(inc)))
        z = noise(k)
        y = SO.em_step(y, f, g, dt, z, dtype) if milstein is None else milstein(y, f, g, dt, z)
        acc = acc1
        states.append(y)
        cums.append(acc)
    return np.stack(states), np.stack(cums), incs


def cum_at(cums, grid, t):
    """The cumulative sums at the output times ``t``: the first grid step whose end has reached t[j] (tests/_sde_oracle.py: rows_at);
    the value at either end, else ``L_a + w*(L_b - L_a)`` with ``w = (t - t_a)/(t_b - t_a)`` in the time dtype, as a double."""
    d = -1 if grid[-1] < grid[0] else 1
    n = len(grid) - 1
    rows = [cums[0]]
    for tj in t[1:]:
        if n == 0:
            rows.append(cums[0])
            continue
        k = min(max(int(np.searchsorted(d * grid, d * tj, side="left")) - 1, 0), n - 1)
        ta, tb = grid[k], grid[k + 1]
        if tj == ta:
            rows.append(cums[k])
        elif tj == tb:
            rows.append(cums[k + 1])
        else:
            w = float((tj - ta) / (tb - ta))
            rows.append(cums[k] + w * (cums[k + 1] - cums[k]))
    return np.stack(rows)


def logqp_of(cum_rows, dtype):
    """``logqp[..., i] = L(t_{i+1}) - L(t_i)`` rounded to the state dtype: [*lead, T-1]."""
    return np.moveaxis(cum_rows[1:] - cum_rows[:-1], 0, -1).astype(dtype)
