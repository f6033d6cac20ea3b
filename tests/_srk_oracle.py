"""Test-side restatement of sdeint's SRK step (include/xde_hip_sde.h), in numpy, written from the header and not from the kernel:
Roessler's derivative-free strong order 1.5 scheme SRI1W1 for Ito SDEs with diagonal noise, in the state dtype's op order —

    w = s*Z    p = 0.5*(w + (s*V)*r3)    q = c*(w*w - a)    u = c3*((w*w - 3*a)*w)
    Y2 = (y + a1*(0.75*dt)) + b1*(1.5*p)      G2 = (y + a1*(0.25*dt)) + b1*(0.5*s)      G3 = (y + a1*dt) - b1*s
    G4 = (y + a1*(0.25*dt)) + ((b1*-5 + b2*3) + b3*0.5)*s
    e1 = ((-w - q) + 2*p) - 2*u    e2 = 4/3*((w + q) - p) + 5/3*u    e3 = 2/3*((w - p) - u) - 1/3*q    e4 = u
    y1 = ((((y + (1/3*a1 + 2/3*a2)*dt) + b1*e1) + b2*e2) + b3*e3) + b4*e4

with s = sqrt(|dt|), c = 0.5/sqrt(|dt|) and c3 = 1/(6|dt|) computed in float64 and rounded to the state dtype (c = c3 = 0 when
dt == 0), a = |dt| in the state dtype.  Z is the draw of tests/_sde_oracle.py (counter word 3 = 0); V, the second draw, is the same
mapping at counter word 3 = 1, built here from that module's Philox, uniforms and Box-Muller."""
import numpy as np

from . import _milstein_oracle as MO
from . import _sde_oracle as SO

_MASK = np.uint64(0xFFFFFFFF)


def consts(dtype):
    """(r3, 1/3, 2/3, 4/3, 5/3): the header's decimal literals rounded to the state dtype."""
    T = np.dtype(dtype).type
    return tuple(T(x) for x in ("0.57735026918962576451", "0.33333333333333333333", "0.66666666666666666667", "1.3333333333333333333",
                                "1.6666666666666666667"))


def words(nblk, seed, k, draw):
    """The words of counters (j_lo, j_hi, k, draw), j = 0 .. nblk-1: [nblk, 4] uint32."""
    j = np.arange(nblk, dtype=np.uint64)
    ctr = np.stack([j & _MASK, j >> np.uint64(32), np.full_like(j, k), np.full_like(j, draw)], axis=-1)
    return SO.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def normals(n, seed, k, dtype, draw, with_r=False):
    """The normals of draw ``draw`` for a state of ``dtype``, Box-Muller in float64 (not rounded): float64 [n] (and r of each)."""
    W = 4 if np.dtype(dtype) == np.float32 else 2
    u = SO.uniforms(words(-(-n // W), seed, k, draw), dtype)
    zs, rs = [], []
    for pair in range(W // 2):
        z0, z1, r = SO.box_muller(u[:, 2 * pair], u[:, 2 * pair + 1])
        zs += [z0, z1]
        rs += [r, r]
    z = np.stack(zs, axis=-1).reshape(-1)[:n]
    return (z, np.stack(rs, axis=-1).reshape(-1)[:n]) if with_r else z


def state_normals(shape, seed, k, dtype, draw):
    """The draw of a state of ``shape`` in its dtype (the float64 Box-Muller rounded once); draw 0 is tests/_sde_oracle.py's Z."""
    if draw == 0:
        return SO.state_normals(shape, seed, k, dtype)
    return normals(int(np.prod(shape)), seed, k, dtype, draw).astype(dtype).reshape(shape)


def c3_of(dt, dtype):
    """c3 = 1/(6|dt|) in float64 of the time-dtype dt, rounded to the state dtype; 0 for a zero-length step."""
    T = np.dtype(dtype).type
    a = abs(np.float64(dt))
    return T(1.0 / (6.0 * a)) if a > 0 else T(0.0)


def wp(dt, z, v, dtype):
    T = np.dtype(dtype).type
    s = SO.s_of(dt, dtype)
    w = s * z
    return w, T(0.5) * (w + (s * v) * consts(dtype)[0])


def weights(dt, z, v, dtype):
    """(e1, e2, e3, e4) of a step of size dt on the draws z, v."""
    T = np.dtype(dtype).type
    _, third, two3, four3, five3 = consts(dtype)
    w, p = wp(dt, z, v, dtype)
    a = abs(T(dt))
    q = MO.c_of(dt, dtype) * (w * w - a)
    u = c3_of(dt, dtype) * ((w * w - T(3) * a) * w)
    return (((-w - q) + T(2) * p) - T(2) * u, four3 * ((w + q) - p) + five3 * u, two3 * ((w - p) - u) - third * q, u)


def stage1(y, a1, b1, dt, z, v, dtype):
    T = np.dtype(dtype).type
    s, dt = SO.s_of(dt, dtype), T(dt)
    _, p = wp(dt, z, v, dtype)
    return ((y + a1 * (T(0.75) * dt)) + b1 * (T(1.5) * p), (y + a1 * (T(0.25) * dt)) + b1 * (T(0.5) * s), (y + a1 * dt) - b1 * s)


def stage2(y, a1, b1, b2, b3, dt, dtype):
    T = np.dtype(dtype).type
    return (y + a1 * (T(0.25) * T(dt))) + ((b1 * T(-5) + b2 * T(3)) + b3 * T(0.5)) * SO.s_of(dt, dtype)


def srk_step(y, a1, a2, b1, b2, b3, b4, dt, z, v, dtype):
    T = np.dtype(dtype).type
    _, third, two3, _, _ = consts(dtype)
    e = weights(dt, z, v, dtype)
    return ((((y + (third * a1 + two3 * a2) * T(dt)) + b1 * e[0]) + b2 * e[1]) + b3 * e[2]) + b4 * e[3]


def stage1_backward(gY2, gG2, gG3, dt, z, v, dtype):
    """(gy, ga1, gb1)."""
    T = np.dtype(dtype).type
    s, dt = SO.s_of(dt, dtype), T(dt)
    _, p = wp(dt, z, v, dtype)
    return ((gY2 + gG2) + gG3, (gY2 * (T(0.75) * dt) + gG2 * (T(0.25) * dt)) + gG3 * dt,
            (gY2 * (T(1.5) * p) + gG2 * (T(0.5) * s)) - gG3 * s)


def stage2_backward(gG4, dt, dtype):
    """(ga1, gb1, gb2, gb3)."""
    T = np.dtype(dtype).type
    s = SO.s_of(dt, dtype)
    return gG4 * (T(0.25) * T(dt)), gG4 * (T(-5) * s), gG4 * (T(3) * s), gG4 * (T(0.5) * s)


def step_backward(gy1, dt, z, v, dtype):
    """(ga1, ga2, gb1, gb2, gb3, gb4)."""
    T = np.dtype(dtype).type
    _, third, two3, _, _ = consts(dtype)
    return (gy1 * (third * T(dt)), gy1 * (two3 * T(dt))) + tuple(gy1 * e for e in weights(dt, z, v, dtype))


def srk_walk(drift, diffusion, y0, grid, seed, dtype, noise=None):
    """The states at every point of ``grid`` (time dtype), step k on the draws of (seed, k) — ``noise(k, draw)``, when given, supplies
    them instead (the GPU's own).  Returns [len(grid), *y0.shape]."""
    tt = grid.dtype.type
    y = np.asarray(y0, dtype=dtype)
    out = [y]
    for k in range(len(grid) - 1):
        t0, t1 = grid[k], grid[k + 1]
        dt = t1 - t0
        z, v = (noise(k, d) if noise is not None else state_normals(y.shape, seed, k, dtype, d) for d in (0, 1))
        t34, t14 = t0 + dt * tt(0.75), t0 + dt * tt(0.25)
        a1, b1 = drift(t0, y), diffusion(t0, y)
        Y2, G2, G3 = stage1(y, a1, b1, dt, z, v, dtype)
        a2, b2, b3 = drift(t34, Y2), diffusion(t14, G2), diffusion(t1, G3)
        b4 = diffusion(t14, stage2(y, a1, b1, b2, b3, dt, dtype))
        y = srk_step(y, a1, a2, b1, b2, b3, b4, dt, z, v, dtype)
        out.append(y)
    return np.stack(out)
