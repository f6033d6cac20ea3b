"""Test-side restatement of sdeint's noise and step (include/xde_hip_sde.h), in numpy, written from the header's mapping and not from
the kernel: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11), the uniform mapping,
Box-Muller in float64, and the Ito Euler-Maruyama walk ``y1 = (y0 + f*dt) + g*(s*Z)`` in the state dtype's op order."""
import os

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)

# (counter, key, output) — Philox4x32-10 known-answer vectors
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key):
    """``counter``: uint [..., 4]; ``key``: two 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & _MASK
            k1 = (k1 + np.uint64(W1)) & _MASK
        p0 = np.uint64(M0) * c0  # (32 x 32 bits: exact in 64)
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(nblk, seed, k):
    """The words of counters j = 0 .. nblk-1 at grid step k: [nblk, 4] uint32."""
    j = np.arange(nblk, dtype=np.uint64)
    ctr = np.stack([j & _MASK, j >> np.uint64(32), np.full_like(j, k), np.zeros_like(j)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(w, dtype):
    """fp32: one uniform per word, [nblk, 4]; fp64: one per word pair (hi:lo = w1:w0, w3:w2), [nblk, 2].  float64, in (0, 1]."""
    w = w.astype(np.uint64)
    if np.dtype(dtype) == np.float32:
        return ((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0**-24
    a = ((w[:, 1] << np.uint64(32)) | w[:, 0]) >> np.uint64(11)
    b = ((w[:, 3] << np.uint64(32)) | w[:, 2]) >> np.uint64(11)
    return np.stack([a + np.uint64(1), b + np.uint64(1)], axis=-1).astype(np.float64) * 2.0**-53


def cos_sin_2pi(u):
    """cos(2 pi u), sin(2 pi u) in float64 for the uniforms u (multiples of 2^-53).  u is first reduced EXACTLY to f = u - q/4, q the
    nearest quarter (|f| <= 1/8), so the rounded angle 2 pi f is off by at most about 2^-53 — forming 2 pi u directly is off by up to
    6 * 2^-53 near u = 1 (the rounding of np.pi included), more than the error bound of the GPU's normals allows for the oracle."""
    u = np.asarray(u, dtype=np.float64)
    q = np.rint(4.0 * u)
    a = 2.0 * np.pi * (u - 0.25 * q)
    c, s = np.cos(a), np.sin(a)
    quad = [(q % 4) == i for i in range(4)]
    return np.select(quad, [c, -s, -c, s]), np.select(quad, [s, c, -s, -c])


def box_muller(u1, u2):
    r = np.sqrt(-2.0 * np.log(u1))
    c, s = cos_sin_2pi(u2)
    return r * c, r * s, r


def normals(n, seed, k, dtype, with_r=False):
    """Z[0 .. n-1] of (seed, k) for a state of ``dtype``, Box-Muller in float64 (not rounded): float64 [n] (and r of each element)."""
    W = 4 if np.dtype(dtype) == np.float32 else 2
    nblk = -(-n // W)
    u = uniforms(words(nblk, seed, k), dtype)
    zs, rs = [], []
    for p in range(W // 2):
        z0, z1, r = box_muller(u[:, 2 * p], u[:, 2 * p + 1])
        zs += [z0, z1]
        rs += [r, r]
    z = np.stack(zs, axis=-1).reshape(-1)[:n]
    return (z, np.stack(rs, axis=-1).reshape(-1)[:n]) if with_r else z


def state_normals(shape, seed, k, dtype):
    """The Z of a state of ``shape`` in its dtype (the float64 Box-Muller rounded once)."""
    return normals(int(np.prod(shape)), seed, k, dtype).astype(dtype).reshape(shape)


def wrap_n(dtype):
    """A size past the step kernels' grid cap (XDE_GRID_BLOCKS, default 2048, at most 4096 workgroups of 256 lanes, W = 4 fp32 or 2 fp64
    elements a lane): every lane of the capped grid runs its loop once, the first workgroup's lanes a second time, and the 3 elements
    left over make the second workgroup's first lane (fp64: first two lanes) wrap too, the last on a ragged tail — a vector body, a
    wrapped second pass and the scalar tail in one launch."""
    cap = min(int(os.environ.get("XDE_GRID_BLOCKS", 2048)), 4096)
    W = 16 // np.dtype(dtype).itemsize
    return cap * 256 * W + 256 * W + 3


def s_of(dt, dtype):
    """s = sqrt(|dt|) in float64 of the time-dtype dt, rounded to the state dtype."""
    return np.dtype(dtype).type(np.sqrt(abs(np.float64(dt))))


def em_step(y, f, g, dt, z, dtype):
    T = np.dtype(dtype).type
    return (y + f * T(dt)) + g * (s_of(dt, dtype) * z)


def em_walk(drift, diffusion, y0, grid, seed, dtype, noise=None):
    """The states at every point of ``grid`` (time dtype), step k on the noise of (seed, k) — ``noise(k)``, when given, supplies Z
    instead (the GPU's own).  Returns [len(grid), *y0.shape]."""
    y = np.asarray(y0, dtype=dtype)
    out = [y]
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        z = noise(k) if noise is not None else state_normals(y.shape, seed, k, dtype)
        y = em_step(y, drift(grid[k], y), diffusion(grid[k], y), dt, z, dtype)
        out.append(y)
    return np.stack(out)


def rows_at(states, grid, t):
    """Output rows at the times ``t`` from the states on ``grid``: the first grid step whose end has reached t[j]; an exact copy at
    either end, else ``y_a + w*(y_b - y_a)`` with ``w = (t - t_a)/(t_b - t_a)`` in the time dtype, rounded to the state dtype."""
    T = states.dtype.type
    d = -1 if grid[-1] < grid[0] else 1
    n = len(grid) - 1
    rows = [states[0]]
    for tj in t[1:]:
        if n == 0:
            rows.append(states[0])
            continue
        k = min(max(int(np.searchsorted(d * grid, d * tj, side="left")) - 1, 0), n - 1)
        ta, tb = grid[k], grid[k + 1]
        if tj == ta:
            rows.append(states[k])
        elif tj == tb:
            rows.append(states[k + 1])
        else:
            w = T((tj - ta) / (tb - ta))
            rows.append(states[k] + w * (states[k + 1] - states[k]))
    return np.stack(rows)


def layout(rows):
    """[T, *lead, L, D] -> the fixed solvers' [*lead, T*L, D]."""
    T = rows.shape[0]
    x = np.moveaxis(rows, 0, -3)  # [*lead, T, L, D]
    return x.reshape(x.shape[:-3] + (T * x.shape[-2], x.shape[-1]))
