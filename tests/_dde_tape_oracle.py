"""include/xde_hip_dde.h and the walk of ``ddeint_steps`` restated in numpy: the Hermite weights (float64, the header's formulas), the
gather and its cotangent in the written op order (weights rounded to the state dtype ``T``, every product and sum in ``T``), the
interval rule as a plain scan over the complete intervals, the history's forward-difference derivative, and the walk — the oracle's
own fixed-step stages (``oracle.xde_oracle.FixedSolver`` driven over a grid by tests/_substep_oracle.py) around a ``func`` that is
handed the delayed states of its stage."""
import numpy as np

from oracle import xde_oracle as O

from . import _substep_oracle as SS

STAGES = {"euler": (0.0,), "midpoint": (0.0, 0.5), "rk4": (0.0, 1 / 3, 2 / 3, 1.0), "rk4_classic": (0.0, 0.5, 0.5, 1.0)}


def weights(sigma, h):
    """((a0, a1, a2, a3), (b0, b1, b2, b3)) in float64."""
    sigma, h = np.float64(sigma), np.float64(h)
    s2 = sigma * sigma
    s3 = s2 * sigma
    a0 = 2 * s3 - 3 * s2 + 1
    a1 = h * (s3 - 2 * s2 + sigma)
    a2 = -2 * s3 + 3 * s2
    a3 = h * (s3 - s2)
    b0 = -(6 * s2 - 6 * sigma) / h
    b1 = -(3 * s2 - 4 * sigma + 1)
    b2 = -b0
    b3 = -(3 * s2 - 2 * sigma)
    return (float(a0), float(a1), float(a2), float(a3)), (float(b0), float(b1), float(b2), float(b3))


def combine(ya, fa, yb, fb, c, T):
    """(ya c0 + fa c1) + (yb c2 + fb c3) with the four weights rounded to T."""
    c0, c1, c2, c3 = (T(x) for x in c)
    return (ya * c0 + fa * c1) + (yb * c2 + fb * c3)


def gather(srcs, w, wd, T):
    """srcs: 4 L arrays [rows, D]; w, wd: 4 L floats (wd None: no dtau).  Returns (out, dtau) as [rows, L, D]."""
    L = len(srcs) // 4
    out = np.stack([combine(*srcs[4 * j : 4 * j + 4], w[4 * j : 4 * j + 4], T) for j in range(L)], axis=1)
    dtau = None if wd is None else np.stack([combine(*srcs[4 * j : 4 * j + 4], wd[4 * j : 4 * j + 4], T) for j in range(L)], axis=1)
    assert out.dtype == T
    return out, dtau


def gather_backward(g, terms, j0, T):
    """g [rows, Ltot, D]; terms: per output a list of (lag, weight).  The first product starts the sum, the rest are added in order."""
    outs = []
    for ts in terms:
        acc = None
        for lag, wt in ts:
            p = g[:, j0 + lag, :] * T(wt)
            acc = p if acc is None else acc + p
        outs.append(acc)
    return outs


def history_derivative(his, his_t, T):
    """The forward difference of the samples ([..., Th, D]) over their times, the last node repeating the one before, in T."""
    t = np.asarray(his_t, dtype=np.float64).astype(T)
    d = (his[..., 1:, :] - his[..., :-1, :]) / (t[1:] - t[:-1])[:, None]
    return np.concatenate([d, d[..., -1:, :]], axis=-2).astype(T)


def pick(theta, his_t, grid, k, stage):
    """The last complete interval whose left end is <= theta: ("his" | "tape", index, a, b), or None.  Complete: every interval of the
    history; of the tape, [grid[m], grid[m + 1]] once f_{m + 1} is known — f_k is known from the second stage of step k on."""
    known_f = k - 1 if stage == 0 else k  # the newest tape node whose derivative is known
    cands = [("his", i, float(his_t[i]), float(his_t[i + 1])) for i in range(len(his_t) - 1)]
    cands += [("tape", m, float(grid[m]), float(grid[m + 1])) for m in range(0, known_f)]
    best = None
    for c in cands:
        if c[2] <= theta:
            best = c
    return best


def stage_time(grid, k, c):
    a, b = np.float64(grid[k]), np.float64(grid[k + 1])
    return float(a) if c == 0 else (float(b) if c == 1 else float(a + (b - a) * np.float64(c)))


def delayed(s, lags, his, hf, his_t, grid, tape_y, tape_f, k, stage, T, with_dtau=False):
    """y_lags [..., L, D] of the stage at host time s (and dtau): his / hf are [..., Th, D], tape_y / tape_f lists of [..., 1, D]."""
    his_t = np.asarray(his_t, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float64)
    vals, ders = [], []
    for tau in np.asarray(lags, dtype=np.float64):
        theta = s - float(tau)
        kind, m, a, b = pick(theta, his_t, grid, k, stage)
        sigma = (theta - a) / (b - a)
        assert 0.0 <= sigma <= 1.0, (theta, a, b)
        wa, wb = weights(sigma, b - a)
        if kind == "his":
            ops = (his[..., m : m + 1, :], hf[..., m : m + 1, :], his[..., m + 1 : m + 2, :], hf[..., m + 1 : m + 2, :])
        else:
            ops = (tape_y[m], tape_f[m], tape_y[m + 1], tape_f[m + 1])
        vals.append(combine(*ops, wa, T))
        ders.append(combine(*ops, wb, T))
    out = np.concatenate(vals, axis=-2)
    return (out, np.concatenate(ders, axis=-2)) if with_dtau else out


def walk(func, his, his_t, t, lags, method, T, grid=None, hf=None):
    """The solution at the output times t ([..., len(t), D]) of y' = func(t, y, y_lags) from the history his [..., Th, D] at his_t, over
    grid (None: t itself), every time in T."""
    t = np.asarray(t, dtype=T)
    grid = t if grid is None else np.asarray(grid, dtype=T)
    hf = history_derivative(his, his_t, T) if hf is None else hf
    stages = STAGES[method]
    tape_y, tape_f, n = [], [], [0]

    def f(t0, y):
        k, i = divmod(n[0], len(stages))
        n[0] += 1
        if i == 0:
            tape_y.append(y)
        y_lags = delayed(stage_time(grid, k, stages[i]), lags, his, hf, his_t, grid, tape_y, tape_f, k, i, T)
        out = np.asarray(func(t0, y, y_lags), dtype=T)
        if i == 0:
            tape_f.append(out)
        return out

    solver = O.FixedSolver(f, np.ascontiguousarray(his[..., -1:, :]), method=method, rtol=1e-7, atol=1e-9, norm=O._rms_norm, interp="linear")
    return SS.walk(solver, t, grid, "linear")
