"""The walk the reference meant for ``step_size`` / ``grid_constructor`` (paddlexde/solver/base_fixed_solver.py:103-144 with the
commented-out ``while`` at :130; torchdiffeq's rule), test-side: the oracle's ``FixedSolver.step`` / ``DDEFixedSolver.step`` driven over
a grid, the output rows from the oracle's ``linear_interp`` and ``cubic_hermite_interp``.  ``oracle/`` itself still refuses the options
(SURVEY D7)."""
import math

import numpy as np

from oracle import xde_oracle as O


def grid_from_step_size(t, h):
    """A numpy restatement of the grid formula (time dtype of ``t``), with the strictly-monotone deviation: interior points that are
    not strictly before t[-1] in the span's direction are dropped."""
    tt = t.dtype.type
    d = -1.0 if t[-1] < t[0] else 1.0
    step = tt(d) * tt(h)
    niters = int(math.ceil(float((t[-1] - t[0]) / step + tt(1))))
    g = np.arange(0, niters, dtype=tt) * step + t[0]
    g[-1] = t[-1]
    interior = [x for x in g[1:-1] if (x < t[-1] if d > 0 else x > t[-1])]
    return np.array([g[0]] + interior + ([g[-1]] if niters > 1 else []), dtype=tt)


def walk(solver, t, grid, interp):
    """Integrate ``solver`` (an oracle FixedSolver, constructed without the options) over ``grid``; rows at the output times ``t``."""
    d = -1 if grid[-1] < grid[0] else 1
    y0 = solver.y0
    sol = [y0]
    j = 1
    for k in range(1, len(grid)):
        t0, t1 = grid[k - 1 : k], grid[k : k + 1]
        y1, dy0 = solver.step(t0, t1, y0)
        produced = []
        while j < len(t) and d * (t[j] - t1[0]) <= 0:
            produced.append(j)
            j += 1
        dy1 = None
        if produced and interp == "cubic":
            _, dy1 = solver.step(t1, t1, y1)
        for jj in produced:
            tj = t[jj : jj + 1]
            if tj[0] == t0[0]:
                sol.append(y0)
            elif tj[0] == t1[0]:
                sol.append(y1)
            elif interp == "linear":
                sol.append(O.linear_interp(t0, t1, y0, y1, tj))
            elif interp == "cubic":
                sol.append(O.cubic_hermite_interp(t0, y0, dy0, t1, y1, dy1, tj))
            else:
                raise ValueError("off-grid output with interp={!r}".format(interp))
        y0 = y1
    assert j == len(t) or len(grid) == 1
    while len(sol) < len(t):  # (a one-point grid: every output is the start)
        sol.append(solver.y0)
    return np.concatenate(sol, axis=-2)


def odeint(func, y0, t, method, grid, interp="linear"):
    s = O.FixedSolver(func, np.asarray(y0), method=method, rtol=1e-7, atol=1e-9, norm=O._rms_norm, interp=interp)
    return walk(s, t, grid, interp), s.nfe


def ddeint(func, y0, t, y_lags, method, grid, interp="linear"):
    s = O.DDEFixedSolver(func, np.asarray(y0), np.asarray(y_lags), method=method, rtol=1e-7, atol=1e-9, norm=O._rms_norm, interp=interp)
    return walk(s, t, grid, interp), s.nfe
