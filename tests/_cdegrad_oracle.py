"""ORACLE of the control-gradient entry points (include/xde_hip_cdegrad.h), independent of the double: float64 throughout.  The spline
coefficients, the spline's value and ``X'(t)`` are LINEAR in the data they read, so their exact Jacobians are what comes out when unit
vectors are pushed through the forward oracles — tests/_spline_oracle.py (the dense ``numpy.linalg.solve``, the textbook evaluation)
and tests/_cde_oracle.py (the oracle's own spline classes) — and the gradient is ``J^T g``: no finite differences, no step-size error.

Every function returns the gradient AND the sum of the absolute values of the terms that make up each element (``|J|^T |g|``), the
scale a rounding error is measured against."""
import numpy as np

from . import _cde_oracle as CO
from . import _spline_oracle as SO


def gdx(gout, F):
    """``gdX[b, c] = sum_h gout[b, h] F[b, h, c]`` and ``sum_h |gout F|``."""
    g, f = np.asarray(gout, dtype=np.float64), np.asarray(F, dtype=np.float64)
    return np.einsum("bh,bhc->bc", g, f), np.einsum("bh,bhc->bc", np.abs(g), np.abs(f))


def der_rows(knots, t, method):
    """``w[k] = d X'(t) / d series[k]`` of the linear / cubic control (the same for every column): the oracle's spline through the
    unit series."""
    Tn = len(knots)
    unit = np.eye(Tn)[None]  # [1, Tn, Tn]: column k is the unit vector e_k
    return np.asarray(CO.dX(unit, np.asarray(knots, dtype=np.float64), t, method, np.float64), dtype=np.float64)[0]


def natural_rows(knots, tq):
    """``(dval/dY, dval/dM, dder/dY, dder/dM) [L, Tn]`` of the path (Y, M) on the knot grid: the textbook evaluation of
    tests/_spline_oracle.py with every knot a node, through unit vectors."""
    k64 = np.asarray(knots, dtype=np.float64)
    Tn = len(k64)
    tq = np.asarray(tq, dtype=np.float64).reshape(-1)
    out = [np.empty((len(tq), Tn)) for _ in range(4)]
    zero = np.zeros(Tn)
    for k in range(Tn):
        e = np.zeros(Tn)
        e[k] = 1.0
        out[0][:, k], out[2][:, k], _ = SO.evaluate(k64, e, zero, tq)
        out[1][:, k], out[3][:, k], _ = SO.evaluate(k64, zero, e, tq)
    return out


def control_grad(gout, F, knots, t, method):
    """(a) for the linear / cubic control: ``gSeries [B, Tn, C]`` and its scale."""
    g, a = gdx(gout, F)
    w = der_rows(knots, t, method)
    return w[None, :, None] * g[:, None, :], np.abs(w)[None, :, None] * a[:, None, :]


def control_grad_natural(gout, F, knots, t):
    """(a) for the natural control: ``gY, gM [B, Tn, C]`` and their scales."""
    g, a = gdx(gout, F)
    _, _, wy, wm = natural_rows(knots, [t])
    return (wy[0][None, :, None] * g[:, None, :], wm[0][None, :, None] * g[:, None, :],
            np.abs(wy[0])[None, :, None] * a[:, None, :], np.abs(wm[0])[None, :, None] * a[:, None, :])


def gather_backward(gval, gder, knots, tq):
    """(c): ``gY, gM [outer, Tn, D]`` from ``gval`` / ``gder [outer, L, D]`` (either may be None), and their scales."""
    vy, vm, dy, dm = natural_rows(knots, tq)
    outs = []
    for absolute in (False, True):
        f = np.abs if absolute else (lambda x: x)
        gY = gM = 0.0
        for g, jy, jm in ((gval, vy, vm), (gder, dy, dm)):
            if g is not None:
                g = np.asarray(g, dtype=np.float64)
                gY = gY + np.einsum("lk,old->okd", f(jy), f(g))
                gM = gM + np.einsum("lk,old->okd", f(jm), f(g))
        outs += [gY, gM]
    return tuple(outs)


def coeffs_jacobian(column, knots):
    """``(JY, JM) [Tn, Tn]``: ``d Y_j / d y_k`` and ``d M_j / d y_k`` of one column (NaN = not observed; the columns k of an unobserved
    entry are zero): the dense-solve oracle evaluated on the knot grid, through the unit series with the column's NaN pattern."""
    column = np.asarray(column, dtype=np.float64)
    k64 = np.asarray(knots, dtype=np.float64)
    Tn = len(column)
    obs = np.flatnonzero(~np.isnan(column))
    unit = np.where(np.isnan(column)[:, None], np.nan, 0.0) * np.ones((1, len(obs)))  # [Tn, nobs]
    unit[obs, np.arange(len(obs))] = 1.0
    val, _, M = SO.spline(unit[None], k64, k64)  # val at the knots is Y on the knot grid
    JY, JM = np.zeros((Tn, Tn)), np.zeros((Tn, Tn))
    JY[:, obs], JM[:, obs] = val[0], M[0]
    return JY, JM


def coeffs_backward(gY, gM, series, knots):
    """(b): ``gSeries [B, Tn, C]`` and its scale."""
    gY, gM = np.asarray(gY, dtype=np.float64), np.asarray(gM, dtype=np.float64)
    B, Tn, C = series.shape
    out, scale = np.zeros((B, Tn, C)), np.zeros((B, Tn, C))
    cache = {}
    for b in range(B):
        for c in range(C):
            key = tuple(np.isnan(series[b, :, c]))
            if key not in cache:
                cache[key] = coeffs_jacobian(series[b, :, c], knots)
            JY, JM = cache[key]
            out[b, :, c] = JY.T @ gY[b, :, c] + JM.T @ gM[b, :, c]
            scale[b, :, c] = np.abs(JY).T @ np.abs(gY[b, :, c]) + np.abs(JM).T @ np.abs(gM[b, :, c])
    return out, scale
