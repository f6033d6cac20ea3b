"""ORACLE of the natural cubic spline (include/xde_hip_spline.h), independent of the double: float64 throughout, the second derivatives
from a dense ``numpy.linalg.solve`` of the textbook tridiagonal system through each column's nodes (the observed points, plus the first
and the last knot by the header's end rule), and the textbook evaluation on the node intervals

    S(x) = M_a (x_b - x)^3 / (6 h) + M_b (x - x_a)^3 / (6 h) + (y_a / h - M_a h / 6) (x_b - x) + (y_b / h - M_b h / 6) (x - x_a).

Nothing here knows the dense Y / M arrays of the kernels: a missing row is simply not a node.
"""
import numpy as np


def nodes(column, knots):
    """(x, y) of the nodes of one column (1-d, NaN = not observed) by the end rule; None when nothing is observed."""
    column = np.asarray(column, dtype=np.float64)
    obs = ~np.isnan(column)
    if not obs.any():
        return None
    y = column.copy()
    if not obs[0]:
        y[0] = column[obs][0]
    if not obs[-1]:
        y[-1] = column[obs][-1]
    keep = ~np.isnan(y)
    return np.asarray(knots, dtype=np.float64)[keep], y[keep]


def second_derivatives(x, y):
    """M at the nodes: natural ends, the dense solve of  h_l M_a + 2 (h_l + h_r) M_i + h_r M_b = 6 (s_r - s_l)."""
    n = len(x)
    A, r = np.zeros((n, n)), np.zeros(n)
    A[0, 0] = A[-1, -1] = 1.0
    for i in range(1, n - 1):
        hl, hr = x[i] - x[i - 1], x[i + 1] - x[i]
        A[i, i - 1], A[i, i], A[i, i + 1] = hl, 2.0 * (hl + hr), hr
        r[i] = 6.0 * ((y[i + 1] - y[i]) / hr - (y[i] - y[i - 1]) / hl)
    return np.linalg.solve(A, r)


def evaluate(x, y, M, tq):
    """(value, derivative, second derivative) of the spline through the nodes at the times ``tq`` (the end intervals are continued
    outside the nodes)."""
    tq = np.asarray(tq, dtype=np.float64)
    a = np.clip(np.searchsorted(x, tq, side="right") - 1, 0, len(x) - 2)
    b = a + 1
    h = x[b] - x[a]
    p, q = x[b] - tq, tq - x[a]
    ca, cb = y[a] / h - M[a] * h / 6.0, y[b] / h - M[b] * h / 6.0
    val = M[a] * p**3 / (6.0 * h) + M[b] * q**3 / (6.0 * h) + ca * p + cb * q
    der = -M[a] * p**2 / (2.0 * h) + M[b] * q**2 / (2.0 * h) - ca + cb
    return val, der, (M[a] * p + M[b] * q) / h


def spline(series, knots, tq):
    """``val, der [B, L, C]`` at ``tq [L]`` and the second derivative on the knot grid ``M [B, Tn, C]`` of ``series [B, Tn, C]``."""
    B, Tn, C = series.shape
    tq = np.asarray(tq, dtype=np.float64)
    val, der, M = np.empty((B, len(tq), C)), np.empty((B, len(tq), C)), np.empty((B, Tn, C))
    for b in range(B):
        for c in range(C):
            x, y = nodes(series[b, :, c], knots)
            m = second_derivatives(x, y)
            val[b, :, c], der[b, :, c], _ = evaluate(x, y, m, tq)
            M[b, :, c] = evaluate(x, y, m, knots)[2]
    return val, der, M
