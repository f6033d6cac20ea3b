"""Inputs shared by tests/test_spline_host.py and tests/test_gpu_spline.py: irregular knots, the patterns of missing values, and series
whose neighbouring columns carry different patterns (so neighbouring lanes of the coefficient kernel branch differently)."""
import numpy as np

TNS = (2, 3, 4, 9, 33)
PATTERNS = ("none", "one interior", "a run of three", "leading", "trailing", "a single observed value", "exactly two observed")


def knots(rs, Tn, T):
    """Strictly increasing knots with spacings in [0.25, 4]; with three or more knots both ends of that range occur (ratio 16)."""
    h = 0.25 * 16.0 ** rs.rand(Tn - 1)
    if Tn >= 3:
        h[0], h[-1] = 4.0, 0.25
    return np.concatenate([[0.0], np.cumsum(h)]).astype(T)


def missing(pattern, Tn):
    """The time rows that ``pattern`` leaves unobserved, or None where ``Tn`` rows cannot carry it."""
    m = Tn // 2
    rows = {"none": [],
            "one interior": [m] if Tn >= 3 else None,
            "a run of three": [m - 1, m, m + 1] if Tn >= 5 else None,
            "leading": [0, 1] if Tn >= 4 else ([0] if Tn >= 2 else None),
            "trailing": [Tn - 2, Tn - 1] if Tn >= 4 else [Tn - 1],
            "a single observed value": [k for k in range(Tn) if k != m],
            "exactly two observed": list(range(1, Tn - 1)) if Tn >= 3 else None}[pattern]
    return rows


def series(rs, B, Tn, C, T, patterns=PATTERNS):
    """A random-walk series [B, Tn, C] in which column e = b C + c carries the (e mod n)-th of the ``patterns`` that fit ``Tn``."""
    x = np.cumsum(0.5 * rs.randn(B, Tn, C), axis=1).astype(T)
    fit = [missing(p, Tn) for p in patterns if missing(p, Tn) is not None]
    for b in range(B):
        for c in range(C):
            x[b, fit[(b * C + c) % len(fit)], c] = np.nan
    return x


def cde_problem(dtype, channels=None, share=0.2, seed=4):
    """tests/_cde_cases.py's inputs (series [B, T, C], a [H, C], z0 [B, H]) as numpy, on irregular knots with ``share`` of the
    interior entries missing; ``channels`` keeps the first so many channels."""
    from ._cde_cases import B, C, T, inputs

    x, a, z0 = inputs(dtype)
    rs = np.random.RandomState(seed)
    kn = knots(rs, T, x.dtype.type)
    x = x.copy()
    x[:, 1:-1][rs.rand(B, T - 2, C) < share] = np.nan
    if channels is not None:
        x, a = np.ascontiguousarray(x[:, :, :channels]), np.ascontiguousarray(a[:, :channels])
    return x, kn, a, z0
