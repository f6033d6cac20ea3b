"""include/xde_hip_logsig.h restated in numpy, forward and backward, in the written op order: every subtraction of points rounded in the
state dtype ``T``, every product and sum in float64, the sums sequential (over k in the forward, over j in the backward), one
rounding to ``T`` at the end.  ``x`` is ``[B, T, C]``; the windows are ``[B, W, K]``."""
import numpy as np


def channels(C, depth):
    return C if depth == 1 else C + C * (C - 1) // 2


def pair(C, i, j):
    return C + i * (2 * C - i - 1) // 2 + (j - i - 1)


def n_windows(Tn, L):
    return -(-(Tn - 1) // L)


def spans(Tn, L):
    """(t0, n) of every window: the points t0 .. t0 + n."""
    return [(t0, min(L, Tn - 1 - t0)) for t0 in range(0, Tn - 1, L)]


def windows(x, L, depth):
    T = x.dtype.type
    B, Tn, C = x.shape
    iu, ju = np.triu_indices(C, 1)  # (lexicographic: pair(C, i, j) - C is their position)
    out = np.empty((B, n_windows(Tn, L), channels(C, depth)), dtype=T)
    for w, (t0, n) in enumerate(spans(Tn, L)):
        p = x[:, t0 : t0 + n + 1]
        out[:, w, :C] = p[:, n] - p[:, 0]
        if depth == 1:
            continue
        acc = np.zeros((B, C, C), dtype=np.float64)
        for k in range(1, n):
            u = (p[:, k] - p[:, 0]).astype(np.float64)
            d = (p[:, k + 1] - p[:, k]).astype(np.float64)
            acc = acc + (u[:, :, None] * d[:, None, :] - u[:, None, :] * d[:, :, None])
        out[:, w, C:] = (0.5 * acc)[:, iu, ju].astype(T)
    return out


def backward(gout, x, L, depth):
    T = x.dtype.type
    B, Tn, C = x.shape
    iu, ju = np.triu_indices(C, 1)
    total = [None] * Tn  # per point: the contributions of its windows, the earlier window first
    for w, (t0, n) in enumerate(spans(Tn, L)):
        g = gout[:, w]
        G = np.zeros((B, C, C), dtype=T)
        if depth == 2:
            G[:, iu, ju] = g[:, C:]
            G[:, ju, iu] = -g[:, C:]
        g1 = g[:, :C].astype(np.float64)
        p = x[:, t0 : t0 + n + 1]
        for m in range(n + 1):
            d = (p[:, m + 1 if m < n else 0] - p[:, m - 1 if m > 0 else n]).astype(np.float64)
            s = np.zeros((B, C), dtype=np.float64)
            for j in range(C if depth == 2 else 0):
                keep = np.arange(C) != j
                s[:, keep] = s[:, keep] + G[:, keep, j].astype(np.float64) * d[:, j, None]
            q = 0.5 * s
            if m == n:
                q = q + g1
            if m == 0:
                q = q - g1
            total[t0 + m] = q if total[t0 + m] is None else total[t0 + m] + q
    return np.stack(total, axis=1).astype(T)
