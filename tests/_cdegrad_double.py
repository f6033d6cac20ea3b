"""TEST DOUBLE of the control-gradient entry points (include/xde_hip_cdegrad.h) in numpy, written from the header's op statements: the
spline double plus ``_cde_control_grad``, ``_cde_control_grad_natural``, ``_cde_control_grad_plan``,
``_spline_natural_coeffs_backward`` and ``_spline_natural_gather_backward``.

Every op is an element-wise numpy op in the series dtype (IEEE, rounded op by op).  What depends on the time and the knots alone — the
(row, weight) entries, the Thomas coefficients — is scalar arithmetic on numpy scalars of that dtype; the columns of a launch are worked
side by side.  The coefficient transpose branches on a column's NaN pattern only, so it runs once per distinct pattern."""
import numpy as np
import torch

from ._cpu_double import _NP, _np
from ._spline_double import SplineDoubleBackend

GRID_CAP = 2048  # the library's default grid cap (XDE_GRID_BLOCKS)


def partials(H):
    """P of the header: min(32, the least power of two >= H)."""
    P = 1
    while P < min(H, 32):
        P *= 2
    return P


def gdx_in_header_order(gout, F):
    """``gdX[b, c] = sum_h gout[b, h] * F[b, h, c]`` for numpy ``gout [B, H]``, ``F [B, H, C]`` of one dtype, in the header's order."""
    T = F.dtype.type
    B, H, C = F.shape
    P = partials(H)
    v = np.zeros((B, P, C), dtype=T)
    for h in range(H):  # (ascending h visits every partial's rows in that partial's order)
        v[:, h % P, :] = v[:, h % P, :] + gout[:, h, None] * F[:, h, :]
    off = P // 2
    while off:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off //= 2
    return v[:, 0, :]


def _tau(t, T):
    if torch.is_tensor(t):
        assert t.numel() == 1 and t.dtype in (torch.float32, torch.float64), "t: one float32 / float64 element"
        t = _np(t).reshape(-1)[0]
    return np.asarray([t]).astype(T)[0]  # (the time in the series dtype first)


def linear_entries(knots, tau):
    T = knots.dtype.type
    Tn = len(knots)
    i = int(np.clip(np.searchsorted(knots, tau, side="left") - 1, 0, Tn - 1))  # #{t_k < tau} - 1
    scale1 = lambda j: knots[min(j, Tn - 2) + 1] - knots[min(j, Tn - 2)]  # noqa: E731
    return [(i, T(-1) / scale1(i)), (min(i + 1, Tn - 1), T(1) / scale1(max(i - 1, 0)))]


def cubic_entries(knots, tau):
    T = knots.dtype.type
    Tn = len(knots)
    i = int(np.clip(np.searchsorted(knots, tau, side="left") - 1, 0, Tn - 1))
    h = lambda j: knots[min(j, Tn - 2) + 1] - knots[min(j, Tn - 2)]  # noqa: E731
    h1, h2, ha, hb = h(i), h(0) if i == 0 else h(i - 1), h(i), h(i + 1)
    sx = (tau - knots[i]) / h1
    s2 = sx * sx
    g0 = T(6) * s2 - T(6) * sx
    g1 = T(-6) * s2 + T(6) * sx
    g2 = (T(3) * s2 - T(4) * sx) + T(1)
    g3 = T(3) * s2 - T(2) * sx
    a0, a1, b0, b1 = g0 / h1, g1 / h2, g2 / ha, g3 / hb
    i1 = min(i + 1, Tn - 1)
    if i <= Tn - 3:
        return [(i, a0), (i1, a1), (i1, b0), (i, -b0), (i + 2, b1), (i1, -b1)]
    if i == Tn - 2:
        return [(i, a0), (i1, a1), (i1, b0), (i, -b0), (i1, b1), (i, -b1)]
    return [(i, a0), (i1, a1), (i, b0), (Tn - 2, -b0), (i, b1), (Tn - 2, -b1)]


def natural_ihs(knots, tau):
    """(i, h, s) of xde_hip_spline.h EVALUATION."""
    Tn = len(knots)
    i = int(np.clip(np.searchsorted(knots, tau, side="right") - 1, 0, Tn - 2))  # #{t_k <= tau} - 1
    return i, knots[i + 1] - knots[i], tau - knots[i]


def der_weights(T, h, s):
    """d der / d (Y_i, Y_{i+1}, M_i, M_{i+1})."""
    rh = T(1) / h
    q = (s * s) / (T(2) * h)
    return -rh, rh, (s - h / T(3)) - q, q - h / T(6)


def val_weights(T, h, s):
    """d val / d (Y_a, Y_b, M_a, M_b): l, r, wa, wb of the header's FOLD."""
    r = s / h
    s2 = s * s
    s3 = s2 * s
    return T(1) - r, r, (-(s * h) / T(3) + s2 / T(2)) - s3 / (T(6) * h), -(s * h) / T(6) + s3 / (T(6) * h)


def scatter(entries, gdx, Tn):
    """PHASE 2: ``out[b, k, c]`` = +0, plus ``w_j * gdX[b, c]`` for the entries of row k in ascending j."""
    B, C = gdx.shape
    out = np.zeros((B, Tn, C), dtype=gdx.dtype)
    for row, w in entries:
        out[:, row, :] = out[:, row, :] + w * gdx
    return out


def control_grad(gout, F, knots, tau, method):
    with np.errstate(all="ignore"):
        gdx = gdx_in_header_order(gout, F)
        return scatter({"linear": linear_entries, "cubic": cubic_entries}[method](knots, tau), gdx, len(knots))


def control_grad_natural(gout, F, knots, tau):
    T = knots.dtype.type
    with np.errstate(all="ignore"):
        gdx = gdx_in_header_order(gout, F)
        i, h, s = natural_ihs(knots, tau)
        y0, y1, m0, m1 = der_weights(T, h, s)
        return scatter([(i, y0), (i + 1, y1)], gdx, len(knots)), scatter([(i, m0), (i + 1, m1)], gdx, len(knots))


def _coeffs_backward_pattern(obs, gy, gm, t):
    """(b) for the columns that share the NaN pattern ``obs [Tn]``: ``gy, gm [Tn, n]`` -> ``gSeries [Tn, n]``."""
    T = t.dtype.type
    Tn = len(t)
    out = np.zeros_like(gy)
    if not obs.any():
        return out
    nodes = sorted({0, Tn - 1} | set(np.flatnonzero(obs).tolist()))
    GY = {n: gy[n].copy() for n in nodes}
    GM = {n: gm[n].copy() for n in nodes}
    for a, b in zip(nodes[:-1], nodes[1:]):  # FOLD
        h = t[b] - t[a]
        for j in range(a + 1, b):
            l, r, wa, wb = val_weights(T, h, t[j] - t[a])
            GY[a] = GY[a] + l * gy[j]
            GY[b] = GY[b] + r * gy[j]
            GM[a] = (GM[a] + wa * gy[j]) + l * gm[j]
            GM[b] = (GM[b] + wb * gy[j]) + r * gm[j]
    zero = np.zeros_like(gy[0])
    cp, dl = {nodes[0]: T(0)}, {nodes[0]: zero}
    for a, i, b in zip(nodes[:-2], nodes[1:-1], nodes[2:]):  # SOLVE, ascending
        hl, hr = t[i] - t[a], t[b] - t[i]
        den = T(2) * (hl + hr) - hl * cp[a]
        cp[i] = hr / den
        dl[i] = (GM[i] - hl * dl[a]) / den
    lam = {nodes[0]: zero, nodes[-1]: zero}
    for i, b in zip(nodes[-2:0:-1], nodes[:1:-1]):  # descending: (i, the node above it)
        lam[i] = dl[i] - cp[i] * lam[b]
    u = {(p, q): (T(6) * (lam[p] - lam[q])) / (t[q] - t[p]) for p, q in zip(nodes[:-1], nodes[1:])}  # RIGHT-HAND SIDE
    G = {}
    for k, n in enumerate(nodes):
        g = GY[n]
        if k > 0:
            g = g + u[(nodes[k - 1], n)]
        if k + 1 < len(nodes):
            g = g - u[(n, nodes[k + 1])]
        G[n] = g
    for n in nodes:  # END RULE
        if obs[n]:
            out[n] = G[n]
    seen = np.flatnonzero(obs)
    if not obs[0]:
        out[seen[0]] = out[seen[0]] + G[0]
    if not obs[Tn - 1]:
        out[seen[-1]] = out[seen[-1]] + G[Tn - 1]
    return out


def natural_coeffs_backward(gY, gM, series, knots):
    """``gSeries [B, Tn, C]`` of numpy ``gY, gM, series [B, Tn, C]`` over ``knots [Tn]`` (one dtype), in the header's order."""
    B, Tn, C = series.shape
    cols = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(Tn, B * C)  # noqa: E731
    y, gy, gm = cols(series), cols(gY), cols(gM)
    obs = ~np.isnan(y)
    out = np.zeros_like(gy)
    patterns, which = np.unique(obs.T, axis=0, return_inverse=True)
    which = which.reshape(-1)
    with np.errstate(all="ignore"):
        for p, pattern in enumerate(patterns):
            sel = which == p
            out[:, sel] = _coeffs_backward_pattern(pattern, gy[:, sel], gm[:, sel], knots)
    return np.ascontiguousarray(out.reshape(Tn, B, C).transpose(1, 0, 2))


def natural_gather_backward(gval, gder, knots, tq, Tn):
    """``gY, gM [outer, Tn, D]`` from numpy ``gval`` / ``gder [outer, L, D]`` (either may be None) at ``tq [L]``, in the header's order."""
    g = gval if gval is not None else gder
    T = g.dtype.type
    outer, L, D = g.shape
    gY, gM = np.zeros((outer, Tn, D), dtype=T), np.zeros((outer, Tn, D), dtype=T)
    with np.errstate(all="ignore"):
        for l in range(L):
            i, h, s = natural_ihs(knots, tq[l])
            wv, wd = val_weights(T, h, s), der_weights(T, h, s)
            for x, row in enumerate((i, i + 1)):
                if gval is not None:
                    gY[:, row] = gY[:, row] + wv[x] * gval[:, l]
                    gM[:, row] = gM[:, row] + wv[2 + x] * gval[:, l]
                if gder is not None:
                    gY[:, row] = gY[:, row] + wd[x] * gder[:, l]
                    gM[:, row] = gM[:, row] + wd[2 + x] * gder[:, l]
    return gY, gM


class CdeGradDoubleBackend(SplineDoubleBackend):
    name = SplineDoubleBackend.name.replace("(test)", "+cdegrad(test)")

    def _grad_operands(self, outs, gout, F, knots):
        assert F.dim() == 3 and F.is_contiguous() and gout.is_contiguous() and gout.shape == F.shape[:2]
        for o in outs:
            assert o.is_contiguous() and o.shape == (F.shape[0], knots.shape[0], F.shape[2]) and o.dtype == F.dtype
        assert knots.shape[0] >= 2 and F.dtype == gout.dtype == knots.dtype

    def _cde_control_grad(self, gSeries, gout, F, knots, t, method):
        self.launches.append("cde_control_grad")
        assert method in ("linear", "cubic"), "XDE_HISTORY_BEZIER is refused"
        self._grad_operands((gSeries,), gout, F, knots)
        _np(gSeries)[...] = control_grad(_np(gout), _np(F), _np(knots), _tau(t, _NP[F.dtype]), method)

    def _cde_control_grad_natural(self, gY, gM, gout, F, knots, t):
        self.launches.append("cde_control_grad_natural")
        self._grad_operands((gY, gM), gout, F, knots)
        y, m = control_grad_natural(_np(gout), _np(F), _np(knots), _tau(t, _NP[F.dtype]))
        _np(gY)[...] = y
        _np(gM)[...] = m

    def _cde_control_grad_plan(self, F, B, H, channels):
        W = 4 if F.dtype == torch.float32 else 2
        P = partials(H)
        NV = -(-channels // W)
        CL = 256 // P
        blocks = min(B, GRID_CAP)
        return {"vec": int(channels % W == 0 and F.data_ptr() % 16 == 0), "P": P, "CL": CL, "chunks": -(-NV // CL), "rows": -(-H // P),
                "strided": int(B > blocks), "blocks": blocks}

    def _spline_natural_coeffs_backward(self, gSeries, gY, gM, series, knots):
        self.launches.append("spline_natural_coeffs_backward")
        assert series.dim() == 3 and all(x.is_contiguous() for x in (gSeries, gY, gM, series))
        assert gSeries.shape == gY.shape == gM.shape == series.shape and gSeries.dtype == gY.dtype == gM.dtype == series.dtype == knots.dtype
        _np(gSeries)[...] = natural_coeffs_backward(_np(gY), _np(gM), _np(series), _np(knots))

    def _spline_natural_gather_backward(self, gY, gM, gval, gder, knots, tq):
        self.launches.append("spline_natural_gather_backward")
        assert gval is not None or gder is not None
        if gY.numel() == 0:
            return
        Tn, D = gY.shape[-2:]
        flat = lambda g: None if g is None else _np(g).reshape(-1, tq.numel(), D)  # noqa: E731
        y, m = natural_gather_backward(flat(gval), flat(gder), _np(knots), _np(tq).reshape(-1), Tn)
        _np(gY)[...] = y.reshape(gY.shape)
        _np(gM)[...] = m.reshape(gM.shape)
