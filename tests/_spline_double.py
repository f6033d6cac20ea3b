"""TEST DOUBLE of the natural cubic spline's entry points (include/xde_hip_spline.h) in numpy, in the header's op order: the cdeint
double plus ``_spline_natural_coeffs``, ``_spline_natural_gather``, ``_cde_contract_natural`` and ``_cde_contract_natural_backward``.

Every op is an element-wise numpy op in the series dtype (IEEE, rounded op by op, as the kernels are built with -ffp-contract=off);
the columns of a launch are worked side by side with masks where the kernel's lanes branch, so the sweeps run over the time rows only.
"""
import numpy as np
import torch

from ._cde_double import CdeDoubleBackend, contract_in_header_order
from ._cpu_double import _NP, _np


def natural_eval(T, h, s, Y0, Y1, M0, M1):
    """``val, der`` of the header's EVALUATION for a step ``s`` into an interval of length ``h`` (arrays of dtype ``T``)."""
    h6, s2, s6 = h / T(6), s / T(2), s / T(6)
    sl = (Y1 - Y0) / h
    d0 = sl - h6 * (T(2) * M0 + M1)
    e = (M1 - M0) / h
    val = Y0 + s * (d0 + s * (M0 / T(2) + s6 * e))
    der = d0 + s * (M0 + s2 * e)
    return val, der


def natural_coeffs(series, knots):
    """``Y, M [B, Tn, C]`` of numpy ``series [B, Tn, C]`` over ``knots [Tn]`` (one dtype), in the header's order."""
    T = series.dtype.type
    B, Tn, C = series.shape
    assert knots.dtype == series.dtype and knots.shape == (Tn,) and Tn >= 2
    y = np.ascontiguousarray(series.transpose(0, 2, 1)).reshape(B * C, Tn)  # a column per row
    N = y.shape[0]
    n = np.arange(N)
    t = knots
    Yw, Mw = np.empty_like(y), np.empty_like(y)
    obs_all = ~np.isnan(y)
    some = obs_all.any(axis=1)
    yfirst = y[n, np.argmax(obs_all, axis=1)]  # (NaN where nothing is observed: the whole column becomes NaN below)
    with np.errstate(all="ignore"):
        # 1. forward elimination, lagging one node
        zero = np.zeros(N, dtype=T)
        ta, ya, cpa, dpa = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        have_a = np.zeros(N, dtype=bool)
        ti, yi, ylast = np.full(N, t[0], dtype=T), yfirst.copy(), yfirst.copy()
        ki = np.zeros(N, dtype=np.int64)
        for k in range(1, Tn):
            yb = y[:, k]
            obs = obs_all[:, k]
            ylast = np.where(obs, yb, ylast)
            node = obs | (k == Tn - 1)
            yb = np.where(obs, yb, ylast)
            tb = np.full(N, t[k], dtype=T)
            hl, hr = ti - ta, tb - ti
            sl, sr = (yi - ya) / hl, (yb - yi) / hr
            rhs = T(6) * (sr - sl)
            den = T(2) * (hl + hr) - hl * cpa
            cp = np.where(have_a, hr / den, T(0))
            dp = np.where(have_a, (rhs - hl * dpa) / den, T(0))
            r = n[node]
            Yw[r, ki[r]] = cp[r]
            Mw[r, ki[r]] = dp[r]
            ta, ya, cpa, dpa = np.where(node, ti, ta), np.where(node, yi, ya), np.where(node, cp, cpa), np.where(node, dp, dpa)
            have_a = have_a | node
            ti, yi, ki = np.where(node, tb, ti), np.where(node, yb, yi), np.where(node, k, ki)
        # 2. back substitution over the interior nodes
        Mb = zero.copy()
        Mw[:, Tn - 1] = T(0)
        for k in range(Tn - 2, 0, -1):
            obs = obs_all[:, k]
            Mk = Mw[:, k] - Yw[:, k] * Mb
            Mw[:, k] = np.where(obs, Mk, Mw[:, k])
            Mb = np.where(obs, Mk, Mb)
        Mw[:, 0] = T(0)
        # 3. the values at the nodes, then every missing row from the nodes a < j < b around it
        node = obs_all.copy()
        node[:, 0] = node[:, Tn - 1] = True
        Yn = y.copy()
        Yn[:, 0] = yfirst
        Yn[:, Tn - 1] = ylast
        idx = np.broadcast_to(np.arange(Tn), (N, Tn))
        a = np.maximum.accumulate(np.where(node, idx, 0), axis=1)
        b = np.minimum.accumulate(np.where(node, idx, Tn - 1)[:, ::-1], axis=1)[:, ::-1]
        rows = n[:, None]
        tj = np.broadcast_to(t, (N, Tn))
        ta2, tb2 = t[a], t[b]
        ya2, yb2, Ma2, Mb2 = Yn[rows, a], Yn[rows, b], Mw[rows, a], Mw[rows, b]
        h, s = tb2 - ta2, tj - ta2
        val, _ = natural_eval(T, h, s, ya2, yb2, Ma2, Mb2)
        Mfill = Ma2 + (s / h) * (Mb2 - Ma2)
        Y = np.where(node, Yn, val)
        M = np.where(node, Mw, Mfill)
    Y[~some] = np.nan
    M[~some] = np.nan
    back = lambda x: np.ascontiguousarray(x.reshape(B, C, Tn).transpose(0, 2, 1))  # noqa: E731
    return back(Y.astype(T)), back(M.astype(T))


def natural_gather(Y, M, knots, tq):
    """``val, der [outer, L, D]`` of numpy ``Y, M [outer, Tn, D]`` at ``tq [L]`` (all one dtype), in the header's order."""
    T = Y.dtype.type
    Tn = Y.shape[1]
    assert M.shape == Y.shape and knots.dtype == Y.dtype == tq.dtype and M.dtype == Y.dtype
    i = np.clip(np.searchsorted(knots, tq, side="right") - 1, 0, Tn - 2)  # #{t_k <= tau} - 1
    h = (knots[i + 1] - knots[i])[None, :, None]
    s = (tq - knots[i])[None, :, None]
    with np.errstate(all="ignore"):
        return natural_eval(T, h, s, Y[:, i, :], Y[:, i + 1, :], M[:, i, :], M[:, i + 1, :])


class SplineDoubleBackend(CdeDoubleBackend):
    name = CdeDoubleBackend.name.replace("(test)", "+spline(test)")

    def _spline_natural_coeffs(self, Y, M, series, knots):
        self.launches.append("spline_natural_coeffs")
        assert series.dim() == 3 and series.is_contiguous() and Y.is_contiguous() and M.is_contiguous()
        assert Y.shape == M.shape == series.shape and Y.dtype == M.dtype == series.dtype == knots.dtype
        y, m = natural_coeffs(_np(series), _np(knots))
        _np(Y)[...] = y
        _np(M)[...] = m

    def _spline_natural_gather(self, val, der, Y, M, knots, tq):
        self.launches.append("spline_natural_gather")
        if val.numel() == 0:
            return
        Tn, D = Y.shape[-2:]
        v, d = natural_gather(_np(Y).reshape(-1, Tn, D), _np(M).reshape(-1, Tn, D), _np(knots), _np(tq).reshape(-1))
        _np(val)[...] = v.reshape(val.shape)
        if der is not None:
            _np(der)[...] = d.reshape(der.shape)

    def _natural_dx(self, Y, M, knots, t):
        assert Y.dim() == 3 and Y.is_contiguous() and M.is_contiguous() and M.shape == Y.shape and knots.shape == (Y.shape[1],)
        if torch.is_tensor(t):
            assert t.numel() == 1 and t.dtype in (torch.float32, torch.float64), "t: one float32 / float64 element"
            t = _np(t).reshape(-1)[0]
        tau = np.asarray([t]).astype(_NP[Y.dtype])  # (the time in the series dtype first)
        return natural_gather(_np(Y), _np(M), _np(knots), tau)[1][:, 0, :]

    def _cde_contract_natural(self, out, F, Y, M, knots, t):
        self.launches.append("cde_contract_natural")
        assert F.dim() == 3 and F.is_contiguous() and out.is_contiguous() and out.shape == F.shape[:2]
        assert F.shape[0] == Y.shape[0] and F.shape[2] == Y.shape[2] and F.dtype == Y.dtype == out.dtype == knots.dtype == M.dtype
        _np(out)[...] = contract_in_header_order(_np(F), self._natural_dx(Y, M, knots, t))

    def _cde_contract_natural_backward(self, gF, gout, Y, M, knots, t):
        self.launches.append("cde_contract_natural_backward")
        assert gF.dim() == 3 and gF.is_contiguous() and gout.is_contiguous() and gout.shape == gF.shape[:2]
        assert gF.shape[0] == Y.shape[0] and gF.shape[2] == Y.shape[2] and gF.dtype == Y.dtype == gout.dtype == knots.dtype == M.dtype
        _np(gF)[...] = _np(gout)[:, :, None] * self._natural_dx(Y, M, knots, t)[:, None, :]
