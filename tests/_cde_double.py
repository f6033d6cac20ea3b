"""TEST DOUBLE of cdeint's entry points: the reversible Heun double plus ``_cde_contract`` and ``_cde_contract_backward``
(include/xde_hip_cde.h) in numpy.  dX is the ``der`` of the double's own ``history_gather`` for the one query tau = T(t) (the kernels use
the history gathers' device functions); the sum over c runs in the header's order: lane j of a team of R takes the vectors j, j + R, ...
in ascending c, then the shuffle tree."""
import numpy as np
import torch

from ._cpu_double import _NP, _np
from ._rheun_double import RheunDoubleBackend


def team_lanes(C, T):
    """(W, NV, R) of the header: elements per 16 bytes, vectors per row, lanes per row team."""
    W = 4 if T == np.float32 else 2
    NV = -(-C // W)
    R = 1
    while R < min(NV, 64):
        R *= 2
    return W, NV, R


def contract_in_header_order(F, dX):
    """``out[b, h] = sum_c F[b, h, c] * dX[b, c]`` for numpy ``F [B, H, C]``, ``dX [B, C]`` of one dtype, in the header's order."""
    T = F.dtype.type
    B, H, C = F.shape
    W, NV, R = team_lanes(C, T)
    v = np.zeros((B, H, R), dtype=T)
    for q in range(NV):  # (ascending q visits every lane's vectors in that lane's order)
        j = q % R
        for c in range(q * W, min(q * W + W, C)):
            v[:, :, j] = v[:, :, j] + F[:, :, c] * dX[:, None, c]
    off = R // 2
    while off:
        v[:, :, :off] = v[:, :, :off] + v[:, :, off:2 * off]
        off //= 2
    return v[:, :, 0]


class CdeDoubleBackend(RheunDoubleBackend):
    name = "numpy-double+sde+milstein+srk+rheun+cde(test)"

    def _cde_dx(self, series, knots, t, method):
        assert method in ("linear", "cubic"), "XDE_HISTORY_BEZIER is refused"
        assert series.dim() == 3 and series.is_contiguous() and knots.shape == (series.shape[1],) and series.shape[1] >= 2
        if torch.is_tensor(t):
            assert t.numel() == 1 and t.dtype in (torch.float32, torch.float64), "t: one float32 / float64 element"
            t = _np(t).reshape(-1)[0]
        T = _NP[series.dtype]
        tau = torch.from_numpy(np.asarray([t]).astype(T))  # (the time in the series dtype first)
        B, _, C = series.shape
        val, der = torch.empty(B, 1, C, dtype=series.dtype), torch.empty(B, 1, C, dtype=series.dtype)
        n = len(self.launches)
        self.history_gather(val, der, series, knots, tau, method)
        del self.launches[n:]  # (dX is built inside the contraction's launch)
        return _np(der)[:, 0, :]

    def _cde_contract(self, out, F, series, knots, t, method):
        self.launches.append("cde_contract")
        assert F.dim() == 3 and F.is_contiguous() and out.is_contiguous() and out.shape == F.shape[:2]
        assert F.shape[0] == series.shape[0] and F.shape[2] == series.shape[2] and F.dtype == series.dtype == out.dtype == knots.dtype
        _np(out)[...] = contract_in_header_order(_np(F), self._cde_dx(series, knots, t, method))

    def _cde_contract_backward(self, gF, gout, series, knots, t, method):
        self.launches.append("cde_contract_backward")
        assert gF.dim() == 3 and gF.is_contiguous() and gout.is_contiguous() and gout.shape == gF.shape[:2]
        assert gF.shape[0] == series.shape[0] and gF.shape[2] == series.shape[2] and gF.dtype == series.dtype == gout.dtype == knots.dtype
        _np(gF)[...] = _np(gout)[:, :, None] * self._cde_dx(series, knots, t, method)[:, None, :]
