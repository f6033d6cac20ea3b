"""TEST DOUBLE of sdeint's Milstein entry points: the SDE double plus ``_sde_milstein_support``, ``_sde_milstein_support_backward``,
``_sde_milstein_step`` and ``_sde_milstein_backward`` (include/xde_hip_sde.h) in numpy, in the op order of csrc/xde_sde.hip, on the
normals of tests/_sde_oracle.py rounded to the state dtype."""
import numpy as np

from . import _sde_oracle as SO
from ._cpu_double import _NP
from ._sde_double import SdeDoubleBackend


def _np(x):
    return x.detach().numpy()


class MilsteinDoubleBackend(SdeDoubleBackend):
    name = "numpy-double+sde+milstein(test)"

    def _sde_milstein_support(self, yb, y0, f, g, dt, s):
        self.launches.append("sde_milstein_support")
        T = _NP[y0.dtype]
        assert yb.shape == y0.shape == f.shape == g.shape and y0.is_contiguous() and f.is_contiguous() and g.is_contiguous()
        _np(yb)[...] = np.asarray((_np(y0) + _np(f) * T(dt)) + _np(g) * T(s), dtype=T)

    def _sde_milstein_support_backward(self, gf, gg, gyb, dt, s):
        self.launches.append("sde_milstein_support_backward")
        T = _NP[gyb.dtype]
        if gf is not None:
            _np(gf)[...] = _np(gyb) * T(dt)
        if gg is not None:
            _np(gg)[...] = _np(gyb) * T(s)

    @staticmethod
    def _wq(shape, dt, s, c, seed, k, T):
        w = T(s) * SO.state_normals(tuple(shape), seed, k, T)
        return w, T(c) * (w * w - abs(T(dt)))

    def _sde_milstein_step(self, y1, y0, f, g, gb, dt, s, c, seed, k):
        self.launches.append("sde_milstein_step")
        T = _NP[y0.dtype]
        assert y1.shape == y0.shape == f.shape == g.shape == gb.shape and all(x.is_contiguous() for x in (y0, f, g, gb))
        w, q = self._wq(y0.shape, dt, s, c, seed, k, T)
        v = ((_np(y0) + _np(f) * T(dt)) + _np(g) * w) + (_np(gb) - _np(g)) * q
        _np(y1)[...] = np.asarray(v, dtype=T)

    def _sde_milstein_backward(self, gf, gg, ggb, gy1, dt, s, c, seed, k):
        self.launches.append("sde_milstein_backward")
        T = _NP[gy1.dtype]
        gy = _np(gy1)
        if gf is not None:
            _np(gf)[...] = gy * T(dt)
        if gg is not None or ggb is not None:
            w, q = self._wq(gy1.shape, dt, s, c, seed, k, T)
            if gg is not None:
                _np(gg)[...] = gy * (w - q)
            if ggb is not None:
                _np(ggb)[...] = gy * q
