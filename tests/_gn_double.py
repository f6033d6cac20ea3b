"""TEST DOUBLE of the general-noise entry points: the KL double (the newest SDE double) plus ``_sde_gn_step`` and ``_sde_gn_backward``
(include/xde_hip_gn.h) in numpy, through tests/_gn_oracle.py, on the normals of tests/_sde_oracle.py over the flat ``[rows, M]`` array
rounded to the state dtype.  The launch log says ``"sde_gn_step"`` / ``"sde_gn_backward"``."""
import numpy as np

from . import _gn_oracle as GN
from . import _sde_oracle as SO
from ._cpu_double import _NP
from ._kl_double import KlDoubleBackend
from ._srk_double import _np, _same


class GnDoubleBackend(KlDoubleBackend):
    name = "numpy-double+sde+milstein+srk+rheun+kl+gn(test)"

    @staticmethod
    def _matrix_ok(g, like):
        return g.is_contiguous() and g.dtype == like.dtype and g.dim() == like.dim() + 1 and g.shape[:-1] == like.shape and g.shape[-1] >= 1

    def _sde_gn_step(self, y1, y0, f, g, dt, s, seed, k):
        self.launches.append("sde_gn_step")
        assert _same(y1, y0, f) and self._matrix_ok(g, y0)
        T = _NP[y0.dtype]
        z = SO.state_normals(GN.noise_shape(tuple(y0.shape), g.shape[-1]), seed, k, T)
        _np(y1)[...] = GN.gn_step(_np(y0), _np(f), _np(g), T(dt), T(s), z, T)

    def _sde_gn_backward(self, gf, gg, gy1, M, dt, s, seed, k):
        self.launches.append("sde_gn_backward")
        assert gy1.is_contiguous() and (gf is None or _same(gf, gy1)) and (gg is None or (self._matrix_ok(gg, gy1) and gg.shape[-1] == M))
        T = _NP[gy1.dtype]
        z = SO.state_normals(GN.noise_shape(tuple(gy1.shape), M), seed, k, T)
        for dst, val in zip((gf, gg), GN.gn_backward(_np(gy1), T(dt), T(s), z, T)):
            if dst is not None:
                _np(dst)[...] = np.asarray(val, dtype=T)
