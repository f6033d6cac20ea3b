"""TEST DOUBLE of sdeint's reversible Heun entry points: the SRK double plus ``_sde_rheun_predict``, ``_sde_rheun_correct``,
``_sde_rheun_adjoint_stage`` and ``_sde_rheun_adjoint_step`` (include/xde_hip_sde.h) in numpy, in the op order of csrc/xde_sde.hip, on
the normals of tests/_sde_oracle.py rounded to the state dtype; the generator is skipped where s == 0."""
import numpy as np

from . import _sde_oracle as SO
from ._cpu_double import _NP
from ._srk_double import SrkDoubleBackend, _np, _same


class RheunDoubleBackend(SrkDoubleBackend):
    name = "numpy-double+sde+milstein+srk+rheun(test)"

    @staticmethod
    def _w(shape, s, seed, k, T):
        return T(s) * SO.state_normals(tuple(shape), seed, k, T) if s != 0 else np.full(tuple(shape), T(s))

    def _sde_rheun_predict(self, yh1, y0, yh0, f0, g0, dt, s, direction, seed, k):
        self.launches.append("sde_rheun_predict")
        assert direction in (1, -1) and _same(yh1, y0, yh0, f0, g0)
        T = _NP[y0.dtype]
        dt, s = float(direction) * dt, float(direction) * s
        y = _np(y0)
        v = (((y + y) - _np(yh0)) + _np(f0) * T(dt)) + _np(g0) * self._w(y0.shape, s, seed, k, T)
        _np(yh1)[...] = np.asarray(v, dtype=T)

    def _sde_rheun_correct(self, y1, y0, f0, f1, g0, g1, dt, s, direction, seed, k):
        self.launches.append("sde_rheun_correct")
        assert direction in (1, -1) and _same(y1, y0, f0, f1, g0, g1)
        T = _NP[y0.dtype]
        dt, s = float(direction) * dt, float(direction) * s
        v = (_np(y0) + (_np(f0) + _np(f1)) * (T(0.5) * T(dt))) + (_np(g0) + _np(g1)) * (T(0.5) * self._w(y0.shape, s, seed, k, T))
        _np(y1)[...] = np.asarray(v, dtype=T)

    def _sde_rheun_adjoint_stage(self, bf, bg, af1, ag1, ay1, dt, s, seed, k):
        self.launches.append("sde_rheun_adjoint_stage")
        assert (af1 is None) == (ag1 is None), "af1 and ag1 are null together"
        assert _same(bf, bg, ay1, *([af1, ag1] if af1 is not None else []))
        T = _NP[ay1.dtype]
        a = _np(ay1)
        hf, hg = a * (T(0.5) * T(dt)), a * (T(0.5) * self._w(ay1.shape, s, seed, k, T))
        if af1 is not None:
            hf, hg = _np(af1) + hf, _np(ag1) + hg
        _np(bf)[...] = np.asarray(hf, dtype=T)
        _np(bg)[...] = np.asarray(hg, dtype=T)

    def _sde_rheun_adjoint_step(self, ay0, ayh0, af0, ag0, ay1, ayh1, v, dt, s, seed, k):
        self.launches.append("sde_rheun_adjoint_step")
        assert _same(ay0, ayh0, af0, ag0, ay1, v, *([ayh1] if ayh1 is not None else []))
        T = _NP[ay1.dtype]
        w = self._w(ay1.shape, s, seed, k, T)
        a = _np(ay1)
        A = _np(v) if ayh1 is None else _np(ayh1) + _np(v)
        outs = (a + (A + A), -A, a * (T(0.5) * T(dt)) + A * T(dt), a * (T(0.5) * w) + A * w)  # (all read before any is written)
        for dst, val in zip((ay0, ayh0, af0, ag0), outs):
            _np(dst)[...] = np.asarray(val, dtype=T)
