"""TEST DOUBLE of the latent-SDE KL entry points: the reversible Heun double (the newest SDE double) plus ``_sde_kl_step`` and
``_sde_kl_backward`` (include/xde_hip_kl.h) in numpy, through tests/_kl_oracle.py, on the normals of tests/_sde_oracle.py rounded to the
state dtype.  The launch log says ``"sde_kl_step"`` / ``"sde_kl_backward"``."""
import numpy as np
import torch

from . import _kl_oracle as KL
from . import _sde_oracle as SO
from ._cpu_double import _NP
from ._rheun_double import RheunDoubleBackend
from ._srk_double import _np, _same


class KlDoubleBackend(RheunDoubleBackend):
    name = "numpy-double+sde+milstein+srk+rheun+kl(test)"

    @staticmethod
    def _acc_ok(acc, like):
        return acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() * like.shape[-1] == like.numel()

    def _sde_kl_step(self, y1, acc1, y0, f, g, h, acc0, dt, s, seed, k):
        self.launches.append("sde_kl_step")
        assert (y1 is None) == (y0 is None), "y1 and y0 are given or null together"
        assert _same(f, g, h, *([y1, y0] if y1 is not None else []))
        assert self._acc_ok(acc1, f) and (acc0 is None or self._acc_ok(acc0, f))
        T = _NP[f.dtype]
        a0 = None if acc0 is None else _np(acc0).reshape(f.shape[:-1]).copy()
        if y1 is not None:
            z = SO.state_normals(tuple(y0.shape), seed, k, T)
            _np(y1)[...] = np.asarray((_np(y0) + _np(f) * T(dt)) + _np(g) * (T(s) * z), dtype=T)  # (_sde_em_step's expression)
        _np(acc1).reshape(f.shape[:-1])[...] = KL.accumulate(a0, _np(f), _np(g), _np(h), T(dt), T)[0]

    def _sde_kl_backward(self, gf, gg, gh, gy1, gacc, f, g, h, dt, s, seed, k):
        self.launches.append("sde_kl_backward")
        assert _same(f, g, h, *[x for x in (gf, gg, gh, gy1) if x is not None]) and self._acc_ok(gacc, f)
        T = _NP[f.dtype]
        z = SO.state_normals(tuple(f.shape), seed, k, T) if gy1 is not None else None
        outs = KL.kl_backward(None if gy1 is None else _np(gy1), _np(gacc).reshape(f.shape[:-1]), _np(f), _np(g), _np(h), T(dt), T(s), z, T)
        for dst, val in zip((gf, gg, gh), outs):
            if dst is not None:
                _np(dst)[...] = np.asarray(val, dtype=T)
