"""TEST DOUBLE of sdeint's entry points: the sub-stepping double plus ``_sde_em_step``, ``_sde_em_backward`` and ``_sde_noise``
(include/xde_hip_sde.h) in numpy, in the op order of csrc/xde_sde.hip, on the normals of tests/_sde_oracle.py rounded to the state
dtype.  HipBackend keeps the methods private (its public methods are the contract tests/test_cabi.py freezes against
tests/_cpu_double.py), so they live in this subclass of their own."""
import numpy as np

from . import _sde_oracle as SO
from ._cpu_double import _NP
from ._substep_double import SubstepDoubleBackend


class SdeDoubleBackend(SubstepDoubleBackend):
    name = "numpy-double+sde(test)"

    def _sde_em_step(self, y1, y0, f, g, dt, s, seed, k):
        self.launches.append("sde_em_step")
        T = _NP[y0.dtype]
        assert y1.shape == y0.shape == f.shape == g.shape and y0.is_contiguous() and f.is_contiguous() and g.is_contiguous()
        z = SO.state_normals(tuple(y0.shape), seed, k, T)
        v = (y0.detach().numpy() + f.detach().numpy() * T(dt)) + g.detach().numpy() * (T(s) * z)
        y1.detach().numpy()[...] = np.asarray(v, dtype=T)

    def _sde_em_backward(self, gf, gg, gy1, dt, s, seed, k):
        self.launches.append("sde_em_backward")
        T = _NP[gy1.dtype]
        g = gy1.detach().numpy()
        if gf is not None:
            gf.detach().numpy()[...] = g * T(dt)
        if gg is not None:
            gg.detach().numpy()[...] = g * (T(s) * SO.state_normals(tuple(gy1.shape), seed, k, T))

    def _sde_noise(self, out, seed, k, bits=False):
        self.launches.append("sde_noise")
        n = out.numel()
        if bits:
            w = SO.words(-(-n // 4), seed, k).reshape(-1)[:n]
            out.detach().numpy().reshape(-1)[...] = w.view(np.int32) if out.dtype.is_signed else w
        else:
            T = _NP[out.dtype]
            out.detach().numpy().reshape(-1)[...] = SO.normals(n, seed, k, T).astype(T)
