"""TEST DOUBLE of sdeint's SRK entry points: the Milstein double plus ``_sde_srk_stage1``, ``_sde_srk_stage2``, ``_sde_srk_step``, their
three backwards and ``_sde_noise(..., draw=)`` (include/xde_hip_sde.h) in numpy, in the op order of csrc/xde_sde.hip, on the two draws
of tests/_srk_oracle.py rounded to the state dtype."""
import numpy as np

from . import _srk_oracle as KO
from ._cpu_double import _NP
from ._milstein_double import MilsteinDoubleBackend


def _np(x):
    return x.detach().numpy()


def _same(*xs):
    return all(x.shape == xs[0].shape and x.dtype == xs[0].dtype and x.is_contiguous() for x in xs)


def _groups(outs, groups):
    """A group of outputs is given whole or not at all."""
    for lo, hi in groups:
        given = [o is not None for o in outs[lo:hi]]
        assert all(given) or not any(given), "the outputs of a group are given or skipped together"


class SrkDoubleBackend(MilsteinDoubleBackend):
    name = "numpy-double+sde+milstein+srk(test)"

    @staticmethod
    def _draws(shape, seed, k, T):
        return (KO.state_normals(tuple(shape), seed, k, T, 0), KO.state_normals(tuple(shape), seed, k, T, 1))

    @staticmethod
    def _wp(z, v, s, T):
        w = T(s) * z
        return w, T(0.5) * (w + (T(s) * v) * KO.consts(T)[0])

    @classmethod
    def _weights(cls, z, v, dt, s, c, c3, T):
        _, third, two3, four3, five3 = KO.consts(T)
        w, p = cls._wp(z, v, s, T)
        a = abs(T(dt))
        ww = w * w
        q, u = T(c) * (ww - a), T(c3) * ((ww - T(3) * a) * w)
        return (((-w - q) + T(2) * p) - T(2) * u, four3 * ((w + q) - p) + five3 * u, two3 * ((w - p) - u) - third * q, u)

    def _sde_srk_stage1(self, Y2, G2, G3, y0, a1, b1, dt, s, seed, k):
        self.launches.append("sde_srk_stage1")
        T = _NP[y0.dtype]
        assert _same(Y2, G2, G3, y0, a1, b1)
        z, v = self._draws(y0.shape, seed, k, T)
        _, p = self._wp(z, v, s, T)
        y, a, b, dt, s = _np(y0), _np(a1), _np(b1), T(dt), T(s)
        o2, g2, g3 = (y + a * (T(0.75) * dt)) + b * (T(1.5) * p), (y + a * (T(0.25) * dt)) + b * (T(0.5) * s), (y + a * dt) - b * s
        for dst, val in ((Y2, o2), (G2, g2), (G3, g3)):
            _np(dst)[...] = np.asarray(val, dtype=T)

    def _sde_srk_stage2(self, G4, y0, a1, b1, b2, b3, dt, s):
        self.launches.append("sde_srk_stage2")
        T = _NP[y0.dtype]
        assert _same(G4, y0, a1, b1, b2, b3)
        v = (_np(y0) + _np(a1) * (T(0.25) * T(dt))) + ((_np(b1) * T(-5) + _np(b2) * T(3)) + _np(b3) * T(0.5)) * T(s)
        _np(G4)[...] = np.asarray(v, dtype=T)

    def _sde_srk_step(self, y1, y0, a1, a2, b1, b2, b3, b4, dt, s, c, c3, seed, k):
        self.launches.append("sde_srk_step")
        T = _NP[y0.dtype]
        assert _same(y1, y0, a1, a2, b1, b2, b3, b4)
        _, third, two3, _, _ = KO.consts(T)
        e = self._weights(*self._draws(y0.shape, seed, k, T), dt, s, c, c3, T)
        v = ((((_np(y0) + (third * _np(a1) + two3 * _np(a2)) * T(dt)) + _np(b1) * e[0]) + _np(b2) * e[1]) + _np(b3) * e[2]) + _np(b4) * e[3]
        _np(y1)[...] = np.asarray(v, dtype=T)

    def _sde_srk_stage1_backward(self, gy, ga1, gb1, gY2, gG2, gG3, dt, s, seed, k):
        self.launches.append("sde_srk_stage1_backward")
        T = _NP[gY2.dtype]
        assert _same(gY2, gG2, gG3)
        g2, h2, h3, dt, s = _np(gY2), _np(gG2), _np(gG3), T(dt), T(s)
        if gy is not None:
            _np(gy)[...] = (g2 + h2) + h3
        if ga1 is not None:
            _np(ga1)[...] = (g2 * (T(0.75) * dt) + h2 * (T(0.25) * dt)) + h3 * dt
        if gb1 is not None:
            _, p = self._wp(*self._draws(gY2.shape, seed, k, T), s, T)
            _np(gb1)[...] = (g2 * (T(1.5) * p) + h2 * (T(0.5) * s)) - h3 * s

    def _sde_srk_stage2_backward(self, ga1, gb1, gb2, gb3, gG4, dt, s):
        self.launches.append("sde_srk_stage2_backward")
        T = _NP[gG4.dtype]
        _groups((ga1, gb1, gb2, gb3), ((0, 1), (1, 4)))
        g, s = _np(gG4), T(s)
        if ga1 is not None:
            _np(ga1)[...] = g * (T(0.25) * T(dt))
        if gb1 is not None:
            for dst, f in ((gb1, T(-5)), (gb2, T(3)), (gb3, T(0.5))):
                _np(dst)[...] = g * (f * s)

    def _sde_srk_step_backward(self, ga1, ga2, gb1, gb2, gb3, gb4, gy1, dt, s, c, c3, seed, k):
        self.launches.append("sde_srk_step_backward")
        T = _NP[gy1.dtype]
        _groups((ga1, ga2, gb1, gb2, gb3, gb4), ((0, 2), (2, 6)))
        _, third, two3, _, _ = KO.consts(T)
        g = _np(gy1)
        if ga1 is not None:
            _np(ga1)[...] = g * (third * T(dt))
            _np(ga2)[...] = g * (two3 * T(dt))
        if gb1 is not None:
            e = self._weights(*self._draws(gy1.shape, seed, k, T), dt, s, c, c3, T)
            for dst, ei in zip((gb1, gb2, gb3, gb4), e):
                _np(dst)[...] = g * ei

    def _sde_noise(self, out, seed, k, bits=False, draw=0):
        if not draw:
            return super()._sde_noise(out, seed, k, bits=bits)
        self.launches.append("sde_noise")
        n = out.numel()
        if bits:
            w = KO.words(-(-n // 4), seed, k, draw).reshape(-1)[:n]
            out.detach().numpy().reshape(-1)[...] = w.view(np.int32) if out.dtype.is_signed else w
        else:
            T = _NP[out.dtype]
            out.detach().numpy().reshape(-1)[...] = KO.normals(n, seed, k, T, draw).astype(T)
