"""TEST DOUBLE of the per-sample entry points: the general-noise double (the newest one) plus ``_rows_stage_combine``,
``_rows_norm_control``, ``_rows_dense_commit`` and ``_rows_scaled_norm`` (include/xde_hip_rows.h) in numpy, through
tests/_rows_oracle.py.  The launch log says ``"rows_stage_combine"`` / ``"rows_norm_control"`` / ``"rows_dense_commit"`` /
``"rows_scaled_norm"``."""
import types

import numpy as np

from . import _rows_oracle as RO
from ._cpu_double import _NP
from ._gn_double import GnDoubleBackend
from ._srk_double import _np, _same


def _ctl(ctl):
    """A ``_hip.RowsCtl`` as the oracle's view of it (numpy views of the planes: written in place)."""
    return types.SimpleNamespace(t_stage=_np(ctl.t_stage), **{n: _np(getattr(ctl, n)) for n in RO.F64 + RO.I32})


def _2d(x, rows):
    return _np(x).reshape(rows, -1)


class RowsDoubleBackend(GnDoubleBackend):
    name = GnDoubleBackend.name.replace("(test)", "+rows(test)")

    def _rows_stage_combine(self, out, y0, ks, coef, ctl, *, out2=None, coef2=None):
        self.launches.append("rows_stage_combine")
        assert _same(out, y0, *ks) and (out2 is None) == (coef2 is None) and 1 <= len(ks) <= 7 and len(coef) == len(ks)
        R = ctl.rows
        o, o2 = RO.stage_combine(_2d(y0, R), [_2d(k, R) for k in ks], list(coef), _ctl(ctl), None if coef2 is None else list(coef2))
        _2d(out, R)[...] = o
        if out2 is not None:
            _2d(out2, R)[...] = o2

    def _rows_norm_control(self, ks, c_err, y0, y1, ctl, params, t_span_dev, *, e_pre=None):
        self.launches.append("rows_norm_control")
        assert _same(y0, y1, *ks) and (e_pre is None or len(ks) == 1)
        R = ctl.rows
        RO.norm_control([_2d(k, R) for k in ks], list(c_err), None if e_pre is None else _2d(e_pre, R), _2d(y0, R), _2d(y1, R), _ctl(ctl),
                        params, t_span_dev.numpy(), t_span_dev.numel())

    def _rows_dense_commit(self, out, ks, mid, y0, y1, f1, ctl, params, t_span_dev):
        self.launches.append("rows_dense_commit")
        assert _same(y0, y1, f1, *ks) and out.is_contiguous() and tuple(out.shape) == (t_span_dev.numel(),) + tuple(y0.shape)
        R = ctl.rows
        RO.dense_commit(_np(out).reshape(t_span_dev.numel(), R, -1), [_2d(k, R) for k in ks], list(mid), _2d(y0, R), _2d(y1, R), _2d(f1, R),
                        _ctl(ctl), params, t_span_dev.numpy(), t_span_dev.numel())

    def _rows_scaled_norm(self, out, a, b, y0, rtol, atol):
        self.launches.append("rows_scaled_norm")
        assert _same(a, y0) and (b is None or _same(b, y0)) and out.dtype.is_floating_point and out.numel() == y0.shape[0]
        R = y0.shape[0]
        T = _NP[y0.dtype]
        _np(out)[...] = RO.scaled_norm(_2d(a, R), None if b is None else _2d(b, R), _2d(y0, R), T(rtol), T(atol)).astype(np.float64)
