"""TEST DOUBLE of the Hermite-tape entry points: the logsignature double (the newest one) plus ``_dde_tape_gather`` and
``_dde_tape_gather_backward`` (include/xde_hip_dde.h) in numpy, through tests/_dde_tape_oracle.py.  The launch log says
``"dde_tape_gather"`` / ``"dde_tape_gather_backward"``, one entry per launch: a gather of more than ``XDE_DDE_MAX_LAGS`` delays logs one
per tile, as the binding launches one per tile."""
from paddlexde_amd import _hip

from . import _dde_tape_oracle as DO
from ._cpu_double import _NP
from ._logsig_double import LogsigDoubleBackend
from ._srk_double import _np


class DdeTapeDoubleBackend(LogsigDoubleBackend):
    name = LogsigDoubleBackend.name.replace("(test)", "+dde_tape(test)")

    def _dde_tape_gather(self, out, dtau, srcs, w, wd=None):
        rows, L, D = out.shape
        assert out.is_contiguous() and (dtau is None) == (wd is None) and (dtau is None or (dtau.is_contiguous() and dtau.shape == out.shape))
        assert len(srcs) == 4 * L == len(w) and all(tuple(x.shape) == (rows, D) and x.dtype == out.dtype for x in srcs)
        self.launches += ["dde_tape_gather"] * -(-L // _hip.XDE_DDE_MAX_LAGS)
        val, der = DO.gather([_np(x) for x in srcs], list(w), None if wd is None else list(wd), _NP[out.dtype])
        _np(out)[...] = val
        if dtau is not None:
            _np(dtau)[...] = der

    def _dde_tape_gather_backward(self, gouts, terms, g, j0=0):
        rows, L, D = g.shape
        assert g.is_contiguous() and 1 <= len(gouts) == len(terms) <= 4 * _hip.XDE_DDE_MAX_LAGS
        assert all(o.is_contiguous() and tuple(o.shape) == (rows, D) and o.dtype == g.dtype for o in gouts)
        assert all(len(ts) >= 1 and all(0 <= lag < _hip.XDE_DDE_MAX_LAGS and j0 + lag < L for lag, _ in ts) for ts in terms)
        assert sum(len(ts) for ts in terms) <= 4 * _hip.XDE_DDE_MAX_LAGS
        self.launches.append("dde_tape_gather_backward")
        for o, val in zip(gouts, DO.gather_backward(_np(g), terms, j0, _NP[g.dtype])):
            _np(o)[...] = val
