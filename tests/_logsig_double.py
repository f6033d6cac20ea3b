"""TEST DOUBLE of the logsignature entry points: the per-sample double (the newest one) plus ``_logsig_windows`` and
``_logsig_windows_backward`` (include/xde_hip_logsig.h) in numpy, through tests/_logsig_oracle.py.  The launch log says
``"logsig_windows"`` / ``"logsig_windows_backward"``.  The doubles of the CDE contraction and its control gradient (the other branch
of the doubles, tests/_cdegrad_double.py) are mixed in: the path these windows make is a control of cdeint."""
from ._cdegrad_double import CdeGradDoubleBackend
from . import _logsig_oracle as LO
from ._rows_double import RowsDoubleBackend
from ._srk_double import _np, _same


def _3d(x):
    return _np(x).reshape((-1,) + tuple(x.shape[-2:]))


class LogsigDoubleBackend(RowsDoubleBackend, CdeGradDoubleBackend):
    name = RowsDoubleBackend.name.replace("(test)", "+logsig(test)")

    @staticmethod
    def _windows_ok(inc, x, L, depth):
        want = tuple(x.shape[:-2]) + (LO.n_windows(x.shape[-2], L), LO.channels(x.shape[-1], depth))
        return inc.is_contiguous() and inc.dtype == x.dtype and tuple(inc.shape) == want

    def _logsig_windows(self, out, x, window_length, depth):
        self.launches.append("logsig_windows")
        assert x.is_contiguous() and x.dim() >= 2 and self._windows_ok(out, x, window_length, depth)
        _3d(out)[...] = LO.windows(_3d(x), window_length, depth)

    def _logsig_windows_backward(self, gx, gout, x, window_length, depth):
        self.launches.append("logsig_windows_backward")
        assert _same(gx, x) and x.dim() >= 2 and self._windows_ok(gout, x, window_length, depth)
        _3d(gx)[...] = LO.backward(_3d(gout), _3d(x), window_length, depth)
