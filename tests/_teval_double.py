"""TEST DOUBLE of the per-sample output-time entry points: the newest double (the DDE tape's) plus ``_teval_dense`` and
``_teval_cotangent`` (include/xde_hip_teval.h) in numpy, through tests/_teval_oracle.py.  The launch log says ``"teval_dense"`` /
``"teval_cotangent"``."""
import numpy as np
import torch

from paddlexde_amd import _hip

from . import _teval_oracle as TO
from ._dde_tape_double import DdeTapeDoubleBackend
from ._srk_double import _np, _same


def _tt(time_dtype):
    return np.float32 if time_dtype == _hip.XDE_F32 else np.float64


class TevalDoubleBackend(DdeTapeDoubleBackend):
    name = DdeTapeDoubleBackend.name.replace("(test)", "+teval(test)")

    @staticmethod
    def _times(big, tq, cnt, like):
        rows, Q = tq.shape
        assert like.dim() >= 2 and like.shape[0] == rows and tq.dtype == torch.float64 and tq.is_contiguous()
        assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (rows,) and big.is_contiguous() and big.dtype == like.dtype
        assert tuple(big.shape) == (Q,) + tuple(like.shape)
        return rows, Q

    def _teval_dense(self, out, tq, cnt, ks, mid, y0, y1, f0, f1, t0, t1, dt, direction, time_dtype):
        self.launches.append("teval_dense")
        assert _same(y0, y1, f0, f1, *ks) and 1 <= len(ks) <= _hip.XDE_MAX_K and len(mid) == len(ks)
        rows, Q = self._times(out, tq, cnt, y0)
        two = lambda x: _np(x).reshape(rows, -1)  # noqa: E731
        TO.dense(_np(out).reshape(Q, rows, -1), _np(tq), _np(cnt), [two(k) for k in ks], list(mid), two(y0), two(y1), two(f0), two(f1),
                 t0, t1, dt, direction, _tt(time_dtype))

    def _teval_cotangent(self, outs, g, tq, cnt, t0, t1, dt, direction, time_dtype, acc_mask=0):
        self.launches.append("teval_cotangent")
        given = [o for o in outs if o is not None]
        assert len(outs) == 5 and given and _same(*given)
        rows, Q = self._times(g, tq, cnt, given[0])
        TO.cotangent([None if o is None else _np(o).reshape(rows, -1) for o in outs], _np(g).reshape(Q, rows, -1), _np(tq), _np(cnt), t0, t1, dt,
                     direction, _tt(time_dtype), acc_mask)
