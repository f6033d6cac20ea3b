"""TEST DOUBLE of the sub-stepping entry point: NumpyDoubleBackend plus ``_interp_rows`` (xde_interp_rows, include/xde_hip_grid.h)
in numpy, in the op order of csrc/xde_interp.hip.  HipBackend keeps the method private (its public methods are the contract
tests/test_cabi.py freezes against tests/_cpu_double.py), so it lives in this subclass of its own."""
import numpy as np

from paddlexde_amd import _hip

from ._cpu_double import _NP, NumpyDoubleBackend


class SubstepDoubleBackend(NumpyDoubleBackend):
    name = "numpy-double+substep(test)"

    def _interp_rows(self, dsts, kinds, weights, y_a, y_b, f_a=None, f_b=None):
        assert len(dsts) == len(kinds) == len(weights) >= 1
        T = _NP[y_a.dtype]
        cubic = f_a is not None
        ya, yb = y_a.detach().numpy(), y_b.detach().numpy()
        fa, fb = (f_a.detach().numpy(), f_b.detach().numpy()) if cubic else (None, None)
        for r0 in range(0, len(dsts), _hip.XDE_INTERP_MAX_ROWS):
            self.launches.append("interp_rows")
            for dst, kind, w in list(zip(dsts, kinds, weights))[r0 : r0 + _hip.XDE_INTERP_MAX_ROWS]:
                assert dst.shape == y_a.shape
                if kind == _hip.XDE_ROW_COPY_A:
                    v = ya
                elif kind == _hip.XDE_ROW_COPY_B:
                    v = yb
                elif cubic:
                    v = ((T(w[0]) * ya + T(w[1]) * fa) + T(w[2]) * yb) + T(w[3]) * fb
                else:
                    v = ya + T(w[0]) * (yb - ya)
                dst.detach().numpy()[...] = np.asarray(v, dtype=T)
