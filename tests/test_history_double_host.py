"""What the numpy double of the history gathers (tests/_cpu_double.py) is worth where the GPU kernels are held to it bit for bit
(tests/test_gpu_history_kernels.py): T = 2, L = 129, lags on knots and outside the grid.  Runs on the CPU.

The double's three gathers, fp32 and fp64, are compared ELEMENT-WISE with `oracle.xde_oracle.HISTORY_SPLINES[method]` evaluated in
`np.longdouble` on the same rounded inputs.  Each error is scaled by the magnitude its rounding errors live at, not by the result
(`test_reference_interpolation_fixtures_on_the_history_kernels` argues for it: both outputs are sums of history rows divided by knot
spacings, the value multiplied by one spacing afterwards):

    value:       eps(dtype) * max|his| * hmax / hmin          derivative:  eps(dtype) * max|his| / hmin

The bound is what the ORACLE ALONE does: the same classes evaluated in the working dtype against the long-double ones, worst figure
over the grid per method, dtype and output, measured here.  The double must stay within 2 times that: the oracle forms its 2-4
products through a numpy matmul and the double left to right — rounding neighbours, not equal."""
import numpy as np
import pytest
import torch

from oracle import xde_oracle as O

from . import _history_grid as G
from . import problems as P
from ._cpu_double import NumpyDoubleBackend

LONGDOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_double_history_gathers_against_the_long_double_oracle(method, dtype):
    if dtype == np.float64 and not LONGDOUBLE_IS_WIDER:
        pytest.skip("np.longdouble is no wider than float64 on this platform: nothing to compare fp64 with")
    dbl = NumpyDoubleBackend()
    eps = float(np.finfo(dtype).eps)
    worst = {"oracle": [0.0, 0.0], "double": [0.0, 0.0]}  # [value, derivative], in the units above
    at = {"oracle": [None, None], "double": [None, None]}
    cases = 0
    for T in G.t_values(method):
        for uniform in (True, False):
            t = G.knots(T, uniform, dtype)
            h = np.diff(t.astype(np.float64))
            hmin, hmax = float(h.min()), float(h.max())
            for lags in [G.lag_pool(t)] + [G.lags_of_length(t, L, seed=1) for L in G.LAG_COUNTS if L > 0]:
                for D in (3, 64, 250):
                    his = G.history((2,), T, D, dtype)
                    ref = O.HISTORY_SPLINES[method](his, t, dtype=np.longdouble)
                    work = O.HISTORY_SPLINES[method](his, t, dtype=dtype)
                    truth = (ref.evaluate(lags), ref.derivative(lags))
                    assert truth[0].dtype == np.longdouble
                    val = torch.full((2, len(lags), D), float("nan"), dtype=torch.from_numpy(his).dtype)
                    der = torch.full_like(val, float("nan"))
                    dbl.history_gather(val, der, torch.from_numpy(his), torch.from_numpy(t), torch.from_numpy(lags), method)
                    got = {"oracle": (work.evaluate(lags), work.derivative(lags)), "double": (val.numpy(), der.numpy())}
                    amp = float(np.abs(his).max())
                    unit = (eps * amp * hmax / hmin, eps * amp / hmin)
                    for who, outs in got.items():
                        for k in (0, 1):
                            assert outs[k].dtype == dtype and np.isfinite(outs[k]).all(), (who, method, T, uniform, len(lags), D)
                            e = float(np.abs(outs[k].astype(np.longdouble) - truth[k]).max() / unit[k])
                            if e > worst[who][k]:
                                worst[who][k], at[who][k] = e, (T, uniform, len(lags), D)
                    cases += 1
    rec = {"method": method, "dtype": np.dtype(dtype).name, "cases": cases,
           "oracle_value": worst["oracle"][0], "oracle_derivative": worst["oracle"][1],
           "double_value": worst["double"][0], "double_derivative": worst["double"][1],
           "double_worst_at": [list(map(int, a)) if a else None for a in at["double"]]}
    P.report("history_double_vs_longdouble_oracle", rec)
    assert worst["oracle"][0] > 0 and worst["oracle"][1] > 0  # (a bound of zero would mean the comparison saw nothing)
    assert worst["double"][0] <= 2.0 * worst["oracle"][0], rec
    assert worst["double"][1] <= 2.0 * worst["oracle"][1], rec
