"""What cdeint's contraction computes, written from include/xde_hip_cde.h and the oracle's spline classes
(oracle.xde_oracle.HISTORY_SPLINES), not from the kernel: the float64 contraction of F with the control spline's ``derivative``."""
import numpy as np

from oracle import xde_oracle as O


def control(series, knots, method, dtype):
    """The oracle's spline through ``series [..., T, C]`` over ``knots [T]``, computing in ``dtype``."""
    return O.HISTORY_SPLINES[method](np.asarray(series), np.asarray(knots), dtype=dtype)


def dX(series, knots, t, method, dtype):
    """``X'(t) [..., C]`` of the oracle's spline (the time converted to ``dtype`` first, as the spline does)."""
    return control(series, knots, method, dtype).derivative(np.asarray(t).reshape(-1)[:1])[..., 0, :]


def contract(F, series, knots, t, method, dtype):
    """``out[..., h] = sum_c F[..., h, c] * X'(t)[..., c]`` in float64."""
    return np.einsum("...hc,...c->...h", np.asarray(F, dtype=np.float64), np.asarray(dX(series, knots, t, method, dtype), dtype=np.float64))


def contract_backward(gout, series, knots, t, method, dtype):
    """``gF[..., h, c] = gout[..., h] * X'(t)[..., c]`` in float64."""
    return np.asarray(gout, dtype=np.float64)[..., :, None] * np.asarray(dX(series, knots, t, method, dtype), dtype=np.float64)[..., None, :]


def gamma(C, dtype):
    """The standard bound of a length-C inner product in any summation order: |err| <= gamma_C * sum_c |F * dX|."""
    u = 2.0**-24 if np.dtype(dtype) == np.float32 else 2.0**-53
    return C * u / (1.0 - C * u)
