"""Heun: the stochastic trapezoidal rule for Stratonovich SDEs, under diagonal, general and scalar noise (FixedSolver._heun_step)."""
from ..base_fixed_solver import FixedSolver


class Heun(FixedSolver):
    """The Heun (predictor-corrector trapezoidal) scheme: ``yp = y0 + f0 dt + g0 dW``, then
    ``y1 = y0 + (f0 + f(t1, yp)) dt/2 + (g0 + g(t1, yp)) dW/2``.  It converges to the STRATONOVICH solution (Euler, Milstein and SRK are
    Ito) with strong order 1 for commutative noise and 1/2 in general, and it is the one Stratonovich scheme that steps general and
    scalar noise: there the predictor launch keeps its product ``g0 dW`` for the corrector, so a step streams the ``[rows, D, M]``
    diffusion twice, not three times (include/xde_hip_gn.h).  Two drift and two diffusion evaluations and two launches per step."""

    order = 1
    steps_sde = True
    steps_matrix_noise = True
    logqp_refusal = ("its drift is the mean of the evaluations at both ends of the step, so the KL term would need the prior drift at both; "
                     "Euler and Milstein accumulate the KL term")

    time_values = ((1.0, False),)  # dt

    def __init__(self, xde, y0, **kwargs):
        super().__init__(xde, y0, **kwargs)
        if not self._sde:
            raise NotImplementedError("Heun steps SDEs only (sdeint): for an ODE use Midpoint or RK4")

    def step(self, t0, t1, y0):
        dt = self._host_dt(t0, t1)
        (dtt,) = self._times(t0, dt)
        return self._heun_step(t0, t1, dtt, y0, dt)
