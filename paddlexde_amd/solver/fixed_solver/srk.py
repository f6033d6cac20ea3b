"""SRK: strong order 1.5 steps for Ito SDEs with diagonal noise (Roessler's derivative-free SRI1W1; FixedSolver._srk_step).  Ito, as
Euler and Milstein under sdeint; ReversibleHeun is the one Stratonovich solver."""
from ..base_fixed_solver import FixedSolver


class SRK(FixedSolver):
    """``nfe`` counts one per step, as Euler's and Milstein's do; here that stands for 2 drift and 4 diffusion evaluations."""

    order = 1.5
    steps_sde = True
    logqp_refusal = "its drift is a two-stage mean, so the KL term would need the prior drift at the second stage as well"

    time_values = ((1.0, False), (0.75, True), (0.25, True))  # dt, t0 + 3/4 dt, t0 + 1/4 dt

    def __init__(self, xde, y0, **kwargs):
        super().__init__(xde, y0, **kwargs)
        if not self._sde:
            raise NotImplementedError("SRK steps SDEs only (sdeint): its tableau is built on the Brownian increment; use Euler, RK4 "
                                      "or an adaptive solver for an ODE")

    def step(self, t0, t1, y0):
        dt = self._host_dt(t0, t1)
        dtt, t34, t14 = self._times(t0, dt)
        return self._srk_step(t0, t1, dtt, t34, t14, y0, dt)
