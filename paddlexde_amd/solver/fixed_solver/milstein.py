"""Milstein: strong order 1.0 steps for Ito SDEs with diagonal noise (the derivative-free form; FixedSolver._milstein_step).  Ito, as Euler and SRK under
sdeint; ReversibleHeun is the one Stratonovich solver."""
from ..base_fixed_solver import FixedSolver


class Milstein(FixedSolver):
    order = 1
    steps_sde = True
    steps_logqp = True  # (its two launches, and one accumulate-only launch: FixedSolver._kl_accumulate)

    time_values = ((1.0, False),)  # dt

    def __init__(self, xde, y0, **kwargs):
        super().__init__(xde, y0, **kwargs)
        if not self._sde:
            raise NotImplementedError("Milstein steps SDEs only (sdeint): Milstein of an ODE is Euler; use Euler")

    def step(self, t0, t1, y0):
        dt = self._host_dt(t0, t1)
        (dtt,) = self._times(t0, dt)
        return self._milstein_step(t0, dtt, y0, dt)
