"""Euler (reference: paddlexde/solver/fixed_solver/euler.py:4-11).  Under sdeint it is Euler-Maruyama and reads the equation in the Ito sense,
as Milstein and SRK do; ReversibleHeun is the one Stratonovich solver."""
from ... import _hip
from ..base_fixed_solver import FixedSolver


class Euler(FixedSolver):
    order = 1
    steps_sde = True  # a BaseSDE is stepped as Ito Euler-Maruyama (FixedSolver._em_step)
    steps_logqp = True  # ... and with logqp by the fused step + KL launch (FixedSolver._kl_em_step)
    steps_matrix_noise = True  # ... and under general or scalar noise by xde_sde_gn_step, in the same place

    time_values = ((1.0, False),)  # dt

    def step(self, t0, t1, y0):
        dt = self._host_dt(t0, t1)
        (dtt,) = self._times(t0, dt)
        if self._sde:
            return self._em_step(t0, dtt, y0, dt)
        dy = self._f(t0, dtt, y0)
        y1 = self._combine(y0, [dy], [1.0], _hip.COMBINE_FUSE, dt, out=self._y1_out)
        return y1, dy
