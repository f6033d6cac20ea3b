"""ReversibleHeun: algebraically reversible steps for Stratonovich SDEs with diagonal noise (FixedSolver._rheun_step) — the scheme
``sdeint_adjoint`` differentiates in constant memory."""
from ..base_fixed_solver import FixedSolver


class ReversibleHeun(FixedSolver):
    """Kidger, Foster, Li and Lyons' reversible Heun method ("Efficient and Accurate Gradients for Neural SDEs", NeurIPS 2021): one
    drift and one diffusion evaluation per step, converging to the STRATONOVICH solution (Euler, Milstein and SRK are Ito) with strong
    order 1 where element i of the diffusion depends on ``y_i`` only (1/2 in general).  The step carries ``(yh, fh, gh)`` besides the
    state; from the state at the end of a step the one before it is recomputed exactly up to rounding, which is what
    ``sdeint_adjoint`` sweeps backwards on."""

    order = 1
    steps_sde = True
    logqp_refusal = "its drift is the mean of two evaluations, one of them carried over from the step before, so the KL term would need the prior drift at both"

    matrix_noise_refusal = "its predict, correct and adjoint kernels are diagonal (general noise for them is a follow-up)"

    time_values = ((1.0, False),)  # dt

    def __init__(self, xde, y0, **kwargs):
        super().__init__(xde, y0, **kwargs)
        if not self._sde:
            raise NotImplementedError("ReversibleHeun steps SDEs only (sdeint, sdeint_adjoint): for an ODE use Midpoint or RK4")

    def step(self, t0, t1, y0):
        dt = self._host_dt(t0, t1)
        (dtt,) = self._times(t0, dt)
        return self._rheun_step(t0, t1, dtt, y0, dt)
