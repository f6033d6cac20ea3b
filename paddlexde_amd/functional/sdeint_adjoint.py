"""Adjoint of the stochastic-equation caller.

The reference's ``sdeint_adjoint`` is a copy of ``odeint_adjoint`` that calls ``sdeint`` with arguments it does not take, so it never
ran.  The name is kept so that ``from paddlexde_amd.functional import sdeint_adjoint`` works (example/sde_demo.py imports it behind
``--adjoint``), and the call fails with a pointer to what does work: back-propagating through ``sdeint(..., solver=Euler)``
(discretise-then-optimise), which reaches y0 and the parameters of both drift and diffusion.
"""

_MESSAGE = (
    "sdeint_adjoint is not implemented (the stochastic adjoint needs a Brownian path that can be queried backwards in time); "
    "differentiate through sdeint(..., solver=Euler) or sdeint(..., solver=Milstein) or SRK instead"
)


def sdeint_adjoint(*args, **kwargs):
    raise NotImplementedError(_MESSAGE)
