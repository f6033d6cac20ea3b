"""``sdeint`` — stochastic differential equations (reference: paddlexde/functional/sdeint.py:9-36, example/sde_demo.py).

Same signature as the reference.  ``dy = drift(t, y) dt + diffusion(t, y) dW`` with diagonal noise (``diffusion`` returns a tensor of
``y``'s shape and dtype), integrated by Ito Euler-Maruyama with ``solver=Euler`` (strong order 1/2: one xde_sde_em_step launch per step)
or by the derivative-free Milstein scheme with ``solver=Milstein`` (strong order 1: a support launch, a second evaluation of
``diffusion`` and one xde_sde_milstein_step launch per step; element i of ``diffusion`` must depend on ``y_i`` only) or by the
derivative-free stochastic Runge-Kutta scheme SRI1W1 with ``solver=SRK`` (strong order 1.5 under the same contract: three launches, 2
``drift`` and 4 ``diffusion`` evaluations per step, on two in-kernel draws) — these three read the equation in the ITO sense — or by
the reversible Heun scheme with ``solver=ReversibleHeun``, which reads it in the STRATONOVICH sense (strong order 1 under the same
contract, 1/2 in general: two launches, one ``drift`` and one ``diffusion`` evaluation per step; the scheme ``sdeint_adjoint``
differentiates in memory that does not grow with the number of steps), the Brownian
increment ``sqrt(|dt|) * Z`` generated inside the kernel (include/xde_hip_sde.h).  The reference's version never ran (its ``fuse`` is a
TODO and it calls an ``xde.format`` that does not exist); this is the step it meant.  The result has odeint's fixed-solver layout
``[..., T*L, D]``.  Gradients with respect to y0 and the parameters of ``drift`` and ``diffusion`` flow through the steps (the autograd
graph keeps every step's operands; ``sdeint_adjoint(..., solver=ReversibleHeun)`` gives the same gradients without keeping them).
"""
from typing import Union

import torch

from ..solver.base_fixed_solver import FixedSolver
from ..utils.ode_utils import _rms_norm
from ..xde.base_sde import BaseSDE


def sdeint(
    drift: callable,
    diffusion: callable,
    y0: Union[tuple, torch.Tensor],
    t,
    solver,
    *,
    rtol=1e-7,
    atol=1e-9,
    reverse=False,
    options: object = {"norm": _rms_norm},
):
    """Integrate ``dy = drift(t, y) dt + diffusion(t, y) dW, y(t[0]) = y0`` and return one sample path at every ``t`` point.

    ``options["seed"]`` (an int, 0 <= seed < 2**64) fixes the Brownian path; without it the seed is drawn from torch's default CPU
    generator, so ``torch.manual_seed`` makes a run repeatable.  The other options are the fixed solvers' (``step_size`` /
    ``grid_constructor`` sub-stepping with ``interp="linear"``, ``pipeline`` "auto" or "sync").  ``reverse`` is accepted and has
    no effect, as in the reference; a decreasing ``t`` integrates backwards with ``dW = sqrt(|dt|) * Z``."""
    if isinstance(y0, (tuple, list)):
        raise NotImplementedError("sdeint takes a tensor y0, not a tuple: stack the members into one state tensor")
    if not (isinstance(solver, type) and issubclass(solver, FixedSolver)):
        raise NotImplementedError("sdeint steps with a fixed-step solver (solver=Euler, Euler-Maruyama, or solver=Milstein or SRK, or ReversibleHeun): adaptive steps would need "
                                  "a Brownian path that can be queried on any interval, which this library does not build")
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError("sdeint gives no gradient with respect to t; detach t (gradients reach y0 and the parameters "
                                  "of drift and diffusion)")
    options = dict(options)
    seed = options.pop("seed", None)

    xde = BaseSDE(f=drift, g=diffusion, y0=y0, t_span=t, reverse=reverse, seed=seed)

    s = solver(xde=xde, y0=xde.y0, rtol=rtol, atol=atol, **options)
    solution = s.integrate(t)

    solution = xde.format(solution)

    return solution
