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
from ..xde.base_sde import BaseSDE, check_noise_type


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
    no effect, as in the reference; a decreasing ``t`` integrates backwards with ``dW = sqrt(|dt|) * Z``.

    ``options={"logqp": True, "prior_drift": h}`` (a latent SDE; ``solver=Euler`` or ``Milstein``): returns ``(ys, logqp)``, ``ys`` the
    same path bit for bit and ``logqp[..., i]`` — shape ``y0.shape[:-1] + (T - 1,)``, the state dtype — the KL divergence over
    ``[t[i], t[i+1]]`` between the path's law and that of ``dy = h(t, y) dt + diffusion(t, y) dW``: the scheme's sum of
    ``0.5 * |(drift - h) / diffusion|**2 * dt`` over the last axis, accumulated in float64 by the step launch itself
    (include/xde_hip_kl.h).  ``h(t, y)`` returns a tensor of ``y``'s shape and dtype; ``diffusion`` must be non-zero.  Gradients reach
    ``y0`` and the parameters of all three functions, from ``ys`` and from ``logqp``.

    ``options={"noise_type": "general"}`` (``solver=Euler``): ``diffusion(t, y)`` returns a tensor of shape ``y.shape + (M,)`` and
    ``y``'s dtype, ``M >= 1`` fixed by its first evaluation, and every row of the state (its last axis, D elements) is driven by an
    M-dimensional Brownian motion through its ``[D, M]`` matrix: ``y1 = (y0 + f*dt) + g @ (sqrt(|dt|) * Z)``, Z one normal per row and
    m, the sum over m taken sequentially.  One xde_sde_gn_step launch per step streams ``g`` once and builds the increment on chip; the
    backward is one launch that regenerates Z and keeps nothing of the forward but ``(dt, seed, k)`` (include/xde_hip_gn.h).
    ``"scalar"`` is general noise with ``M == 1`` (``diffusion`` returns ``y.shape + (1,)``); ``"diagonal"``, the default, is the
    element-wise noise described above, unchanged.  Any other value is a ``ValueError``.  Milstein, SRK, ReversibleHeun,
    ``sdeint_adjoint`` and ``logqp`` take diagonal noise only and say so."""
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
    logqp = bool(options.pop("logqp", False))
    prior = options.pop("prior_drift", None)
    noise_type = check_noise_type(options.pop("noise_type", "diagonal"))
    if logqp and prior is None:
        raise ValueError("options['logqp'] needs the prior drift: options={'logqp': True, 'prior_drift': h} with h(t, y) a tensor of y's "
                         "shape and dtype (the KL term is between dy = drift dt + diffusion dW and dy = h dt + diffusion dW)")
    if prior is not None and not logqp:
        raise ValueError("options['prior_drift'] is only read with options['logqp'] = True (sdeint then returns (ys, logqp)); drop it, "
                         "or ask for logqp")

    xde = BaseSDE(f=drift, g=diffusion, y0=y0, t_span=t, reverse=reverse, seed=seed, prior=prior, noise_type=noise_type)

    if logqp:
        options["logqp"] = True  # (refused by the solvers whose step cannot accumulate it, before the first launch)
    s = solver(xde=xde, y0=xde.y0, rtol=rtol, atol=atol, **options)
    solution = s.integrate(t)

    solution = xde.format(solution)

    if logqp:
        return solution, s.logqp
    return solution
