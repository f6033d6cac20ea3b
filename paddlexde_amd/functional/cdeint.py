"""``cdeint`` / ``cdeint_adjoint`` — neural controlled differential equations ``dz = func(t, z) dX(t), z(t[0]) = z0`` (the reference
has the wrapper, paddlexde/xde/base_cde.py, with the control derivative left as a todo, and no entry point).

``X`` is a ``NaturalCubicSpline``, ``CubicHermiteSpline`` or ``LinearInterpolation`` (paddlexde_amd.interpolation) through a time series
``[..., T, C]``;
``func(t, z)`` returns ``[..., H, C]`` for ``z`` of shape ``[..., H]``.  The solve is ``odeint`` / ``odeint_adjoint`` on the vector
field ``CDEField(func, X)`` = ``func(t, z) . X'(t)`` (xde/base_cde.py): same solvers, options, output layouts and adjoint keywords, one
xde_cde_contract launch per function evaluation (include/xde_hip_cde.h; xde_cde_contract_natural of include/xde_hip_spline.h for the
natural spline).  A typical model takes ``z0`` from ``X.evaluate(t0)`` through
a linear layer, and reads the answer off ``z`` at the last time.

``CubicHermiteSpline`` and ``LinearInterpolation`` keep the reference's scale conventions as written; these are exact on a uniform
knot grid (the default ``t=None``) only.  For irregularly sampled data, or a series with missing values (NaN), use
``NaturalCubicSpline``: the C2 natural cubic spline through each column's observed points on arbitrary knots, served by every solver.
"""
import torch

from ..solver.base_fixed_solver import FixedSolver
from ..utils.ode_utils import _rms_norm
from ..xde.base_cde import CDEField, check_cde_problem
from .odeint import odeint
from .odeint_adjoint import odeint_adjoint


def _control_adjoint_params(field, options, adjoint_options, adjoint_params):
    """The adjoint parameters of a solve whose control asks for a gradient (``differentiable=True`` on a series that requires grad):
    ``func``'s parameters (or the explicit ``adjoint_params``) followed by the control's tensors — the series (linear / cubic), ``Y``
    and ``M`` (natural).  They enter ``OdeintAdjointMethod`` as inputs, so the adjoint's vjp differentiates up to them and no further,
    and what lies before them (the coefficient build, an encoder) is differentiated once per backward pass.  None when the control
    asks for nothing.  Refuses what cannot carry the control's adjoint."""
    control = field.control_tensors() if torch.is_grad_enabled() else ()
    if not control:
        return None
    opts = options if isinstance(options, dict) else {}
    aopts = adjoint_options if isinstance(adjoint_options, dict) else {}
    if opts.get("process_group") is not None or aopts.get("process_group") is not None:
        raise NotImplementedError("a differentiable control with process_group: the control's adjoint is per batch row and must not "
                                  "enter the parameter all-reduce; run the sharded solve on a control built with differentiable=False, "
                                  "or an unsharded one")
    if opts.get("backprop") == "steps":
        raise NotImplementedError("a differentiable control with options['backprop'] = 'steps': the recorded steps carry no gradient "
                                  "to the control; use a fixed-step solver (gradients flow through its steps) or the adjoint "
                                  "(the default for an adaptive solver, and cdeint_adjoint)")
    if aopts.get("vjp") is not None:
        raise NotImplementedError("a differentiable control with adjoint_options['vjp'] / AdjointProblem: the caller's "
                                  "vector-Jacobian product does not return the control's cotangent; leave the vjp to torch autograd "
                                  "(drop the key), or build the control with differentiable=False")
    mode = aopts.get("graph_func", "auto")
    if mode is True or isinstance(mode, dict):
        raise NotImplementedError("a differentiable control with adjoint_options['graph_func'] = True: the captured dynamics "
                                  "differentiates func's parameters only; leave it at \"auto\" (the eager dynamics are used) or False")
    params = tuple(field.parameters()) if adjoint_params is None else tuple(adjoint_params)
    return params + tuple(control)


def cdeint(func, X, z0, t_span, solver, *, rtol=1e-7, atol=1e-9, options={"norm": _rms_norm}):
    """Integrate ``dz = func(t, z) dX(t), z(t_span[0]) = z0`` and return z at every ``t_span`` point, in odeint's layout for
    ``solver``.  Gradients reach ``z0`` and ``func``'s parameters as they do in ``odeint`` (through the steps of a fixed solver; an
    adaptive solver is served by the adjoint) — and the series of a control built with ``differentiable=True``, by the same two routes
    (with such a control ``process_group`` and ``options["backprop"] = "steps"`` are refused).

    Refused: a ``BezierSpline``; a ``LinearInterpolation`` with an adaptive solver (its derivative jumps at every knot: use
    ``CubicHermiteSpline`` or ``NaturalCubicSpline``, or a fixed-step solver with the knots on its grid); a series whose dtype or leading dimensions differ from
    ``z0``'s; a ``t_span`` that leaves ``X.interval`` or requires grad; a tuple ``z0``."""
    t_span = check_cde_problem(X, z0, t_span, solver)
    field = CDEField(func, X)
    params = _control_adjoint_params(field, options, None, None)
    if params is not None and not (isinstance(solver, type) and issubclass(solver, FixedSolver)):
        # an adaptive solve whose control asks for a gradient is served by the adjoint, with the control among its parameters (a fixed
        # solver carries the gradient through its recorded steps: nothing to do)
        options = {k: v for k, v in options.items() if k != "backprop"}
        return odeint_adjoint(field, z0, t_span, rtol=rtol, atol=atol, solver=solver, options=options, adjoint_params=params)
    return odeint(field, z0, t_span, solver, rtol=rtol, atol=atol, options=options)


def cdeint_adjoint(func, X, z0, t_span, *, rtol=1e-7, atol=1e-9, solver=None, options={"norm": _rms_norm}, event_fn=None,
                   adjoint_rtol=None, adjoint_atol=None, adjoint_solver=None, adjoint_options=None, adjoint_params=None):
    """``cdeint`` with the continuous adjoint: ``odeint_adjoint`` on ``CDEField(func, X)``, with its keywords.  ``adjoint_params``
    defaults to ``func``'s parameters when ``func`` is a module; pass them for a plain callable.

    A control built with ``differentiable=True`` on a series that requires grad gets its gradient too: its tensors (the series; ``Y``
    and ``M`` of a natural spline) are appended to the adjoint parameters, so the augmented state grows by ``B Tn C`` (``2 B Tn C``)
    elements, which the adjoint's error norm sees.  Refused with such a control: ``process_group``, ``adjoint_options["vjp"]``, an
    explicit ``adjoint_options["graph_func"] = True`` ("auto" takes the eager dynamics)."""
    adj_solver = adjoint_solver if adjoint_solver is not None else solver
    t_span = check_cde_problem(X, z0, t_span, solver)
    if adj_solver is not solver:
        check_cde_problem(X, z0, t_span, adj_solver)
    field = CDEField(func, X)
    params = _control_adjoint_params(field, options, adjoint_options, adjoint_params)
    if params is not None:
        adjoint_params = params
    return odeint_adjoint(field, z0, t_span, rtol=rtol, atol=atol, solver=solver, options=options, event_fn=event_fn,
                          adjoint_rtol=adjoint_rtol, adjoint_atol=adjoint_atol, adjoint_solver=adjoint_solver,
                          adjoint_options=adjoint_options, adjoint_params=adjoint_params)
