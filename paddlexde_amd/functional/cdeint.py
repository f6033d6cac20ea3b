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
from ..utils.ode_utils import _rms_norm
from ..xde.base_cde import CDEField, check_cde_problem
from .odeint import odeint
from .odeint_adjoint import odeint_adjoint


def cdeint(func, X, z0, t_span, solver, *, rtol=1e-7, atol=1e-9, options={"norm": _rms_norm}):
    """Integrate ``dz = func(t, z) dX(t), z(t_span[0]) = z0`` and return z at every ``t_span`` point, in odeint's layout for
    ``solver``.  Gradients reach ``z0`` and ``func``'s parameters as they do in ``odeint`` (through the steps of a fixed solver; an
    adaptive solver is served by the adjoint).

    Refused: a ``BezierSpline``; a ``LinearInterpolation`` with an adaptive solver (its derivative jumps at every knot: use
    ``CubicHermiteSpline`` or ``NaturalCubicSpline``, or a fixed-step solver with the knots on its grid); a series whose dtype or leading dimensions differ from
    ``z0``'s; a ``t_span`` that leaves ``X.interval`` or requires grad; a tuple ``z0``."""
    t_span = check_cde_problem(X, z0, t_span, solver)
    return odeint(CDEField(func, X), z0, t_span, solver, rtol=rtol, atol=atol, options=options)


def cdeint_adjoint(func, X, z0, t_span, *, rtol=1e-7, atol=1e-9, solver=None, options={"norm": _rms_norm}, event_fn=None,
                   adjoint_rtol=None, adjoint_atol=None, adjoint_solver=None, adjoint_options=None, adjoint_params=None):
    """``cdeint`` with the continuous adjoint: ``odeint_adjoint`` on ``CDEField(func, X)``, with its keywords.  ``adjoint_params``
    defaults to ``func``'s parameters when ``func`` is a module; pass them for a plain callable."""
    adj_solver = adjoint_solver if adjoint_solver is not None else solver
    t_span = check_cde_problem(X, z0, t_span, solver)
    if adj_solver is not solver:
        check_cde_problem(X, z0, t_span, adj_solver)
    return odeint_adjoint(CDEField(func, X), z0, t_span, rtol=rtol, atol=atol, solver=solver, options=options, event_fn=event_fn,
                          adjoint_rtol=adjoint_rtol, adjoint_atol=adjoint_atol, adjoint_solver=adjoint_solver,
                          adjoint_options=adjoint_options, adjoint_params=adjoint_params)
