"""Controlled differential equations ``dz = F(t, z) dX(t)`` (reference: paddlexde/xde/base_cde.py, whose ``move`` is a stub: "todo:
differentiate the handled data, compute control_gradient").

A CDE driven by a spline ``X`` through a time series is the ODE ``dz/dt = F(t, z) . X'(t)``: ``CDEField`` is that vector field as a
module, ``BaseCDE`` the problem wrapper over it, and every solver, pipeline and adjoint of the ODE path serves it unchanged.  The one
operation a CDE adds, per function evaluation, is the batched contraction ``out[b, h] = sum_c F[b, h, c] * X'(t)[b, c]`` (and on the way
back the outer product ``gF[b, h, c] = gout[b, h] * X'(t)[b, c]``): one launch each of xde_cde_contract / xde_cde_contract_backward
(include/xde_hip_cde.h), which build ``X'(t)`` on chip from the series with the device functions of the history gathers — the bits
``X.derivative(t)`` returns — and never write it out.

The control path.  ``NaturalCubicSpline`` (this project's own: xde_cde_contract_natural / _backward, include/xde_hip_spline.h) is the
C2 natural cubic spline through the observed entries of the series on arbitrary knots — NaN means "not observed" — so ``X'(t)`` is C1
and every solver serves it: the control for irregularly sampled or partly observed data.  ``CubicHermiteSpline`` (one-sided node
differences: the reference's) has a continuous derivative and works with every solver.  ``LinearInterpolation`` has a derivative that
jumps at every knot: fixed-step solvers with the knots on their grid integrate it, adaptive ones are refused.  ``BezierSpline`` is
refused: its sliding four-row window is not a path through the data.  ``CubicHermiteSpline`` and ``LinearInterpolation`` keep the
reference's scale conventions as written; these are exact on a uniform knot grid — the default ``t=None`` — only: for irregularly
sampled data use ``NaturalCubicSpline``.
"""
import torch

from .. import _hip
from ..interpolation import BezierSpline, CubicHermiteSpline, InterpolationBase, LinearInterpolation, NaturalCubicSpline
from .base_ode import BaseODE

__all__ = ["BaseCDE", "CDEField", "CdeContractFn", "CdeControlContractFn"]


# The natural control has entry points of its own (its rows are ``Y`` and ``M``); every other control names its method.  Each kind of
# launch makes that choice in one place: the contraction in the nodes' one forward, its cotangent in ``_launch_contract_backward``, the
# control's cotangent in ``CdeControlContractFn.backward``.
def _contract_forward(ctx, F, series, knots, t, method, coef, keep_F):
    """The forward of both nodes: the launch, and what the backward needs — the control's tensors, ``t`` (saved when it is a tensor),
    ``F``'s shape, and ``F`` itself only with ``keep_F`` (the node that differentiates the control)."""
    be = _hip.get_backend()
    F = F.contiguous()
    out = torch.empty(F.shape[:2], dtype=F.dtype, device=F.device)  # (torch's allocator: capture-safe)
    if method == "natural":
        be._cde_contract_natural(out, F, series, coef, knots, t)
    else:
        be._cde_contract(out, F, series, knots, t, method)
    ctx.method, ctx.t_host = method, None if torch.is_tensor(t) else t
    ctx.f_shape = F.shape
    ctx.save_for_backward(series, knots, *([coef] if method == "natural" else []), *([t] if torch.is_tensor(t) else []),
                          *([F] if keep_F else []))
    return out


def _contract_saved(ctx):
    """``series, coef, knots, t, F`` as the forward left them (``coef`` and ``F`` None where they were not saved)."""
    series, knots, *rest = ctx.saved_tensors
    coef = rest.pop(0) if ctx.method == "natural" else None
    t = rest.pop(0) if ctx.t_host is None else ctx.t_host
    return series, coef, knots, t, rest[0] if rest else None


def _launch_contract_backward(gF, gout, series, coef, knots, t, method):
    be = _hip.get_backend()
    if method == "natural":
        be._cde_contract_natural_backward(gF, gout, series, coef, knots, t)
    else:
        be._cde_contract_backward(gF, gout, series, knots, t, method)


class CdeContractFn(torch.autograd.Function):
    """``out[b, h] = sum_c F[b, h, c] * X'(t)[b, c]`` for contiguous ``F [B, H, C]``, ``series [B, Tn, C]``, ``knots [Tn]`` and ``t`` a
    one-element device tensor (read by the kernel: no synchronisation, so a captured call replays with the element's current value) or
    a Python number.  With ``method`` "natural", ``series`` is the spline's ``Y`` and ``coef [B, Tn, C]`` its second derivatives ``M``.
    Gradient to ``F`` only — the contraction is linear in it, so ``F`` is not kept; the series, the coefficients, the knots and ``t``
    get none."""

    @staticmethod
    def forward(ctx, F, series, knots, t, method, coef=None):
        return _contract_forward(ctx, F, series, knots, t, method, coef, False)

    @staticmethod
    def backward(ctx, gout):
        series, coef, knots, t, _ = _contract_saved(ctx)
        gout = gout.contiguous()
        gF = torch.empty(ctx.f_shape, dtype=gout.dtype, device=gout.device)
        _launch_contract_backward(gF, gout, series, coef, knots, t, ctx.method)
        return gF, None, None, None, None, None


class CdeControlContractFn(torch.autograd.Function):
    """``CdeContractFn`` for a control that opted in with ``differentiable=True``: the same two launches give ``out`` and ``gF`` (the
    same bits), and the control gets its cotangent too — ``gdX[b, c] = sum_h gout[b, h] F[b, h, c]`` scattered to the rows ``X'(t)``
    read, one xde_cde_control_grad / _natural launch (include/xde_hip_cdegrad.h (a)) that runs only when the series (``Y`` and ``M``
    for the natural control) asks for a gradient.  ``F`` is kept for it.  The knots and ``t`` get none."""

    @staticmethod
    def forward(ctx, F, series, knots, t, method, coef=None):
        return _contract_forward(ctx, F, series, knots, t, method, coef, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        series, coef, knots, t, F = _contract_saved(ctx)
        gout = gout.contiguous()
        gF = g_series = g_coef = None
        if ctx.needs_input_grad[0]:
            gF = torch.empty_like(F)
            _launch_contract_backward(gF, gout, series, coef, knots, t, ctx.method)
        if ctx.needs_input_grad[1] or (coef is not None and ctx.needs_input_grad[5]):
            g_series = torch.empty_like(series)  # (every element is written by the launch: no memset)
            if coef is not None:
                g_coef = torch.empty_like(coef)
                _hip.get_backend()._cde_control_grad_natural(g_series, g_coef, gout, F, knots, t)
            else:
                _hip.get_backend()._cde_control_grad(g_series, gout, F, knots, t, ctx.method)
        return gF, g_series, None, None, None, g_coef


def _kernel_time(t, series):
    """``t`` as the kernels take it: one float32 / float64 element on the series' device, else a Python number."""
    if not torch.is_tensor(t):
        return float(t)
    if t.numel() != 1:
        raise ValueError("CDEField: t must hold one time, got shape {}".format(tuple(t.shape)))
    t = t.detach()
    if t.device != series.device:
        return float(t)  # (a host time: a number for the launch, nothing to read on the device)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t


class CDEField(torch.nn.Module):
    """The vector field ``(t, z) -> func(t, z) . X'(t)`` of the CDE ``dz = func(t, z) dX(t)``.

    ``func(t, z)`` returns ``[..., H, C]`` for ``z`` of shape ``[..., H]``, in ``z``'s dtype on ``z``'s device; ``X`` is a
    ``NaturalCubicSpline``, ``CubicHermiteSpline`` or ``LinearInterpolation`` over a series ``[..., T, C]`` with the same leading dimensions (flattened to one
    batch dimension for the kernel).  ``func`` is a submodule when it is a module, so its parameters are this module's."""

    def __init__(self, func, X):
        super().__init__()
        if isinstance(X, BezierSpline):
            raise NotImplementedError("a BezierSpline is not a control path: its sliding four-row window does not pass through the "
                                      "data; use CubicHermiteSpline (or LinearInterpolation with a fixed-step solver), or NaturalCubicSpline for "
                                      "irregularly sampled or partly observed data")
        if not isinstance(X, (LinearInterpolation, CubicHermiteSpline, NaturalCubicSpline)):
            raise TypeError("X must be a paddlexde_amd.interpolation CubicHermiteSpline or LinearInterpolation, or NaturalCubicSpline, got {}".format(
                type(X).__name__ if isinstance(X, InterpolationBase) else type(X)))
        self.func = func
        d = self.__dict__
        d["X"] = X
        series = X._series
        d["_lead"] = tuple(series.shape[:-2])
        d["_series"] = series.reshape((-1,) + tuple(series.shape[-2:]))
        d["_knots"] = X._t
        d["_method"] = X.method
        d["_coef"] = X._coef.reshape(d["_series"].shape) if isinstance(X, NaturalCubicSpline) else None
        # a control built with differentiable=True goes through CdeControlContractFn; every other one through CdeContractFn, as before
        d["_contract"] = CdeControlContractFn if getattr(X, "differentiable", False) else CdeContractFn

    def control_tensors(self):
        """The tensors of a differentiable control that ask for a gradient, as the contraction takes them: the series (linear /
        cubic), ``Y`` and ``M`` (natural).  ``cdeint_adjoint`` appends them to the adjoint parameters.  Empty for any other control."""
        if self._contract is not CdeControlContractFn:
            return ()
        return tuple(x for x in (self._series, self._coef) if x is not None and x.requires_grad)

    def forward(self, t, z):
        F = self.func(t, z)
        series = self._series
        C = series.shape[-1]
        if not torch.is_tensor(F) or F.dim() != z.dim() + 1 or tuple(F.shape[:-1]) != tuple(z.shape) or F.shape[-1] != C:
            raise ValueError("func(t, z) must return [..., H, C] = {} for z of shape {} and a control of {} channels, got {}".format(
                tuple(z.shape) + (C,), tuple(z.shape), C, tuple(F.shape) if torch.is_tensor(F) else type(F)))
        if F.dtype != z.dtype or F.device != z.device:
            raise ValueError("func(t, z) must return z's dtype on z's device ({}, {}), got {}, {}".format(z.dtype, z.device, F.dtype, F.device))
        if F.dtype != series.dtype:
            raise ValueError("the control's series is {} and the state is {}: build X from a series of the state's dtype".format(
                series.dtype, F.dtype))
        if tuple(z.shape[:-1]) != self._lead:
            raise ValueError("z has leading dimensions {} and the control's series {}: they must be the same".format(
                tuple(z.shape[:-1]), self._lead))
        H = z.shape[-1]
        out = self._contract.apply(F.reshape(-1, H, C), series, self._knots, _kernel_time(t, series), self._method, self._coef)
        return out.reshape(z.shape)


def check_cde_problem(X, z0, t_span, solver):
    """What cdeint refuses before anything runs (one host read: ``t_span`` against ``X.interval``).  Returns ``t_span`` as a tensor."""
    from ..solver.base_fixed_solver import FixedSolver

    if isinstance(z0, (tuple, list)):
        raise NotImplementedError("cdeint takes a tensor z0, not a tuple: stack the members into one state tensor [..., H]")
    if isinstance(X, BezierSpline):
        raise NotImplementedError("a BezierSpline is not a control path: its sliding four-row window does not pass through the "
                                  "data; use CubicHermiteSpline (or LinearInterpolation with a fixed-step solver), or NaturalCubicSpline for "
                                      "irregularly sampled or partly observed data")
    if not isinstance(X, (LinearInterpolation, CubicHermiteSpline, NaturalCubicSpline)):
        raise TypeError("X must be a paddlexde_amd.interpolation CubicHermiteSpline or LinearInterpolation, or NaturalCubicSpline, got {}".format(
            type(X)))
    fixed = isinstance(solver, type) and issubclass(solver, FixedSolver)
    if isinstance(X, LinearInterpolation) and not fixed:
        raise NotImplementedError("LinearInterpolation with an adaptive solver: the control's derivative jumps at every knot and the "
                                  "adaptive solvers do not take jump times (jump_t), so the step size underflows at tight tolerances; "
                                  "use CubicHermiteSpline, whose derivative is continuous, or a fixed-step solver with the knots on "
                                  "its grid (or NaturalCubicSpline, which is C2)")
    if not torch.is_tensor(t_span):
        t_span = torch.as_tensor(t_span)
    if torch.is_grad_enabled() and t_span.requires_grad:
        raise NotImplementedError("cdeint gives no gradient with respect to t_span; detach it (gradients reach z0 and the parameters "
                                  "of func)")
    if z0.dim() < 1:
        raise ValueError("z0 must be [..., H], got a 0-dim tensor")
    if X._series.dtype != z0.dtype:
        raise ValueError("the control's series is {} and z0 is {}: build X from a series of z0's dtype".format(X._series.dtype, z0.dtype))
    if tuple(X._series.shape[:-2]) != tuple(z0.shape[:-1]):
        raise ValueError("z0 has leading dimensions {} and the control's series {}: they must be the same".format(
            tuple(z0.shape[:-1]), tuple(X._series.shape[:-2])))
    if t_span.numel():
        ts = t_span.detach().to(device=X._t.device, dtype=torch.float64)
        lo, hi, first, last = torch.stack([ts.min(), ts.max(), X._t[0].to(torch.float64), X._t[-1].to(torch.float64)]).tolist()
        if lo < first or hi > last:
            raise ValueError("t_span [{}, {}] leaves the control's interval X.interval = [{}, {}]: the spline does not extrapolate".format(
                lo, hi, first, last))
    return t_span


class BaseCDE(BaseODE):
    """The CDE problem wrapper: ``BaseODE`` over ``CDEField(func, X)`` (``fuse`` is BaseODE's, so the solvers map it onto the same
    kernels)."""

    def __init__(self, func, X, y0, t_span):
        super().__init__(CDEField(func, X), y0=y0, t_span=t_span)
        self.__dict__["name"] = "CDE"
