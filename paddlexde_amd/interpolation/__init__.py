"""The history splines as objects — the reference's ``paddlexde.interpolation`` classes (interpolation/__init__.py:1:
``LinearInterpolation``, ``CubicHermiteSpline``, ``BezierSpline`` over interpolation/interpolate_base.py:7-107) on the history kernels.

``HistoryIndex`` (xde/base_dde.py:104-121) builds one of these per call and asks it for ``evaluate(lags)`` and ``derivative(lags)``; the
kernels (xde_history_gather / xde_hermite_gather) compute both in one pass over the series, so here the classes are a thin front on that
launch: same constructor (``series [..., T, D]``, ``t [T]`` or None), same ``evaluate(t)`` / ``derivative(t)`` ``-> [..., len(t), D]``,
same conventions as written in the reference (``index = clip(bucketize(t) - 1, 0, T - 1)``, one-sided node derivatives for the cubic,
row scales ``scale1..4``), in the package's default dtype float32 (interpolate_base.py:18,27-28) unless the series is float64.  Held to
the reference's own tests for these classes (tests/interpolation/test_interpolation.py:13-85) in tests/_dde_cases.py.

``NaturalCubicSpline`` is this project's own (the reference has none): the C2 natural cubic spline through the observed entries of a
series on arbitrary strictly increasing knots, NaN meaning "not observed" — the control path of ``cdeint`` for irregularly sampled,
partly observed data (include/xde_hip_spline.h states the path op for op).

``logsig_windows`` / ``logsig_path`` are the log-ODE method's transform of a long series (include/xde_hip_logsig.h): windows of
``window_length`` steps replaced by their depth-1 or depth-2 logsignatures, the path to hand to one of the classes above.
"""
import torch

from .. import _hip

__all__ = ["LinearInterpolation", "CubicHermiteSpline", "BezierSpline", "NaturalCubicSpline", "logsignature_channels", "logsig_windows",
           "logsig_path", "window_times"]


def _gather_buffers(rows, t):
    """What a gather of rows ``[..., T, D]`` at the times ``t`` takes: the query times ``tq [L]`` (detached, contiguous, in the rows'
    dtype on their device) and the empty outputs ``val, der [..., L, D]``."""
    tq = torch.as_tensor(t).detach().to(device=rows.device, dtype=rows.dtype).contiguous().reshape(-1)
    val = torch.empty(tuple(rows.shape[:-2]) + (tq.numel(), rows.shape[-1]), dtype=rows.dtype, device=rows.device)
    return tq, val, torch.empty_like(val)


class InterpolationBase:
    method = None  # "linear" | "cubic" | "bez": the kernels' name of the spline
    min_times = 2

    def __init__(self, series, t=None, differentiable=False, **kwargs):
        be = _hip.get_backend()
        series = torch.as_tensor(series)
        be.require_device(series)
        dtype = series.dtype if series.dtype == torch.float64 else torch.float32  # (`default_type`: float32)
        # differentiable: the spline stays attached to the series' autograd graph, so that a control path of cdeint can come from
        # something that is trained (xde/base_cde.py CdeControlContractFn); the knots never get a gradient
        self.differentiable = bool(differentiable)
        self._series = (series if self.differentiable else series.detach()).to(dtype).contiguous()
        n_times = self._series.shape[-2]
        if n_times < self.min_times:
            raise ValueError("{} needs at least {} time points".format(type(self).__name__, self.min_times))
        if t is None:
            # the reference's default grid is linspace(0, T, T + 1) (:20-25): its first T points are the series' times, the extra one is
            # never indexed (`index` is clipped to T - 1) and its spacing repeats the last one — the unit grid 0..T-1 is the same spline
            t = torch.arange(n_times, dtype=dtype, device=self._series.device)
        self._t = torch.as_tensor(t).detach().to(device=self._series.device, dtype=dtype).contiguous().reshape(-1)
        if self._t.numel() != n_times:
            raise ValueError("t must have one entry per time row of the series ({} != {})".format(self._t.numel(), n_times))
        self._backend = be

    @property
    def grid_points(self):
        """The time points (interpolate_base.py:39-42)."""
        return self._t

    @property
    def interval(self):
        """The time interval between the first and the last time point (:44-47)."""
        return torch.stack([self._t[0], self._t[-1]])

    def _gather(self, t):
        if self.differentiable:
            raise NotImplementedError(
                "{}(differentiable=True): evaluate / derivative are not differentiable; the values at the knots are the series rows "
                "themselves (index the series, e.g. series[..., 0, :] for z0), and cdeint differentiates X'(t) inside its "
                "contraction; NaturalCubicSpline(differentiable=True) has differentiable evaluate / derivative".format(type(self).__name__))
        tq, val, der = _gather_buffers(self._series, t)
        self._backend.history_gather(val, der, self._series, self._t, tq, self.method)
        return val, der

    def evaluate(self, t):
        """The value at the time points ``t`` (:72-90): ``[..., len(t), D]``."""
        return self._gather(t)[0]

    def derivative(self, t):
        """The time derivative at ``t`` (:92-107)."""
        return self._gather(t)[1]


class LinearInterpolation(InterpolationBase):
    """interpolation/interpolate.py:6-99."""

    method = "linear"
    min_times = 2


class CubicHermiteSpline(InterpolationBase):
    """interpolation/interpolate.py:100-204 (node derivatives: one-sided differences, the last one repeated)."""

    method = "cubic"
    min_times = 2


class BezierSpline(InterpolationBase):
    """interpolation/interpolate.py:207-298 (four rows per interval, cubic Bernstein weights)."""

    method = "bez"
    min_times = 4

    def __init__(self, series, t=None, differentiable=False, **kwargs):
        if differentiable:
            raise NotImplementedError("BezierSpline(differentiable=True): a BezierSpline is not a control path of cdeint, and the "
                                      "history gathers give no gradient to the series; LinearInterpolation, CubicHermiteSpline and "
                                      "NaturalCubicSpline take differentiable=True")
        super().__init__(series, t, **kwargs)


class _NaturalCoeffsFn(torch.autograd.Function):
    """``Y, M = xde_spline_natural_coeffs(columns, knots)`` with the gradient to ``columns [B, Tn, C]``: one
    xde_spline_natural_coeffs_backward launch (include/xde_hip_cdegrad.h (b)).  An unobserved entry gets ``+0``; the knots get none."""

    @staticmethod
    def forward(ctx, columns, knots):
        Y, M = torch.empty_like(columns), torch.empty_like(columns)
        _hip.get_backend()._spline_natural_coeffs(Y, M, columns, knots)
        ctx.save_for_backward(columns, knots)
        return Y, M

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gY, gM):
        columns, knots = ctx.saved_tensors
        g = torch.empty_like(columns)
        _hip.get_backend()._spline_natural_coeffs_backward(g, gY.contiguous(), gM.contiguous(), columns, knots)
        return g, None


class _NaturalGatherFn(torch.autograd.Function):
    """``val, der = xde_spline_natural_gather(Y, M, knots, tq)`` with the gradient to ``Y`` and ``M``: one
    xde_spline_natural_gather_backward launch ((c) of the same header) over whichever of the two cotangents arrived."""

    @staticmethod
    def forward(ctx, Y, M, knots, t):
        tq, val, der = _gather_buffers(Y, t)
        _hip.get_backend()._spline_natural_gather(val, der, Y, M, knots, tq)
        ctx.save_for_backward(knots, tq)
        ctx.shape = tuple(Y.shape)
        ctx.set_materialize_grads(False)
        return val, der

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gval, gder):
        if gval is None and gder is None:
            return None, None, None, None
        knots, tq = ctx.saved_tensors
        gY = torch.empty(ctx.shape, dtype=knots.dtype, device=knots.device)
        gM = torch.empty_like(gY)
        cont = lambda g: None if g is None else g.contiguous()  # noqa: E731
        _hip.get_backend()._spline_natural_gather_backward(gY, gM, cont(gval), cont(gder), knots, tq)
        return gY, gM, None, None


class NaturalCubicSpline(InterpolationBase):
    """The natural cubic spline through the observed entries of ``series [..., T, C]`` over strictly increasing ``t [T]`` (any spacing;
    default the unit grid).  A NaN entry is "not observed": each column is interpolated through its own observed points; a NaN at
    the first (last) time takes the column's first (last) observed value, so the path is C2 on the whole ``interval`` and its
    derivative — what ``cdeint`` contracts with — is C1.  A column with no observed value is refused.

    Construction runs one coefficient launch (xde_spline_natural_coeffs) after one host read that checks ``t`` and the columns;
    ``evaluate`` / ``derivative`` are one xde_spline_natural_gather launch, and give the bits the CDE contraction builds on chip.
    ``_series`` holds the values on the full knot grid (missing entries filled from the spline), ``_coef`` the second derivatives.

    ``differentiable=True`` keeps the spline on ``series``' autograd graph (a control path of ``cdeint`` that comes from something
    trained): ``Y`` and ``M`` then carry a gradient back to the observed entries of the series through one
    xde_spline_natural_coeffs_backward launch per backward pass (unobserved entries get ``+0``), and ``evaluate`` / ``derivative`` are
    differentiable through xde_spline_natural_gather_backward (include/xde_hip_cdegrad.h).  The knots get no gradient."""

    method = "natural"
    min_times = 2

    def __init__(self, series, t=None, differentiable=False, **kwargs):
        super().__init__(series, t, differentiable, **kwargs)
        raw = self._series
        columns = raw.reshape((-1,) + tuple(raw.shape[-2:]))
        rising = (self._t[1:] > self._t[:-1]).all()  # (false for a NaN time too)
        empty = torch.isnan(columns.detach()).all(dim=-2).any()
        rising, empty = torch.stack([rising, empty]).tolist()  # the one host read
        if not rising:
            raise ValueError("NaturalCubicSpline: t must be strictly increasing")
        if empty:
            raise ValueError("NaturalCubicSpline: a column of the series has no observed (non-NaN) value: there is nothing to "
                             "interpolate; drop the channel or fill it")
        if self.differentiable:
            # Y and M stay on the series' graph: their cotangents flow back through ONE coefficient-backward launch per backward pass
            Y, M = _NaturalCoeffsFn.apply(columns, self._t)
        else:
            Y, M = torch.empty_like(columns), torch.empty_like(columns)
            self._backend._spline_natural_coeffs(Y, M, columns, self._t)
        self._series = Y.reshape(raw.shape)
        self._coef = M.reshape(raw.shape)

    def _gather(self, t):
        if self.differentiable:
            return _NaturalGatherFn.apply(self._series, self._coef, self._t, torch.as_tensor(t).detach())
        tq, val, der = _gather_buffers(self._series, t)
        self._backend._spline_natural_gather(val, der, self._series, self._coef, self._t, tq)
        return val, der


class LogsigWindowsFn(torch.autograd.Function):
    """``out = xde_logsig_windows(x)`` with the gradient to ``x [B.., T, C]``: one xde_logsig_windows_backward launch
    (include/xde_hip_logsig.h).  The forward saves the series only; an absent cotangent stays absent."""

    @staticmethod
    def forward(ctx, x, window_length, depth):
        T, C = x.shape[-2:]
        out = torch.empty(tuple(x.shape[:-2]) + (-(-(T - 1) // window_length), _hip.logsig_channels(C, depth)), dtype=x.dtype, device=x.device)
        _hip.get_backend()._logsig_windows(out, x, window_length, depth)
        ctx.save_for_backward(x)
        ctx.plan = (window_length, depth)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        if gout is None:
            return None, None, None
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        _hip.get_backend()._logsig_windows_backward(gx, gout.contiguous(), x, *ctx.plan)
        return gx, None, None


def logsignature_channels(channels, depth=2):
    """Channels of a logsignature of ``channels`` channels: ``channels`` at depth 1, ``channels (channels + 1) / 2`` at depth 2."""
    return _hip.logsig_channels(channels, depth)


def _windows_args(series, depth, window_length):
    """What logsig_windows refuses, before the first launch; returns the series (contiguous) and the window length."""
    be = _hip.get_backend()
    if not torch.is_tensor(series) or not series.is_floating_point() or series.dtype not in (torch.float32, torch.float64):
        raise TypeError("logsig_windows: the series must be a float32 or float64 tensor, got {}".format(
            series.dtype if torch.is_tensor(series) else type(series).__name__))
    if series.dim() < 2:
        raise ValueError("logsig_windows: the series is [..., T, C], got shape {}".format(tuple(series.shape)))
    if isinstance(window_length, bool) or int(window_length) != window_length or int(window_length) < 1:
        raise ValueError("logsig_windows: window_length must be an integer >= 1, got {!r}".format(window_length))
    if isinstance(depth, bool) or int(depth) != depth:
        raise ValueError("logsig_windows: depth must be 1 or 2, got {!r}".format(depth))
    _hip.logsig_channels(series.shape[-1], depth)  # (depth and the channel cap)
    if series.shape[-2] < 2:
        raise ValueError("logsig_windows: the series needs at least 2 time points (T >= 2), got T = {}".format(series.shape[-2]))
    be.require_device(series)
    return series.contiguous(), int(window_length)


def logsig_windows(series, depth=2, window_length=1):
    """The logsignatures of the windows of ``window_length`` steps of ``series [..., T, C]``: ``[..., W, K]`` with
    ``W = ceil((T - 1) / window_length)`` (the last window may be shorter) and ``K = logsignature_channels(C, depth)`` — per window its
    increment (the first ``C`` channels) and, at depth 2, its Levy areas ``A_ij = 1/2 * sum_k (u_k[i] D_k[j] - u_k[j] D_k[i])`` for the pairs
    ``i < j`` in lexicographic order (``u_k`` the offset of point k from the window's first point, ``D_k`` step k).  One launch
    (xde_logsig_windows), accumulated in float64 in a fixed order; differentiable with respect to the series through one launch
    (xde_logsig_windows_backward).  A NaN entry poisons its own windows only: fill unobserved entries first."""
    series, window_length = _windows_args(series, depth, window_length)
    return LogsigWindowsFn.apply(series, window_length, int(depth))


def logsig_path(series, depth=2, window_length=1):
    """The control path of the log-ODE method: ``[..., W + 1, K]``, a zero row followed by the cumulative sum of ``logsig_windows`` along
    the window axis.  Hand it to ``LinearInterpolation(path, differentiable=...)`` (its derivative on window w is that window's
    logsignature over the window's length) or ``NaturalCubicSpline(path, t=window_times(t, window_length))``, and that to ``cdeint``
    with ``step_size`` sub-stepping inside the windows.

    THE VECTOR FIELD the path is contracted with has K columns: ``func(t, z)`` returns ``[..., H, K]``.  Its first C columns are the
    fields ``V_c(z)`` of the CDE ``dz = sum_c V_c(z) dX_c`` on the original series.  Column ``pair(i, j)`` (``C + i (2 C - i - 1) / 2 +
    (j - i - 1)``, ``i < j``) is the Lie bracket ``[V_i, V_j](z) = DV_j(z) V_i(z) - DV_i(z) V_j(z)``; for linear fields
    ``V_c(z) = A_c z`` that is ``(A_j A_i - A_i A_j) z``.  With the opposite sign the depth-2 solve is worse than the depth-1 one."""
    inc = logsig_windows(series, depth, window_length)
    return torch.cat([torch.zeros_like(inc[..., :1, :]), torch.cumsum(inc, dim=-2)], dim=-2)


def window_times(t, window_length):
    """The knots of the windows of ``window_length`` steps over the times ``t [T]``: ``t[0], t[L], t[2 L], ..., t[T - 1]``."""
    t = torch.as_tensor(t).reshape(-1)
    if isinstance(window_length, bool) or int(window_length) != window_length or int(window_length) < 1:
        raise ValueError("window_times: window_length must be an integer >= 1, got {!r}".format(window_length))
    if t.numel() < 2:
        raise ValueError("window_times: t needs at least 2 time points")
    idx = list(range(0, t.numel() - 1, int(window_length))) + [t.numel() - 1]
    return t[torch.as_tensor(idx, device=t.device)]
