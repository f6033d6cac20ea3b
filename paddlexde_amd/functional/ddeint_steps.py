"""``ddeint_steps`` — delay differential equations whose delays reach into the solution being computed:

    y'(t) = func(t, y(t), [y(t - lags[0]), ..., y(t - lags[L-1])]),    y(t) = the initial function for t <= t_span[0].

``ddeint`` mirrors the reference: it gathers the delayed states ONCE from the given history and then solves an ODE with a constant
extra input.  Here the window moves with ``t``: every stage of every step reads ``y(s - lags[j])`` from a tape of the initial
function's samples followed by the solver's own steps, through a cubic Hermite interpolant evaluated for all delays in one launch
(include/xde_hip_dde.h, xde/steps_dde.py).  Gradients flow through the steps, as in ``ddeint``: into ``func``'s parameters, the state
``y0 = his[..., -1:, :]`` and the delays; the other history rows receive none.
"""
import numpy as np
import torch

from ..solver import RK4, Euler, Midpoint
from ..solver._common import t_span_to_host
from ..solver.base_fixed_solver import FixedSolver, _one_third, _two_thirds
from ..utils.ode_utils import _rms_norm
from ..xde.steps_dde import StepsDDE

# per served solver: the multiples of the step at which its stages evaluate func, in evaluation order (the solver's time_values)
_STAGES = {Euler: (0.0,), Midpoint: (0.0, 0.5), RK4: (0.0, _one_third, _two_thirds, 1.0)}
_STAGES_RK4_CLASSIC = (0.0, 0.5, 0.5, 1.0)
_MAX_LAGS = 2048  # (the delay gradient's reduction launch takes up to 2048 delays)


def _host64(x):
    """One device-to-host read of a small 1-D tensor, as float64."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    return x.detach().to("cpu", torch.float64).numpy(), x


def _problem(func, his, his_span, t_span, lags, solver, his_derivative, options, rtol=1e-7, atol=1e-9):
    """Validates the call, builds the wrapper and the solver and plans the whole walk — nothing is launched.  Returns
    ``(xde, solver, walk_args)``: ``solver._walk(*walk_args)`` is the solve."""
    if isinstance(his, (tuple, list)):
        raise NotImplementedError("ddeint_steps takes a tensor history [..., Th, D], not a tuple: stack the members into one state tensor")
    if not (isinstance(solver, type) and solver in _STAGES):
        name = getattr(solver, "__name__", repr(solver))
        raise NotImplementedError("ddeint_steps does not step with {}: the tape needs a fixed grid known before the solve and one-step "
                                  "schemes (AdamsBashforthMoulton keeps a history of its own, adaptive solvers choose their steps on the "
                                  "device); use solver=Euler, Midpoint or RK4".format(name))
    options = dict(options) if options is not None else {}
    options.setdefault("norm", _rms_norm)
    interp = options.setdefault("interp", "linear")
    if interp != "linear":
        raise NotImplementedError("ddeint_steps: interp={!r} is not served: a cubic output row needs the derivative at the end of a step, an "
                                  "extra evaluation outside the plan; use interp='linear'".format(interp))
    if options.get("pipeline", "auto") == "graph":
        raise NotImplementedError("ddeint_steps: pipeline='graph' replays one captured step, but every stage here reads other tape nodes with "
                                  "other weights; use pipeline='sync' (or the default 'auto', which keeps the eager loop)")
    if not torch.is_tensor(his) or his.dim() < 2 or his.dtype not in (torch.float32, torch.float64):
        raise ValueError("ddeint_steps: his must be a float32 or float64 tensor [..., Th, D], got {}".format(
            "{} {}".format(tuple(his.shape), his.dtype) if torch.is_tensor(his) else type(his).__name__))
    Th = his.shape[-2]
    if Th < 2:
        raise ValueError("ddeint_steps: his holds Th = {} sample(s) of the initial function; at least 2 are needed (an interval)".format(Th))
    if his_derivative is not None and (not torch.is_tensor(his_derivative) or his_derivative.shape != his.shape
                                       or his_derivative.dtype != his.dtype or his_derivative.device != his.device):
        raise ValueError("ddeint_steps: his_derivative must have his' shape {}, dtype {} and device, got {}".format(
            tuple(his.shape), his.dtype, "{} {}".format(tuple(his_derivative.shape), his_derivative.dtype)
            if torch.is_tensor(his_derivative) else type(his_derivative).__name__))
    if not torch.is_tensor(lags):
        lags = torch.as_tensor(lags)
    if lags.dim() != 1 or lags.numel() < 1 or lags.numel() > _MAX_LAGS:
        raise ValueError("ddeint_steps: lags must be a 1-D tensor of 1 to {} positive delays, got shape {}".format(_MAX_LAGS, tuple(lags.shape)))
    lags_host, _ = _host64(lags)  # (device-to-host read 1 of 2)
    if not np.all(np.isfinite(lags_host)) or np.any(lags_host <= 0):
        j = int(np.nonzero(~(np.isfinite(lags_host) & (lags_host > 0)))[0][0])
        raise ValueError("ddeint_steps: lags[{}] = {!r} is not a positive delay (lags are delays tau > 0: func receives y(t - tau); "
                         "positions in his_span are what ddeint takes)".format(j, float(lags_host[j])))
    his_t, his_span = _host64(his_span)  # (read 2 of 2)
    if his_t.ndim != 1 or len(his_t) != Th:
        raise ValueError("ddeint_steps: his_span must hold the Th = {} sample times of his, got shape {}".format(Th, his_t.shape))
    if not np.all(np.diff(his_t) > 0):
        raise ValueError("ddeint_steps: his_span must be strictly increasing, got {}".format(his_t.tolist()))
    if not torch.is_tensor(t_span):
        t_span = torch.as_tensor(t_span)
    if torch.is_grad_enabled() and t_span.requires_grad:
        raise NotImplementedError("ddeint_steps gives no gradient with respect to t_span; detach it")
    t_dtype = t_span.dtype if t_span.dtype in (torch.float32, torch.float64) else torch.float32
    t_own = t_span_to_host(t_span, np.float32 if t_dtype == torch.float32 else np.float64)  # (the one read of a device t_span)
    t_host = t_own.astype(np.float64)
    if t_host.ndim != 1 or len(t_host) < 1:
        raise ValueError("ddeint_steps: t_span must be a 1-D tensor of output times, got shape {}".format(t_host.shape))
    if len(t_host) > 1 and not np.all(np.diff(t_host) > 0):
        i = int(np.nonzero(~(np.diff(t_host) > 0))[0][0])
        raise ValueError("ddeint_steps: t_span must be strictly increasing, but t_span[{}] = {!r} is followed by {!r} (delays look back in "
                         "time: a delay equation is solved forwards)".format(i, float(t_host[i]), float(t_host[i + 1])))
    if his_t[-1] != t_host[0]:
        raise ValueError("ddeint_steps: his_span[-1] = {!r} must equal t_span[0] = {!r}: the initial function ends where the solve starts "
                         "(the state is his[..., -1:, :])".format(float(his_t[-1]), float(t_host[0])))
    if t_host[0] - lags_host.max() < his_t[0]:
        j = int(lags_host.argmax())
        raise ValueError("ddeint_steps: t_span[0] - lags[{}] = {!r} lies before his_span[0] = {!r}: the history must cover "
                         "[t_span[0] - max(lags), t_span[0]]".format(j, float(t_host[0] - lags_host[j]), float(his_t[0])))

    xde = StepsDDE(func, his, his_t, t_span, lags, lags_host, his_derivative=his_derivative)
    s = solver(xde=xde, y0=xde.y0, rtol=rtol, atol=atol, **options)
    assert isinstance(s, FixedSolver) and s._step_end_hook  # (the eager loop, a state per step)
    walk_args = s._plan(torch.from_numpy(t_own))
    grid = np.asarray(walk_args[0], dtype=np.float64)
    if len(grid) > 1:
        steps = np.diff(grid)
        k = int(steps.argmax())
        if lags_host.min() < steps[k]:
            j = int(lags_host.argmin())
            raise ValueError("ddeint_steps: lags[{}] = {!r} is smaller than the largest grid step {!r} (step {}, from t = {!r}): a delay "
                             "shorter than a step reaches into the step being taken; pass options['step_size'] <= {!r}".format(
                                 j, float(lags_host[j]), float(steps[k]), k, float(grid[k]), float(lags_host[j])))
    classic = solver is RK4 and s.variant == "classic"  # (its stage times are constants of rk4_step_func, not time_values)
    offsets = _STAGES_RK4_CLASSIC if classic else _STAGES[solver]
    # the table above against the solver's own: the stage times strictly inside a step are time_values' offsets, in order
    if not classic and [c for c in offsets if 0.0 < c < 1.0] != [c for c, is_time in s.time_values if is_time]:
        raise RuntimeError("ddeint_steps: {}.time_values {} no longer match the stage multiples {} the tape is planned with".format(
            solver.__name__, s.time_values, offsets))
    xde.plan(grid, offsets)
    return xde, s, walk_args


def ddeint_steps(func, his, his_span, t_span, lags, solver=RK4, his_derivative=None, options=None):
    """Integrate ``y'(t) = func(t, y(t), y_lags(t))`` from the initial function sampled in ``his`` and return y at every ``t_span`` point.

    ``his [..., Th, D]`` (``Th >= 2``) holds samples of the initial function at the strictly increasing times ``his_span [Th]``, with
    ``his_span[-1] == t_span[0]``; the state is ``y0 = his[..., -1:, :]``.  ``func(t, y, y_lags)`` takes ``y [..., 1, D]`` and
    ``y_lags [..., L, D]``, ``y_lags[..., j, :] = y(t - lags[j])``, and returns ``[..., 1, D]``.  ``lags [L]`` are positive delays (they
    may require grad), each at least as long as the largest grid step.  ``t_span`` is strictly increasing.  The result is
    ``[..., T, D]``.

    ``solver`` is ``Euler``, ``Midpoint`` or ``RK4``; ``options`` takes the fixed solvers' ``step_size`` / ``grid_constructor`` with
    ``interp="linear"``.  ``his_derivative`` (``his``' shape): the derivative of the initial function at its samples; without it the
    forward difference of the samples is taken (its last two rows are ``(y0 - his[..., -2, :]) / dt``, and the gradient with respect to
    ``y0`` includes that dependence; the other history rows are constants).

    The delayed states come from the cubic Hermite interpolant of the tape of nodes ``(time, state, derivative)`` — the history's, then
    ``(grid[k], y_k, f_k)`` of every step, ``f_k`` the step's first-stage derivative — in the last interval both of whose end
    derivatives are known when the stage runs.  The whole plan is validated before the first launch; the walk reads nothing back."""
    _, s, walk_args = _problem(func, his, his_span, t_span, lags, solver, his_derivative, options)
    return s._walk(*walk_args)
