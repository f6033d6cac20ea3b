"""Per-sample output times of a joint adaptive solve: ``odeint(func, y0, t_span, solver, options={"t_eval": tq})`` (kernels:
include/xde_hip_teval.h).

Axis 0 of ``y0`` is the sample axis, ``t_span`` the two ends of the interval of integration, ``tq [rows, Q]`` every row's own times:
monotone in the direction of integration, inside the interval, trailing NaN meaning "no observation" (NaturalCubicSpline's
convention).  The result is ``[Q, rows, *y0.shape[1:]]``: ``sol[q, r]`` is row r of the solver's dense output at ``tq[r, q]``, 0
where that is NaN.

The solve is the ordinary joint solve over ``t_span`` on the "sync" pipeline: one step sequence for the batch, ``func(t, y)`` called
with a scalar ``t`` and the whole batch.  The controller never looks at output times when it chooses a step, so the accepted steps
are those of a solve on any list of times over the same interval — in particular of the solve on the sorted union of all rows' times,
whose result this one equals bit for bit without writing ``rows * Q`` full states.  The solve's ``_step_hook`` sees every accepted
step; where the step ``(t0, t1]`` holds a query of some row (two ``searchsorted`` in a sorted host array of all times), one
``xde_teval_dense`` launch writes, for every row, the queries of that row the step holds.  The kernels find a row's queries by
binary search in the row: there is no cursor, and nothing is recorded for the backward but what "steps" mode records anyway.

Gradients (grad mode on, ``y0`` or a parameter of an ``nn.Module`` func requiring grad) are those of ``options["backprop"] =
"steps"``: back-propagation through the accepted steps with the step sizes held constant (solver/_rk_backprop.py).  ``TevalRun`` is
that sweep with its two seams overridden: a step that holds a query turns the queries' cotangents into those of the quartic's
operands with one ``xde_teval_cotangent`` launch; a step that holds none skips the launch and the dense terms.
"""
import numpy as np
import torch

from ..utils.ode_utils import _rms_norm
from ._common import direction_of, np_dtype, t_span_to_host, upload
from ._rk_backprop import StepsBackprop, StepsRun, _Step

_UNION = "solve on the sorted union of the times (t_span = the union) and gather the rows"


class _Queries:
    """The validated times of a solve: their device copy, the rows' counts, and the host arrays the hook decides with."""

    def __init__(self, tq, t_host, device):
        TT = t_host.dtype.type
        self.rows, self.Q = tq.shape
        self.dir = d = direction_of(t_host)
        host = tq.detach().to("cpu").numpy().astype(TT)  # the solve's only read of tq; times are taken in the time dtype
        nan = np.isnan(host)
        cnt = (~nan).cumprod(axis=1).sum(axis=1).astype(np.int32)  # leading observations of every row
        late = ~nan & (np.arange(self.Q)[None, :] >= cnt[:, None])
        if late.any():
            r, q = (int(v[0]) for v in np.nonzero(late))
            raise ValueError("options['t_eval']: row {} has the time {} in column {} after a NaN; NaN entries (no observation) come "
                             "last in a row".format(r, host[r, q], q))
        t0, t1 = t_host[0], t_host[1]
        key = d * host
        with np.errstate(invalid="ignore"):
            outside = ~nan & ~((key >= d * t0) & (key <= d * t1))
            back = np.zeros_like(nan)
            back[:, 1:] = ~nan[:, 1:] & (key[:, 1:] < key[:, :-1])
        for bad, why in ((outside, "lies outside the interval of integration [{}, {}]".format(t0, t1)),
                         (back, "lies behind the time before it: a row's times are monotone in the direction of integration")):
            if bad.any():
                r, q = (int(v[0]) for v in np.nonzero(bad))
                raise ValueError("options['t_eval']: row {}, column {}: the time {} {}".format(r, q, host[r, q], why))
        self.padded = bool(nan.any())
        start = ~nan & (host == t0)
        self.n_start = start.sum(axis=1).astype(np.int32)  # (monotone rows inside the interval: the leading entries)
        self.flat = np.sort(key[~nan & ~start])  # dir * every time a step can hold, in the time dtype
        self.tq_dev = upload(np.where(nan, np.nan, host).astype(np.float64), device)
        self.cnt_dev = upload(cnt, device)
        self.start_dev = upload(self.n_start, device) if self.n_start.any() else None

    def held(self, t0, t1):
        """``(lo, hi)``: the times of ``flat`` the step ``(t0, t1]`` holds are ``flat[lo:hi]`` (compared in the time dtype)."""
        TT = self.flat.dtype.type
        return (int(np.searchsorted(self.flat, TT(self.dir) * TT(t0), side="right")),
                int(np.searchsorted(self.flat, TT(self.dir) * TT(t1), side="right")))

    def start_mask(self, q, like):
        """Rows whose query ``q`` is at the start time, shaped to broadcast against a state."""
        return (self.start_dev > q).view((self.rows,) + (1,) * (like.dim() - 1))


def _refuse(func, y0, t_span, solver, tq, mode, options):
    """Everything ``t_eval`` does not serve, refused before the first launch with a message that says what works."""
    from .base_adaptive_solver_rk import AdaptiveRKSolver
    from .base_fixed_solver import FixedSolver

    if not isinstance(solver, type) or issubclass(solver, FixedSolver) or not issubclass(solver, AdaptiveRKSolver):
        raise NotImplementedError("options['t_eval'] reads the dense output of the adaptive solvers (Dopri5, Dopri8, Bosh3, Fehlberg2, "
                                  "AdaptiveHeun), not a fixed-step solver: " + _UNION)
    if isinstance(y0, (tuple, list)):
        raise NotImplementedError("options['t_eval'] takes a tensor y0 whose axis 0 is the sample axis, not a tuple: concatenate the "
                                  "members along the last axis, or " + _UNION)
    if not torch.is_tensor(y0) or y0.dim() < 2:
        raise ValueError("options['t_eval']: y0 must be a tensor [rows, ...] with y0.dim() >= 2, axis 0 the sample axis (a 1-D state is "
                         "one sample: use y0[None] and a [1, Q] t_eval)")
    if not y0.is_contiguous():
        raise ValueError("options['t_eval']: y0 must be contiguous (pass y0.contiguous())")
    if y0.shape[0] < 1 or y0.numel() < 1:
        raise ValueError("options['t_eval']: y0 has no rows or no elements")
    np_dtype(y0.dtype)
    if t_span.dim() != 1 or t_span.numel() != 2:
        raise ValueError("options['t_eval']: t_span holds exactly two times, the ends of the interval of integration (got {}); the "
                         "output times are t_eval's".format(tuple(t_span.shape)))
    if not torch.is_tensor(tq):
        raise TypeError("options['t_eval'] must be a torch tensor [rows, Q] (got {}): torch.as_tensor(...) on y0's device".format(
            type(tq).__name__))
    if tq.dim() != 2 or tq.shape[0] != y0.shape[0] or tq.shape[1] < 1:
        raise ValueError("options['t_eval'] must be [rows, Q] with rows = y0.shape[0] = {} and Q >= 1 (got {}); pad short rows with "
                         "trailing NaN".format(y0.shape[0], tuple(tq.shape)))
    if tq.dtype not in (torch.float32, torch.float64):
        raise TypeError("options['t_eval'] must be float32 or float64 (got {}): t_eval.to(torch.float64)".format(tq.dtype))
    if tq.device != y0.device:
        raise ValueError("options['t_eval'] lives on {}, y0 on {}: pass t_eval.to(y0.device)".format(tq.device, y0.device))
    if tq.requires_grad:
        raise NotImplementedError("options['t_eval'] gives no gradient with respect to the observation times (a follow-up): pass "
                                  "t_eval.detach()")
    if mode not in (None, "steps", "adjoint"):
        raise ValueError("options['backprop'] must be 'steps' or 'adjoint', got {!r}".format(mode))
    if mode == "adjoint":
        raise NotImplementedError("options['t_eval'] trains through the accepted steps (backprop='steps', or no key): the continuous "
                                  "adjoint would need a jump at every distinct time; for it, " + _UNION)
    if options.get("process_group") is not None:
        raise NotImplementedError("options['t_eval'] runs on one device: shard the batch (and t_eval's rows) over the ranks and call it "
                                  "per rank, without process_group")
    if options.get("pipeline", "auto") not in ("auto", "sync"):
        raise NotImplementedError("options['t_eval'] writes its rows from the host's view of every accepted step (pipeline 'auto' or "
                                  "'sync'), not {!r}".format(options["pipeline"]))
    for key in ("step_t", "jump_t"):
        if options.get(key) is not None:
            raise NotImplementedError("options['t_eval'] does not take options[{!r}]: forced step times change the step sequence; drop "
                                      "it, or {}".format(key, _UNION))
    if options.get("dtype", torch.float32) not in (torch.float32, torch.float64):
        raise TypeError("dtype (time dtype) must be torch.float32 or torch.float64")
    if torch.is_grad_enabled() and t_span.requires_grad:
        raise NotImplementedError("options['t_eval'] gives no gradient with respect to t_span; odeint_adjoint on the union of the "
                                  "times does")


class TevalRun(StepsRun):
    """``StepsRun`` whose accepted steps put out every row's own queries.  ``retain`` False: the forward alone (nothing is kept)."""

    def __init__(self, func, t_span, solver, rtol, atol, options, params, queries, retain):
        super().__init__(func, t_span, solver, rtol, atol, options, params)
        self.q, self.retain = queries, retain
        self.out = None

    def _record(self, c, y0, y1, ks):
        q = self.q
        lo, hi = q.held(c.t0, c.t1)
        if hi > lo:
            idx, coef = self.mid_plan
            self.be._teval_dense(self.out, q.tq_dev, q.cnt_dev, [ks[j] for j in idx], coef, y0, y1, ks[0], ks[-1], float(c.t0), float(c.t1),
                                 float(c.dt_last), q.dir, self.tcode)
        if not self.retain:
            return None
        return _Step(float(c.t0), float(c.t1), float(c.dt_last), lo, hi, y0, ks[0])

    def _step_cotangents(self, st, g, lam):
        if st.oe <= st.ob:
            return None
        q = self.q
        y0bar, ymbar, f0bar, f1bar = (torch.empty_like(lam) for _ in range(4))
        self.be._teval_cotangent([y0bar, lam, ymbar, f0bar, f1bar], g.view((q.Q,) + tuple(lam.shape)), q.tq_dev, q.cnt_dev, st.t0, st.t1,
                                 st.dt, q.dir, self.tcode, acc_mask=0b10)
        dts = float(np_dtype(self.sdtype)(self.tdtype(st.dt)))  # `dt.astype(y0.dtype)` of the dense kernel
        return y0bar, ymbar, f0bar, f1bar, dts

    def _start_terms(self, g):
        q = self.q
        zero = torch.zeros(self.shape, dtype=self.sdtype, device=self.device)
        return [(torch.where(q.start_mask(j, zero), g[j].view(self.shape), zero), 1.0) for j in range(int(q.n_start.max()))]

    def forward(self, y0):
        q = self.q
        # (every query later than the start lies in exactly one accepted step, the ones at the start are written here: only
        # the padding is left to a fill)
        self.out = out = (torch.zeros if q.padded else torch.empty)((q.Q,) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
        for j in range(int(q.n_start.max())):
            out[j] = torch.where(q.start_mask(j, y0), y0, out[j])
        super().forward(y0)  # (its two-row solution is not what this solve is for)
        self.out = None
        return out


def odeint_teval(func, y0, t_span, solver, *, rtol, atol, options):
    options = dict(options)
    tq = options.pop("t_eval")
    mode = options.pop("backprop", None)
    _refuse(func, y0, t_span, solver, tq, mode, options)
    options.pop("pipeline", None)
    options.setdefault("norm", _rms_norm)
    t_host = t_span_to_host(t_span, np_dtype(options.get("dtype", torch.float32)))
    queries = _Queries(tq, t_host, y0.device)
    params = [p for p in func.parameters() if p.requires_grad] if isinstance(func, torch.nn.Module) else []
    if torch.is_grad_enabled() and (y0.requires_grad or params):
        return StepsBackprop.apply(TevalRun(func, t_span, solver, rtol, atol, options, params, queries, True), y0, *params)
    with torch.no_grad():
        return TevalRun(func, t_span, solver, rtol, atol, options, [], queries, False).forward(y0.detach())
