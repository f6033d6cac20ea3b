"""Per-sample adaptive stepping: ``odeint(..., options={"per_sample": True})`` (kernels: include/xde_hip_rows.h).

Axis 0 of ``y0`` is the sample axis.  Every row carries its own time, step size, error ratio, verdict, output cursor and counters
(``_hip.RowsCtl``), and ``solution[:, r]`` is what the same solver gives for ``y0[r:r+1]`` solved alone: the reference's
``select_initial_step``, I-controller, dense output and ``max_num_steps`` row by row, the RMS norm taken over the row.

One attempt is the stage launches (xde_rows_stage_combine, a ``func`` call each, FSAL kept), xde_rows_norm_control and
xde_rows_dense_commit.  The host looks at the rows' ``done`` / ``status`` every ``options["check_every"]`` attempts: a row that has
written its last output is frozen (``func`` still sees it, at its final state and time; nothing of it is committed), so an attempt
enqueued after every row is done changes nothing — a late look costs time, never bits.

``func(t, y)`` receives ``t`` as a tensor of shape ``[rows] + [1] * (y.dim() - 1)`` in the state dtype, row r's own stage time, and
must map sample r to sample r only (it is the caller's statement that the samples are independent; it cannot be checked).
"""
import numpy as np
import torch

from .. import _hip
from ..utils.ode_utils import _rms_norm
from ._common import direction_of, np_dtype, storage_ptr, t_span_to_host, upload
from ._rk_plans import build_plans
from .base_adaptive_solver_rk import _STATUS_MSG

_PLANS = {}
_OPTIONS = ("norm", "dtype", "first_step", "min_step", "max_step", "safety", "ifactor", "dfactor", "max_num_steps", "pipeline", "controller",
            "seam", "process_group", "_replay", "step_t", "jump_t", "check_every", "stats_out", "backprop")
_CALLBACKS = ("callback_step", "callback_accept_step", "callback_reject_step", "callback_accept", "callback_reject")
_SERVED = "Dopri5, Bosh3, Fehlberg2 and AdaptiveHeun"
_FORWARD_ONLY = ("options['per_sample'] is forward-only: y0, func's parameters (or tensors func closes over) or t_span require grad (or "
                 "options['backprop'] is set).  Wrap the call in torch.no_grad(), or drop per_sample; back-propagation and the "
                 "adjoint per row are a follow-up")


def _refuse(func, y0, t_span, solver, options):
    """Everything ``per_sample`` does not serve, refused before the first launch with a message that says what works."""
    from .base_adaptive_solver_rk import AdaptiveRKSolver
    from .base_fixed_solver import FixedSolver

    if not isinstance(solver, type) or issubclass(solver, FixedSolver) or not issubclass(solver, AdaptiveRKSolver):
        raise NotImplementedError("options['per_sample'] steps every row with its own adaptive step size: it takes the adaptive solvers "
                                  "{}, not a fixed-step solver (drop per_sample: a fixed grid is the same for every row)".format(_SERVED))
    if len(solver.tableau.alpha) + 1 > _hip.XDE_ROWS_MAX_K:
        raise NotImplementedError("options['per_sample'] serves {}; {} has {} stages, more than one row launch takes (a follow-up): "
                                  "drop per_sample, or pick one of those solvers".format(_SERVED, solver.__name__, len(solver.tableau.alpha)))
    if isinstance(y0, (tuple, list)):
        raise NotImplementedError("options['per_sample'] takes a tensor y0 whose axis 0 is the sample axis, not a tuple: "
                                  "concatenate the members along the last axis, or drop per_sample")
    if not torch.is_tensor(y0) or y0.dim() < 2:
        raise ValueError("options['per_sample']: y0 must be a tensor [rows, ...] with y0.dim() >= 2, axis 0 the sample axis "
                         "(a 1-D state is one sample: use y0[None], or drop per_sample)")
    if not y0.is_contiguous():
        raise ValueError("options['per_sample']: y0 must be contiguous (pass y0.contiguous())")
    if y0.shape[0] < 1 or y0.numel() < 1:
        raise ValueError("options['per_sample']: y0 has no rows or no elements")
    grads = torch.is_grad_enabled() and (y0.requires_grad or t_span.requires_grad or (
        isinstance(func, torch.nn.Module) and any(p.requires_grad for p in func.parameters())))
    if grads or "backprop" in options:
        raise NotImplementedError(_FORWARD_ONLY)
    for key in ("step_t", "jump_t"):
        if options.get(key) is not None:
            raise NotImplementedError("options['per_sample'] does not take options[{!r}]: forced step times are shared by all rows; "
                                      "put them into t_span, or drop per_sample".format(key))
    for key in _CALLBACKS:
        if options.get(key) is not None or callable(getattr(func, key, None)):
            raise NotImplementedError("options['per_sample'] calls no step callbacks ({}): the rows' attempts have no common time; "
                                      "drop the callback, or drop per_sample".format(key))
    if options.get("controller", "I") != "I":
        raise NotImplementedError("options['per_sample'] runs the reference's I-controller (controller='I'), not {!r}".format(
            options["controller"]))
    if options.get("norm", _rms_norm) is not _rms_norm:
        raise NotImplementedError("options['per_sample'] takes the RMS norm of each row (norm=_rms_norm, the default); another norm "
                                  "needs the joint solve: drop per_sample")
    if options.get("process_group") is not None:
        raise NotImplementedError("options['per_sample'] runs on one device: shard the batch over the ranks and call it per rank, "
                                  "without process_group")
    if options.get("pipeline", "auto") not in ("auto", "sync"):
        raise NotImplementedError("options['per_sample'] drives its attempts from the host (pipeline 'auto' or 'sync'), not {!r}".format(
            options["pipeline"]))
    if options.get("seam", "auto") == "resident":
        raise NotImplementedError("options['per_sample'] has no resident seam launch: seam='auto' or 'launches'")
    if options.get("_replay") is not None:
        raise NotImplementedError("options['per_sample'] does not replay a prescribed step sequence (_replay)")
    unknown = sorted(set(options) - set(_OPTIONS) - set(_CALLBACKS))
    if unknown:
        raise NotImplementedError("options['per_sample'] does not take the option(s) {}; it takes {}".format(
            unknown, sorted(set(_OPTIONS) - {"backprop", "_replay", "step_t", "jump_t", "process_group"})))
    if options.get("dtype", torch.float32) not in (torch.float32, torch.float64):
        raise TypeError("dtype (time dtype) must be torch.float32 or torch.float64")
    if int(options.get("check_every", 4)) < 1:
        raise ValueError("options['check_every'] must be >= 1")


def odeint_rows(func, y0, t_span, solver, *, rtol, atol, options):
    options = dict(options)
    _refuse(func, y0, t_span, solver, options)
    probe = torch.is_grad_enabled()  # (parameters a plain callable closes over show only in what it returns: _RowsSolve.run)
    with torch.no_grad():
        return _RowsSolve(func, y0, t_span, solver, rtol, atol, options, probe).run()


class _RowsSolve:
    def __init__(self, func, y0, t_span, solver, rtol, atol, o, probe=False):
        self.probe = probe
        self.be = be = _hip.get_backend()
        be.require_device(y0)
        self.func = func
        self.tdtype = o.get("dtype", torch.float32)
        tt = self.tt = np_dtype(self.tdtype)
        self.Y = y0.dtype
        np_dtype(self.Y)  # (float32 / float64 states)
        self.rows = y0.shape[0]
        self.shape = tuple(y0.shape)
        self.tshape = (self.rows,) + (1,) * (y0.dim() - 1)
        self.dev = y0.device
        self.t_host = t_span_to_host(t_span, tt)
        if self.t_host.ndim != 1 or len(self.t_host) < 1:
            raise ValueError("t_span must be a 1-D sequence of output times")
        self.dir = direction_of(self.t_host)
        self.check_every = int(o.get("check_every", 4))
        self.stats_out = o.get("stats_out")
        self.first_step = None if o.get("first_step") is None else tt(o["first_step"])
        self.max_num_steps = int(o.get("max_num_steps", 2**31 - 1))
        plans = _PLANS.get(solver)
        if plans is None:
            plans = _PLANS[solver] = build_plans(solver.tableau, solver.mid)
        self.pl = plans
        self.order = solver.order
        p = self.params = _hip.XdeCtrlParams()
        p.rtol, p.atol = float(tt(rtol)), float(tt(atol))
        p.min_step, p.max_step = float(tt(o.get("min_step", 0))), float(tt(o.get("max_step", float("inf"))))
        p.safety, p.ifactor, p.dfactor = float(tt(o.get("safety", 0.9))), float(tt(o.get("ifactor", 10.0))), float(tt(o.get("dfactor", 0.2)))
        p.order = float(self.order)
        p.max_num_steps = self.max_num_steps
        p.time_dtype, p.state_dtype = _hip.dtype_code(self.tdtype), _hip.dtype_code(self.Y)
        p.direction = self.dir
        p.norm_kind = _hip.NORM_RMS
        p.n_stage, p.n_seg = plans.n_stage, 1
        for i, a in enumerate(solver.tableau.alpha):
            p.alpha[i] = float(a)
        p.seg_count[0] = float(y0.numel() // self.rows)
        self.y0 = y0.detach().clone()  # (committed in place: never the caller's tensor)
        self.nfe = 0

    # ------------------------------------------------------------------------------------------
    def _eval(self, t, y, live=()):
        """``func(t, y)`` as a kernel operand that aliases nothing still in use."""
        self.nfe += 1
        f = self.func(t.view(self.tshape), y)
        if not torch.is_tensor(f) or tuple(f.shape) != self.shape:
            raise ValueError("options['per_sample']: func must return a tensor of y's shape {}, got {}".format(
                self.shape, tuple(f.shape) if torch.is_tensor(f) else type(f).__name__))
        if f.dtype != self.Y:
            f = f.to(self.Y)
        if not f.is_contiguous():
            f = f.contiguous()
        sp = storage_ptr(f)
        if sp == storage_ptr(y) or sp in live:
            f = f.clone()
        return f

    def _times(self, ctl):
        """The stage times of the pending attempt and its checks, from ``t`` and ``h`` (plan_next's arithmetic, once per solve)."""
        p, d = self.params, float(self.dir)
        t0, h = ctl.t.to(self.tdtype), ctl.h.to(self.tdtype)
        t1 = t0 + h
        live = ctl.done == 0
        bad = live & ~(d * t1 > d * t0)
        ctl.status.masked_fill_(bad, _hip.STATUS_DT_UNDERFLOW)
        if self.max_num_steps <= 0:
            ctl.status.masked_fill_(live & (ctl.status == 0), _hip.STATUS_MAX_STEPS)
        t0y, hy, t1y = t0.to(self.Y), h.to(self.Y), t1.to(self.Y)
        for i in range(p.n_stage):
            a = torch.tensor(p.alpha[i], dtype=self.Y).item()
            ctl.t_stage[i].copy_(t1y if a == 1.0 else t0y + a * hy)

    def _first_step(self, ctl, f0):
        """``select_initial_step`` row by row (base_adaptive_solver.py:33-72): the three norms are launches, the scalars between them
        framework ops on [rows] vectors in the reference's dtypes and op order.  Leaves the signed first steps in ``ctl.h``."""
        be, Y, y0 = self.be, self.Y, self.y0
        p = self.params
        d0, d1, d2 = (torch.empty(self.rows, dtype=torch.float64, device=self.dev) for _ in range(3))
        be._rows_scaled_norm(d0, y0, None, y0, p.rtol, p.atol)
        be._rows_scaled_norm(d1, f0, None, y0, p.rtol, p.atol)
        d0, d1 = d0.abs().to(Y), d1.abs().to(Y)
        c = lambda v: torch.tensor(v, dtype=Y, device=self.dev)  # noqa: E731
        h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), c(1e-6), c(0.01) * d0 / d1).abs()
        hs0 = -h0 if self.dir < 0 else h0  # the Euler probe is taken in the direction of integration
        ctl.h.copy_(hs0)
        y1 = torch.empty_like(y0)
        be._rows_stage_combine(y1, y0, [f0], [1.0], ctl)  # fuse(f0, h0, y0)
        pt = torch.promote_types(self.tdtype, Y)
        t_probe = (ctl.t.to(self.tdtype).to(pt) + hs0.to(pt)).to(Y)
        f1 = self._eval(t_probe, y1, live=(storage_ptr(f0),))
        be._rows_scaled_norm(d2, f1, f0, y0, p.rtol, p.atol)
        d2 = (d2.to(Y) / h0).abs()
        m = torch.where(d2 > d1, d2, d1)  # Python's max(d1, d2)
        e = torch.tensor(1.0 / float(self.order), dtype=Y).item()
        big = ((c(0.01) / m).double() ** e).to(Y)  # the correctly rounded power, as the device controller's pow_
        a, b = c(1e-6), h0 * c(1e-3)
        h1 = torch.where((d1 <= 1e-15) & (d2 <= 1e-15), torch.where(b > a, b, a), big).abs()
        first = torch.fmin(c(100.0) * h0, h1).to(self.tdtype)
        ctl.h.copy_(float(self.dir) * first.abs())

    # ------------------------------------------------------------------------------------------
    def run(self):
        be, pl, p, y0 = self.be, self.pl, self.params, self.y0
        T, d = len(self.t_host), float(self.dir)
        for i in range(1, T):
            if not d * self.t_host[i] >= d * self.t_host[i - 1]:
                raise ValueError("t_span must be monotonic")
        solution = torch.empty((T,) + self.shape, dtype=self.Y, device=self.dev)
        ctl = _hip.RowsCtl(self.rows, pl.n_stage, self.Y, self.dev)
        n0 = 1
        while n0 < T and d * self.t_host[n0] <= d * self.t_host[0]:
            n0 += 1
        solution[:n0] = y0
        ctl.t.fill_(float(self.t_host[0]))
        ctl.t_prev.fill_(float(self.t_host[0]))
        ctl.next_out.fill_(n0)
        if n0 >= T:
            return self._finish(ctl, solution)
        t_span_dev = upload(self.t_host.astype(np.float64), self.dev)
        # The first evaluation runs with the caller's grad mode: a func that is no Module but closes over tensors that require grad
        # cannot be seen by _refuse, its result can.  Still before the first launch.
        with torch.enable_grad() if self.probe else torch.no_grad():
            f0 = self._eval(ctl.t.to(self.tdtype).to(self.Y), y0)
        if f0.requires_grad:
            raise NotImplementedError(_FORWARD_ONLY)
        f0 = f0.clone()  # (committed in place: never func's tensor)
        if self.first_step is None:
            self._first_step(ctl, f0)
        else:
            ctl.h.fill_(float(self.tt(d) * abs(self.first_step)))
        self._times(ctl)
        scratch, y1buf, ebuf = torch.empty_like(y0), torch.empty_like(y0), (torch.empty_like(y0) if pl.fuse_err else None)
        S = pl.n_stage
        attempts = 0
        while True:
            ks = [f0]
            live = {storage_ptr(x) for x in (y0, f0, scratch, y1buf)}
            y_stage = None
            for i in range(S):
                idx, coef = pl.stage_plan[i]
                out = y1buf if (i == S - 1 and pl.fsal) else scratch
                if i == S - 1 and pl.fuse_err:
                    be._rows_stage_combine(out, y0, [ks[j] for j in idx], coef, ctl, out2=ebuf, coef2=pl.err2_coef)
                else:
                    be._rows_stage_combine(out, y0, [ks[j] for j in idx], coef, ctl)
                ks.append(self._eval(ctl.t_stage[i], out, live=live))
                live.add(storage_ptr(ks[-1]))
                y_stage = out
            if pl.fsal:
                y1 = y_stage
            else:
                idx, coef = pl.sol_plan
                y1 = y1buf
                be._rows_stage_combine(y1, y0, [ks[j] for j in idx], coef, ctl)
            idx, coef = pl.err_plan
            if pl.fuse_err:
                be._rows_norm_control([ks[-1]], [coef[-1]], y0, y1, ctl, p, t_span_dev, e_pre=ebuf)
            else:
                be._rows_norm_control([ks[j] for j in idx], coef, y0, y1, ctl, p, t_span_dev)
            idx, coef = pl.mid_plan
            be._rows_dense_commit(solution, [ks[j] for j in idx], coef, y0, y1, ks[-1], ctl, p, t_span_dev)
            attempts += 1
            if attempts % self.check_every == 0:
                look = ctl.i32.cpu()  # (one copy: done, status and the counters)
                status = look[_hip.RowsCtl.I32.index("status")]
                if bool((status != 0).any()):
                    self._raise(ctl, int(torch.nonzero(status)[0]))
                if bool((look[_hip.RowsCtl.I32.index("done")] != 0).all()):
                    break
        return self._finish(ctl, solution)

    def _raise(self, ctl, r):
        status = int(ctl.status[r])
        row = " (row {} of the batch)".format(r)
        if status == _hip.STATUS_DT_UNDERFLOW:
            raise AssertionError(_STATUS_MSG[status].format(float(ctl.h[r])) + row)
        if status == _hip.STATUS_NONFINITE:
            raise AssertionError(_STATUS_MSG[status].format("{} non-finite element(s)".format(int(ctl.nonfinite[r]))) + row)
        if status == _hip.STATUS_MAX_STEPS:
            raise AssertionError(_STATUS_MSG[status].format(int(ctl.steps_in_interval[r]), self.max_num_steps) + row)
        raise AssertionError("solver status {}".format(status) + row)

    def _finish(self, ctl, solution):
        if self.stats_out is not None:
            self.stats_out.update({"n_accept": ctl.n_accept.clone(), "n_reject": ctl.n_reject.clone(), "nfe": int(self.nfe),
                                   "t": ctl.t.clone(), "dt_next": ctl.h.clone()})
        return solution
