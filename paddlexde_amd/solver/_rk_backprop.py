"""Back-propagation through the accepted steps of an adaptive solve: ``odeint(..., options={"backprop": "steps"})``.

The reference trains ``pred = odeint(func, y0, t, solver=Dopri5); loss.backward()`` by back-propagating through its eager step
ops ("discretise-then-optimise"): every stage derivative stays in the graph (solver/base_adaptive_solver_rk.py:150-170,
utils/ode_utils.py:100-109) while the step-size controller is ``no_grad`` (ode_utils.py:85).  This module computes that gradient —
of the discrete map with every accepted ``(t0, dt)`` and every stage time held constant — with respect to ``y0`` and the
parameters of ``func``.

Forward: the ordinary solve on the "sync" pipeline.  Its ``_step_hook`` sees every attempt's verdict; for each ACCEPTED one it records
``(t0, t1, dt, out_begin, out_end)`` and retains the step's base ``(y_n, f_n)`` — tensors the solve allocated afresh for that
attempt, so retaining them costs memory (about ``2 * n_accept * N`` elements) and no copy.  Rejected attempts leave nothing behind.

Backward, step by step from the last one, with ``lam = dL/dy_{n+1}``:
  1. the stage inputs are recomputed with the forward's own operand plans and kernels (host ``dt``: same bits), and ``func`` is
     called on leaf copies of them at the forward's stage times;
  2. if the step produced output rows: one ``xde_dense_cotangent`` launch turns their cotangents into those of the quartic's
     operands (y_n, y_{n+1} — added into ``lam`` —, y_mid, f_n, f_{n+1});
  3. for i = S .. 1: ``mu_i = dt (b_i lam + sum_{m>i} a_mi nu_m + mid_i ybar_mid) [+ fbar_1 + mu_0 of step n+1 at i = S]`` in one
     ``xde_stage_cotangent`` launch, then ``nu_i = J_i^T mu_i`` (and the parameter gradients) from one ``torch.autograd.grad``;
  4. stage 0: one launch writes both ``mu_0`` (handed to step n-1, whose last stage produced that derivative: ``ks[-1]`` becomes the
     next step's ``k_0``, FSAL or not, as in ``_attempt``) and ``dL/dy_n = lam + sum_m nu_m + ybar_0``.
The first step's ``k_0 = func(t_0, y0)`` gets the last VJP; the rows at the start time add their cotangent to ``y0`` directly.
Each step's retained tensors are released as soon as its backward is done.  S + 1 element-wise launches per accepted step (+1 for a
step that covers an output time; Dopri8's stage 0 takes two launches then: 17 operands > XDE_BP_MAX_X).

Two methods are seams a subclass overrides (solver/_rk_teval.py, per-sample output times): ``_record`` — what the hook keeps of an
accepted step — and ``_step_cotangents`` — how the cotangents of what a step put out become those of the quartic's operands (step 2);
``_start_terms`` are the cotangents that reach ``y0`` directly.  This class's own versions are the joint route, launch for launch.

Deviation from the reference: its first step size comes from ``select_initial_step``, which is not ``no_grad`` and
so carries a graph to y0 and func; here it is held constant like every other step size.
"""
import collections

import numpy as np
import torch

from .. import _hip
from ._common import as_operand, np_dtype, t_span_to_host

_Step = collections.namedtuple("_Step", "t0, t1, dt, ob, oe, y, f")


def quartic_weights(x, dt):
    """Weights of (y0, y1, y_mid, f0, f1) in the dense-output quartic at fraction ``x`` (csrc/xde_dense.hip: quartic_)."""
    x2 = x * x
    x3 = x2 * x
    x4 = x3 * x
    return (1.0 - 11.0 * x2 + 18.0 * x3 - 8.0 * x4,
            -5.0 * x2 + 14.0 * x3 - 8.0 * x4,
            16.0 * x2 - 32.0 * x3 + 16.0 * x4,
            dt * (x - 4.0 * x2 + 5.0 * x3 - 2.0 * x4),
            dt * (x2 - 3.0 * x3 + 2.0 * x4))


class StepsRun:
    """One solve in "steps" mode: ``forward(y0)`` integrates and retains, ``backward(grad_solution)`` sweeps and releases."""

    def __init__(self, func, t_span, solver, rtol, atol, options, params):
        from ..xde import BaseODE

        self.func, self.t_span, self.solver_cls, self.rtol, self.atol = func, t_span, solver, rtol, atol
        self.options = dict(options)
        self.params = list(params)
        self.probe = self.options.pop("_backprop_probe", None)  # test hook: (n, y1 recomputed, y1 retained, stage times)
        self._user_hook = self.options.pop("_step_hook", None)
        self._BaseODE = BaseODE
        self.steps = []
        self.y_last = None

    def _hook(self, index, y0, y1, ks, c):
        if self._user_hook is not None:
            self._user_hook(index, y0, y1, ks, c)
        if c.accept and c.status == _hip.STATUS_OK:
            rec = self._record(c, y0, y1, ks)
            if rec is not None:
                self.steps.append(rec)
            self.y_last = y1 if self.probe is not None else None

    # -- the two seams a subclass overrides (solver/_rk_teval.py): what an accepted step leaves behind, and how the cotangents of what
    # it put out become those of the quartic's operands --------------------------------------------------------------------------
    def _record(self, c, y0, y1, ks):
        """What the backward keeps of the accepted step the hook has just seen (None: nothing)."""
        return _Step(float(c.t0), float(c.t1), float(c.dt_last), int(c.out_begin), int(c.out_end), y0, ks[0])

    def _step_cotangents(self, st, g, lam):
        """The cotangents ``g`` of what step ``st`` put out, as those of the quartic's operands: ``lam += y1bar`` in place, and
        ``(y0bar, ymbar, f0bar, f1bar, dts)`` returned; None for a step that put out nothing (no launch)."""
        if st.oe <= st.ob:
            return None
        TT, Y = self.tdtype, np_dtype(self.sdtype)
        ts = self.t_host
        t0, t1 = TT(st.t0), TT(st.t1)
        dts = float(Y(TT(st.dt)))  # `dt.astype(y0.dtype)` of the dense kernel
        w = []
        for r in range(st.ob, st.oe):
            x = float(Y((TT(ts[r]) - t0) / (t1 - t0)))
            p0, p1, pm, q0, q1 = quartic_weights(x, dts)
            w.append((p0 + pm, p1, pm, q0, q1))  # (y_mid = y0 + ...: its cotangent reaches y0 as well)
        y0bar, ymbar, f0bar, f1bar = (torch.empty_like(lam) for _ in range(4))
        self.be.dense_cotangent([y0bar, lam, ymbar, f0bar, f1bar], g[st.ob : st.oe], w, acc_mask=0b10)
        return y0bar, ymbar, f0bar, f1bar, dts

    def _start_terms(self, g):
        """The cotangents that reach ``y0`` directly, as ``[(tensor, 1.0)]``: the output rows at the start time."""
        ts = self.t_host
        d = 1.0 if len(ts) < 2 or ts[-1] >= ts[0] else -1.0
        e = 1
        while e < len(ts) and d * ts[e] <= d * ts[0]:
            e += 1
        return [(g[r].view(self.shape), 1.0) for r in range(min(e, g.shape[0]))]

    def _adopt(self, s):
        """What the backward needs of the solver ``s`` (known once it is constructed: the hook may use it during the solve)."""
        self.be = s.backend
        self.tdtype = np_dtype(s.dtype)
        self.tcode = _hip.dtype_code(s.dtype)
        self.t_host = t_span_to_host(self.t_span, self.tdtype)
        (self.S, self.stage_plan, self.fsal, self.sol_plan, self.presum, self.mid_plan) = (
            s._n_stage, s._stage_plan, s._fsal, s._sol_plan, s._presum, s._mid_plan)

    def forward(self, y0):
        xde = self._BaseODE(self.func, y0=y0, t_span=self.t_span)
        s = self.solver_cls(xde=xde, y0=xde.y0, rtol=self.rtol, atol=self.atol, pipeline="sync", _step_hook=self._hook,
                            **self.options)
        self._adopt(s)
        solution = s.integrate(self.t_span)
        self.shape, self.sdtype, self.device = tuple(solution.shape[1:]), solution.dtype, solution.device
        tab = s.tableau
        self.alpha = [float(a) for a in tab.alpha]
        self.beta = [[float(b) for b in row] for row in tab.beta]
        self.b = [float(c) for c in tab.c_sol]
        self.mid = [float(m) for m in s.mid]
        # The stepper and its pipeline objects refer to each other (a reference cycle), and it still holds this solve's scratch
        # buffers and last state: left alone, they would live until the next cycle collection.  The solver is not used again —
        # drop everything it holds now, so that what this mode retains is exactly the (y_n, f_n) of the accepted steps.
        s.__dict__.clear()
        return solution

    # -- backward ---------------------------------------------------------------------------------------------------------
    def _stage_times(self, st):
        Y = np_dtype(self.sdtype)
        t0, t1, dt = Y(st.t0), Y(st.t1), Y(st.dt)
        return [Y(t1) if a == 1.0 else t0 + Y(a) * dt for a in self.alpha]  # (xde_control_device.hpp: the stage times of an attempt)

    def _recompute(self, st):
        """Stage inputs (bit-identical to the forward's: same plans, same kernels, dt from the host) and func on leaf copies."""
        be, S = self.be, self.S
        y, dt = st.y, st.dt
        ks = [st.f]  # kernel operands (no graph)
        kg, leaves = [None], [None]
        sbuf = torch.empty_like(y) if self.presum else None
        times = []
        for i, ti in enumerate(self._stage_times(st)):
            idx, coef = self.stage_plan[i]
            pre, emit = self.presum.get(i), self.presum.get(i + 1)
            out = torch.empty_like(y)
            if pre is not None:
                be.stage_combine_pre(out, y, sbuf, [ks[j] for j in pre[1]], pre[2], dt_host=dt)
            elif emit is not None:
                be.stage_combine(out, y, [ks[j] for j in idx], coef, _hip.COMBINE_RK, dt_host=dt, out2=sbuf, coef2=emit[0])
            else:
                be.stage_combine(out, y, [ks[j] for j in idx], coef, _hip.COMBINE_RK, dt_host=dt)
            t = torch.tensor(ti, dtype=self.sdtype, device=self.device)
            times.append(t)
            leaf = out.requires_grad_()
            with torch.enable_grad():
                k = self.func(t, leaf)
            if not torch.is_tensor(k) or k.shape != y.shape:
                raise RuntimeError("func returned {} for a state of shape {}".format(
                    tuple(k.shape) if torch.is_tensor(k) else type(k).__name__, tuple(y.shape)))
            leaves.append(leaf)
            kg.append(k)
            ks.append(as_operand(k.detach(), like=y))
        return leaves, kg, ks, times

    def _probe(self, n, ks, leaves, times):
        st = self.steps[n]
        if self.fsal:
            y1 = leaves[-1].detach()
        else:
            idx, coef = self.sol_plan
            y1 = torch.empty_like(st.y)
            self.be.stage_combine(y1, st.y, [ks[j] for j in idx], coef, _hip.COMBINE_RK, dt_host=st.dt)
        kept = self.y_last  # (the base of step n + 1, or the solve's last state)
        self.y_last = st.y
        self.probe(n, y1, kept, [t.detach().clone() for t in times])

    def _lincomb(self, out, terms, out2=None, terms2=None):
        """out = sum c x over ``terms`` [(x, c)]; out2 likewise over ``terms2``, from the same launch when the operands fit."""
        be = self.be
        if out2 is None:
            be.stage_cotangent(out, [x for x, _ in terms], [c for _, c in terms])
            return
        ops, c1, c2 = [], [], []
        pos = {}
        for which, ts in ((0, terms), (1, terms2)):
            for x, c in ts:
                j = pos.get(id(x))
                if j is None:
                    j = pos[id(x)] = len(ops)
                    ops.append(x)
                    c1.append(0.0)
                    c2.append(0.0)
                (c1 if which == 0 else c2)[j] += c
        if len(ops) <= _hip.XDE_BP_MAX_X:
            be.stage_cotangent(out, ops, c1, out2=out2, coef2=c2)
        else:
            be.stage_cotangent(out, [x for x, _ in terms], [c for _, c in terms])
            be.stage_cotangent(out2, [x for x, _ in terms2], [c for _, c in terms2])

    def _accum_params(self, pg, grads):
        for j, g in enumerate(grads):
            if g is not None:
                pg[j] = g if pg[j] is None else pg[j] + g

    def backward(self, grad_solution):
        S, shape = self.S, self.shape
        T_rows = grad_solution.shape[0]
        g = as_operand(grad_solution.detach().to(self.sdtype).reshape(T_rows, -1))
        like = torch.empty(shape, dtype=self.sdtype, device=self.device)
        lam = torch.zeros_like(like)
        carry = None
        pg = [None] * len(self.params)
        TT = self.tdtype
        ts = self.t_host
        for n in range(len(self.steps) - 1, -1, -1):
            st = self.steps[n]
            dt = st.dt
            leaves, kg, ks, times = self._recompute(st)
            if self.probe is not None:
                self._probe(n, ks, leaves, times)
            cot = self._step_cotangents(st, g, lam)
            dense = cot is not None
            if dense:
                y0bar, ymbar, f0bar, f1bar, dts = cot
            nus = [None] * (S + 1)
            for i in range(S, -1, -1):
                terms = []
                if self.b[i] != 0.0:
                    terms.append((lam, dt * self.b[i]))
                for m in range(i + 1, S + 1):
                    a = self.beta[m - 1][i] if i < len(self.beta[m - 1]) else 0.0
                    if a != 0.0 and nus[m] is not None:
                        terms.append((nus[m], dt * a))
                if dense and self.mid[i] != 0.0:
                    terms.append((ymbar, dts * self.mid[i]))
                if dense and i == 0:
                    terms.append((f0bar, 1.0))
                if i == S:
                    if dense:
                        terms.append((f1bar, 1.0))
                    if carry is not None:
                        terms.append((carry, 1.0))
                if i == 0:
                    ybar = torch.empty_like(lam)
                    terms2 = [(lam, 1.0)] + [(nu, 1.0) for nu in nus[1:] if nu is not None] + ([(y0bar, 1.0)] if dense else [])
                    carry = None
                    if terms:
                        carry = torch.empty_like(lam)
                        self._lincomb(carry, terms, ybar, terms2)
                    else:
                        self._lincomb(ybar, terms2)
                    lam = ybar
                    break
                if not terms:
                    continue
                mu = torch.empty_like(lam)
                self._lincomb(mu, terms)
                grads = torch.autograd.grad(kg[i], [leaves[i]] + self.params, mu, allow_unused=True)
                if grads[0] is not None:
                    nus[i] = as_operand(grads[0], like=lam)
                self._accum_params(pg, grads[1:])
            del leaves, kg, ks, nus
            self.steps[n] = None  # this step's (y_n, f_n) are released here
        self.steps = []
        self.y_last = None
        # the first step's k_0 = func(t_0, y0), and the rows at the start time
        terms = [(lam, 1.0)]
        if carry is not None:
            y0 = self.y0_leaf
            t = torch.tensor(TT(ts[0]), dtype=torch.float32 if TT is np.float32 else torch.float64, device=self.device)
            with torch.enable_grad():
                leaf = y0.detach().requires_grad_()
                k = self.func(t, leaf)
                grads = torch.autograd.grad(k, [leaf] + self.params, carry, allow_unused=True)
            if grads[0] is not None:
                terms.append((as_operand(grads[0], like=lam), 1.0))
            self._accum_params(pg, grads[1:])
        terms += self._start_terms(g)
        gy0 = torch.empty_like(lam)
        while len(terms) > _hip.XDE_BP_MAX_X:  # (only with more than 14 rows at the start time)
            part = torch.empty_like(lam)
            self._lincomb(part, terms[: _hip.XDE_BP_MAX_X])
            terms = [(part, 1.0)] + terms[_hip.XDE_BP_MAX_X :]
        self._lincomb(gy0, terms)
        return gy0, [p if p is None else p.to(q.dtype) for p, q in zip(pg, self.params)]


class StepsBackprop(torch.autograd.Function):
    """Forward: the solve, retaining each accepted step's base.  Backward: ``StepsRun.backward``."""

    @staticmethod
    def forward(ctx, run, y0, *params):
        run.y0_leaf = y0.detach()
        solution = run.forward(y0.detach())
        ctx.run = run
        return solution

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_solution):
        run, ctx.run = ctx.run, None
        gy0, gp = run.backward(grad_solution)
        return (None, gy0.reshape(run.y0_leaf.shape)) + tuple(gp)


def odeint_steps(func, y0, t_span, solver, *, rtol, atol, options, params):
    """The solve of ``options["backprop"] = "steps"`` when a gradient is wanted (see the module docstring)."""
    run = StepsRun(func, t_span, solver, rtol, atol, options, params)
    return StepsBackprop.apply(run, y0, *params)
