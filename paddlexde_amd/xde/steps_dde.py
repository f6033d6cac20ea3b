"""Delay-equation problem wrapper whose delays reach into the solution being computed: ``y'(t) = f(t, y(t), y(t - tau_1), ...)``
(``functional.ddeint_steps``; no counterpart in the reference, whose ``BaseDDE`` gathers the delayed states once from the given history).

``StepsDDE`` is an ODE wrapper (``BaseODE.fuse``: the fixed-step solvers map it onto xde_stage_combine without damping) whose ``move``
hands ``func`` the delayed states of the stage: the cubic Hermite interpolant of a TAPE of ``(time, state, derivative)`` nodes — the
samples of the initial function, then one node per grid step, ``(grid[k], y_k, f_k)`` with ``f_k`` the step's own first-stage
derivative — evaluated at all delays in one xde_dde_tape_gather launch (solver/_autograd.py: ``DdeTapeGatherFn``).

The whole solve is PLANNED ON THE HOST before the first launch (``plan``): per stage of every step, in float64, the stage time ``s``,
``theta_j = s - tau_j``, the interval of the tape ``theta_j`` falls into — the last COMPLETE interval (both end derivatives known when
the stage runs) whose left end is ``<= theta_j`` — ``sigma = (theta_j - a) / h`` and the Hermite weights (include/xde_hip_dde.h).  A plan
that would need ``sigma > 1`` (a delay that reaches into the step being taken) or ``theta_j < his_span[0]`` is refused there.  The walk
itself reads nothing back from the device.

The wrapper overrides ``on_integrate_step_end``: the solvers then keep the eager loop (no captured graph), every step makes a state of
its own (the tape holds them), and the hook is where the step counter advances and, with grad mode off, where nodes no later stage
reads are dropped.
"""
import numpy as np
import torch

from ..solver._autograd import DdeTapeGatherFn
from ..solver._common import as_operand
from .base_ode import BaseODE


def hermite_weights(sigma, h):
    """The float64 weights of include/xde_hip_dde.h at ``sigma`` in an interval of length ``h``: ``(a0, a1, a2, a3)`` of the value on
    ``(ya, fa, yb, fb)`` and ``(b0, b1, b2, b3)`` of its derivative with respect to the delay, ``-H'(theta)``."""
    sigma, h = float(sigma), float(h)
    s2 = sigma * sigma
    s3 = s2 * sigma
    a = (2.0 * s3 - 3.0 * s2 + 1.0, h * (s3 - 2.0 * s2 + sigma), -2.0 * s3 + 3.0 * s2, h * (s3 - s2))
    b0 = -((6.0 * s2 - 6.0 * sigma) / h)
    b = (b0, -(3.0 * s2 - 4.0 * sigma + 1.0), -b0, -(3.0 * s2 - 2.0 * sigma))
    return a, b


def stage_time(grid, k, c):
    """The host time of a stage at the multiple ``c`` of step ``k``, float64: the grid's own values at either end."""
    a, b = float(grid[k]), float(grid[k + 1])
    return a if c == 0.0 else (b if c == 1.0 else a + (b - a) * c)


def pick_interval(theta, his_t, grid, k, stage):
    """The interval rule.  ``his_t`` and ``grid`` are float64 arrays with ``his_t[-1] == grid[0]``.  When stage ``stage`` of step ``k``
    runs, the history's ``Th - 1`` intervals are complete and so are the tape's intervals ``[grid[m], grid[m + 1]]`` with ``m + 1 <=
    k - 1`` (at the first stage: ``f_k`` is not known yet) or ``m + 1 <= k`` (later stages).  Returns ``("his" | "tape", index, a, b)``
    of the last complete interval whose left end is ``<= theta``, or None when ``theta < his_t[0]``."""
    n_tape = max(k - 1 if stage == 0 else k, 0)  # the tape's complete intervals are 0 .. n_tape - 1
    if n_tape > 0 and theta >= grid[0]:
        m = min(int(np.searchsorted(grid, theta, side="right")) - 1, n_tape - 1)
        return "tape", m, float(grid[m]), float(grid[m + 1])
    i = min(int(np.searchsorted(his_t, theta, side="right")) - 1, len(his_t) - 2)
    if i < 0:
        return None
    return "his", i, float(his_t[i]), float(his_t[i + 1])


class StagePlan:
    """What one ``DdeTapeGatherFn`` application needs: ``src[4 j + s]``, the operands ``ya, fa, yb, fb`` of delay ``j`` — a ``[rows, D]``
    history row (a tensor) or an index into ``keys``, the distinct tape tensors ``(node, 0: state | 1: derivative)`` the stage reads —
    and the weights ``w`` / ``wd`` (``4 L`` floats each).  ``dep[4 j + s]`` is None, or ``(index into keys, scale)`` where a HISTORY
    operand is itself a function of a tape tensor with that derivative: the forward-difference derivative of the history's last two
    nodes is ``(y0 - his[Th - 2]) / dt``, so its cotangent reaches tape node 0's state scaled by ``1 / dt``."""

    __slots__ = ("src", "keys", "dep", "w", "wd", "rows", "L", "D", "lead", "like", "lags_shape", "lags_dtype", "lags_device", "first_node")


class StepsDDE(BaseODE):
    def __init__(self, func, his, his_span_host, t_span, lags, lags_host, his_derivative=None):
        """``his [..., Th, D]`` (floating, on the device), ``his_span_host`` / ``lags_host`` float64 host copies (validated by the caller,
        functional.ddeint_steps); the state is ``his[..., -1:, :]``."""
        y0 = his[..., -1:, :]
        super().__init__(func, y0=y0, t_span=t_span)
        d = self.__dict__
        d["lags"] = lags
        d["lags_host"] = np.asarray(lags_host, dtype=np.float64)
        d["his_t"] = np.asarray(his_span_host, dtype=np.float64)
        from .. import _hip

        d["_backend"] = _hip.get_backend()
        d["_backend"].require_device(his)
        hc = his.detach()
        hc = hc if hc.is_contiguous() else hc.contiguous()
        Th, D = hc.shape[-2], hc.shape[-1]
        rows = hc.numel() // (Th * D)
        d["_hf_pending"] = None
        if his_derivative is None:
            hf = d["_hf_pending"] = torch.empty_like(hc)  # (filled by plan(), once the plan stands: nothing runs before a refusal)
        else:
            hf = his_derivative.detach()
            hf = hf if hf.is_contiguous() else hf.contiguous()
        his2, hf2 = hc.view(rows, Th, D), hf.view(rows, Th, D)
        d["_his_y"] = [his2[:, i, :] for i in range(Th)]
        d["_his_f"] = [hf2[:, i, :] for i in range(Th)]
        d["_geom"] = (rows, D, tuple(hc.shape[:-2]), hc)
        d["_plans"] = None
        d["_tape"] = {}
        d["_k"] = 0
        d["_stage"] = 0
        d["tape_high_water"] = 0

    # -- the host plan ----------------------------------------------------------------------------
    def plan(self, grid, offsets):
        """Plans every stage of every step of a walk over ``grid`` (host, time dtype) with the stage multiples ``offsets`` of the solver,
        and validates all of it: raises ValueError, before anything is launched, on a delay that reaches into the step being taken or
        behind the history."""
        rows, D, lead, like = self._geom
        his_t, lags = self.his_t, self.lags_host
        g64 = np.asarray(grid, dtype=np.float64)
        Th, L = len(his_t), len(lags)
        diffed = self._hf_pending is not None  # the history's derivative is the forward difference of its samples
        t_state = torch.as_tensor(his_t).to(like.dtype)
        y0_scale = 1.0 / float(t_state[-1] - t_state[-2])  # (the spacing as the difference below divides by it, in the state dtype)
        plans, first = [], []
        for k in range(len(g64) - 1):
            stages = []
            for i, c in enumerate(offsets):
                s = stage_time(g64, k, float(c))
                sp = StagePlan()
                sp.src, sp.keys, sp.dep, sp.w, sp.wd = [], [], [], [], []
                sp.rows, sp.L, sp.D, sp.lead, sp.like = rows, L, D, lead, like
                sp.lags_shape, sp.lags_dtype, sp.lags_device = tuple(self.lags.shape), self.lags.dtype, self.lags.device
                index = {}

                def node(m, which):
                    key = (m, which)
                    if key not in index:
                        index[key] = len(sp.keys)
                        sp.keys.append(key)
                    return index[key]

                for j in range(L):
                    theta = s - float(lags[j])
                    got = pick_interval(theta, his_t, g64, k, i)
                    if got is None:
                        raise ValueError("lags[{}] = {!r} reaches t = {!r} at the stage at t = {!r} of step {}, before his_span[0] = {!r}: "
                                         "give a history that covers t_span[0] - max(lags)".format(j, float(lags[j]), theta, s, k, float(his_t[0])))
                    kind, m, a, b = got
                    h = b - a
                    sigma = (theta - a) / h
                    if sigma > 1.0:
                        raise ValueError("lags[{}] = {!r} reaches t = {!r} at the stage at t = {!r} of step {}, past the last complete interval "
                                         "[{!r}, {!r}] of the tape (sigma = {!r} > 1): a delay must be at least as long as the step it is "
                                         "read in; take shorter steps (options['step_size'] <= the delay)".format(
                                             j, float(lags[j]), theta, s, k, a, b, sigma))
                    wa, wb = hermite_weights(sigma, h)
                    if kind == "his":
                        # (history node Th - 1 and tape node 0 share the state and keep separate derivatives)
                        sp.src += [self._his_y[m], self._his_f[m], node(0, 0) if m + 1 == Th - 1 else self._his_y[m + 1], self._his_f[m + 1]]
                        # (the forward difference's last two rows are (y0 - his[Th - 2]) / dt: their cotangent reaches y0)
                        sp.dep += [None, (node(0, 0), y0_scale) if (diffed and m >= Th - 2) else None, None,
                                   (node(0, 0), y0_scale) if (diffed and m + 1 >= Th - 2) else None]
                    else:
                        sp.src += [node(m, 0), node(m, 1), node(m + 1, 0), node(m + 1, 1)]
                        sp.dep += [None] * 4
                    sp.w += wa
                    sp.wd += wb
                sp.first_node = min([m for m, _ in sp.keys] + [k])
                stages.append(sp)
            plans.append(stages)
            first.append(min(sp.first_node for sp in stages))
        # the oldest node any stage from step k on still reads: with grad mode off the older ones are dropped after step k - 1
        for k in range(len(first) - 2, -1, -1):
            first[k] = min(first[k], first[k + 1])
        d = self.__dict__
        if self._hf_pending is not None:
            # the forward difference of the samples, the last node repeating the one before: framework ops, once per call
            hf, d["_hf_pending"] = self._hf_pending, None
            t = torch.as_tensor(his_t).to(device=like.device, dtype=like.dtype)
            diff = (like[..., 1:, :] - like[..., :-1, :]) / (t[1:] - t[:-1]).unsqueeze(-1)
            hf[..., :-1, :].copy_(diff)
            hf[..., -1, :].copy_(diff[..., -1, :])
        d["_plans"], d["_keep_from"] = plans, first
        d["_tape"], d["_k"], d["_stage"], d["tape_high_water"] = {}, 0, 0, 0

    # -- the walk -----------------------------------------------------------------------------------
    def move(self, t0, dt, y0):
        k, i = self._k, self._stage
        if self._plans is None or k >= len(self._plans) or i >= len(self._plans[k]):
            raise RuntimeError("StepsDDE.move: stage {} of step {} is not in the plan (the wrapper is driven by ddeint_steps' walk)".format(i, k))
        if i == 0:
            self._tape[k] = [y0, None]
            self.__dict__["tape_high_water"] = max(self.tape_high_water, len(self._tape))
        sp = self._plans[k][i]
        nodes = [self._tape[m][which] for m, which in sp.keys]
        lags = self.lags if (torch.is_grad_enabled() and self.lags.requires_grad) else None
        y_lags = DdeTapeGatherFn.apply(self._backend, sp, lags, *nodes)
        f = as_operand(self.func(t0, y0, y_lags), like=y0)
        if i == 0:
            self._tape[k][1] = f
        self.__dict__["_stage"] = i + 1
        return f

    def call_func(self, t, y0):
        raise NotImplementedError("StepsDDE evaluates func(t, y, y_lags) through move(): the delayed states belong to a planned stage")

    def on_integrate_step_end(self, y0=None, y1=None, t0=None, t1=None):
        d = self.__dict__
        d["_k"], d["_stage"] = self._k + 1, 0
        if not torch.is_grad_enabled() and self._k < len(self._keep_from):
            keep = self._keep_from[self._k]
            for m in [m for m in self._tape if m < keep]:
                del self._tape[m]
