"""Fixed-grid solvers on the HIP combine kernel.

Reference: paddlexde/solver/base_fixed_solver.py:14-197.  The loop structure, the ``step`` protocol
``(t0, t1, y0) -> (y1, dy0)``, the option names and the output layout (``concat(axis=-2)``,
SURVEY D3) are the reference's; every ``fuse`` (``dy * dt + y0``, xde/base_ode.py:58) and every
stage formula is one xde_stage_combine launch instead of 2-9 eager element-wise ops.

Times: the reference slices ``time_grid[i-1:i]`` (shape ``[1]`` tensors) and derives stage times with
eager ops.  Here the whole table of stage times is computed once on the host, in the time dtype and
with the reference's op order, and uploaded once; ``func`` receives shape-``[1]`` device views of it.
"""
import abc
import ctypes as C
import threading

import numpy as np
import torch

from .. import _hip
from ..xde.base_dde import DDE_DAMPING, BaseDDE
from ..xde.base_ode import BaseODE
from ..xde.base_sde import BaseSDE
from ..xde.base_xde import BaseXDE
from ._autograd import (CombineFn, InterpRowsFn, SdeEulerFn, SdeGnEulerFn, SdeKlAccFn, SdeKlEulerFn, SdeMilsteinFn, SdeRheunCorrectFn, SdeRheunPredictFn,
                        SdeSrkStage1Fn, SdeSrkStage2Fn, SdeSrkStepFn, SdeSupportFn)
from ._common import as_operand, np_dtype, storage_ptr, t_span_to_host, upload

_one_third = 1 / 3
_two_thirds = 2 / 3
_one_sixth = 1 / 6
# what rk4_alt_step_func hands to move (FixedSolver.time_values): dt, dt/3, t0 + dt/3, t0 + 2dt/3 (base_fixed_solver.py:168-174)
RK4_ALT_TIME_VALUES = ((1.0, False), (_one_third, False), (_one_third, True), (_two_thirds, True))


def sde_step_scalars(dt, dtype):
    """``(dt, s)`` of an SDE step as the kernels take them (Python floats): ``s = sqrt(|dt|)`` computed in float64 from the host ``dt``
    (time dtype) and rounded to the state dtype."""
    return float(dt), float(np_dtype(dtype)(np.sqrt(abs(np.float64(dt)))))


def _step_size_value(step_size):
    """``step_size``: a Python or numpy number or a 1-element tensor, read once on the host; finite and > 0."""
    size = step_size.numel() if torch.is_tensor(step_size) else np.size(step_size)
    if size != 1:
        raise ValueError("step_size must be a number or a 1-element tensor, got {} elements".format(size))
    if torch.is_tensor(step_size):
        h = float(step_size.detach().reshape(-1)[0].item())
    else:
        h = float(np.asarray(step_size, dtype=np.float64).reshape(-1)[0])
    if not np.isfinite(h) or h <= 0:
        raise ValueError("step_size must be finite and > 0, got {!r}".format(h))
    return h


def step_size_grid(t_host, h):
    """The grid of ``step_size = h`` over the output times ``t_host`` (numpy, time dtype): the reference's formula
    (base_fixed_solver.py:67-89) in the direction ``d`` of the span, computed in the time dtype —
    ``niters = ceil((t[-1] - t[0]) / (d*h) + 1)``, ``grid = arange(niters) * (d*h) + t[0]``, ``grid[-1] = t[-1]``.  Deviation: every
    interior point that is not strictly before ``t[-1]`` in direction ``d`` (rounding can put one there) is dropped, so the grid is
    strictly monotone where the reference's would step backwards."""
    tt = t_host.dtype.type
    t0, t1 = t_host[0], t_host[-1]
    d = -1 if t1 < t0 else 1
    dh = tt(d * tt(h))
    niters = int(np.ceil((t1 - t0) / dh + tt(1)))
    grid = np.arange(0, niters, dtype=tt) * dh + t0
    grid[-1] = t1
    inner = grid[1:-1]
    keep = (inner < t1) if d > 0 else (inner > t1)
    return np.concatenate([grid[:1], inner[keep], grid[-1:]]) if niters > 1 else grid


class _SubSteps:
    """The host plan of a solve, for all grid steps at once: per step, the output rows it produces —
    ``(j, kind, (w0, w1, w2, w3))`` with ``kind`` one of ``_hip.XDE_ROW_*`` — in output order.  ``grid`` None is the plain plan: the
    grid is ``t_host`` itself and step ``k`` produces row ``k + 1`` as a copy of the step's end, whatever the times are (repeated
    and non-monotone ones included: every interval is a step)."""

    def __init__(self, t_host, grid, interp):
        self.plain = grid is None
        if self.plain:
            self.rows = [[(k + 1, _hip.XDE_ROW_COPY_B, (0.0, 0.0, 0.0, 0.0))] for k in range(len(t_host) - 1)]
            self.end_row = list(range(1, len(t_host)))
            return
        tt = t_host.dtype.type
        d = -1 if grid[-1] < grid[0] else 1
        n_steps = len(grid) - 1
        self.rows = [[] for _ in range(n_steps)]
        self.end_row = [None] * n_steps  # per step: the output row that is a copy of the step's end (the final combine may write it)
        if n_steps == 0 or len(t_host) < 2:
            return
        tj = t_host[1:]
        # the step that produces output j: the first whose end has reached t[j] (torchdiffeq's rule; the reference's commented-out
        # `while` at base_fixed_solver.py:130)
        k = np.clip(np.searchsorted(d * grid, d * tj, side="left") - 1, 0, n_steps - 1)
        ta, tb = grid[k], grid[k + 1]
        kinds = np.where(tj == ta, _hip.XDE_ROW_COPY_A, np.where(tj == tb, _hip.XDE_ROW_COPY_B, _hip.XDE_ROW_INTERP))
        with np.errstate(all="ignore"):
            h = (tj - ta) / (tb - ta)  # interp_fn.py:4-20, in the time dtype, the reference's op order
            if interp == "cubic":
                dt = tb - ta
                w = [(1 + 2 * h) * (1 - h) * (1 - h), h * (1 - h) * (1 - h) * dt, h * h * (3 - 2 * h), h * h * (h - 1) * dt]
            else:
                z = np.zeros_like(h)
                w = [h, z, z, z]
        w = np.stack([np.asarray(x, dtype=tt) for x in w], axis=1).astype(np.float64)
        if interp not in ("linear", "cubic"):
            off = np.nonzero(kinds == _hip.XDE_ROW_INTERP)[0]
            if len(off):
                raise ValueError("output time {} lies strictly inside a grid step: interp={!r} takes outputs on grid points only "
                                 "(use interp='linear' or 'cubic')".format(tj[off[0]].item(), interp))
        for j in range(len(tj)):
            self.rows[int(k[j])].append((j + 1, int(kinds[j]), tuple(w[j])))
            if kinds[j] == _hip.XDE_ROW_COPY_B and self.end_row[int(k[j])] is None:
                self.end_row[int(k[j])] = j + 1

    def needs_a(self, k):
        return any(kind != _hip.XDE_ROW_COPY_B for _, kind, _ in self.rows[k])


class FixedSolver(metaclass=abc.ABCMeta):
    order: int

    steps_sde = False  # the step is a convergent scheme for SDEs (a BaseSDE problem): Euler, as Euler-Maruyama, Milstein and SRK (Ito), ReversibleHeun (Stratonovich)
    steps_logqp = False  # the SDE step also accumulates the KL term of a latent SDE (sdeint's options logqp / prior_drift): Euler, Milstein
    logqp_refusal = "its step has no KL accumulation"  # why not, where steps_sde and not steps_logqp (SRK, ReversibleHeun)
    steps_matrix_noise = False  # the SDE step takes general and scalar noise (BaseSDE(..., noise_type=...)): Euler (xde_sde_gn_step)
    # why not, where steps_sde and not steps_matrix_noise (Milstein and SRK; ReversibleHeun states its own)
    matrix_noise_refusal = "its scheme assumes commutative, diagonal noise; for a [D, M] diffusion it would need Levy areas"

    graphable = True  # the step's control flow does not depend on data (False: AdamsBashforthMoulton)
    GRAPH_MIN_STEPS = 4
    AUTO_GRAPH_MIN_STEPS = 24  # pipeline="auto": steps needed to amortise a capture (~2 ms against ~100 us saved per step)
    AUTO_GRAPH_MAX_BYTES = 8 << 20  # ... and only for launch-bound (small) states

    def __init__(self, xde, y0, step_size=None, grid_constructor=None, interp="linear", perturb=False, pipeline="auto", logqp=False,
                 **kwargs):
        self.xde = xde
        self._logqp = bool(logqp)
        self.logqp = None  # what the last walk accumulated: the KL term per output interval (``_walk``)
        self.y0 = y0
        self.dtype = y0.dtype
        self.step_size = step_size
        self.interp = interp
        self.perturb = perturb
        if pipeline not in ("auto", "sync", "lag", "graph"):
            raise ValueError("pipeline must be 'auto', 'sync' or 'graph' ('lag' means 'sync' for a fixed grid)")
        self.pipeline = pipeline
        self._arm()  # (idle)

        # base_fixed_solver.py:45-47 — KeyError when absent, as in the reference
        self.atol = kwargs["atol"]
        self.rtol = kwargs["rtol"]
        self.norm = kwargs["norm"]

        if step_size is not None and grid_constructor is not None:
            raise ValueError("step_size and grid_constructor are mutually exclusive arguments.")
        # Sub-stepping (base_fixed_solver.py:49-89): the solve walks a grid of its own and produces each output time by interpolating
        # inside the grid step that brackets it — what the reference meant; its loop walks only len(t_span) grid points (:126-127), so
        # there it never worked.
        self._substep = step_size is not None or grid_constructor is not None
        if step_size is not None:
            self.step_size = _step_size_value(step_size)
            self.grid_constructor = None
        elif grid_constructor is not None:
            self.grid_constructor = grid_constructor
        else:
            self.grid_constructor = lambda y0, t: t

        self.move = self.xde.move
        self.fuse = self.xde.fuse
        self.on_integrate_step_end = self.xde.on_integrate_step_end
        # The reference binds this hook (base_fixed_solver.py:64) and never calls it; here it IS called, once per step of the eager
        # loop, as `xde.on_integrate_step_end(y0, y1, t0, t1)` (state before / after the step, device tensors; t0 / t1 the shape-[1]
        # device views the step itself received).  The base classes' hook does nothing, so only a wrapper that overrides it sees a
        # difference — and such a wrapper keeps the solve on the eager loop: a captured step cannot call back into Python, so
        # pipeline="graph" refuses it and "auto" does not capture.
        self._step_end_hook = getattr(type(xde), "on_integrate_step_end", None) is not BaseXDE.on_integrate_step_end
        if self._step_end_hook and pipeline == "graph":
            raise NotImplementedError("pipeline='graph' replays a captured step and cannot call xde.on_integrate_step_end; "
                                      "use pipeline='sync' (or the default 'auto', which then keeps the eager loop)")
        # the wrapper's fuse is what xde_stage_combine computes: BaseODE's `dy*dt + y0` or BaseDDE's damped form; BaseSDE's
        # Euler-Maruyama update is xde_sde_em_step (Milstein adds its correction to it: xde_sde_milstein_step; SRK is xde_sde_srk_*)
        fuse_impl = getattr(type(xde), "fuse", None)
        self._sde = fuse_impl is BaseSDE.fuse
        self._matrix_noise = False  # SDE: the diffusion is a [D, M] matrix per row (BaseSDE's noise_type "general" or "scalar")
        if self._sde:
            if not self.steps_sde:
                raise NotImplementedError("{} does not step SDEs: its tableau does not converge for Ito SDEs; use Euler "
                                          "(Euler-Maruyama) or Milstein or SRK (or ReversibleHeun, Stratonovich)".format(type(self).__name__))
            if pipeline == "graph":
                raise NotImplementedError("pipeline='graph' replays one captured step, which cannot advance the SDE's grid-step "
                                          "counter; use pipeline='sync' (or the default 'auto', which keeps the eager loop for SDEs)")
            if interp == "cubic":
                raise NotImplementedError("interp='cubic' needs the derivative at both ends of a step, which an SDE path does not "
                                          "have; use interp='linear'")
            self._damping = 0.0
            self._matrix_noise = getattr(xde, "noise_type", "diagonal") != "diagonal"
            if self._matrix_noise and not self.steps_matrix_noise:
                raise NotImplementedError("{} does not step {} noise: {}; solver=Euler steps general and scalar noise (one fused launch "
                                          "per step)".format(type(self).__name__, xde.noise_type, self.matrix_noise_refusal))
            if self._matrix_noise and self._logqp:
                raise NotImplementedError("logqp takes diagonal noise only: with a [D, M] diffusion (f - h)/g would become a linear solve "
                                          "per row; solver=Euler steps general and scalar noise without logqp, and logqp with "
                                          "noise_type='diagonal'")
            if self._logqp and not self.steps_logqp:
                raise NotImplementedError(
                    "{} does not accumulate logqp: {}; use solver=Euler (one fused launch per step) or solver=Milstein".format(
                        type(self).__name__, self.logqp_refusal))
            if self._logqp and getattr(xde, "h", None) is None:
                raise ValueError("logqp needs the prior drift: BaseSDE(..., prior=h) (sdeint: options={'logqp': True, 'prior_drift': h})")
        elif self._logqp:
            raise NotImplementedError("logqp is the KL term of a latent SDE: only sdeint(..., solver=Euler) or solver=Milstein accumulate it")
        elif fuse_impl is BaseODE.fuse:
            self._damping = 0.0
        elif fuse_impl is BaseDDE.fuse:
            self._damping = DDE_DAMPING
        else:
            raise NotImplementedError("only BaseODE.fuse / BaseDDE.fuse / BaseSDE.fuse are mapped onto the HIP kernels")

        self.backend = _hip.get_backend()
        self.nfe = 0
        self._tdev_cache = {}
        self._carry = None  # ReversibleHeun: the (yh, fh, gh) the last step left
        self._acc = None  # logqp: the running KL sum of every row the last step left (float64 y0.shape[:-1]; None: zero)

    # -- per-step state ---------------------------------------------------------------------------
    def _arm(self, dt=None, t0_host=None, row=None, y1_out=None, k=None, ctrls=None, rec=None):
        """The state ``step`` reads while a walk drives it, set here and nowhere else.  ``_arm()`` is the idle state, in which a
        ``step()`` called from outside reads its times from the device: whoever arms does so inside a ``try`` whose ``finally`` is
        ``self._arm()``, so the state is idle again also after ``func`` raised or a capture was refused."""
        self._dt = dt  # host dt (numpy scalar of the time dtype)
        self._t0_host = t0_host  # host t0 of the step
        self._row = row  # the step's row of the uploaded time table
        self._y1_out = y1_out  # where the step's final combine should write (a slice of the output, a hand-over buffer)
        self._k = k  # SDE: the 0-based grid step of the walk (the generator's counter); None: a bare step() is step 0
        self._g_ctrls = ctrls  # graph pipeline: device dt sources of the step's combines, in call order ...
        self._g_slot = 0  # ... and the next one to hand out
        self._rec = rec  # recording pass: the dt every combine of a step receives, for all steps at once

    # -- framework call -----------------------------------------------------------------------
    def _f(self, t, dt, y):
        if self._rec is not None:
            return None
        self.nfe += 1
        f = self.move(t, dt, y)
        f = as_operand(f, like=y)
        if storage_ptr(f) == storage_ptr(y):
            f = f.clone()
        return f

    def _combine(self, y0, ks, coef, mode, dt, scale=1.0, out=None, emit=None):
        """One xde_stage_combine launch.  ``emit`` (a FUSE launch that is not being differentiated): the weights of the step's final
        sum over the operands this launch holds — it then also writes that partial sum and ``(out, partial)`` is returned."""
        if self._rec is not None:
            self._rec.append(dt)
            return None if emit is None else (None, None)
        damp = self._damping if mode != _hip.COMBINE_RK else 0.0
        part = torch.empty_like(y0) if emit is not None else None
        if self._g_ctrls is not None:  # graph pipeline: dt is read from device memory (rewritten before every replay)
            ctrl = self._g_ctrls[self._g_slot]
            self._g_slot += 1
            if out is None:
                out = torch.empty_like(y0)
            self.backend.stage_combine(out, y0, ks, coef, mode, scale=scale, ctrl=ctrl, damping=damp, out2=part, coef2=emit)
            return out if emit is None else (out, part)
        if emit is None and torch.is_grad_enabled() and (y0.requires_grad or any(k.requires_grad for k in ks)):
            # discretise-then-optimise: keep the autograd graph through the combine
            return CombineFn.apply(self.backend, list(coef), mode, scale, float(dt), damp, y0, *ks)
        if out is None:
            out = torch.empty_like(y0)
        self.backend.stage_combine(out, y0, ks, coef, mode, scale=scale, dt_host=float(dt), damping=damp, out2=part, coef2=emit)
        return out if emit is None else (out, part)

    def _sde_prologue(self, t0, dtt, y0, dt):
        """What every SDE step starts from: drift and diffusion at ``(t0, y0)`` as operands, ``dt``, ``s = sqrt(|dt|)``,
        ``c = 0.5/sqrt(|dt|)`` and ``c3 = 1/(6|dt|)`` (both 0 for a zero-length step) computed in float64 and rounded to the state dtype,
        the grid step ``k``, and whether an operand is being differentiated.  Returns ``(f, g, dt, s, c, c3, k, grad)``, the scalars as
        Python floats."""
        self.nfe += 1
        f, g = self.move(t0, dtt, y0)
        f, g = as_operand(f, like=y0), (as_operand(g) if self._matrix_noise else as_operand(g, like=y0))  # (general: [.., D, M])
        T = np_dtype(y0.dtype)
        root = np.sqrt(abs(np.float64(dt)))
        c = T(0.5 / root) if root > 0 else T(0.0)
        c3 = T(1.0 / (6.0 * abs(np.float64(dt)))) if root > 0 else T(0.0)
        k = self._k if self._k is not None else 0  # (a step() call outside integrate() is the first step of a walk)
        grad = torch.is_grad_enabled() and (y0.requires_grad or f.requires_grad or g.requires_grad)
        return f, g, float(dt), float(T(root)), float(c), float(c3), k, grad

    def _em_step(self, t0, dtt, y0, dt):
        """One Ito Euler-Maruyama step of a BaseSDE: ``y1 = (y0 + f*dt) + g*(s*Z)``, ``s = sqrt(|dt|)`` in the state dtype, Z the
        normals of (xde.seed, grid step k) — one xde_sde_em_step launch (SdeEulerFn when an operand is differentiated).  Under general
        or scalar noise ``g`` is ``[.., D, M]`` and the step is ``y1 = (y0 + f*dt) + sum_m g[.., m]*(s*Z[.., m])``, Z over the flat
        ``[rows, M]`` array: one xde_sde_gn_step launch in its place (SdeGnEulerFn).  Returns ``(y1, f)``."""
        f, g, dt, s, _, _, k, grad = self._sde_prologue(t0, dtt, y0, dt)
        if self._matrix_noise:
            if grad:
                return SdeGnEulerFn.apply(self.backend, dt, s, self.xde.seed, k, y0, f, g), f
            out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
            self.backend._sde_gn_step(out, y0, f, g, dt, s, self.xde.seed, k)
            return out, f
        if self._logqp:
            return self._kl_em_step(t0, y0, f, g, dt, s, k, grad), f
        if grad:
            return SdeEulerFn.apply(self.backend, dt, s, self.xde.seed, k, y0, f, g), f
        out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
        self.backend._sde_em_step(out, y0, f, g, dt, s, self.xde.seed, k)
        return out, f

    def _kl_em_step(self, t0, y0, f, g, dt, s, k, grad):
        """The Euler-Maruyama step of a latent SDE (``logqp``): the prior drift ``h = prior(t0, y0)`` next to ``f`` and ``g``, and ONE
        xde_sde_kl_step launch in the place of xde_sde_em_step — the same ``y1`` bit for bit, and the running KL sum of every row
        (``self._acc``: float64 ``y0.shape[:-1]``, None before the first step) advanced by ``sum(((f - h)/g)**2, -1) * (0.5*dt)``.
        Through SdeKlEulerFn when an operand is differentiated.  Returns ``y1``."""
        h = as_operand(self.xde.prior(t0, y0), like=y0)
        acc0 = self._acc
        if grad or (torch.is_grad_enabled() and (h.requires_grad or (acc0 is not None and acc0.requires_grad))):
            y1, self._acc = SdeKlEulerFn.apply(self.backend, dt, s, self.xde.seed, k, y0, f, g, h, acc0)
            return y1
        out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
        acc1 = torch.empty(y0.shape[:-1], dtype=torch.float64, device=y0.device)
        self.backend._sde_kl_step(out, acc1, y0, f, g, h, acc0, dt, s, self.xde.seed, k)
        self._acc = acc1
        return out

    def _kl_accumulate(self, t0, y0, f, g, dt):
        """The KL sum of a latent SDE advanced over a step whose state update has launches of its own (Milstein: the KL column has zero
        diffusion, so its Milstein update is the Euler one): ``h = prior(t0, y0)`` and one accumulate-only xde_sde_kl_step launch, which
        reads ``f, g, h`` only.  Through SdeKlAccFn when an operand is differentiated."""
        h = as_operand(self.xde.prior(t0, y0), like=y0)
        acc0 = self._acc
        if torch.is_grad_enabled() and (f.requires_grad or g.requires_grad or h.requires_grad or (acc0 is not None and acc0.requires_grad)):
            self._acc = SdeKlAccFn.apply(self.backend, dt, f, g, h, acc0)
            return
        acc1 = torch.empty(y0.shape[:-1], dtype=torch.float64, device=y0.device)
        self.backend._sde_kl_step(None, acc1, None, f, g, h, acc0, dt, 0.0, 0, 0)
        self._acc = acc1

    def _milstein_step(self, t0, dtt, y0, dt):
        """One derivative-free Milstein step of a BaseSDE (Kloeden & Platen's explicit strong order 1.0 scheme, Ito, diagonal noise):
        the support point ``yb = (y0 + f*dt) + g*s`` (one launch), ``gb = diffusion(t0, yb)``, and
        ``y1 = ((y0 + f*dt) + g*w) + (gb - g)*q`` with ``w = s*Z``, ``q = c*(w*w - |dt|)`` (one xde_sde_milstein_step launch) —
        ``s = sqrt(|dt|)`` and ``c = 0.5/sqrt(|dt|)`` computed in float64 and rounded to the state dtype, ``c = 0`` for a zero-length
        step (which then returns y0), Z the normals of (xde.seed, grid step k) as in ``_em_step``.  Through SdeSupportFn /
        SdeMilsteinFn when an operand is differentiated.  ``nfe`` counts steps, as Euler's does: one per step, which here stands for
        one drift and two diffusion evaluations.  Returns ``(y1, f)``."""
        f, g, dt, s, c, _, k, grad = self._sde_prologue(t0, dtt, y0, dt)
        if grad:
            yb = SdeSupportFn.apply(self.backend, dt, s, y0, f, g)
            gb = as_operand(self.xde.diffusion(t0, yb), like=y0)
            y1 = SdeMilsteinFn.apply(self.backend, dt, s, c, self.xde.seed, k, y0, f, g, gb)
            if self._logqp:
                self._kl_accumulate(t0, y0, f, g, dt)
            return y1, f
        yb = torch.empty_like(y0)
        self.backend._sde_milstein_support(yb, y0, f, g, dt, s)
        gb = as_operand(self.xde.diffusion(t0, yb), like=y0)
        out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
        self.backend._sde_milstein_step(out, y0, f, g, gb, dt, s, c, self.xde.seed, k)
        if self._logqp:  # (after the step's own two launches, which stay as they are; y0 is not the step's output buffer)
            self._kl_accumulate(t0, y0, f, g, dt)
        return out, f

    def _srk_step(self, t0, t1, dtt, t34, t14, y0, dt):
        """One SRK step of a BaseSDE (Roessler's SRI1W1: derivative-free, strong order 1.5, Ito, diagonal noise), three launches
        around the evaluations they feed (the formulas in their written op order: include/xde_hip_sde.h) —
        stage 1 writes ``Y2, G2, G3`` from ``a1 = drift(t0, y0)``, ``b1 = diffusion(t0, y0)``; then ``a2 = drift(t0 + 3/4 dt, Y2)``,
        ``b2 = diffusion(t0 + 1/4 dt, G2)``, ``b3 = diffusion(t1, G3)``; stage 2 writes ``G4``; ``b4 = diffusion(t0 + 1/4 dt, G4)``; the
        step writes ``y1``.  Stage 1 and the step draw Z and V of (xde.seed, grid step k) in registers; ``s``, ``c`` and ``c3`` as in
        ``_sde_prologue``, ``c = c3 = 0`` for a zero-length step (which then returns y0).  Through SdeSrkStage1Fn / SdeSrkStage2Fn /
        SdeSrkStepFn when an operand is differentiated.  ``nfe`` counts steps, as Euler's does: one per step, which here stands for 2
        drift and 4 diffusion evaluations.  Returns ``(y1, a1)``."""
        a1, b1, dt, s, c, c3, k, grad = self._sde_prologue(t0, dtt, y0, dt)
        xde, seed = self.xde, self.xde.seed
        drift = lambda t, y: as_operand(xde.call_func(t, y), like=y0)  # noqa: E731
        diffusion = lambda t, y: as_operand(xde.diffusion(t, y), like=y0)  # noqa: E731
        if grad:
            Y2, G2, G3 = SdeSrkStage1Fn.apply(self.backend, dt, s, seed, k, y0, a1, b1)
            a2, b2, b3 = drift(t34, Y2), diffusion(t14, G2), diffusion(t1, G3)
            b4 = diffusion(t14, SdeSrkStage2Fn.apply(self.backend, dt, s, y0, a1, b1, b2, b3))
            return SdeSrkStepFn.apply(self.backend, dt, s, c, c3, seed, k, y0, a1, a2, b1, b2, b3, b4), a1
        Y2, G2, G3, G4 = (torch.empty_like(y0) for _ in range(4))
        self.backend._sde_srk_stage1(Y2, G2, G3, y0, a1, b1, dt, s, seed, k)
        a2, b2, b3 = drift(t34, Y2), diffusion(t14, G2), diffusion(t1, G3)
        self.backend._sde_srk_stage2(G4, y0, a1, b1, b2, b3, dt, s)
        b4 = diffusion(t14, G4)
        out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
        self.backend._sde_srk_step(out, y0, a1, a2, b1, b2, b3, b4, dt, s, c, c3, seed, k)
        return out, a1

    def _rheun_step(self, t0, t1, dtt, y0, dt):
        """One reversible Heun step of a BaseSDE (Kidger, Foster, Li, Lyons 2021: Stratonovich, diagonal noise), two launches around the
        one evaluation they feed (the formulas in their written op order: include/xde_hip_sde.h) — predict writes
        ``yh1 = (((y0 + y0) - yh0) + fh0*dt) + gh0*w``; then ``fh1 = drift(t1, yh1)``, ``gh1 = diffusion(t1, yh1)``; correct writes
        ``y1 = (y0 + (fh0 + fh1)*(0.5*dt)) + (gh0 + gh1)*(0.5*w)``, ``w = s*Z`` on the Z of (xde.seed, grid step k) as in ``_em_step``.
        The carried ``(yh, fh, gh)`` lives in ``self._carry``: at grid step 0 and on a step() outside a walk it is
        ``(y0, drift(t0, y0), diffusion(t0, y0))``, afterwards what the step before left.  Through SdeRheunPredictFn /
        SdeRheunCorrectFn when an operand is differentiated.  ``nfe`` counts steps.  Returns ``(y1, fh0)``."""
        self.nfe += 1
        xde, seed = self.xde, self.xde.seed
        k = self._k if self._k is not None else 0
        if not self._k or self._carry is None:
            f, g = self.move(t0, dtt, y0)
            self._carry = (y0, as_operand(f, like=y0), as_operand(g, like=y0))
        yh0, f0, g0 = self._carry
        dt, s = sde_step_scalars(dt, y0.dtype)
        grad = torch.is_grad_enabled() and any(x.requires_grad for x in (y0, yh0, f0, g0))
        if grad:
            yh1 = SdeRheunPredictFn.apply(self.backend, dt, s, seed, k, y0, yh0, f0, g0)
        else:
            yh1 = torch.empty_like(y0)
            self.backend._sde_rheun_predict(yh1, y0, yh0, f0, g0, dt, s, 1, seed, k)
        f1, g1 = as_operand(xde.call_func(t1, yh1), like=y0), as_operand(xde.diffusion(t1, yh1), like=y0)
        self._carry = (yh1, f1, g1)
        if grad or (torch.is_grad_enabled() and (f1.requires_grad or g1.requires_grad)):
            return SdeRheunCorrectFn.apply(self.backend, dt, s, seed, k, y0, f0, f1, g0, g1), f0
        out = self._y1_out if self._y1_out is not None else torch.empty_like(y0)
        self.backend._sde_rheun_correct(out, y0, f0, f1, g0, g1, dt, s, 1, seed, k)
        return out, f0

    def _combine_pre(self, y0, pre, ks, coef, dt, scale, out=None):
        """The final weighted sum with its leading terms pre-summed (xde_stage_combine_pre_weighted): reads y0, ``pre`` and the newest
        derivative(s)."""
        if self._rec is not None:
            self._rec.append(dt)
            return None
        if out is None:
            out = torch.empty_like(y0)
        ctrl = None
        if self._g_ctrls is not None:
            ctrl = self._g_ctrls[self._g_slot]
            self._g_slot += 1
        self.backend.stage_combine_pre_weighted(out, y0, pre, ks, coef, scale=scale, dt_host=0.0 if ctrl is not None else float(dt), ctrl=ctrl,
                                                damping=self._damping)
        return out

    def _presum_ok(self, y0, ks):
        """Whether the last stage-input launch may emit the final sum's leading terms: nothing here is being differentiated (the
        autograd node of a combine has one output).  Same bits either way."""
        if self._rec is not None:
            return True  # (recording pass: the same launches, in the same order, either way)
        return not (torch.is_grad_enabled() and (y0.requires_grad or any(k.requires_grad for k in ks)))

    # -- time handling ----------------------------------------------------------------------------
    def _host_dt(self, t0, t1):
        if self._dt is not None:
            return self._dt
        return np_dtype(t0.dtype)((t1 - t0).item())  # direct step() call outside integrate(): one device read

    # per value the step hands to ``move`` besides t0 / t1, in the order ``_times`` returns them: (multiple of dt, whether the value
    # is that offset from t0 — a stage time — or the multiple itself)
    time_values = ()

    def _time_table(self, t_host):
        """Per step of ``t_host`` (host, time dtype): the values the step passes to ``move``, for all steps at once — element-wise
        numpy arithmetic in the time dtype gives the values the per-step scalar expressions of ``_times`` give."""
        dts = t_host[1:] - t_host[:-1]
        cols = [t_host[:-1] + dts * c if offset else dts * c for c, offset in self.time_values]
        return np.stack(cols, axis=1).astype(t_host.dtype, copy=False) if cols else np.empty((len(dts), 0), dtype=t_host.dtype)

    def _times(self, t0, dt):
        if self._row is not None:
            return [self._row[j : j + 1] for j in range(len(self.time_values))]
        # a step() outside a walk, or the cubic's extra step: constants, one device read of t0 when a value is a stage time
        t0h = type(dt)(t0.item()) if any(offset for _, offset in self.time_values) else None
        return [self._tdev(t0h + dt * c if offset else dt * c, t0) for c, offset in self.time_values]

    def _tdev(self, value, like):
        key = (float(value), like.dtype)
        t = self._tdev_cache.get(key)
        if t is None:
            t = torch.full((1,), float(value), dtype=like.dtype, device=like.device)
            if len(self._tdev_cache) < 1024:
                self._tdev_cache[key] = t
        return t

    @abc.abstractmethod
    def step(self, t0, t1, y0):
        """Propose a step from t0 to t1. Returns (y1, dy0)."""
        raise NotImplementedError

    # -- base_fixed_solver.py:103-144 ------------------------------------------------------------
    def integrate(self, t_span):
        return self._walk(*self._plan(t_span))

    def _plan(self, t_span):
        """What ``_walk`` takes for a solve over the output times ``t_span``: ``(grid, grid_dev, plan, pred_len)``."""
        if not torch.is_tensor(t_span):
            t_span = torch.as_tensor(t_span)
        y0 = self.y0
        self.backend.require_device(y0)
        if y0.dim() < 2:
            raise ValueError("fixed solvers concatenate on axis -2: y0 needs >= 2 dims (reference layout [..., L, D])")
        t_dtype = t_span.dtype if t_span.dtype in (torch.float32, torch.float64) else torch.float32
        t_host = t_span_to_host(t_span, np_dtype(t_dtype))
        grid = self._grid(t_host, t_span) if self._substep else t_host
        if grid is t_host or np.array_equal(grid, t_host):  # (a grid that IS t_span: the plain plan, bit for bit)
            # (values rounded to the time dtype on the host, as t_span.astype would; no blocking pageable copy)
            t_dev = t_span.detach().to(device=y0.device, dtype=t_dtype) if t_span.is_cuda else upload(t_host, y0.device)
            return t_host, t_dev, _SubSteps(t_host, None, self.interp), len(t_host)
        plan = _SubSteps(t_host, grid, self.interp)  # (validated before the first launch)
        return grid, upload(grid, y0.device), plan, len(t_host)

    def _grid(self, t_host, t_span):
        """The grid of a sub-stepped solve (step_size / grid_constructor) on the host, in the time dtype, validated (before anything
        runs)."""
        tt = t_host.dtype.type
        d = -1 if t_host[-1] < t_host[0] else 1
        if len(t_host) > 1 and np.any(d * np.diff(t_host) < 0):
            raise ValueError("with step_size / grid_constructor, t_span must be monotone in one direction (repeated times are allowed)")
        if self.grid_constructor is None:
            return step_size_grid(t_host, self.step_size)
        grid = t_span_to_host(self.grid_constructor(self.y0, t_span), tt)
        if grid.ndim != 1 or len(grid) < 1:
            raise ValueError("grid_constructor must return a 1-D grid, got shape {}".format(grid.shape))
        # (the reference asserts paddle.equal_all on both ends, base_fixed_solver.py:120-121)
        assert grid[0] == t_host[0] and grid[-1] == t_host[-1], "grid_constructor's grid must start at t_span[0] and end at t_span[-1]"
        if len(grid) > 1 and not np.all(d * np.diff(grid) > 0):
            raise ValueError("grid_constructor's grid must be strictly monotone in the direction of t_span")
        return grid

    def _walk(self, grid, grid_dev, plan, pred_len):
        """The solve over ``grid`` (host, time dtype; ``grid_dev`` its device copy), one step per grid interval, writing the
        ``pred_len`` output rows ``plan`` assigns to the steps.  Plain plan: every step's end is a row, stored by the step's final
        combine where it can write into the solution (rows that are contiguous, 16-byte aligned slices, nothing differentiated) and by
        a copy where it cannot.  Sub-stepped plan: output ``j`` is produced by the first grid step whose end has reached its time — an
        exact copy of the state at either end of the step, or the interpolant (``interp``) inside it — with one xde_interp_rows
        launch per step that produces rows (per XDE_INTERP_MAX_ROWS of them); a row at the step's end may be written by the final
        combine directly, and steps hand the state over through a ping-pong pair of buffers."""
        y0 = self.y0
        n_steps = len(grid) - 1
        # one upload: per step [t-like values the step passes to move()]
        table = upload(self._time_table(grid), y0.device) if (n_steps > 0 and self.time_values) else None

        tracking = torch.is_grad_enabled() and y0.requires_grad
        y0 = as_operand(y0 if tracking else y0.detach())
        L, D = y0.shape[-2], y0.shape[-1]
        lead = y0.shape[:-2]
        out = torch.empty(*lead, pred_len * L, D, dtype=y0.dtype, device=y0.device)
        direct = (int(np.prod(lead)) == 1) if len(lead) else True  # output rows are contiguous slices
        out.narrow(-2, 0, L).copy_(y0)
        # logqp: the cumulative KL sum of every row at every output time (float64; [0] is zero), from the steps' running sums
        self._acc, self.logqp = None, None
        cum = [torch.zeros(y0.shape[:-1], dtype=torch.float64, device=y0.device)] + [None] * (pred_len - 1) if self._logqp else None
        if n_steps == 0:  # a one-point grid (every output time is t[0]): every row is y0, as the plain walk's zero-length steps give
            for j in range(1, pred_len):
                out.narrow(-2, j * L, L).copy_(y0)
            if cum is not None:
                self.logqp = self._logqp_intervals([cum[0]] * pred_len, y0)
            return out

        # pipeline="graph": one captured step replayed over the grid (no autograd, data-independent step).  "auto" (default)
        # takes it for inference-style calls (grad mode off) on small states with enough steps to pay for the capture, behind
        # the capture guard, and falls back to the eager loop below if the capture is refused or fails.
        can_graph = (self.graphable and not self._sde and not self._step_end_hook and not tracking and not torch.is_grad_enabled() and table is not None and y0.is_cuda
                     and self.interp != "cubic" and n_steps >= self.GRAPH_MIN_STEPS
                     and threading.current_thread() is threading.main_thread() and not torch.cuda.is_current_stream_capturing())
        if self.pipeline == "graph" and can_graph:
            return self._integrate_graph(grid, grid_dev, table, y0, out, L, sub=plan)
        if (self.pipeline == "auto" and can_graph and n_steps >= self.AUTO_GRAPH_MIN_STEPS
                and y0.numel() * y0.element_size() <= self.AUTO_GRAPH_MAX_BYTES):
            nfe0 = self.nfe
            try:
                return self._integrate_graph(grid, grid_dev, table, y0, out, L, guard=True, sub=plan)
            except Exception:  # refused by the guard, or func cannot be captured: eager loop, from the start
                self.nfe = nfe0

        cubic = self.interp == "cubic"
        # (the plain walk makes a state per step; a hook may keep the states it is handed, and autograd keeps them anyway)
        # (logqp in grad mode: the prior's autograd graph may keep the state it was evaluated at even where the step itself is not
        # differentiated — y0, drift and diffusion without a gradient — so every step makes a state of its own: neither a hand-over
        # buffer, which a later step's kernel would overwrite behind autograd's back, nor a slice of the solution)
        own_state = self._logqp and torch.is_grad_enabled()
        bufs = None if (plan.plain or tracking or self._step_end_hook or own_state) else (torch.empty_like(y0), torch.empty_like(y0))
        y = y0
        try:
            for k in range(n_steps):
                t0, t1 = grid_dev[k : k + 1], grid_dev[k + 1 : k + 2]
                rows, jb = plan.rows[k], plan.end_row[k]
                dst = dst_b = None
                if jb is not None:
                    dst = out.narrow(-2, jb * L, L)
                    dst_b = dst.view(y0.shape) if (direct and dst.data_ptr() % 16 == 0) else None
                y1_out = None if own_state else (dst_b if dst_b is not None else (bufs[k % 2] if bufs is not None else None))
                self._arm(grid[k + 1] - grid[k], grid[k], table[k] if table is not None else None, y1_out, k)
                acc_a = self._acc
                y1, f_a = self.step(t0, t1, y)
                if cum is not None:
                    self._logqp_rows(cum, rows, acc_a, self._acc)
                if rows:
                    f_b = None
                    if cubic:
                        # base_fixed_solver.py:133-137: dy1 is the dy0 of step(t1, t1, y1) — only for steps that produce rows.  (For a
                        # row AT t1 the Hermite cubic is y1 itself, h00 = h10 = h11 = 0 and h01 = 1: only the NFE matter then.)
                        self._arm(dt=grid[k + 1] - grid[k + 1], t0_host=grid[k + 1], k=k)
                        _, f_b = self.step(t1, t1, y1)
                    if dst_b is not None and y1.data_ptr() == dst_b.data_ptr():
                        rows = [r for r in rows if r[0] != jb]  # (the final combine wrote it)
                    if not plan.plain:
                        self._write_rows(out, L, rows, y, y1, f_a, f_b)
                    elif rows:
                        dst.copy_(y1)  # (a differentiable copy when y1 carries an autograd graph)
                if self._step_end_hook:
                    self.on_integrate_step_end(y, y1, t0, t1)
                y = y1
        finally:
            self._arm()
            self._acc = None
        if cum is not None:
            self.logqp = self._logqp_intervals(cum, y0)
        return out

    @staticmethod
    def _logqp_rows(cum, rows, acc_a, acc_b):
        """The cumulative KL sum at the output rows ``(j, kind, w)`` of one grid step, from the running sums at its start (``acc_a``;
        None: zero) and end: a row at either end takes that sum, a row strictly inside takes ``acc_a + w*(acc_b - acc_a)`` with the
        linear weight the state's row takes — the scheme's integrand is constant over a step, so that is exact for the scheme.
        ``[rows]``-sized float64 framework arithmetic, off the hot path."""
        for j, kind, w in rows:
            if kind == _hip.XDE_ROW_COPY_B:
                cum[j] = acc_b
            elif kind == _hip.XDE_ROW_COPY_A:
                cum[j] = acc_a if acc_a is not None else torch.zeros_like(acc_b)
            else:
                cum[j] = acc_b * float(w[0]) if acc_a is None else acc_a + float(w[0]) * (acc_b - acc_a)

    @staticmethod
    def _logqp_intervals(cum, y0):
        """``logqp[..., i] = L(t_{i+1}) - L(t_i)`` from the cumulative sums ``cum`` (float64), in the state dtype: ``y0.shape[:-1] +
        (T - 1,)``."""
        if len(cum) < 2:
            return torch.zeros(y0.shape[:-1] + (0,), dtype=y0.dtype, device=y0.device)
        return torch.stack([b - a for a, b in zip(cum[:-1], cum[1:])], dim=-1).to(y0.dtype)

    def _write_rows(self, out, L, rows, y_a, y_b, f_a=None, f_b=None):
        """Rows ``(j, kind, w)`` of one grid step of a sub-stepped plan into ``out`` (``[..., T*L, D]``).  Through InterpRowsFn when an
        operand carries an autograd graph (discretise-then-optimise), else straight into the solution's layout."""
        if not rows:
            return
        kinds = [kind for _, kind, _ in rows]
        weights = [w for _, _, w in rows]
        cubic = self.interp == "cubic" and any(kind == _hip.XDE_ROW_INTERP for kind in kinds)
        ops = [as_operand(y_a), as_operand(y_b)] + ([as_operand(f_a), as_operand(f_b)] if cubic else [None, None])
        dsts = [out.narrow(-2, j * L, L) for j, _, _ in rows]
        if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in ops):
            vals = InterpRowsFn.apply(self.backend, kinds, weights, *ops)
            for g, dst in enumerate(dsts):
                dst.copy_(vals[g])
            return
        self.backend._interp_rows(dsts, kinds, weights, *ops)

    # -- hipGraph pipeline: one captured step, replayed over the grid ------------------------------------------------
    def _record_combine_dts(self, dts):
        """The ``dt`` argument of every ``_combine`` call of one step, in call order, as arrays over all steps: ``step`` is
        run once on the ARRAY of step sizes with ``func`` and the kernels switched off (its host arithmetic is element-wise
        numpy in the time dtype, so each entry is the scalar the eager loop would pass)."""
        row = torch.zeros(max(len(self.time_values), 1))
        self._arm(dt=dts, row=row, rec=[])
        try:
            self.step(row[0:1], row[0:1], None)
            return [np.broadcast_to(np.asarray(v), dts.shape).astype(np.float64) for v in self._rec]
        finally:
            self._arm()

    def _step_body(self, row, ctrls, y_cur, y_next):
        """One step on static buffers, as a graph replays it: the state in ``y_cur`` (the result is left there, through ``y_next``),
        the step's times in the device ``row`` (t0, t1, the step's time values) and the dt of every combine in the control blocks
        ``ctrls`` — the host-side dt and t0 are placeholders, nothing the kernels use derives from them."""
        tt = np_dtype(row.dtype)
        self._arm(dt=tt(1.0), t0_host=tt(0.0), row=row[2:], y1_out=y_next, ctrls=ctrls)
        try:
            y1, _ = self.step(row[0:1], row[1:2], y_cur)
        finally:
            self._arm()
        y_cur.copy_(y1)

    def _integrate_graph(self, t_host, t_dev, table, y0, out, L, sub, guard=False):
        """``options={"pipeline": "graph"}`` (no autograd, data-independent step): the first step runs eagerly, then ONE step
        — the combines, the framework ops of ``func``, the state hand-over — is captured into a hipGraph and replayed; per
        step the host rewrites the step's times and step sizes in device memory (two small copies) and stores the row.
        Same kernels, same operands: bit-identical to the eager loop.  For launch-latency-bound (small) states.
        ``t_host`` / ``t_dev`` are the grid and ``sub`` the plan: after the replay of a step the rows it produces are written outside
        the graph — the plain plan's by a copy of the state, a sub-stepped plan's by one xde_interp_rows launch from the state before
        the replay (one device copy) and after it."""
        dev = y0.device
        n_steps = len(t_host) - 1
        dts = t_host[1:] - t_host[:-1]
        dt_table = upload(np.stack(self._record_combine_dts(dts), axis=1), dev)  # [n_steps, K] fp64
        K = dt_table.shape[1]
        nb = C.sizeof(_hip.XdeCtrl)
        ctrls = torch.zeros(K * nb, dtype=torch.uint8, device=dev)
        ctrl_dt = ctrls.view(torch.float64).view(K, nb // 8)[:, 2]  # the `dt` field of each control block
        ctrl_list = [ctrls[k * nb : (k + 1) * nb] for k in range(K)]
        times = torch.cat([t_dev[:-1, None], t_dev[1:, None], table], dim=1).contiguous()  # per step: t0, t1, stage times
        row = torch.empty(times.shape[1], dtype=times.dtype, device=dev)
        y_cur, y_next = y0.clone(), torch.empty_like(y0)

        def body():
            self._step_body(row, ctrl_list, y_cur, y_next)

        def load(i):
            row.copy_(times[i])
            ctrl_dt.copy_(dt_table[i])

        def store(i, y_a):
            if sub.plain:
                out.narrow(-2, (i + 1) * L, L).copy_(y_cur)
            else:
                self._write_rows(out, L, sub.rows[i], y_a, y_cur)

        nfe0 = self.nfe
        load(0)
        if guard:  # "auto": a func that differentiates w.r.t. parameter leaves must never be captured (utils/graphed.py)
            from ..utils.graphed import _AutogradTargetProbe

            with _AutogradTargetProbe() as probe:
                body()
            if probe.hit is not None:
                raise RuntimeError("capture refused: func calls " + probe.hit)
        else:
            body()  # step 1, eagerly (warm-up of func and of the allocator)
        store(0, y0)
        per_step = self.nfe - nfe0
        from ..utils.graphed import CapturedGraph

        g = CapturedGraph()  # (replays of a graph that holds memset nodes are synchronised: see its docstring)
        with g.capture(capture_error_mode="thread_local"):
            body()
        g.finish()
        self.nfe = nfe0 + per_step  # recording executes nothing
        y_prev = None if sub.plain else torch.empty_like(y0)
        for i in range(1, n_steps):
            load(i)
            if sub.needs_a(i):
                y_prev.copy_(y_cur)
            g.replay()
            store(i, y_prev)
            self.nfe += per_step
        return out

    # -- re-armable one-step solves: odeint_adjoint's backward over a fixed grid -----------------------------------------
    # The backward sweep of a fixed-grid solve is one STEP per output interval, each from a fresh solver: with the captured
    # dynamics that was 2 input copies + 1 clone around every evaluation.  Here ONE solver is kept for the sweep (and the next
    # backward pass): the state lives in a static buffer, the step's times and step sizes go up in one host-to-device copy, and
    # the whole step — func's framework ops, the combines, the hand-over — is one graph replay.  Same kernels, same operands as
    # the eager step: bit-identical.
    _IV_SLOTS = 8

    def intervals_supported(self):
        # Sub-stepping: an interval is several steps over a grid of its own — the per-interval solves serve it.  The re-armable solve
        # replays ONE step per interval, so it is off whenever step_size / grid_constructor is given, even where an interval's grid
        # happens to be its two end points (the grid is only known per interval; the gradients are the same either way).
        return bool(self.graphable and not self._step_end_hook and self.interp != "cubic" and self.y0.is_cuda and self.y0.dim() >= 2
                    and self.pipeline in ("auto", "sync", "graph") and not self._substep)

    def _iv_host_rows(self, t_host):
        """(times row in the time dtype: t0, t1, the step's time values; the dt of every combine of the step, fp64) for one step."""
        row = np.concatenate([t_host, self._time_table(t_host)[0]])
        return row, np.asarray([v[0] for v in self._record_combine_dts(t_host[1:] - t_host[:-1])], dtype=np.float64)

    def intervals_prepare(self, t_span, t_dtype, capture=True):
        """Static buffers for one-step solves, one eager step over ``t_span`` (two host times) from the constructor's ``y0`` as
        warm-up, and — ``capture`` — the step's graph.  Main thread, outside autograd nodes (utils/graphed.py)."""
        from ..utils.graphed import CapturedGraph

        dev = self.y0.device
        self.backend.require_device(self.y0)
        y0 = as_operand(self.y0.detach())
        self._iv_tt = tt = np_dtype(t_dtype)
        row, dtrow = self._iv_host_rows(np.asarray([t_span[0], t_span[1]], dtype=tt))
        K, nb, item = len(dtrow), C.sizeof(_hip.XdeCtrl), np.dtype(tt).itemsize
        # one static device block: K control blocks (the combines read their `dt` field), then the step's times; its pinned mirror
        size = K * nb + len(row) * 8
        # (the host never waits for a step here, so the mirror is a ring: a slot is rewritten only after the copy that read it ran)
        self._iv_pinned = torch.zeros(self._IV_SLOTS, size, dtype=torch.uint8).pin_memory()
        self._iv_events = [None] * self._IV_SLOTS
        self._iv_slot = 0
        self._iv_block = torch.zeros(size, dtype=torch.uint8, device=dev)
        self._iv_ctrl_list = [self._iv_block[k * nb : (k + 1) * nb] for k in range(K)]
        self._iv_row = self._iv_block[K * nb : K * nb + len(row) * item].view(t_dtype)
        host = self._iv_pinned.numpy()
        self._iv_host_dt = [h[: K * nb].view(np.float64).reshape(K, nb // 8)[:, 2] for h in host]  # (the `dt` field of each control block)
        self._iv_host_row = [h[K * nb : K * nb + len(row) * item].view(tt) for h in host]
        self._iv_y = (y0.clone(), torch.empty_like(y0))
        self._iv_graph = None
        with torch.no_grad(), torch.autograd.set_multithreading_enabled(False):
            nfe0 = self.nfe
            self.interval_solve(t_span)  # eager: func's lazy initialisations, the allocator's blocks
            self._iv_per_step = self.nfe - nfe0
            if capture:
                torch.cuda.synchronize(dev)
                g = CapturedGraph()
                with g.capture(capture_error_mode="thread_local"):
                    self._step_body(self._iv_row, self._iv_ctrl_list, *self._iv_y)
                g.finish()
                self._iv_graph = g
            self.nfe = nfe0
        return self

    @property
    def interval_state(self):
        """The static state buffer a one-step solve starts from and leaves its result in."""
        return self._iv_y[0]

    def interval_solve(self, t_span):
        """One step from ``t_span[0]`` to ``t_span[1]`` (host times) on ``interval_state``, in place; returns it."""
        row, dtrow = self._iv_host_rows(np.asarray([t_span[0], t_span[1]], dtype=self._iv_tt))
        i = self._iv_slot
        self._iv_slot = (i + 1) % self._IV_SLOTS
        if self._iv_events[i] is not None:
            self._iv_events[i].synchronize()
        self._iv_host_row[i][:] = row
        self._iv_host_dt[i][:] = dtrow
        self._iv_block.copy_(self._iv_pinned[i], non_blocking=True)
        if self._iv_events[i] is None:
            self._iv_events[i] = torch.cuda.Event()
        self._iv_events[i].record()
        with torch.no_grad():
            if self._iv_graph is not None:
                self._iv_graph.replay()
                self.nfe += self._iv_per_step
            else:
                self._step_body(self._iv_row, self._iv_ctrl_list, *self._iv_y)
        return self._iv_y[0]

    # -- base_fixed_solver.py:146-164 (classical RK4; unused by the reference's RK4 class) ------------
    def rk4_step_func(self, t0, t1, y0, f0=None):
        dt = self._host_dt(t0, t1)
        half_dt = dt * 0.5
        t0h = self._t0_host if self._t0_host is not None else type(dt)(t0.item())
        dtt, hdt, t_half = self._tdev(dt, t0), self._tdev(half_dt, t0), self._tdev(t0h + half_dt, t0)
        k1 = f0
        if k1 is None:
            k1 = self._f(t0, dtt, y0)
        k2 = self._f(t_half, hdt, self._combine(y0, [k1], [1.0], _hip.COMBINE_FUSE, half_dt))
        k3 = self._f(t_half, hdt, self._combine(y0, [k2], [1.0], _hip.COMBINE_FUSE, half_dt))
        k4 = self._f(t1, hdt, self._combine(y0, [k3], [1.0], _hip.COMBINE_FUSE, dt))
        return self._combine(y0, [k1, k2, k3, k4], [1.0, 2.0, 2.0, 1.0], _hip.COMBINE_WFUSE, dt, scale=_one_sixth,
                             out=self._y1_out)

    # -- base_fixed_solver.py:166-197 ---------------------------------------------------------------
    def rk4_alt_step_func(self, t0, t1, y0, f0=None):
        """The reference's "3/8-rule" variant as written: stage-3 input is ``k1 - k2/3``."""
        dt = self._host_dt(t0, t1)
        dtt, d13, t_one_third, t_two_thirds = self._times(t0, dt)
        k1 = f0
        if k1 is None:
            k1 = self._f(t0, dtt, y0)
        k2 = self._f(t_one_third, d13, self._combine(y0, [k1], [1.0], _hip.COMBINE_FUSE, dt * _one_third))
        k3 = self._f(t_two_thirds, d13, self._combine(y0, [k1, k2], [1.0, -_one_third], _hip.COMBINE_FUSE, dt))
        if self._presum_ok(y0, [k1, k2, k3]):
            # the launch that forms k4's input holds k1..k3 anyway: it also emits `fuse(k1) + 3 fuse(k2) + 3 fuse(k3)` (left to right), and
            # the final launch reads y0, that partial sum and k4 — 18 N -> 17 N elements per step, same association, same bits
            y4, part = self._combine(y0, [k1, k2, k3], [1.0, -1.0, 1.0], _hip.COMBINE_FUSE, dt, emit=[1.0, 3.0, 3.0])
            k4 = self._f(t1, t_one_third, y4)
            if self._rec is not None or not (torch.is_grad_enabled() and k4.requires_grad):
                return self._combine_pre(y0, part, [k4], [1.0], dt, 0.125, out=self._y1_out)
        else:
            k4 = self._f(t1, t_one_third, self._combine(y0, [k1, k2, k3], [1.0, -1.0, 1.0], _hip.COMBINE_FUSE, dt))
        return self._combine(y0, [k1, k2, k3, k4], [1.0, 3.0, 3.0, 1.0], _hip.COMBINE_WFUSE, dt, scale=0.125,
                             out=self._y1_out)
