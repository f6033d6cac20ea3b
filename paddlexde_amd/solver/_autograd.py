"""Autograd nodes around the step kernels (xde_stage_combine, xde_interp_rows, xde_sde_em_step, xde_sde_milstein_step, xde_sde_srk_*, xde_sde_rheun_*, xde_sde_kl_*, xde_sde_gn_*, xde_dde_tape_gather) for discretise-then-optimise training.

The reference trains by back-propagating through its eager solver ops (example/ode_demo.py:51-53:
``pred_y = odeint(func, batch_y0, t_span, solver=RK4); loss.backward()``).  Here the forward is one combine launch
and the backward one fan-out launch (every input gradient is a scalar multiple of the output gradient);
``func`` itself is differentiated by the framework as usual.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _hip


def _cotangent(g):
    """The incoming cotangent as a launch operand: contiguous and 16-byte aligned."""
    g = g.contiguous()
    return g.clone() if g.data_ptr() % 16 else g


def _sde_backward(launch, g, needs, meta):
    """The backward of an SDE step node: ``needs`` = (y0, then the operands of ``launch``'s outputs).  The cotangent of y0 is ``g``
    itself; the wanted others are allocated and written by one ``launch(*outs, g, *meta)`` (None: skipped), if any is wanted."""
    g = _cotangent(g)
    outs = [torch.empty_like(g) if need else None for need in needs[1:]]
    if any(o is not None for o in outs):
        launch(*outs, g, *meta)
    return (g if needs[0] else None, *outs)


class CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, backend, coef, mode, scale, dt, damp, y0, *ks):
        out = torch.empty_like(y0)
        backend.stage_combine(out, y0.detach(), [k.detach() for k in ks], coef, mode, scale=scale, dt_host=float(dt),
                              damping=float(damp))
        ctx.backend = backend
        ctx.meta = (tuple(float(c) for c in coef), mode, float(scale), float(dt), float(damp))
        ctx.needs = (y0.requires_grad,) + tuple(k.requires_grad for k in ks)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        coef, mode, scale, dt, damp = ctx.meta
        # damped fuse: (dy - damp*(dy*dt + y0))*dt + y0 = dy*dt*(1 - damp*dt) + y0*(1 - damp*dt)
        g_damp = 1.0 - damp * dt
        if mode == _hip.COMBINE_RK or mode == _hip.COMBINE_FUSE:
            # out = y0 + sum_j k_j (c_j dt)   |   out = fuse(sum_j c_j k_j, dt, y0)
            fy0 = g_damp
            fk = [c * dt * g_damp for c in coef]
        else:
            # out = scale * sum_j w_j fuse(k_j, dt, y0)
            fy0 = scale * sum(coef) * g_damp
            fk = [scale * w * dt * g_damp for w in coef]
        g = _cotangent(g)
        factors = [fy0] + fk
        outs, todo_o, todo_f = [], [], []
        for need, f in zip(ctx.needs, factors):
            if not need:
                outs.append(None)
            elif f == 1.0:
                outs.append(g)
            else:
                o = torch.empty_like(g)
                outs.append(o)
                todo_o.append(o)
                todo_f.append(f)
        if todo_o:
            ctx.backend.scale_fanout(todo_o, g, todo_f)
        return (None, None, None, None, None, None) + tuple(outs)


class InterpRowsFn(torch.autograd.Function):
    """The output rows of one grid step of a sub-stepped fixed-grid solve (``HipBackend._interp_rows``) as ONE autograd node: forward
    writes the G rows into a fresh ``[G, *y_a.shape]`` tensor; backward turns the G row cotangents into the cotangents of
    ``(y_a, y_b, f_a, f_b)`` with xde_dense_cotangent (every row is linear in them; an exact-copy row has weight 1)."""

    @staticmethod
    def forward(ctx, backend, kinds, weights, y_a, y_b, f_a, f_b):
        cubic = f_a is not None
        ops = [y_a.detach(), y_b.detach()] + ([f_a.detach(), f_b.detach()] if cubic else [])
        rows = torch.empty((len(kinds),) + tuple(y_a.shape), dtype=y_a.dtype, device=y_a.device)
        backend._interp_rows([rows[g] for g in range(len(kinds))], kinds, weights, *ops)
        # d row / d (y_a, y_b, y_mid, f_a, f_b): the five outputs of xde_dense_cotangent (no y_mid here)
        w5 = []
        for k, w in zip(kinds, weights):
            if k == _hip.XDE_ROW_COPY_A:
                w5.append((1.0, 0.0, 0.0, 0.0, 0.0))
            elif k == _hip.XDE_ROW_COPY_B:
                w5.append((0.0, 1.0, 0.0, 0.0, 0.0))
            elif cubic:
                w5.append((float(w[0]), float(w[2]), 0.0, float(w[1]), float(w[3])))
            else:
                w5.append((1.0 - float(w[0]), float(w[0]), 0.0, 0.0, 0.0))
        ctx.backend, ctx.w5 = backend, w5
        return rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        need = ctx.needs_input_grad[3:7]
        g = _cotangent(g)
        like = g[0]
        outs = [torch.empty_like(like) if need[0] else None, torch.empty_like(like) if need[1] else None, None,
                torch.empty_like(like) if need[2] else None, torch.empty_like(like) if need[3] else None]
        if any(o is not None for o in outs):
            ctx.backend.dense_cotangent(outs, g, ctx.w5)
        return (None, None, None, outs[0], outs[1], outs[3], outs[4])


class SdeEulerFn(torch.autograd.Function):
    """One Euler-Maruyama step ``y1 = (y0 + f*dt) + g*(s*Z)`` (``HipBackend._sde_em_step``) as an autograd node.  The node keeps
    only ``(dt, s, seed, k)``: backward regenerates Z from the same counter in the launch that writes ``gf = gy1*dt`` and
    ``gg = gy1*(s*Z)`` (xde_sde_em_backward); ``gy0 = gy1`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, f, g):
        out = torch.empty_like(y0)
        backend._sde_em_step(out, y0.detach(), f.detach(), g.detach(), dt, s, seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), int(seed), int(k))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (None,) * 5 + _sde_backward(ctx.backend._sde_em_backward, g, ctx.needs_input_grad[5:8], ctx.meta)


class SdeGnEulerFn(torch.autograd.Function):
    """One Euler-Maruyama step with general or scalar noise, ``y1[.., d] = (y0 + f*dt)[.., d] + sum_m g[.., d, m]*(s*Z[.., m])``
    (``HipBackend._sde_gn_step``), as an autograd node.  The node keeps only ``(dt, s, seed, k)`` and M: backward is one
    xde_sde_gn_backward launch that regenerates Z and writes ``gf = gy1*dt`` and ``gg[.., d, m] = gy1[.., d]*(s*Z[.., m])``, each only
    if wanted (an unwanted cotangent stays None); ``gy0 = gy1`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, f, g):
        out = torch.empty_like(y0)
        backend._sde_gn_step(out, y0.detach(), f.detach(), g.detach(), dt, s, seed, k)
        ctx.backend, ctx.meta, ctx.M = backend, (float(dt), float(s), int(seed), int(k)), int(g.shape[-1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        need_y, need_f, need_g = ctx.needs_input_grad[5:8]
        gy = _cotangent(gy)
        gf = torch.empty_like(gy) if need_f else None
        gg = torch.empty(tuple(gy.shape) + (ctx.M,), dtype=gy.dtype, device=gy.device) if need_g else None
        if gf is not None or gg is not None:
            ctx.backend._sde_gn_backward(gf, gg, gy, ctx.M, *ctx.meta)
        return (None,) * 5 + (gy if need_y else None, gf, gg)


class SdeSupportFn(torch.autograd.Function):
    """Milstein's support point ``yb = (y0 + f*dt) + g*s`` (``HipBackend._sde_milstein_support``) as an autograd node: backward is one
    launch writing ``gf = gyb*dt`` and ``gg = gyb*s`` (xde_sde_milstein_support_backward); ``gy0 = gyb`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, y0, f, g):
        out = torch.empty_like(y0)
        backend._sde_milstein_support(out, y0.detach(), f.detach(), g.detach(), dt, s)
        ctx.backend, ctx.meta = backend, (float(dt), float(s))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (None,) * 3 + _sde_backward(ctx.backend._sde_milstein_support_backward, g, ctx.needs_input_grad[3:6], ctx.meta)


class SdeMilsteinFn(torch.autograd.Function):
    """One Milstein step ``y1 = ((y0 + f*dt) + g*w) + (gb - g)*q``, ``w = s*Z``, ``q = c*(w*w - |dt|)``
    (``HipBackend._sde_milstein_step``) as an autograd node.  The node keeps only ``(dt, s, c, seed, k)``: backward regenerates Z from
    the same counter in the launch that writes ``gf = gy1*dt``, ``gg = gy1*(w - q)`` and ``ggb = gy1*q`` (xde_sde_milstein_backward);
    ``gy0 = gy1`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, c, seed, k, y0, f, g, gb):
        out = torch.empty_like(y0)
        backend._sde_milstein_step(out, y0.detach(), f.detach(), g.detach(), gb.detach(), dt, s, c, seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), float(c), int(seed), int(k))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (None,) * 6 + _sde_backward(ctx.backend._sde_milstein_backward, g, ctx.needs_input_grad[6:10], ctx.meta)


def _sde_group_backward(launch, gs, needs, groups, meta):
    """The backward of an SRK node: ``needs`` = the operands of ``launch``'s outputs, ``groups`` the runs of them that the launch
    writes or skips together.  The outputs of every group with a wanted member are allocated and written by one
    ``launch(*outs, *gs, *meta)`` (None: skipped), if any is wanted; only the wanted ones are handed on."""
    outs = []
    for lo, hi in groups:
        want = any(needs[lo:hi])
        outs += [torch.empty_like(gs[0]) if want else None for _ in range(lo, hi)]
    if any(o is not None for o in outs):
        launch(*outs, *gs, *meta)
    return tuple(o if need else None for o, need in zip(outs, needs))


class SdeSrkStage1Fn(torch.autograd.Function):
    """SRK's stage inputs ``Y2, G2, G3`` (``HipBackend._sde_srk_stage1``) as one autograd node with three outputs.  The node keeps only
    ``(dt, s, seed, k)``: backward regenerates Z and V from the same counters in the launch that turns the three cotangents into
    those of ``y0``, ``a1`` and ``b1`` (xde_sde_srk_stage1_backward)."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, a1, b1):
        outs = tuple(torch.empty_like(y0) for _ in range(3))
        backend._sde_srk_stage1(*outs, y0.detach(), a1.detach(), b1.detach(), dt, s, seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), int(seed), int(k))
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        gs = [_cotangent(g) for g in gs]
        return (None,) * 5 + _sde_group_backward(ctx.backend._sde_srk_stage1_backward, gs, ctx.needs_input_grad[5:8],
                                                 ((0, 1), (1, 2), (2, 3)), ctx.meta)


class SdeSrkStage2Fn(torch.autograd.Function):
    """SRK's last stage input ``G4`` (``HipBackend._sde_srk_stage2``) as an autograd node: backward is one launch writing the cotangents
    of ``a1`` and of ``b1, b2, b3`` (xde_sde_srk_stage2_backward); ``gy0 = gG4`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, y0, a1, b1, b2, b3):
        out = torch.empty_like(y0)
        backend._sde_srk_stage2(out, y0.detach(), a1.detach(), b1.detach(), b2.detach(), b3.detach(), dt, s)
        ctx.backend, ctx.meta = backend, (float(dt), float(s))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _cotangent(g)
        rest = _sde_group_backward(ctx.backend._sde_srk_stage2_backward, [g], ctx.needs_input_grad[4:8], ((0, 1), (1, 4)), ctx.meta)
        return (None,) * 3 + (g if ctx.needs_input_grad[3] else None,) + rest


class SdeSrkStepFn(torch.autograd.Function):
    """One SRK step (``HipBackend._sde_srk_step``) as an autograd node.  The node keeps only ``(dt, s, c, c3, seed, k)``: backward
    regenerates Z and V in the launch that writes the cotangents of ``a1, a2`` and of ``b1 .. b4`` (xde_sde_srk_step_backward);
    ``gy0 = gy1`` needs no launch."""

    @staticmethod
    def forward(ctx, backend, dt, s, c, c3, seed, k, y0, a1, a2, b1, b2, b3, b4):
        out = torch.empty_like(y0)
        backend._sde_srk_step(out, y0.detach(), a1.detach(), a2.detach(), b1.detach(), b2.detach(), b3.detach(), b4.detach(), dt, s, c,
                              c3, seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), float(c), float(c3), int(seed), int(k))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = _cotangent(g)
        rest = _sde_group_backward(ctx.backend._sde_srk_step_backward, [g], ctx.needs_input_grad[8:14], ((0, 2), (2, 6)), ctx.meta)
        return (None,) * 7 + (g if ctx.needs_input_grad[7] else None,) + rest


class SdeRheunPredictFn(torch.autograd.Function):
    """Reversible Heun's prediction ``yh1 = (((y0 + y0) - yh0) + f0*dt) + g0*w`` (``HipBackend._sde_rheun_predict``, direction +1) as an
    autograd node.  The node keeps only ``(dt, s, seed, k)``: backward is xde_sde_em_backward at ``(dt, s)``, which regenerates Z and
    writes ``gf0 = gyh1*dt`` and ``gg0 = gyh1*w``; ``gy0 = gyh1 + gyh1`` and ``gyh0 = -gyh1``."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, yh0, f0, g0):
        out = torch.empty_like(y0)
        backend._sde_rheun_predict(out, y0.detach(), yh0.detach(), f0.detach(), g0.detach(), dt, s, 1, seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), int(seed), int(k))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        needs = ctx.needs_input_grad[5:9]
        g, gf, gg = _sde_backward(ctx.backend._sde_em_backward, g, (True,) + tuple(needs[2:]), ctx.meta)
        return (None,) * 5 + (g + g if needs[0] else None, -g if needs[1] else None, gf, gg)


class SdeRheunCorrectFn(torch.autograd.Function):
    """Reversible Heun's correction ``y1 = (y0 + (f0 + f1)*(0.5*dt)) + (g0 + g1)*(0.5*w)`` (``HipBackend._sde_rheun_correct``, direction
    +1) as an autograd node.  The node keeps only ``(dt, s, seed, k)``: backward is xde_sde_em_backward at ``(0.5*dt, 0.5*s)`` (halving
    is exact), whose ``gf`` is the cotangent of both ``f0`` and ``f1`` and whose ``gg`` that of both ``g0`` and ``g1``; ``gy0 = gy1``."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, f0, f1, g0, g1):
        out = torch.empty_like(y0)
        backend._sde_rheun_correct(out, y0.detach(), f0.detach(), f1.detach(), g0.detach(), g1.detach(), dt, s, 1, seed, k)
        ctx.backend, ctx.meta = backend, (0.5 * float(dt), 0.5 * float(s), int(seed), int(k))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        needs = ctx.needs_input_grad[5:10]
        g, gf, gg = _sde_backward(ctx.backend._sde_em_backward, g, (needs[0], needs[1] or needs[2], needs[3] or needs[4]), ctx.meta)
        return (None,) * 5 + (g, gf if needs[1] else None, gf if needs[2] else None, gg if needs[3] else None, gg if needs[4] else None)


class SdeKlEulerFn(torch.autograd.Function):
    """One Euler-Maruyama step fused with the KL accumulation of a latent SDE (``HipBackend._sde_kl_step``) as an autograd node with two
    outputs: ``y1 = (y0 + f*dt) + g*(s*Z)`` and ``acc1 = acc0 + sum(((f - h)/g)**2, -1) * (0.5*dt)`` (float64 per row; ``acc0`` None:
    zero).  The node saves ``f, g, h`` and ``(dt, s, seed, k)``; backward is one xde_sde_kl_backward launch that regenerates Z
    (``gy0 = gy1`` and ``gacc0 = gacc1`` need none).  A cotangent that is absent stays absent: without ``gacc1`` the backward is
    xde_sde_em_backward, without ``gy1`` the accumulate-only mode's."""

    @staticmethod
    def forward(ctx, backend, dt, s, seed, k, y0, f, g, h, acc0):
        y1 = torch.empty_like(y0)
        acc1 = torch.empty(y0.shape[:-1], dtype=torch.float64, device=y0.device)
        backend._sde_kl_step(y1, acc1, y0.detach(), f.detach(), g.detach(), h.detach(), None if acc0 is None else acc0.detach(), dt, s,
                             seed, k)
        ctx.backend, ctx.meta = backend, (float(dt), float(s), int(seed), int(k))
        ctx.save_for_backward(f, g, h)
        ctx.set_materialize_grads(False)
        return y1, acc1

    @staticmethod
    @once_differentiable
    def backward(ctx, gy1, gacc):
        needs = ctx.needs_input_grad[5:10]
        if gy1 is not None:
            gy1 = _cotangent(gy1)
        gf = gg = gh = None
        if gacc is None:
            if gy1 is not None:
                _, gf, gg = _sde_backward(ctx.backend._sde_em_backward, gy1, (False,) + tuple(needs[1:3]), ctx.meta)
        else:
            gacc = gacc.contiguous()
            f, g, h = ctx.saved_tensors
            gf, gg, gh = (torch.empty_like(f) if need else None for need in needs[1:4])
            if any(o is not None for o in (gf, gg, gh)):
                ctx.backend._sde_kl_backward(gf, gg, gh, gy1, gacc, f, g, h, *ctx.meta)
        return (None,) * 5 + (gy1 if needs[0] else None, gf, gg, gh, gacc if needs[4] else None)


class SdeKlAccFn(torch.autograd.Function):
    """The KL accumulation alone (``HipBackend._sde_kl_step`` in its accumulate-only mode: Milstein's step keeps its own launches) as an
    autograd node: ``acc1 = acc0 + sum(((f - h)/g)**2, -1) * (0.5*dt)``.  The node saves ``f, g, h`` and ``dt``; backward is one
    xde_sde_kl_backward launch without ``gy1`` (no generator); ``gacc0 = gacc1``."""

    @staticmethod
    def forward(ctx, backend, dt, f, g, h, acc0):
        acc1 = torch.empty(f.shape[:-1], dtype=torch.float64, device=f.device)
        backend._sde_kl_step(None, acc1, None, f.detach(), g.detach(), h.detach(), None if acc0 is None else acc0.detach(), dt, 0.0, 0, 0)
        ctx.backend, ctx.dt = backend, float(dt)
        ctx.save_for_backward(f, g, h)
        ctx.set_materialize_grads(False)
        return acc1

    @staticmethod
    @once_differentiable
    def backward(ctx, gacc):
        if gacc is None:
            return (None,) * 6
        needs = ctx.needs_input_grad[2:6]
        gacc = gacc.contiguous()
        f, g, h = ctx.saved_tensors
        gf, gg, gh = (torch.empty_like(f) if need else None for need in needs[:3])
        if any(o is not None for o in (gf, gg, gh)):
            ctx.backend._sde_kl_backward(gf, gg, gh, None, gacc, f, g, h, ctx.dt, 0.0, 0, 0)
        return (None, None, gf, gg, gh, gacc if needs[3] else None)


class DdeTapeGatherFn(torch.autograd.Function):
    """The delayed states of ONE stage of ddeint_steps, ``y_lags[.., j, :] = H(s - lags[j])`` with H the cubic Hermite interpolant of
    the tape (``HipBackend._dde_tape_gather``: one launch per ``XDE_DDE_MAX_LAGS`` delays), as an autograd node.  ``plan`` is the
    stage's host plan (xde/steps_dde.py: ``StagePlan``): per delay the four operands of its interval — a history row (a plain tensor,
    no gradient, unless ``plan.dep`` says that the row is itself a function of one of ``nodes``: the forward-difference derivative of the
    history's last two samples moves with tape node 0's state, scaled by ``1 / dt``) or the index of one of ``nodes``, the distinct tape
    tensors the stage reads — and the float64 weights.  The node saves
    the plan, and ``dtau`` (the derivative of every value with respect to its delay) only when ``lags`` requires grad.  Backward: one
    ``_dde_tape_gather_backward`` launch per tile of delays writes the cotangents of the wanted nodes (a node hit by two tiles is
    summed in tile order), and ``grad_lags = lag_grad(g, dtau)``; an unwanted cotangent stays None."""

    @staticmethod
    def forward(ctx, backend, plan, lags, *nodes):
        rows, L, D = plan.rows, plan.L, plan.D
        flat = [x.detach().view(rows, D) for x in nodes]
        srcs = [flat[s] if isinstance(s, int) else s for s in plan.src]
        like = nodes[0] if nodes else plan.like
        out = torch.empty(rows, L, D, dtype=like.dtype, device=like.device)
        want_tau = lags is not None and lags.requires_grad
        dtau = torch.empty_like(out) if want_tau else None
        backend._dde_tape_gather(out, dtau, srcs, plan.w, plan.wd if want_tau else None)
        ctx.backend, ctx.plan = backend, plan
        ctx.shapes = [tuple(x.shape) for x in nodes]
        if want_tau:
            ctx.save_for_backward(dtau)
        return out.view(plan.lead + (L, D))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        plan, be = ctx.plan, ctx.backend
        rows, L, D = plan.rows, plan.L, plan.D
        g = _cotangent(g).view(rows, L, D)
        needs = ctx.needs_input_grad[3:]
        grads = [None] * len(needs)
        for j0 in range(0, L, _hip.XDE_DDE_MAX_LAGS):
            terms = {}  # node -> its (lag within the tile, weight) terms, in delay and operand order
            for j in range(j0, min(j0 + _hip.XDE_DDE_MAX_LAGS, L)):
                for s in range(4):
                    n, scale = plan.src[4 * j + s], 1.0
                    if not isinstance(n, int):  # a history operand: no gradient, unless it is itself a function of a tape tensor
                        if plan.dep[4 * j + s] is None:
                            continue
                        n, scale = plan.dep[4 * j + s]
                    if needs[n]:
                        terms.setdefault(n, []).append((j - j0, plan.w[4 * j + s] * scale))
            if not terms:
                continue
            order = sorted(terms)
            outs = [torch.empty(rows, D, dtype=g.dtype, device=g.device) for _ in order]
            be._dde_tape_gather_backward(outs, [terms[n] for n in order], g, j0)
            for n, o in zip(order, outs):
                grads[n] = o if grads[n] is None else grads[n] + o
        g_lags = None
        if ctx.needs_input_grad[2]:
            (dtau,) = ctx.saved_tensors
            g_lags = be.lag_grad(g, dtau).reshape(plan.lags_shape).to(device=plan.lags_device, dtype=plan.lags_dtype)
        return (None, None, g_lags) + tuple(None if o is None else o.view(shape) for o, shape in zip(grads, ctx.shapes))
