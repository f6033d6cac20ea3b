"""``sdeint_adjoint`` — the gradient of ``sdeint(..., solver=ReversibleHeun)`` in memory that does not grow with the number of steps.

The reference's ``sdeint_adjoint`` (paddlexde/functional/sdeint_adjoint.py) is a copy of ``odeint_adjoint`` that calls ``sdeint`` with
arguments it does not take, so it never ran; its signature is kept.  Here the forward is the reversible Heun walk under ``no_grad``,
keeping the solution, the carried ``yh`` at the last grid point, the host grid with its row plan, and the seed.  The backward walks the
grid in reverse: each step's state is recomputed from the one after it by the scheme's own two formulas at direction -1
(xde_sde_rheun_predict / xde_sde_rheun_correct), the Brownian increment regenerated in the kernel from ``(seed, k)``, and the
cotangents ``(a_y, a_yh, a_f, a_g)`` are taken one step back by xde_sde_rheun_adjoint_stage, one vjp of ``(drift, diffusion)`` at
``yh`` and xde_sde_rheun_adjoint_step (include/xde_hip_sde.h spells the formulas out).  The result is the exact gradient of the
discretisation — what back-propagating through ``sdeint(..., solver=ReversibleHeun)`` gives, up to rounding — with one drift and one
diffusion evaluation per backward step and every buffer reused in place.

Any other solver is refused: Euler, Milstein and SRK steps cannot be recomputed backwards.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _hip
from ..solver._common import as_operand
from ..solver.base_fixed_solver import sde_step_scalars
from ..solver.fixed_solver.rheun import ReversibleHeun
from ..utils.ode_utils import _rms_norm
from ..xde.base_sde import BaseSDE, check_noise_type

_MESSAGE = (
    "sdeint_adjoint is not implemented (the stochastic adjoint needs a Brownian path that can be queried backwards in time); "
    "differentiate through sdeint(..., solver=Euler) or sdeint(..., solver=Milstein) or SRK instead or use solver=ReversibleHeun"
)


def _solve(drift, diffusion, y0, t, rtol, atol, options):
    """The forward of ``sdeint(..., solver=ReversibleHeun)`` and what the sweep needs of it."""
    options = dict(options)
    seed = options.pop("seed", None)
    options.pop("noise_type", None)  # ("diagonal": sdeint_adjoint has refused any other value)
    xde = BaseSDE(f=drift, g=diffusion, y0=y0, t_span=t, seed=seed)
    solver = ReversibleHeun(xde=xde, y0=xde.y0, rtol=rtol, atol=atol, **options)
    grid, grid_dev, plan, pred_len = solver._plan(t)
    solution = solver._walk(grid, grid_dev, plan, pred_len)
    yh_end = solver._carry[0] if len(grid) > 1 else None
    solver._carry = None
    return xde, solution, yh_end, grid, grid_dev, plan


class _SdeintAdjointFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, drift, diffusion, t, rtol, atol, options, n_params, y0, *params):
        with torch.no_grad():
            xde, solution, yh_end, grid, grid_dev, plan = _solve(drift, diffusion, y0.detach(), t, rtol, atol, options)
        ctx.xde, ctx.grid, ctx.grid_dev, ctx.plan = xde, grid, grid_dev, plan
        ctx.params = params
        ctx.shape = tuple(y0.shape)
        ctx.save_for_backward(solution, *([yh_end] if yh_end is not None else []))
        return solution

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        solution, *rest = ctx.saved_tensors
        grad_y0, grad_params, _ = _sweep(ctx.xde, ctx.params, solution, rest[0] if rest else None, ctx.grid, ctx.grid_dev, ctx.plan,
                                         grad_out, ctx.shape)
        return (None,) * 7 + (grad_y0 if ctx.needs_input_grad[7] else None,) + tuple(grad_params)


def _row(x, j, L, shape):
    """Output row j of a ``[..., T*L, D]`` tensor as a contiguous state."""
    return x.narrow(-2, j * L, L).reshape(shape)


def _sweep(xde, params, solution, yh_end, grid, grid_dev, plan, grad_out, shape):
    """The backward sweep over ``grid``; returns ``(grad_y0, grad_params, y0 as reconstructed)``."""
    backend = _hip.get_backend()
    seed = xde.seed
    L = shape[-2]
    n_steps = len(grid) - 1
    params = tuple(params)
    wanted = [i for i, p in enumerate(params) if p.requires_grad]
    acc = [None] * len(params)
    a_y = as_operand(_row(grad_out, 0, L, shape)).clone()  # (row 0 is a copy of y0; the rest of a one-point grid's rows too)
    if n_steps == 0:
        for j in range(1, grad_out.shape[-2] // L):
            a_y.add_(_row(grad_out, j, L, shape))
        return a_y, acc, _row(solution, 0, L, shape)
    a_0 = a_y
    a_y = torch.zeros_like(a_0)

    def evaluate(k, yh):
        """(yh with grad, fh, gh) at grid point k: the reconstruction's operands and the graph of the next vjp."""
        with torch.enable_grad():
            yh = yh.detach().requires_grad_(True)
            t = grid_dev[k : k + 1]
            return yh, as_operand(xde.call_func(t, yh), like=yh), as_operand(xde.diffusion(t, yh), like=yh)

    def vjp(yh, f, g, bf, bg):
        """The cotangent of yh; the parameters' accumulate in ``acc``."""
        outs = [x for x in (f, g) if x.requires_grad]
        cots = [b for x, b in ((f, bf), (g, bg)) if x.requires_grad]
        if not outs:
            return torch.zeros_like(bf)
        got = torch.autograd.grad(outs, (yh,) + tuple(params[i] for i in wanted), cots, allow_unused=True)
        for i, gp in zip(wanted, got[1:]):
            if gp is not None:
                acc[i] = gp.clone() if acc[i] is None else acc[i].add_(gp)
        return as_operand(got[0]) if got[0] is not None else torch.zeros_like(bf)

    def inject(k, end):
        """The cotangents of step k's output rows that belong to the state at its end (1) or start (0), added to a_y."""
        rows = plan.rows[k]
        if plan.plain:
            if end:
                for j, _, _ in rows:
                    a_y.add_(_row(grad_out, j, L, shape))
            return
        w5 = []
        for _, kind, w in rows:
            wb = 1.0 if kind == _hip.XDE_ROW_COPY_B else (0.0 if kind == _hip.XDE_ROW_COPY_A else float(w[0]))
            w5.append((1.0 - wb, wb, 0.0, 0.0, 0.0))
        if not any(x[end] != 0.0 for x in w5):
            return
        g_rows = torch.stack([_row(grad_out, j, L, shape) for j, _, _ in rows])
        outs = [None] * 5
        outs[end] = a_y
        backend.dense_cotangent(outs, g_rows, w5, acc_mask=1 << end)

    y = as_operand(_row(solution, grad_out.shape[-2] // L - 1, L, shape)).clone()  # (the last row is the state at the last grid point)
    yh_bufs = [yh_end.clone(), torch.empty_like(yh_end)]
    yh, f, g = evaluate(n_steps, yh_bufs[0])
    a_yh = a_f = a_g = None
    for k in range(n_steps - 1, -1, -1):
        dt, s = sde_step_scalars(grid[k + 1] - grid[k], y.dtype)
        inject(k, 1)
        bf, bg = (torch.empty_like(y), torch.empty_like(y)) if a_f is None else (a_f, a_g)
        backend._sde_rheun_adjoint_stage(bf, bg, a_f, a_g, a_y, dt, s, seed, k)
        v = vjp(yh, f, g, bf, bg)
        a_f, a_g = bf, bg  # (consumed by the vjp: the step's outputs go there)
        ayh0 = a_yh if a_yh is not None else torch.empty_like(y)
        backend._sde_rheun_adjoint_step(a_y, ayh0, a_f, a_g, a_y, a_yh, v, dt, s, seed, k)
        a_yh = ayh0
        del v
        # the state one grid point back: the forward step's two formulas at direction -1
        f1, g1 = f.detach(), g.detach()
        yh0 = yh_bufs[(n_steps - k) % 2]
        backend._sde_rheun_predict(yh0, y, yh.detach(), f1, g1, dt, s, -1, seed, k)
        yh, f, g = evaluate(k, yh0)
        backend._sde_rheun_correct(y, y, f1, f.detach(), g1, g.detach(), dt, s, -1, seed, k)
        inject(k, 0)
    grad_y0 = a_y.add_(a_yh).add_(vjp(yh, f, g, a_f, a_g)).add_(a_0)
    return grad_y0, acc, y


def sdeint_adjoint(
    drift: callable,
    diffusion: callable,
    y0,
    t,
    *,
    rtol=1e-7,
    atol=1e-9,
    solver=None,
    options={"norm": _rms_norm},
    event_fn=None,
    adjoint_rtol=None,
    adjoint_atol=None,
    adjoint_solver=None,
    adjoint_options=None,
    adjoint_params=None,
):
    """``sdeint(drift, diffusion, y0, t, solver=ReversibleHeun)`` whose backward recomputes the path instead of keeping it: the same
    solution, the same gradients up to rounding, live memory independent of the number of grid steps.  The equation is read in the
    STRATONOVICH sense (ReversibleHeun), with diagonal noise.  ``options`` are ``sdeint``'s (``seed``, ``step_size`` /
    ``grid_constructor`` with ``interp="linear"``); without a seed one is drawn from torch's default CPU generator and kept for the
    backward.  ``adjoint_params``: the tensors besides ``y0`` that get a gradient — by default the parameters of ``drift`` and
    ``diffusion``, which then must be ``nn.Module``s.  The backward is once-differentiable; there is no gradient with respect to ``t``.
    The sweep is the scheme's own, so ``adjoint_solver``, ``adjoint_rtol``, ``adjoint_atol``, ``adjoint_options`` and ``event_fn`` must
    be None."""
    for key in ("logqp", "prior_drift"):
        if key in dict(options):
            raise NotImplementedError("sdeint_adjoint does not take options[{!r}]: the KL term of a latent SDE is accumulated by "
                                      "sdeint(..., solver=Euler) or solver=Milstein, which keep the steps' operands for the "
                                      "backward".format(key))
    noise_type = check_noise_type(dict(options).get("noise_type", "diagonal"))
    if noise_type != "diagonal":
        raise NotImplementedError("sdeint_adjoint does not take options['noise_type'] = {!r}: the reversible Heun kernels and their "
                                  "cotangent sweep are diagonal (general noise for them is a follow-up); sdeint(..., solver=Euler) "
                                  "steps general and scalar noise and keeps the steps' operands for the backward".format(noise_type))
    if solver is not ReversibleHeun:
        raise NotImplementedError(_MESSAGE)
    for name, value in (("adjoint_solver", adjoint_solver), ("adjoint_rtol", adjoint_rtol), ("adjoint_atol", adjoint_atol),
                        ("adjoint_options", adjoint_options), ("event_fn", event_fn)):
        if value is not None:
            raise NotImplementedError("sdeint_adjoint: {} must be None — the backward sweep is the reversible Heun scheme's own, on the "
                                      "forward's grid".format(name))
    if isinstance(y0, (tuple, list)):
        raise NotImplementedError("sdeint_adjoint takes a tensor y0, not a tuple: stack the members into one state tensor")
    if adjoint_params is None:
        if not (isinstance(drift, torch.nn.Module) and isinstance(diffusion, torch.nn.Module)):
            raise ValueError(
                "func must be an instance of nn.Module to specify the adjoint parameters; alternatively they "
                "can be specified explicitly via the `adjoint_params` argument. If there are no parameters "
                "then it is allowable to set `adjoint_params=()`."
            )
        adjoint_params = tuple(drift.parameters()) + tuple(p for p in diffusion.parameters())
    seen, params = set(), []
    for p in adjoint_params:  # (in case adjoint_params is a generator; every tensor once; only those that take a gradient)
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            params.append(p)
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError("sdeint_adjoint gives no gradient with respect to t; detach t (gradients reach y0 and the "
                                  "adjoint_params)")
    return _SdeintAdjointFn.apply(drift, diffusion, t, rtol, atol, options, len(params), y0, *params)
