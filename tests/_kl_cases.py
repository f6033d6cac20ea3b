"""End-to-end cases of ``sdeint(..., options={"logqp": True, "prior_drift": h})``, run on the numpy double (tests/test_kl_host.py) and
on the GPU (tests/test_gpu_kl.py) through the ``dev`` fixture of each module.  The references are tests/_kl_oracle.py fed the backend's
own normals (``_sde_noise``) and the drift, diffusion and prior the backend's device evaluated, the closed form of a constant
integrand, and the same walk written in framework ops."""
import numpy as np
import pytest
import torch

from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler, Milstein
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _kl_oracle as KL
from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from ._sde_cases import _NPT, _opts, _y0, backend_noise

EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}
MU, NU, CC = 0.5, 0.25, 0.75  # exactly representable: the same bits in numpy and in torch on either device
SOLVERS = {"euler": Euler, "milstein": Milstein}
# exactly representable times with exactly representable differences, also on the step_size = 2^-4 grid: dt is exact in both dtypes
T_EXACT = np.array([0.0, 0.125, 0.390625, 0.5, 0.5, 0.84375, 1.0])  # (0.390625: a quarter into its grid step, 0.84375: half way)
H_EXACT = 0.0625


def diffusion(t, y):
    return y * MU + NU


def drift_cg(t, y):
    return diffusion(t, y) * CC


def prior_zero(t, y):
    return torch.zeros_like(y)


def _walks(T):
    t_np = T_EXACT.astype(T)
    return {"plain": ({}, t_np), "step_size": ({"step_size": H_EXACT, "interp": "linear"}, step_size_grid(t_np, H_EXACT))}


class Triple:
    """A small nonlinear latent SDE on D = 5: posterior drift, prior drift and a shared diagonal diffusion bounded away from zero."""

    def __init__(self, dtype, dev, D=5):
        g = torch.Generator().manual_seed(11)
        mk = lambda *s: (0.5 * torch.randn(*s, generator=g, dtype=torch.float64)).to(dev, dtype).requires_grad_(True)  # noqa: E731
        self.p = {n: (mk(D, 8), mk(8), mk(8, D), mk(D)) for n in ("f", "g", "h")}

    def _net(self, n, y):
        w1, b1, w2, b2 = self.p[n]
        return torch.tanh(y @ w1 + b1) @ w2 + b2

    def drift(self, t, y):
        return self._net("f", y)

    def prior(self, t, y):
        return self._net("h", y) * 0.5

    def diffusion(self, t, y):
        return 0.25 + 0.5 * torch.sigmoid(self._net("g", y))

    def params(self):
        return [x for n in ("f", "g", "h") for x in self.p[n]]


def _on_device(fn, dtype, dev):
    """``fn(t, y)`` for the numpy oracle: evaluated by the backend's device on the same bits, so the operands are the launch's own."""
    def call(t, y):
        with torch.no_grad():
            return fn(None, torch.from_numpy(np.ascontiguousarray(y)).to(dev, dtype)).cpu().numpy()
    return call


# ----------------------------------------------------------------------------------------------
# shapes and paths
# ----------------------------------------------------------------------------------------------
def test_logqp_returns_the_path_and_one_value_per_row_and_interval(dev):
    y0 = _y0(torch.float32, dev, shape=(3, 2, 5))
    t = torch.linspace(0.0, 1.0, 7)
    out = sdeint(drift_cg, diffusion, y0, t, solver=Euler, options=_opts(seed=1, logqp=True, prior_drift=prior_zero))
    assert isinstance(out, tuple) and len(out) == 2
    ys, logqp = out
    assert ys.shape == (3, 7 * 2, 5) and logqp.shape == (3, 2, 6) and logqp.dtype == y0.dtype and logqp.device == y0.device
    one = sdeint(drift_cg, diffusion, y0, t[:1], solver=Euler, options=_opts(seed=1, logqp=True, prior_drift=prior_zero))[1]
    assert one.shape == (3, 2, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["euler", "milstein"])
@pytest.mark.parametrize("walk", ["plain", "step_size"])
def test_the_path_keeps_its_bits_under_logqp(dev, dtype, solver, walk):
    o, _ = _walks(_NPT[dtype])[walk]
    y0 = _y0(dtype, dev, shape=(4, 1, 7))
    t = torch.as_tensor(T_EXACT.astype(_NPT[dtype]))
    tr = Triple(dtype, dev, D=7)
    with torch.no_grad():
        ref = sdeint(tr.drift, tr.diffusion, y0, t, solver=SOLVERS[solver], options=_opts(seed=77, **o))
        ys, logqp = sdeint(tr.drift, tr.diffusion, y0, t, solver=SOLVERS[solver], options=_opts(seed=77, logqp=True, prior_drift=tr.prior, **o))
    assert torch.equal(ys, ref)
    assert bool(torch.isfinite(logqp).all()) and bool((logqp >= 0).all())


# ----------------------------------------------------------------------------------------------
# the closed form of a constant integrand
# ----------------------------------------------------------------------------------------------
def closed_form_bound(t_np, grid, D, eps):
    """``(exact, bound)`` per output interval of ``logqp`` with ``h = 0`` and ``drift = c*g``: every term is ``c^2`` up to three roundings
    in the state dtype (``c*g``, the divide, the square: <= 5 eps (1 + o(1)) relative, held as 6 eps), a step adds ``q * (0.5 dt)`` with
    the double sum's (D - 1) 2^-53 and one rounding each for the scale and the add, relative to ``|acc0| + |q * 0.5 dt|``; summed over
    the grid steps that meet the interval, plus one rounding to the state dtype.  The times are exact (T_EXACT), so ``dt`` carries no error."""
    grid = grid.astype(np.float64)
    term = 0.5 * CC * CC * D * np.diff(grid)  # per grid step
    cum = np.concatenate([[0.0], np.cumsum(term)])
    per_step = 6 * eps * term + (D + 2) * 2.0**-53 * (cum[:-1] + term)
    exact, bound = [], []
    for a, b in zip(t_np[:-1].astype(np.float64), t_np[1:].astype(np.float64)):
        e = 0.5 * CC * CC * D * (b - a)
        meets = (grid[:-1] < b) & (grid[1:] > a)
        exact.append(e)
        bound.append(per_step[meets].sum() + eps * e)
    return np.array(exact), np.array(bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["euler", "milstein"])
@pytest.mark.parametrize("walk", ["plain", "step_size"])
@pytest.mark.parametrize("shape", [(3, 2, 5), (2, 1, 67)])
def test_constant_integrand_gives_the_closed_form(dev, dtype, solver, walk, shape):
    """``h = 0`` and ``drift = c*g``: ``logqp[..., i] = 0.5 c^2 D (t[i+1] - t[i])`` whatever the path does."""
    T = _NPT[dtype]
    o, grid = _walks(T)[walk]
    y0 = _y0(dtype, dev, shape=shape)
    with torch.no_grad():
        _, logqp = sdeint(drift_cg, diffusion, y0, torch.as_tensor(T_EXACT.astype(T)), solver=SOLVERS[solver],
                          options=_opts(seed=5, logqp=True, prior_drift=prior_zero, **o))
    exact, bound = closed_form_bound(T_EXACT, grid, shape[-1], EPS[dtype])
    err = np.abs(logqp.cpu().numpy().astype(np.float64) - exact)
    print("closed form: worst error / bound per interval", (err / np.maximum(bound, 1e-300)).reshape(-1, len(exact)).max(0))
    assert np.all(err <= bound), (err.max(-1), bound)
    assert np.all(logqp.cpu().numpy()[..., 3] == 0)  # (the repeated time: a zero-length interval)


# ----------------------------------------------------------------------------------------------
# the oracle's walk
# ----------------------------------------------------------------------------------------------
def oracle_logqp(tr, y0, t_np, grid, seed, dtype, dev, solver):
    """``(ys in the solution's layout, logqp, bound)`` of the oracle's walk on the backend's normals and the device's evaluations; the
    bound is the accumulate bound ``(D + 2) 2^-53 (|acc0| + |q * 0.5 dt|)`` summed over the steps up to the interval's end — an upper
    bound of what the interval can carry — plus one rounding to the state dtype."""
    T = _NPT[dtype]
    D = y0.shape[-1]
    noise = lambda k: backend_noise(tuple(y0.shape), seed, k, dtype, dev)  # noqa: E731
    g_dev = _on_device(tr.diffusion, dtype, dev)
    mil = None
    if solver == "milstein":
        mil = lambda y, f, g, dt, z: MO.milstein_step(y, f, g, g_dev(None, MO.support(y, f, g, dt, T)), dt, z, T)  # noqa: E731
    states, cums, incs = KL.kl_walk(_on_device(tr.drift, dtype, dev), g_dev, _on_device(tr.prior, dtype, dev), y0.cpu().numpy(), grid, T,
                                    noise, milstein=mil)
    cum_rows = KL.cum_at(cums, grid, t_np)
    step_err = np.cumsum([(D + 2) * 2.0**-53 * (a + b) for a, b in incs], axis=0)  # [steps, *lead]: up to the end of every step
    d = -1 if grid[-1] < grid[0] else 1
    ends = np.clip(np.searchsorted(d * grid, d * t_np[1:], side="left") - 1, 0, len(grid) - 2)
    want = KL.logqp_of(cum_rows, T)
    bound = np.moveaxis(step_err[ends], 0, -1) + EPS[dtype] * np.abs(want)
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states), want, bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["euler", "milstein"])
@pytest.mark.parametrize("walk", ["plain", "step_size"])
def test_logqp_of_a_nonlinear_triple_equals_the_oracle_walk(dev, dtype, solver, walk):
    """``y0`` 3 x 2 x 5: 8 steps on the plain walk (16 on the step_size one, whose outputs fall inside grid steps, on grid points and on
    a repeated time)."""
    T = _NPT[dtype]
    t_np = np.array([0.0, 0.125, 0.25, 0.390625, 0.5, 0.5, 0.625, 0.84375, 1.0]).astype(T)
    o, grid = ({}, t_np) if walk == "plain" else ({"step_size": H_EXACT, "interp": "linear"}, step_size_grid(t_np, H_EXACT))
    y0 = _y0(dtype, dev, shape=(3, 2, 5))
    tr = Triple(dtype, dev)
    with torch.no_grad():
        ys, logqp = sdeint(tr.drift, tr.diffusion, y0, torch.as_tensor(t_np), solver=SOLVERS[solver],
                           options=_opts(seed=0xC0FFEE, logqp=True, prior_drift=tr.prior, **o))
    want_ys, want, bound = oracle_logqp(tr, y0, t_np, grid, 0xC0FFEE, dtype, dev, solver)
    assert np.array_equal(ys.cpu().numpy(), want_ys)
    err = np.abs(logqp.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    print("oracle walk: worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), (err.max(), bound.min())
    assert float(np.abs(want).max()) > 1e-3  # (a KL term worth the name)


# ----------------------------------------------------------------------------------------------
# gradients against the same walk in framework ops
# ----------------------------------------------------------------------------------------------
def torch_walk(fns, y0, t_np, grid, seed, dtype, dev, solver="euler", reverse=False):
    """``(ys, logqp)`` of the walk over ``grid`` in framework ops on the backend's normals, in sdeint's layouts at the output times
    ``t_np``: Euler-Maruyama's or Milstein's state update in the kernels' op order, the row sum taken in element order (``reverse``: in
    the reversed order) one add at a time, and an output inside a grid step the linear blend of both the states and the cumulative
    sums.  ``fns = (drift, diffusion, prior)``."""
    T = _NPT[dtype]
    drift, diff, prior = fns
    y, acc = y0, torch.zeros(y0.shape[:-1], dtype=torch.float64, device=y0.device)
    states, cums = [y0], [acc]
    for k in range(len(grid) - 1):
        dt = T(grid[k + 1] - grid[k])
        dtf, sf = float(dt), float(SO.s_of(dt, T))
        z = torch.from_numpy(backend_noise(tuple(y0.shape), seed, k, dtype, dev)).to(dev)
        f, g, h = drift(None, y), diff(None, y), prior(None, y)
        u = (f - h) / g
        tt = (u * u).double()
        q = None
        for d_ in (range(tt.shape[-1] - 1, -1, -1) if reverse else range(tt.shape[-1])):
            q = tt[..., d_] if q is None else q + tt[..., d_]
        acc = acc + q * (0.5 * dtf)
        if solver == "milstein":
            gb = diff(None, (y + f * dtf) + g * sf)
            w = sf * z
            y = ((y + f * dtf) + g * w) + (gb - g) * (float(MO.c_of(dt, T)) * (w * w - abs(dtf)))
        else:
            y = (y + f * dtf) + g * (sf * z)
        states.append(y)
        cums.append(acc)
    d = -1 if grid[-1] < grid[0] else 1
    rows, cum_rows = [states[0]], [cums[0]]
    for tj in t_np[1:]:
        k = min(max(int(np.searchsorted(d * grid, d * tj, side="left")) - 1, 0), len(grid) - 2)
        ta, tb = grid[k], grid[k + 1]
        if tj == ta or tj == tb:
            i = k if tj == ta else k + 1
            rows.append(states[i])
            cum_rows.append(cums[i])
        else:
            w = float(T((tj - ta) / (tb - ta)))
            rows.append(states[k] + w * (states[k + 1] - states[k]))
            cum_rows.append(cums[k] + w * (cums[k + 1] - cums[k]))
    ys = torch.stack(rows, dim=-3)
    logqp = torch.stack([b - a for a, b in zip(cum_rows[:-1], cum_rows[1:])], dim=-1).to(dtype)
    return ys.reshape(ys.shape[:-3] + (ys.shape[-3] * ys.shape[-2], ys.shape[-1])), logqp


def _frozen(fn):
    """``fn`` evaluated without a graph: a coefficient that takes no gradient and hands none on to the state."""
    def call(t, y):
        with torch.no_grad():
            return fn(t, y)
    return call


@pytest.mark.parametrize("leaves", ["all", "prior"])
@pytest.mark.parametrize("walk", ["plain", "step_size"])
@pytest.mark.parametrize("solver", ["euler", "milstein"])
def test_gradients_of_path_and_logqp_equal_the_framework_walk(dev, solver, walk, leaves):
    """fp64, ``y0`` 3 x 2 x 5, 8 steps of unequal size (``step_size``: 16 steps of 2^-4 under five output intervals, outputs inside
    grid steps): the gradients of a weighted sum of ``ys`` and ``logqp`` (fixed random weights, so every cotangent differs) against the
    same walk in framework ops — with respect to ``y0`` and every parameter of the three networks (``all``), and with respect to the
    prior's parameters alone while ``y0`` takes no gradient and drift and diffusion are evaluated without a graph (``prior``: the
    state's steps are then not differentiated, only the prior's own graph keeps the states it was evaluated at).
    The tolerance comes from the reference alone: the largest relative difference (per tensor, relative to its largest entry) between two
    evaluations of the framework walk, the row sum in element order and reversed, times 16 (the kernel's third summation order and the
    one extra rounding of ``a``), with a floor of 2^-40 = 9.1e-13.  Measured: the two framework walks give the same gradients bit for bit
    (the order of a sum does not enter its gradient), so the floor is the bar; the product's gradients differ from the reference's by at
    most 1.1e-15 over the eight cases on the numpy double and on an MI355X alike (the test prints its figures)."""
    dtype = torch.float64
    if walk == "plain":
        t_np, o = np.array([0.0, 0.1, 0.25, 0.3, 0.45, 0.6, 0.7, 0.9, 1.0]), {}
        grid = t_np
    else:
        t_np, o = np.array([0.0, 0.1, 0.33, 0.5, 0.77, 1.0]), {"step_size": H_EXACT, "interp": "linear"}
        grid = step_size_grid(t_np, H_EXACT)
    seed = 0xBEEF
    tr = Triple(dtype, dev)
    y0 = _y0(dtype, dev, shape=(3, 2, 5))
    if leaves == "all":
        y0.requires_grad_(True)
        fns, wrt = (tr.drift, tr.diffusion, tr.prior), [y0] + tr.params()
    else:
        fns, wrt = (_frozen(tr.drift), _frozen(tr.diffusion), tr.prior), list(tr.p["h"])
    gen = torch.Generator().manual_seed(21)
    wy = torch.randn(3, len(t_np) * 2, 5, generator=gen, dtype=dtype).to(dev)
    wl = torch.randn(3, 2, len(t_np) - 1, generator=gen, dtype=dtype).to(dev)

    def grads(ys, logqp):
        loss = (ys * wy).sum() + (logqp * wl).sum()
        return [torch.zeros_like(x) if g is None else g for x, g in zip(wrt, torch.autograd.grad(loss, wrt, allow_unused=True))]

    ref = grads(*torch_walk(fns, y0, t_np, grid, seed, dtype, dev, solver))
    rev = grads(*torch_walk(fns, y0, t_np, grid, seed, dtype, dev, solver, reverse=True))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    measured = max(rel(a, b) for a, b in zip(rev, ref))
    tol = max(16 * measured, 2.0**-40)
    ys, logqp = sdeint(fns[0], fns[1], y0, torch.as_tensor(t_np), solver=SOLVERS[solver],
                       options=_opts(seed=seed, logqp=True, prior_drift=fns[2], **o))
    with torch.no_grad():
        fwd = torch_walk(fns, y0, t_np, grid, seed, dtype, dev, solver)
    assert torch.allclose(ys.detach(), fwd[0], rtol=1e-12, atol=0) and torch.allclose(logqp.detach(), fwd[1], rtol=1e-11, atol=0)
    got = grads(ys, logqp)
    worst = max(rel(a, b) for a, b in zip(got, ref))
    print("gradients[{} {} {}]: reference's own spread {:.3e}, tolerance {:.3e}, product against reference {:.3e}".format(
        solver, walk, leaves, measured, tol, worst))
    assert all(float(b.abs().max()) > 0 for b in ref)  # (every leaf is reached)
    assert worst <= tol, (worst, tol)
