"""End-to-end cases of ``ddeint_steps``, run on the numpy double (tests/test_dde_tape_host.py) and on the GPU
(tests/test_gpu_dde_tape.py) through the ``dev`` fixture of each module.  The references are tests/_dde_tape_oracle.py (the walk in
numpy, bit for bit), the closed form of ``y' = -y(t - 1)`` (the method of steps), and the same recursion written in framework ops."""
import math

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import ddeint_steps
from paddlexde_amd.solver import RK4, Euler, Midpoint
from paddlexde_amd.solver.base_fixed_solver import step_size_grid
from paddlexde_amd.xde.steps_dde import pick_interval, stage_time

from . import _dde_tape_oracle as DO

_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SOLVERS = {"euler": Euler, "midpoint": Midpoint, "rk4": RK4}

# y' = -y(t - 1), phi = 1, h = 1/4, fp64, RK4: the largest error against the closed form on [0, 3], measured on the numpy double (the
# test prints its figure): 1.110e-16; the bar on both backends is 16 times that (DESIGN sections 10 and 19)
EXACT_MEASURED_ON_THE_DOUBLE = 1.110e-16
EXACT_BAR = 16 * EXACT_MEASURED_ON_THE_DOUBLE
# the gradients of test_gradients_equal_the_framework_recursion, relative to the largest gradient magnitude of each leaf, measured on
# the numpy double (the test prints its figure): 3.843e-16, the worst of the six leaves (y0 3.413e-16, the field's four parameters
# 3.736e-16 2.298e-16 3.418e-16 1.814e-16, lags 3.843e-16); the bar on both backends is 16 times that, 6.149e-15
GRAD_MEASURED_ON_THE_DOUBLE = 3.843e-16
GRAD_BAR = 16 * GRAD_MEASURED_ON_THE_DOUBLE


def _tables(D):
    """Four [D] tables of exactly representable constants (multiples of 1/16 in [-1, 1]): the same bits in numpy and in torch."""
    i = np.arange(D)
    return [((i * m) % q - q // 2) / 16.0 for m, q in ((7, 17), (5, 13), (3, 11), (11, 15))]


class Field:
    """A field built from single multiplies and adds, ``(y A + y_lags[0] B) + (y_lags[1] C + y_lags[-1] y E)`` plus one product per
    further delay, as a torch function on ``dev`` and as a numpy function on the same bits."""

    def __init__(self, D, dtype, dev):
        self.np_tabs = [x.astype(_NPT[dtype]) for x in _tables(D)]
        self.tabs = [torch.as_tensor(x).to(dev) for x in self.np_tabs]

    @staticmethod
    def _f(y, yl, tabs):
        A, B, C, E = tabs
        acc = (y * A + yl[..., 0:1, :] * B) + (yl[..., 1:2, :] * C + (yl[..., -1:, :] * y) * E)
        for j in range(2, yl.shape[-2] - 1):  # (every delay reaches the result)
            acc = acc + yl[..., j : j + 1, :] * tabs[j % 4]
        return acc

    def torch(self, t, y, yl):
        return self._f(y, yl, self.tabs)

    def numpy(self, t, y, yl):
        return self._f(y, yl, self.np_tabs)


def _history(lead, Th, D, dtype, seed=0):
    """Samples of an initial function on ``linspace(-1, 0, Th)`` (Th - 1 a power of two: the forward differences divide exactly)."""
    g = torch.Generator().manual_seed(seed)
    his = (0.5 * torch.randn(*lead, Th, D, generator=g, dtype=torch.float64)).to(dtype)
    return his, np.linspace(-1.0, 0.0, Th)


# lags: on the grid (1.0, 0.5), off it (0.6), two in one interval (0.6 and 0.55), the shortest allowed (0.25 = h: the first stage
# falls back one interval)
LAGS = [1.0, 0.6, 0.55, 0.5, 0.25]


# ----------------------------------------------------------------------------------------------
# the walk against the oracle
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["plain", "step_size"])
@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
def test_walk_equals_the_oracle_bit_for_bit(dev, dtype, times, solver):
    T = _NPT[dtype]
    his, his_t = _history((4,), 5, 7, dtype)
    o, grid = {}, None
    if times == "step_size":
        t_np = np.array([0.0, 0.3, 0.75, 0.75 + 1 / 16, 1.5], dtype=T)
        o, grid = {"step_size": 0.25, "interp": "linear"}, step_size_grid(t_np, 0.25)
        assert np.array_equal(grid, np.arange(7, dtype=T) * T(0.25))
    else:
        t_np = (np.arange(7) * 0.25).astype(T)
    field = Field(7, dtype, dev)
    lags = torch.tensor(LAGS, dtype=torch.float64)
    with torch.no_grad():
        sol = ddeint_steps(field.torch, his.to(dev), torch.as_tensor(his_t), torch.as_tensor(t_np), lags, solver=SOLVERS[solver], options=o)
    assert sol.shape == (4, len(t_np), 7) and sol.dtype == dtype
    want = DO.walk(field.numpy, his.numpy(), his_t, t_np, LAGS, solver, T, grid=grid)
    assert np.array_equal(sol.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_more_delays_than_one_launch_takes(dev, dtype):
    """L = XDE_DDE_MAX_LAGS + 1: the binding serves them in two tiles; the same bits as the oracle, which knows no tiles."""
    T = _NPT[dtype]
    L = _hip.XDE_DDE_MAX_LAGS + 1
    his, his_t = _history((2,), 5, 5, dtype, seed=1)
    lag_list = [0.25 + 0.75 * j / (L - 1) for j in range(L)]
    field = Field(5, dtype, dev)
    t_np = (np.arange(4) * 0.25).astype(T)
    with torch.no_grad():
        sol = ddeint_steps(field.torch, his.to(dev), torch.as_tensor(his_t), torch.as_tensor(t_np), torch.tensor(lag_list, dtype=torch.float64))
    assert np.array_equal(sol.cpu().numpy(), DO.walk(field.numpy, his.numpy(), his_t, t_np, lag_list, "rk4", T))


def test_his_derivative_is_taken_as_given(dev):
    dtype, T = torch.float64, np.float64
    his, his_t = _history((3,), 3, 4, dtype, seed=2)
    hf = torch.randn(3, 3, 4, generator=torch.Generator().manual_seed(5), dtype=dtype)
    field = Field(4, dtype, dev)
    t_np = np.arange(5) * 0.25
    with torch.no_grad():
        sol = ddeint_steps(field.torch, his.to(dev), torch.as_tensor(his_t), torch.as_tensor(t_np), torch.tensor(LAGS[:3], dtype=dtype),
                           his_derivative=hf.to(dev))
    assert np.array_equal(sol.cpu().numpy(), DO.walk(field.numpy, his.numpy(), his_t, t_np, LAGS[:3], "rk4", T, hf=hf.numpy()))


# ----------------------------------------------------------------------------------------------
# y' = -y(t - 1), phi = 1: the method of steps
# ----------------------------------------------------------------------------------------------
def closed_form(t):
    """sum_k (-1)^k (t - k + 1)^k / k! over k = 0 .. floor(t) + 1 (t >= 0)."""
    return sum((-1.0) ** k * (t - k + 1.0) ** k / math.factorial(k) for k in range(int(math.floor(t)) + 2))


def _delayed_decay(dev, h, t_end, solver=RK4):
    his = torch.ones(1, 5, 1, dtype=torch.float64, device=dev)
    t = torch.as_tensor(np.arange(int(round(t_end / h)) + 1) * h)
    with torch.no_grad():
        sol = ddeint_steps(lambda t_, y, yl: -yl, his, torch.linspace(-1.0, 0.0, 5, dtype=torch.float64), t, torch.tensor([1.0], dtype=torch.float64),
                           solver=solver)
    want = np.array([closed_form(float(x)) for x in t])
    return float(np.abs(sol.cpu().numpy()[0, :, 0] - want).max())


def test_the_scheme_is_exact_while_the_solution_is_piecewise_cubic(dev):
    """h = 1/4 up to t = 3: the solution is piecewise cubic with its breaks on grid points, which the Hermite tape reproduces and RK4's
    quadrature integrates exactly.  (A tape that merged the two derivatives at t0 would be two orders worse.)"""
    err = _delayed_decay(dev, 0.25, 3.0)
    print("y' = -y(t - 1) on [0, 3], h = 1/4: largest error {:.3e}, bar {:.3e}".format(err, EXACT_BAR))
    assert err <= EXACT_BAR, (err, EXACT_BAR)


def test_the_observed_order_is_four(dev):
    errs = [_delayed_decay(dev, h, 5.0) for h in (0.25, 0.125, 0.0625)]
    order = math.log2(errs[0] / errs[2]) / 2
    print("y' = -y(t - 1) on [0, 5]: errors {:.3e} {:.3e} {:.3e}, observed order {:.2f}".format(*errs, order))
    assert 3.5 <= order <= 4.5, (errs, order)


# ----------------------------------------------------------------------------------------------
# gradients against the same recursion in framework ops
# ----------------------------------------------------------------------------------------------
class _Net:
    """A small MLP field on (y, y_lags): ``tanh([y, y_lags] A + a) B + b``."""

    def __init__(self, D, L, dtype, dev, seed=17):
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: (0.5 * torch.randn(*s, generator=g, dtype=torch.float64)).to(dev, dtype).requires_grad_(True)  # noqa: E731
        self.p = [mk((L + 1) * D, 8), mk(8), mk(8, D), mk(D)]

    def __call__(self, t, y, yl):
        A, a, B, b = self.p
        x = torch.cat([y, yl], dim=-2).flatten(-2).unsqueeze(-2)
        return torch.tanh(x @ A + a) @ B + b


def _twin(net, his, his_t, t_np, lags, hf=None):
    """RK4 (the reference's variant) with the Hermite tape in framework ops, float64: the intervals from the host rule, sigma and the
    weights as differentiable functions of ``lags``, the history's forward-difference derivative as a differentiable function of
    ``y0`` (``his``' last row)."""
    grid = np.asarray(t_np, dtype=np.float64)
    lag_host = lags.detach().cpu().numpy().astype(np.float64)
    if hf is None:
        ht = torch.as_tensor(his_t, dtype=his.dtype, device=his.device)
        d = (his[..., 1:, :] - his[..., :-1, :]) / (ht[1:] - ht[:-1]).unsqueeze(-1)
        hf = torch.cat([d, d[..., -1:, :]], dim=-2)
    # (the history's samples are constants; its forward-difference derivative is not: the last two rows hold y0, his' last row)
    his = his.detach()
    tape_y, tape_f = [], []

    def delayed(k, i, c):
        s = stage_time(grid, k, c)
        vals = []
        for j in range(len(lag_host)):
            kind, m, a, b = pick_interval(s - lag_host[j], np.asarray(his_t, dtype=np.float64), grid, k, i)
            h = b - a
            sg = ((s - a) - lags[j]) / h
            s2 = sg * sg
            s3 = s2 * sg
            w = (2 * s3 - 3 * s2 + 1, h * (s3 - 2 * s2 + sg), -2 * s3 + 3 * s2, h * (s3 - s2))
            if kind == "his":
                yb = tape_y[0] if m + 1 == his.shape[-2] - 1 else his[..., m + 1 : m + 2, :]
                ops = (his[..., m : m + 1, :], hf[..., m : m + 1, :], yb, hf[..., m + 1 : m + 2, :])
            else:
                ops = (tape_y[m], tape_f[m], tape_y[m + 1], tape_f[m + 1])
            vals.append((ops[0] * w[0] + ops[1] * w[1]) + (ops[2] * w[2] + ops[3] * w[3]))
        return torch.cat(vals, dim=-2)

    return delayed, tape_y, tape_f


def _twin_solve(net, his, his_t, t_np, lags, y0):
    delayed, tape_y, tape_f = _twin(net, his, his_t, t_np, lags)
    fuse = lambda dy, dt, y: dy * dt + y  # noqa: E731
    y, out = y0, [y0]
    for k in range(len(t_np) - 1):
        dt = float(t_np[k + 1] - t_np[k])
        tape_y.append(y)
        k1 = net(None, y, delayed(k, 0, 0.0))
        tape_f.append(k1)
        k2 = net(None, fuse(k1, dt * (1 / 3), y), delayed(k, 1, 1 / 3))
        k3 = net(None, fuse(k1 - k2 * (1 / 3), dt, y), delayed(k, 2, 2 / 3))
        k4 = net(None, fuse(k1 - k2 + k3, dt, y), delayed(k, 3, 1.0))
        y = (fuse(k1, dt, y) + 3 * fuse(k2, dt, y) + 3 * fuse(k3, dt, y) + fuse(k4, dt, y)) * 0.125
        out.append(y)
    return torch.cat(out, dim=-2)


def test_gradients_equal_the_framework_recursion(dev):
    """fp64, (rows, D, L) = (3, 5, 2), five RK4 steps, delays off the grid: the gradients of a weighted sum of the path (fixed random
    weights) with respect to y0, every parameter of the field and the delays against the same recursion in framework ops.  The bar is
    16 times the discrepancy measured on the numpy double (GRAD_BAR above), per leaf, relative to that leaf's largest gradient."""
    dtype = torch.float64
    rows, D, L = 3, 5, 2
    hist, his_t = _history((rows,), 5, D, dtype, seed=3)
    hist = hist.to(dev)
    y0 = hist[..., -1:, :].clone().requires_grad_(True)
    lags = torch.tensor([0.7, 0.3], dtype=dtype, device=dev, requires_grad=True)
    net = _Net(D, L, dtype, dev)
    t_np = np.arange(6) * 0.25
    w = torch.randn(rows, len(t_np), D, generator=torch.Generator().manual_seed(3), dtype=dtype).to(dev)
    leaves = [y0] + net.p + [lags]
    his = torch.cat([hist[..., :-1, :], y0], dim=-2)
    sol = ddeint_steps(net, his, torch.as_tensor(his_t), torch.as_tensor(t_np), lags)
    got = torch.autograd.grad((sol * w).sum(), leaves)
    ref = _twin_solve(net, his, his_t, t_np, lags, y0)
    assert torch.allclose(sol.detach(), ref.detach(), rtol=1e-13, atol=1e-14)
    want = torch.autograd.grad((ref * w).sum(), leaves)
    each = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
    print("gradients: per leaf against the framework recursion {}, worst {:.3e}, bar {:.3e}".format(
        " ".join("{:.3e}".format(x) for x in each), max(each), GRAD_BAR))
    assert all(float(b.abs().max()) > 0 for b in want)  # (every leaf is reached)
    assert max(each) <= GRAD_BAR, (each, GRAD_BAR)


@pytest.mark.parametrize("derivative", ["forward_difference", "given"])
def test_gradcheck_through_three_steps(dev, derivative):
    """float64, (rows, D, L) = (2, 3, 2), three RK4 steps, the tool's default tolerances, the delays kept away from theta = t0 (where the
    interpolant's derivative jumps): with respect to y0, a parameter of the field and the delays — with the history's derivative taken
    as the forward difference of the samples (whose last two rows move with y0) and with it given."""
    dtype = torch.float64
    hist, his_t = _history((2,), 5, 3, dtype, seed=4)
    hist = hist.to(dev)
    t = torch.as_tensor(np.arange(4) * 0.25)
    P = torch.randn(3, generator=torch.Generator().manual_seed(6), dtype=dtype).to(dev)
    hf = torch.randn(2, 5, 3, generator=torch.Generator().manual_seed(7), dtype=dtype).to(dev) if derivative == "given" else None

    def fn(y0, a, lags):
        his = torch.cat([hist[..., :-1, :], y0], dim=-2)
        return ddeint_steps(lambda t_, y, yl: torch.tanh(y * a + yl[..., 0:1, :] * P) - yl[..., 1:2, :] * 0.5, his, torch.as_tensor(his_t), t, lags,
                            his_derivative=hf)

    inputs = [hist[..., -1:, :].clone().requires_grad_(True), torch.tensor(-0.6, dtype=dtype, device=dev, requires_grad=True),
              torch.tensor([0.8, 0.35], dtype=dtype, device=dev, requires_grad=True)]
    assert torch.autograd.gradcheck(fn, inputs)


def test_delays_on_the_host_take_their_gradient_there(dev):
    """``lags`` on the CPU beside a history on ``dev``: the plan only reads them, and their gradient comes back to their device."""
    dtype = torch.float64
    hist, his_t = _history((2,), 5, 3, dtype, seed=4)
    lags = torch.tensor([0.8, 0.35], dtype=dtype, requires_grad=True)
    sol = ddeint_steps(lambda t_, y, yl: -yl[..., 0:1, :] * yl[..., 1:2, :], hist.to(dev), torch.as_tensor(his_t), torch.as_tensor(np.arange(4) * 0.25), lags)
    sol.sum().backward()
    assert lags.grad.device == lags.device and float(lags.grad.abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_classic_rk4_variant_walks_its_own_stage_times(dev, dtype):
    """``options={"variant": "classic"}``: stages at 0, 1/2, 1/2, 1 of the step — against the oracle's classic step, bit for bit."""
    T = _NPT[dtype]
    his, his_t = _history((3,), 5, 6, dtype, seed=8)
    field = Field(6, dtype, dev)
    t_np = (np.arange(6) * 0.25).astype(T)
    with torch.no_grad():
        sol = ddeint_steps(field.torch, his.to(dev), torch.as_tensor(his_t), torch.as_tensor(t_np), torch.tensor(LAGS, dtype=torch.float64),
                           solver=RK4, options={"variant": "classic"})
    assert np.array_equal(sol.cpu().numpy(), DO.walk(field.numpy, his.numpy(), his_t, t_np, LAGS, "rk4_classic", T))


def test_an_unwanted_cotangent_is_not_computed(dev):
    """Nothing but the delays takes a gradient: the tape's nodes stay without one."""
    dtype = torch.float64
    hist, his_t = _history((2,), 5, 3, dtype, seed=4)
    lags = torch.tensor([0.8, 0.35], dtype=dtype, device=dev, requires_grad=True)
    sol = ddeint_steps(lambda t_, y, yl: -yl[..., 0:1, :] * yl[..., 1:2, :], hist.to(dev), torch.as_tensor(his_t), torch.as_tensor(np.arange(4) * 0.25), lags)
    (g,) = torch.autograd.grad(sol.sum(), (lags,))
    assert g.shape == (2,) and float(g.abs().max()) > 0
