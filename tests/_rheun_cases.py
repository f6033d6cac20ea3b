"""End-to-end cases of sdeint(..., solver=ReversibleHeun) and sdeint_adjoint, run on the numpy double (tests/test_rheun_host.py) and on
the GPU (tests/test_gpu_rheun.py) through the ``dev`` fixture of each module.  Every walk is compared with tests/_rheun_oracle.py fed
the backend's own draws (``_sde_noise``): on the double those are the oracle's, on the GPU the kernel's."""
import importlib

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint, sdeint_adjoint
from paddlexde_amd.solver import SRK, Euler, Milstein, ReversibleHeun
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _rheun_oracle as RO
from . import _sde_oracle as SO
from ._sde_cases import _NPT, _opts, _y0, backend_noise
from ._srk_cases import LAM, MU, diffusion, drift

ADJ = importlib.import_module("paddlexde_amd.functional.sdeint_adjoint")  # (the package attribute of that name is the function)
_EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}

# Every bar below is 16 times the worst figure measured on the numpy double (the margin covers the change of summation order between
# numpy / torch's CPU kernels and the device); the measured figures are in the docstring of the test that asserts the bar.
# test_gradients_equal_the_autograd_twin: largest discrepancy / largest gradient magnitude
GRAD_MEASURED = 1.748e-16  # (0.79 * 2^-52)
GRAD_BAR = 16 * GRAD_MEASURED
# test_adjoint_equals_the_gradient_through_the_steps: the same ratio, per dtype, the worst of the two runs
ADJ_MEASURED = {torch.float32: 1.343e-07, torch.float64: 2.754e-16}
ADJ_BAR = {k: 16 * v for k, v in ADJ_MEASURED.items()}
# test_the_sweep_reconstructs_y0: max |y0 reconstructed - y0| / max |y0|, per dtype
RECON_MEASURED = {torch.float32: 2.421e-07, torch.float64: 3.382e-16}
RECON_BAR = {k: 16 * v for k, v in RECON_MEASURED.items()}
# test_reverse_after_forward_returns_the_state: max |(y0, yh0) returned - (y0, yh0)| / max |operand|, per dtype
REVERSE_MEASURED = {torch.float32: 1.174e-07, torch.float64: 2.187e-16}
REVERSE_BAR = {k: 16 * v for k, v in REVERSE_MEASURED.items()}


def _oracle(y0, t_np, seed, dtype, dev, grid=None, f=drift, g=diffusion):
    grid = t_np if grid is None else grid
    states = RO.rheun_walk(f, g, y0.cpu().numpy(), grid, seed, _NPT[dtype],
                           noise=lambda k: backend_noise(tuple(y0.shape), seed, k, dtype, dev))
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states)


class _Net(torch.nn.Module):
    """An MLP coefficient 5-8-5 (tanh) that counts its evaluations."""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Tanh(), torch.nn.Linear(8, 5))
        self.calls = 0

    def forward(self, t, y):
        self.calls += 1
        return self.net(y)


def _nets(dtype, dev):
    torch.manual_seed(0)
    return _Net().to(dev, dtype), _Net().to(dev, dtype)


def _weights(sol, seed=1):
    return torch.randn(sol.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(sol.device, sol.dtype)


def _relative(got, want):
    scale = max(float(b.abs().max()) for b in want)
    return max(float((a - b).abs().max()) for a, b in zip(got, want)) / scale


ADJOINT_RUNS = {"plain": (np.linspace(0.0, 1.0, 9), {}), "step_size": (np.array([0.0, 0.1, 0.3, 0.3, 0.45]), {"step_size": 0.05})}


# ----------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["increasing", "decreasing", "repeated", "step_size"])
def test_rheun_walk_equals_the_oracle_bit_for_bit(dev, dtype, times):
    T = _NPT[dtype]
    t_np = {"increasing": np.array([0.0, 0.1, 0.25, 0.3, 0.7, 1.0]), "decreasing": np.array([1.0, 0.8, 0.55, 0.5, 0.0]),
            "repeated": np.array([0.0, 0.2, 0.2, 0.2, 0.5, 0.5, 0.9]),
            "step_size": np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0])}[times].astype(T)
    o, grid = {}, None
    if times == "step_size":
        o, grid = {"step_size": 0.1, "interp": "linear"}, step_size_grid(t_np, 0.1)
    y0 = _y0(dtype, dev, shape=(4, 1, 7))  # (28 elements: a tail of the fp32 vector and fp64 pair at the end)
    seed = 0x1234_5678_9ABC_DEF0
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=ReversibleHeun, options=_opts(seed=seed, **o))
    got = sol.cpu().numpy()
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, _oracle(y0, t_np, seed, dtype, dev, grid=grid))
    if times == "repeated":  # a zero-length step (dt = 0, s = 0) returns the state: exact copies, no NaN
        assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 2], got[:, 3]) and np.array_equal(got[:, 4], got[:, 5])
    # not the Milstein path of the same seed; and sdeint_adjoint's forward is this walk
    mil = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Milstein, options=_opts(seed=seed, **o))
    assert not np.array_equal(got, mil.cpu().numpy())
    adj = sdeint_adjoint(drift, diffusion, y0, torch.as_tensor(t_np), solver=ReversibleHeun, options=_opts(seed=seed, **o), adjoint_params=())
    assert torch.equal(adj, sol)


def test_auto_pipeline_keeps_the_eager_loop_for_rheun(dev):
    y0 = _y0(torch.float32, dev, shape=(1, 2))
    t = torch.linspace(0.0, 1.0, 40)
    with torch.no_grad():
        a = sdeint(drift, diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=3))
        b = sdeint(drift, diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=3, pipeline="sync"))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), _oracle(y0[None], t.numpy(), 3, torch.float32, dev)[0])


def test_evaluation_counts_of_the_forward_and_of_the_sweep(dev):
    """n_steps + 1 drift and n_steps + 1 diffusion evaluations in the forward (one at the first grid point, one per step), and the same
    in the backward sweep (one at the last grid point, one per backward step); nfe counts steps."""
    from paddlexde_amd.xde.base_sde import BaseSDE

    f, g = _nets(torch.float64, dev)
    y0 = _y0(torch.float64, dev, shape=(6, 1, 5)).requires_grad_(True)
    t = torch.tensor([0.0, 0.1, 0.3, 0.3, 0.45], dtype=torch.float64)
    n_steps = len(step_size_grid(t.numpy(), 0.05)) - 1
    sol = sdeint_adjoint(f, g, y0, t, solver=ReversibleHeun, options=_opts(seed=5, step_size=0.05))
    assert (f.calls, g.calls) == (n_steps + 1, n_steps + 1)
    sol.sum().backward()
    assert (f.calls, g.calls) == (2 * (n_steps + 1), 2 * (n_steps + 1))
    s = ReversibleHeun(xde=BaseSDE(drift, diffusion, y0.detach(), t, seed=3), y0=y0.detach(), rtol=1e-7, atol=1e-9, norm=None)
    with torch.no_grad():
        s.integrate(t)
    assert s.nfe == len(t) - 1 and ReversibleHeun.order == 1 and "STRATONOVICH" in ReversibleHeun.__doc__


# ----------------------------------------------------------------------------------------------
# strong order
# ----------------------------------------------------------------------------------------------
def _gbm(direction):
    """dX = 2 X dt + X o dW, X0 = 1: exact exp(2 T + W_T); its Ito form has the drift (2 + direction / 2) X."""
    return (lambda t_, y: 2.0 * y, lambda t_, y: y, 1.0, lambda W: torch.exp(2.0 * direction + W),
            lambda t_, y: (2.0 + 0.5 * direction) * y)


def _arctan():
    """dX = cos^2 X o dW, X0 = 0.3: exact arctan(W_T + tan X0); its Ito form has the drift -sin X cos^3 X."""
    x0 = 0.3

    def g(t_, y):
        c = torch.cos(y)
        return c * c

    def ito(t_, y):
        c = torch.cos(y)
        return -torch.sin(y) * c * c * c

    return lambda t_, y: torch.zeros_like(y), g, x0, lambda W: torch.atan(W + float(np.tan(x0))), ito


@pytest.mark.parametrize("case", ["gbm_increasing", "gbm_decreasing", "arctan"])
def test_strong_order_one(dev, case):
    """fp64, 2^16 paths, seed 11, h = 2^-3 .. 2^-8 on [0, 1] (gbm_decreasing: on [0, -1]); W_T from sdeint(0, 1, Euler) with the same
    seed and grid.  The slope of log E|X_rheun - X| against log h lies in [0.75, 1.25]: order 1, which the scheme attains for noise
    whose element i depends on y_i only.  The h = 2^-8 error is printed next to Milstein's on the Ito form of the same equation (no
    assertion).  The numpy double on the oracle's Philox noise gives
      gbm_increasing  slope 0.985  (errors 1.83, 9.43e-1, 4.73e-1, 2.41e-1, 1.20e-1, 6.06e-2; Milstein 1.74e-1, Milstein / rheun 2.87)
      gbm_decreasing  slope 1.031  (errors 9.29e-2, 4.24e-2, 2.04e-2, 1.02e-2, 5.11e-3, 2.55e-3; Milstein 1.54e-3, ratio 0.60)
      arctan          slope 0.899  (errors 3.27e-2, 1.92e-2, 1.06e-2, 5.61e-3, 2.89e-3, 1.48e-3; Milstein 1.55e-3, ratio 1.05)
    (each inside [0.8, 1.2], the range the statement of the scheme itself was held to before any GPU run)."""
    direction = -1 if case == "gbm_decreasing" else 1
    f, g, x0, exact_of, ito = _arctan() if case == "arctan" else _gbm(direction)
    M, seed = 1 << 16, 11
    hs, errs = [], []
    start = torch.full((1, M), x0, dtype=torch.float64, device=dev)
    o = {"norm": None, "seed": seed}
    with torch.no_grad():
        for p in range(3, 9):
            N = 2**p
            t = direction * torch.arange(N + 1, dtype=torch.float64) / N
            W = sdeint(lambda t_, y: torch.zeros_like(y), lambda t_, y: torch.ones_like(y), torch.zeros_like(start), t, solver=Euler,
                       options=o)[-1]
            X = sdeint(f, g, start, t, solver=ReversibleHeun, options=o)[-1]
            exact = exact_of(W)
            hs.append(1.0 / N)
            errs.append(float((X - exact).abs().mean()))
        milstein = float((sdeint(ito, g, start, t, solver=Milstein, options=o)[-1] - exact).abs().mean())
    slope = float(np.polyfit(np.log(hs), np.log(errs), 1)[0])
    print(case, "slope", slope, "errors", errs, "milstein (Ito form) at the finest h", milstein, "ratio", milstein / errs[-1])
    assert 0.75 <= slope <= 1.25, (slope, errs)


# ----------------------------------------------------------------------------------------------
# gradients through the steps
# ----------------------------------------------------------------------------------------------
def test_gradients_equal_the_autograd_twin(dev):
    """d(sum of the last row)/d(y0, lam, mu) through sdeint(ReversibleHeun), fp64, 8 steps, 64 paths, against the same recursion in
    plain torch ops on the same Z, differentiated by autograd: two float64 statements of one sum in different orders.  Measured on the
    numpy double: the values agree bit for bit; the largest gradient discrepancy is 1.748e-16 (0.79 * 2^-52) of the largest
    gradient magnitude, GRAD_MEASURED.  The bar is 16 times that."""
    dtype, T = torch.float64, np.float64
    t_np = np.linspace(0.0, 1.0, 9)
    y0 = (0.5 + torch.rand((1, 64), generator=torch.Generator().manual_seed(7), dtype=dtype)).to(dev).requires_grad_(True)
    lam = torch.tensor(-0.6, dtype=dtype, device=dev, requires_grad=True)
    mu = torch.tensor(0.4, dtype=dtype, device=dev, requires_grad=True)
    params = [y0, lam, mu]
    sol = sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, y0, torch.as_tensor(t_np), solver=ReversibleHeun, options=_opts(seed=9))
    got = torch.autograd.grad(sol[-1:].sum(), params)
    y = yh = y0
    f, g = lam * y, mu * y
    for k in range(len(t_np) - 1):
        dt = T(t_np[k + 1] - t_np[k])
        s, h = float(SO.s_of(dt, T)), float(dt)
        w = s * torch.as_tensor(backend_noise((1, 64), 9, k, dtype, dev)).to(dev)
        yh1 = (((y + y) - yh) + f * h) + g * w
        f1, g1 = lam * yh1, mu * yh1
        y = (y + (f + f1) * (0.5 * h)) + (g + g1) * (0.5 * w)
        yh, f, g = yh1, f1, g1
    assert torch.equal(sol[-1:].detach(), y.detach())
    want = torch.autograd.grad(y.sum(), params)
    worst = _relative(got, want)
    print("largest gradient discrepancy / largest gradient magnitude:", worst, "=", worst / 2.0**-52, "* 2^-52")
    assert worst <= GRAD_BAR, worst
    assert all(float(x.abs().max()) > 0 for x in got)


# ----------------------------------------------------------------------------------------------
# the adjoint
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("run", ["plain", "step_size"])
def test_adjoint_equals_the_gradient_through_the_steps(dev, dtype, run):
    """sdeint_adjoint(ReversibleHeun) against autograd through sdeint(ReversibleHeun), same seed: MLP drift and diffusion (5-8-5,
    tanh), y0 (6, 1, 5), loss = sum of all rows times fixed random weights; once plain over 9 times and once with step_size = 0.05 on
    t = [0, 0.1, 0.3, 0.3, 0.45] (copies of either end of a step, interpolated rows, a repeated time).  The yardstick is the
    through-the-steps gradient; the solutions are equal bit for bit.  Measured on the numpy double, largest discrepancy over
    (y0, every parameter) relative to the largest gradient magnitude:
      plain      fp32 1.095e-07 (0.92 ulp)   fp64 2.754e-16 (1.24 ulp)
      step_size  fp32 1.343e-07 (1.13 ulp)   fp64 1.669e-16 (0.75 ulp)
    ADJ_MEASURED is the worse of the two runs per dtype and the bar 16 times that."""
    t_np, o = ADJOINT_RUNS[run]
    f, g = _nets(dtype, dev)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    t = torch.as_tensor(t_np.astype(_NPT[dtype]))
    params = [y0] + list(f.parameters()) + list(g.parameters())
    sol = sdeint(f, g, y0, t, solver=ReversibleHeun, options=_opts(seed=5, **o))
    W = _weights(sol)
    want = torch.autograd.grad((sol * W).sum(), params)
    adj = sdeint_adjoint(f, g, y0, t, solver=ReversibleHeun, options=_opts(seed=5, **o))
    assert torch.equal(adj, sol) and adj.requires_grad
    got = torch.autograd.grad((adj * W).sum(), params)
    worst = _relative(got, want)
    print(run, dtype, "largest discrepancy / largest gradient magnitude:", worst, "=", worst / (2 * _EPS[dtype]), "ulp")
    assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in got)
    assert worst <= ADJ_BAR[dtype], worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_sweep_equals_the_oracle_bit_for_bit(dev, dtype):
    """grad_y0 of sdeint_adjoint on the coefficients of tests/_srk_cases.py (single multiplies and adds: the vjp at yh is
    bf*LAM + bg*MU) against tests/_rheun_oracle.py's sweep on the backend's draws, a cotangent on every row: the same bits, and the
    same reconstructed y0."""
    T = _NPT[dtype]
    t_np = np.array([0.0, 0.2, 0.2, 0.5, 0.9, 1.0]).astype(T)
    y0 = _y0(dtype, dev, shape=(4, 1, 7)).requires_grad_(True)
    seed = 77
    sol = sdeint_adjoint(drift, diffusion, y0, torch.as_tensor(t_np), solver=ReversibleHeun, options=_opts(seed=seed), adjoint_params=())
    W = _weights(sol)
    (got,) = torch.autograd.grad((sol * W).sum(), [y0])
    noise = lambda k: backend_noise(tuple(y0.shape), seed, k, dtype, dev)  # noqa: E731
    states, hats = RO.rheun_walk(drift, diffusion, y0.detach().cpu().numpy(), t_np, seed, T, noise=noise, carry=True)
    cots = np.moveaxis(W.cpu().numpy().reshape(4, len(t_np), 1, 7), 1, 0)
    want, y_rec, _ = RO.adjoint_sweep(drift, diffusion, lambda t_, yh, bf, bg: bf * T(LAM) + bg * T(MU), states[-1], hats[-1], t_np, seed,
                                      T, cots, noise=noise)
    assert np.array_equal(got.cpu().numpy(), want)
    with torch.no_grad():
        xde, solution, yh_end, grid, grid_dev, plan = ADJ._solve(drift, diffusion, y0.detach(), torch.as_tensor(t_np), 1e-7, 1e-9,
                                                                 _opts(seed=seed))
        _, _, rec = ADJ._sweep(xde, (), solution, yh_end, grid, grid_dev, plan, W, tuple(y0.shape))
    assert np.array_equal(rec.cpu().numpy(), y_rec)


def test_gradcheck_through_the_adjoint(dev):
    t = torch.tensor([0.0, 0.2, 0.35, 0.6], dtype=torch.float64)

    def fn(y0, a, c, d):
        return sdeint_adjoint(lambda t_, y: y * a, lambda t_, y: y * c + d, y0, t, solver=ReversibleHeun, options=_opts(seed=4),
                              adjoint_params=(a, c, d))

    g = torch.Generator().manual_seed(5)
    inputs = [(0.5 + torch.rand(2, 1, 3, generator=g, dtype=torch.float64)).to(dev).requires_grad_(True)]
    inputs += [torch.tensor(v, dtype=torch.float64, device=dev).requires_grad_(True) for v in (-0.6, 0.4, 0.3)]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_sweep_reconstructs_y0(dev, dtype):
    """The y0 the sweep arrives at, after recomputing every state of the two runs of the adjoint test backwards, against the true y0,
    relative to max |y0|.  Measured on the numpy double:
      plain      fp32 2.421e-07 (2.03 ulp)   fp64 3.382e-16 (1.52 ulp)
      step_size  fp32 1.211e-07 (1.02 ulp)   fp64 2.255e-16 (1.02 ulp)
    RECON_MEASURED is the worse run per dtype and the bar 16 times that."""
    f, g = _nets(dtype, dev)
    y0 = _y0(dtype, dev, shape=(6, 1, 5))
    for run, (t_np, o) in ADJOINT_RUNS.items():
        t = torch.as_tensor(t_np.astype(_NPT[dtype]))
        with torch.no_grad():
            xde, solution, yh_end, grid, grid_dev, plan = ADJ._solve(f, g, y0, t, 1e-7, 1e-9, _opts(seed=5, **o))
        _, _, rec = ADJ._sweep(xde, tuple(f.parameters()) + tuple(g.parameters()), solution, yh_end, grid, grid_dev, plan,
                               _weights(solution), tuple(y0.shape))
        worst = float((rec - y0).abs().max()) / float(y0.abs().max())
        print(run, dtype, "reconstructed y0 off by", worst, "=", worst / (2 * _EPS[dtype]), "ulp of max |y0|")
        assert worst <= RECON_BAR[dtype], (run, worst)


def test_a_seedless_call_reproduces_its_path_in_the_backward(dev):
    """Without options["seed"] the forward draws one from torch's generator and the backward regenerates that path: the gradients are
    those of the through-the-steps call that drew the same seed."""
    dtype = torch.float64
    f, g = _nets(dtype, dev)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    t = torch.linspace(0.0, 1.0, 9, dtype=dtype)
    params = [y0] + list(f.parameters()) + list(g.parameters())
    torch.manual_seed(123)
    adj = sdeint_adjoint(f, g, y0, t, solver=ReversibleHeun)
    torch.manual_seed(999)  # (the backward does not draw again)
    got = torch.autograd.grad(adj[..., -1:, :].sum(), params)
    torch.manual_seed(123)
    sol = sdeint(f, g, y0, t, solver=ReversibleHeun)
    want = torch.autograd.grad(sol[..., -1:, :].sum(), params)
    assert torch.equal(adj, sol)
    assert _relative(got, want) <= ADJ_BAR[dtype]
    torch.manual_seed(124)
    assert not torch.equal(sdeint_adjoint(f, g, y0, t, solver=ReversibleHeun), sol)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_rheun_refusals(dev):
    from paddlexde_amd.functional import odeint

    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="ReversibleHeun steps SDEs only"):
        odeint(drift, y0, t, solver=ReversibleHeun)
    for call, kw in ((sdeint, {}), (sdeint_adjoint, {"adjoint_params": ()})):
        with pytest.raises(NotImplementedError, match="pipeline='graph'"):
            call(drift, diffusion, y0, t, solver=ReversibleHeun, options=_opts(pipeline="graph"), **kw)
        with pytest.raises(NotImplementedError, match="interp='cubic'"):
            call(drift, diffusion, y0, t, solver=ReversibleHeun, options=_opts(interp="cubic", step_size=0.1), **kw)
        for bad in (lambda t_, y: y[..., :1], lambda t_, y: y.float(), lambda t_, y: 0.5):
            with pytest.raises(ValueError, match="diagonal noise"):
                call(drift, bad, y0, t, solver=ReversibleHeun, **kw)
        # the evaluation at t1 is checked too: a diffusion that is well-formed only on its first call
        calls = []

        def second_call_is_bad(t_, y):
            calls.append(1)
            return y * MU if len(calls) == 1 else (y * MU).float()

        with pytest.raises(ValueError, match="diagonal noise"):
            call(drift, second_call_is_bad, y0, t, solver=ReversibleHeun, **kw)
        assert len(calls) == 2
        with pytest.raises(NotImplementedError, match="respect to t"):
            call(drift, diffusion, y0, t.clone().requires_grad_(True), solver=ReversibleHeun, **kw)
    # sdeint_adjoint: the solver check comes first and keeps its text
    for cls, text in ((Euler, r"sdeint\(\.\.\., solver=Euler\)"), (Milstein, r"sdeint\(\.\.\., solver=Euler\).*solver=Milstein"),
                      (SRK, "Brownian path that can be queried backwards"), (None, "or use solver=ReversibleHeun")):
        with pytest.raises(NotImplementedError, match=text):
            sdeint_adjoint(drift, diffusion, y0, t, solver=cls, adjoint_solver=Euler)
    with pytest.raises(ValueError, match="adjoint_params"):
        sdeint_adjoint(drift, diffusion, y0, t, solver=ReversibleHeun)
    with pytest.raises(ValueError, match="adjoint_params"):
        sdeint_adjoint(_Net().to(dev, torch.float64), diffusion, y0, t, solver=ReversibleHeun)
    for kw in ({"adjoint_solver": ReversibleHeun}, {"adjoint_rtol": 1e-3}, {"adjoint_atol": 1e-3}, {"adjoint_options": {}},
               {"event_fn": lambda t_, y: y}):
        with pytest.raises(NotImplementedError, match=next(iter(kw)) + " must be None"):
            sdeint_adjoint(drift, diffusion, y0, t, solver=ReversibleHeun, adjoint_params=(), **kw)
    with pytest.raises(NotImplementedError, match="tensor y0"):
        sdeint_adjoint(drift, diffusion, (y0, y0), t, solver=ReversibleHeun, adjoint_params=())


# ----------------------------------------------------------------------------------------------
# the kernels' reversibility (on the double from tests/test_rheun_host.py, on the GPU from tests/test_gpu_rheun.py)
# ----------------------------------------------------------------------------------------------
def reverse_after_forward(dev, dtype):
    """predict(+1), correct(+1), then the two at direction -1 on the results return (yh0, y0) up to rounding: 4099 standard-normal
    elements per operand, yh0 = y0 + 0.1 * noise, dt = 0.0123.  Measured on the numpy double, max error / max |operand|:
      fp32 1.174e-07 (0.98 ulp)   fp64 2.187e-16 (0.98 ulp)
    REVERSE_MEASURED, and the bar 16 times that."""
    be = _hip.get_backend()
    gen = torch.Generator().manual_seed(3)
    y0, e, f0, g0, f1, g1 = (torch.randn(4099, generator=gen, dtype=torch.float64).to(dev, dtype) for _ in range(6))
    yh0 = (y0 + 0.1 * e).contiguous()
    dt, seed, k = 0.0123, 21, 4
    s = float(SO.s_of(_NPT[dtype](dt), _NPT[dtype]))
    yh1, y1, yh0_back, y0_back = (torch.empty_like(y0) for _ in range(4))
    be._sde_rheun_predict(yh1, y0, yh0, f0, g0, dt, s, 1, seed, k)
    be._sde_rheun_correct(y1, y0, f0, f1, g0, g1, dt, s, 1, seed, k)
    be._sde_rheun_predict(yh0_back, y1, yh1, f1, g1, dt, s, -1, seed, k)
    be._sde_rheun_correct(y0_back, y1, f1, f0, g1, g0, dt, s, -1, seed, k)
    scale = max(float(x.abs().max()) for x in (y0, yh0, f0, g0, f1, g1))
    worst = max(float((y0_back - y0).abs().max()), float((yh0_back - yh0).abs().max())) / scale
    print(dtype, "reverse after forward off by", worst, "=", worst / (2 * _EPS[dtype]), "ulp of the largest operand")
    assert not torch.equal(y1, y0) and not torch.equal(yh1, yh0)
    assert worst <= REVERSE_BAR[dtype], worst
