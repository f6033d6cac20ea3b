"""End-to-end cases of sdeint(..., solver=SRK), run on the numpy double (tests/test_srk_host.py) and on the GPU (tests/test_gpu_srk.py)
through the ``dev`` fixture of each module.  Every walk is compared with tests/_srk_oracle.py fed the backend's own draws
(``_sde_noise(..., draw=0 / 1)``): on the double those are the oracle's, on the GPU the kernel's."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import SRK, Euler, Milstein
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from . import _srk_oracle as KO
from ._sde_cases import _NPT, _opts, _y0

# single multiplies and adds with exactly representable constants: the same bits in numpy and in torch on either device.  Both
# coefficients take t, so a wrong stage time changes the bits.
LAM, MU, NU, TAU = -0.75, 0.5, 0.25, 0.125

# test_gradients_equal_the_autograd_twin: the largest discrepancy measured on the numpy double, relative to the largest gradient
# magnitude (4.708e-17 = 0.21 * 2^-52; see its docstring); the bar is 16 times that, 7.53e-16
GRAD_MEASURED = 4.708e-17
GRAD_BAR = 16 * GRAD_MEASURED


def drift(t, y):
    return y * LAM + t * TAU


def diffusion(t, y):
    return (y * MU + NU) + t * TAU


def backend_draw(shape, seed, k, dtype, dev, draw):
    out = torch.empty(shape, dtype=dtype, device=dev)
    _hip.get_backend()._sde_noise(out, seed, k, draw=draw)
    return out.cpu().numpy()


def _oracle(y0, t_np, seed, dtype, dev, grid=None, f=drift, g=diffusion):
    grid = t_np if grid is None else grid
    states = KO.srk_walk(f, g, y0.cpu().numpy(), grid, seed, _NPT[dtype],
                         noise=lambda k, draw: backend_draw(tuple(y0.shape), seed, k, dtype, dev, draw))
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states)


# ----------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["increasing", "decreasing", "repeated", "step_size"])
def test_srk_walk_equals_the_oracle_bit_for_bit(dev, dtype, times):
    T = _NPT[dtype]
    t_np = {"increasing": np.array([0.0, 0.1, 0.25, 0.3, 0.7, 1.0]), "decreasing": np.array([1.0, 0.8, 0.55, 0.5, 0.0]),
            "repeated": np.array([0.0, 0.2, 0.2, 0.2, 0.5, 0.5, 0.9]),
            "step_size": np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0])}[times].astype(T)
    o, grid = {}, None
    if times == "step_size":
        o, grid = {"step_size": 0.1, "interp": "linear"}, step_size_grid(t_np, 0.1)
    y0 = _y0(dtype, dev, shape=(4, 1, 7))  # (28 elements: a tail of the fp32 vector and fp64 pair at the end)
    seed = 0x1234_5678_9ABC_DEF0
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=SRK, options=_opts(seed=seed, **o))
    got = sol.cpu().numpy()
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, _oracle(y0, t_np, seed, dtype, dev, grid=grid))
    if times == "repeated":  # a zero-length step (dt = 0, s = c = c3 = 0) returns the state: exact copies, no NaN
        assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 2], got[:, 3]) and np.array_equal(got[:, 4], got[:, 5])
    # not the Milstein path of the same seed
    mil = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Milstein, options=_opts(seed=seed, **o))
    assert not np.array_equal(got, mil.cpu().numpy())


def test_auto_pipeline_keeps_the_eager_loop_for_srk(dev):
    y0 = _y0(torch.float32, dev, shape=(1, 2))
    t = torch.linspace(0.0, 1.0, 40)
    with torch.no_grad():
        a = sdeint(drift, diffusion, y0, t, solver=SRK, options=_opts(seed=3))
        b = sdeint(drift, diffusion, y0, t, solver=SRK, options=_opts(seed=3, pipeline="sync"))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), _oracle(y0[None], t.numpy(), 3, torch.float32, dev)[0])


# ----------------------------------------------------------------------------------------------
# strong order
# ----------------------------------------------------------------------------------------------
def _gbm(lam, mu, direction):
    return (lambda t_, y: lam * y, lambda t_, y: mu * y, 1.0,
            lambda W: torch.exp((lam * direction - 0.5 * mu * mu) * 1.0 + mu * W))


def _arctan():
    x0 = 0.3

    def f(t_, y):
        c = torch.cos(y)
        return -torch.sin(y) * c * c * c

    def g(t_, y):
        c = torch.cos(y)
        return c * c

    return f, g, x0, lambda W: torch.atan(W + float(np.tan(x0)))


@pytest.mark.parametrize("case", ["gbm_increasing", "gbm_decreasing", "arctan"])
def test_strong_order_one_and_a_half(dev, case):
    """fp64, 2^16 paths, seed 11, h = 2^-3 .. 2^-8 on [0, 1] (gbm_decreasing: on [0, -1]); W_T from sdeint(0, 1, Euler) with the same
    seed and grid.  gbm: dX = 2 X dt + X dW, X0 = 1, exact exp(2 T - |T| / 2 + W_T); arctan: dX = -sin X cos^3 X dt + cos^2 X dW,
    X0 = 0.3, exact arctan(W_T + tan X0).  The slope of log E|X_SRK - X| against log h lies in [1.25, 1.75], and at h = 2^-8 the error
    is below a quarter of Milstein's on the same paths.  The numpy double on the oracle's Philox noise gives
      gbm_increasing  slope 1.434  (errors 3.68e-1, 1.43e-1, 5.47e-2, 2.02e-2, 7.17e-3, 2.58e-3; Milstein 7.60e-2, Milstein / SRK 29.4)
      gbm_decreasing  slope 1.555  (errors 1.04e-2, 3.50e-3, 1.18e-3, 4.01e-4, 1.36e-4, 4.79e-5; Milstein 1.37e-3, ratio 28.6)
      arctan          slope 1.469  (errors 2.31e-2, 8.46e-3, 3.09e-3, 1.12e-3, 3.99e-4, 1.42e-4; Milstein 1.55e-3, ratio 10.9)
    (each inside [1.35, 1.65] with a ratio above 8, the range the statement of the scheme itself was held to before any GPU run)."""
    direction = -1 if case == "gbm_decreasing" else 1
    f, g, x0, exact_of = _arctan() if case == "arctan" else _gbm(2.0, 1.0, direction)
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
            X = sdeint(f, g, start, t, solver=SRK, options=o)[-1]
            exact = exact_of(W)
            hs.append(1.0 / N)
            errs.append(float((X - exact).abs().mean()))
        milstein = float((sdeint(f, g, start, t, solver=Milstein, options=o)[-1] - exact).abs().mean())
    slope = float(np.polyfit(np.log(hs), np.log(errs), 1)[0])
    print(case, "slope", slope, "errors", errs, "milstein at the finest h", milstein, "ratio", milstein / errs[-1])
    assert 1.25 <= slope <= 1.75, (slope, errs)
    assert errs[-1] < 0.25 * milstein, (errs[-1], milstein)


# ----------------------------------------------------------------------------------------------
# gradients
# ----------------------------------------------------------------------------------------------
def test_gradients_equal_the_autograd_twin(dev):
    """d(sum of the last row)/d(y0, lam, mu) through sdeint(SRK), fp64, 8 steps, 64 paths, against the same recursion in plain torch
    ops on the same Z and V, differentiated by autograd: two float64 statements of one sum in different orders.  Measured on the numpy
    double: the values agree bit for bit; the largest gradient discrepancy is 4.708e-17 (0.21 * 2^-52) of the largest gradient
    magnitude, GRAD_MEASURED.  The bar is 16 times that, 7.53e-16 (the margin covers the change of summation order between
    numpy and the device)."""
    dtype, T = torch.float64, np.float64
    t_np = np.linspace(0.0, 1.0, 9)
    y0 = (0.5 + torch.rand((1, 64), generator=torch.Generator().manual_seed(7), dtype=dtype)).to(dev).requires_grad_(True)
    lam = torch.tensor(-0.6, dtype=dtype, device=dev, requires_grad=True)
    mu = torch.tensor(0.4, dtype=dtype, device=dev, requires_grad=True)
    params = [y0, lam, mu]
    sol = sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, y0, torch.as_tensor(t_np), solver=SRK, options=_opts(seed=9))
    got = torch.autograd.grad(sol[-1:].sum(), params)
    r3, third, two3, four3, five3 = (float(x) for x in KO.consts(T))
    y = y0
    for k in range(len(t_np) - 1):
        dt = T(t_np[k + 1] - t_np[k])
        s, c, c3, a, h = float(SO.s_of(dt, T)), float(MO.c_of(dt, T)), float(KO.c3_of(dt, T)), float(abs(dt)), float(dt)
        z, v = (torch.as_tensor(backend_draw((1, 64), 9, k, dtype, dev, d)).to(dev) for d in (0, 1))
        w = s * z
        p = 0.5 * (w + (s * v) * r3)
        q = c * (w * w - a)
        u = c3 * ((w * w - 3.0 * a) * w)
        e1, e2 = ((-w - q) + 2.0 * p) - 2.0 * u, four3 * ((w + q) - p) + five3 * u
        e3, e4 = two3 * ((w - p) - u) - third * q, u
        a1, b1 = lam * y, mu * y
        a2 = lam * ((y + a1 * (0.75 * h)) + b1 * (1.5 * p))
        b2 = mu * ((y + a1 * (0.25 * h)) + b1 * (0.5 * s))
        b3 = mu * ((y + a1 * h) - b1 * s)
        b4 = mu * ((y + a1 * (0.25 * h)) + ((b1 * -5.0 + b2 * 3.0) + b3 * 0.5) * s)
        y = ((((y + (third * a1 + two3 * a2) * h) + b1 * e1) + b2 * e2) + b3 * e3) + b4 * e4
    assert torch.equal(sol[-1:].detach(), y.detach())
    want = torch.autograd.grad(y.sum(), params)
    scale = max(float(b.abs().max()) for b in want)
    worst = max(float((a_ - b).abs().max()) for a_, b in zip(got, want)) / scale
    print("largest gradient discrepancy / largest gradient magnitude:", worst, "=", worst / 2.0**-52, "* 2^-52")
    assert worst <= GRAD_BAR, worst
    assert all(float(x.abs().max()) > 0 for x in got)


def test_gradients_reach_mlp_parameters_through_every_stage(dev):
    """The parameters of a drift network and of a diffusion network get finite non-zero gradient under step_size sub-stepping."""
    dtype = torch.float64
    torch.manual_seed(0)
    gnet = torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Tanh(), torch.nn.Linear(8, 5)).to(dev, dtype)
    fnet = torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Tanh(), torch.nn.Linear(8, 5)).to(dev, dtype)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    t = torch.tensor([0.0, 0.1, 0.3, 0.3, 0.45], dtype=dtype)
    sol = sdeint(lambda t_, y: fnet(y), lambda t_, y: gnet(y), y0, t, solver=SRK, options=_opts(seed=5, step_size=0.05))
    params = [y0] + list(fnet.parameters()) + list(gnet.parameters())
    grads = torch.autograd.grad(sol.sum(), params)
    assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in grads)


def test_gradients_agree_with_finite_differences(dev):
    t = torch.tensor([0.0, 0.2, 0.35, 0.6], dtype=torch.float64)

    def fn(y0, a, c, d):
        return sdeint(lambda t_, y: y * a, lambda t_, y: y * c + d, y0, t, solver=SRK, options=_opts(seed=4))

    g = torch.Generator().manual_seed(5)
    inputs = [(0.5 + torch.rand(2, 1, 3, generator=g, dtype=torch.float64)).to(dev).requires_grad_(True)]
    inputs += [torch.tensor(v, dtype=torch.float64, device=dev).requires_grad_(True) for v in (-0.6, 0.4, 0.3)]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-6)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_srk_refusals(dev):
    from paddlexde_amd.functional import odeint

    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="SRK steps SDEs only"):
        odeint(drift, y0, t, solver=SRK)
    with pytest.raises(NotImplementedError, match="pipeline='graph'"):
        sdeint(drift, diffusion, y0, t, solver=SRK, options=_opts(pipeline="graph"))
    with pytest.raises(NotImplementedError, match="interp='cubic'"):
        sdeint(drift, diffusion, y0, t, solver=SRK, options=_opts(interp="cubic", step_size=0.1))
    for bad in (lambda t_, y: y[..., :1], lambda t_, y: y.float(), lambda t_, y: 0.5):
        with pytest.raises(ValueError, match="diagonal noise"):
            sdeint(drift, bad, y0, t, solver=SRK)
    # each of the four evaluations of a step is checked: a diffusion that is well-formed except on its i-th call
    for i in range(4):
        calls = []

        def bad_on_call_i(t_, y):
            calls.append(1)
            return (y * MU).float() if len(calls) == i + 1 else y * MU

        with pytest.raises(ValueError, match="diagonal noise"):
            sdeint(drift, bad_on_call_i, y0, t, solver=SRK)
        assert len(calls) == i + 1
