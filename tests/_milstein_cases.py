"""End-to-end cases of sdeint(..., solver=Milstein), run on the numpy double (tests/test_milstein_host.py) and on the GPU
(tests/test_gpu_milstein.py) through the ``dev`` fixture of each module.  Every walk is compared with tests/_milstein_oracle.py fed the
backend's own normals (``_sde_noise``): on the double those are the oracle's, on the GPU the kernel's."""
import numpy as np
import pytest
import torch

from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler, Milstein
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from ._sde_cases import _NPT, _opts, _y0, backend_noise

# single multiplies and adds with exactly representable constants: the same bits in numpy and in torch on either device
LAM, MU, NU = -0.75, 0.5, 0.25

# test_gradients_equal_the_autograd_twin: the largest discrepancy measured on the numpy double, relative to the largest gradient
# magnitude (6.678e-17 = 0.30 * 2^-52; see its docstring); the bar is 16 times that, 1.07e-15
GRAD_MEASURED = 6.7e-17
GRAD_BAR = 16 * GRAD_MEASURED


def drift(t, y):
    return y * LAM


def diffusion(t, y):
    return y * MU + NU


def _oracle(y0, t_np, seed, dtype, dev, grid=None, f=drift, g=diffusion):
    grid = t_np if grid is None else grid
    states = MO.milstein_walk(f, g, y0.cpu().numpy(), grid, seed, _NPT[dtype],
                              noise=lambda k: backend_noise(tuple(y0.shape), seed, k, dtype, dev))
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states)


# ----------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["increasing", "decreasing", "repeated", "step_size"])
def test_milstein_walk_equals_the_oracle_bit_for_bit(dev, dtype, times):
    T = _NPT[dtype]
    t_np = {"increasing": np.array([0.0, 0.1, 0.25, 0.3, 0.7, 1.0]), "decreasing": np.array([1.0, 0.8, 0.55, 0.5, 0.0]),
            "repeated": np.array([0.0, 0.2, 0.2, 0.2, 0.5, 0.5, 0.9]),
            "step_size": np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0])}[times].astype(T)
    o, grid = {}, None
    if times == "step_size":
        o, grid = {"step_size": 0.1, "interp": "linear"}, step_size_grid(t_np, 0.1)
    y0 = _y0(dtype, dev, shape=(4, 1, 7))  # (28 elements: a tail of the fp32 vector and fp64 pair at the end)
    seed = 0x1234_5678_9ABC_DEF0
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Milstein, options=_opts(seed=seed, **o))
    got = sol.cpu().numpy()
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, _oracle(y0, t_np, seed, dtype, dev, grid=grid))
    if times == "repeated":  # a zero-length step (dt = 0, s = 0, c = 0) returns the state: exact copies, no NaN
        assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 2], got[:, 3]) and np.array_equal(got[:, 4], got[:, 5])
    # the correction is there: not the Euler-Maruyama path of the same seed
    em = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=seed, **o))
    assert not np.array_equal(got, em.cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_state_independent_diffusion_gives_the_euler_path(dev, dtype):
    """gb - g == 0 and the first three terms of the step are Euler-Maruyama's expression: the same rows, bit for bit."""
    t = torch.as_tensor(np.array([0.0, 0.1, 0.25, 0.25, 0.7, 1.0], dtype=_NPT[dtype]))
    y0 = _y0(dtype, dev, shape=(3, 2, 5))
    f = lambda t_, y: y * LAM + (y * y) * 0.125  # noqa: E731
    g = lambda t_, y: torch.ones_like(y)  # noqa: E731
    for o in ({}, {"step_size": 0.15}):
        a = sdeint(f, g, y0, t, solver=Milstein, options=_opts(seed=21, **o))
        b = sdeint(f, g, y0, t, solver=Euler, options=_opts(seed=21, **o))
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert not np.array_equal(a.cpu().numpy(), sdeint(f, g, y0, t, solver=Milstein, options=_opts(seed=22, **o)).cpu().numpy())


def test_auto_pipeline_keeps_the_eager_loop_for_milstein(dev):
    y0 = _y0(torch.float32, dev, shape=(1, 2))
    t = torch.linspace(0.0, 1.0, 40)
    with torch.no_grad():
        a = sdeint(drift, diffusion, y0, t, solver=Milstein, options=_opts(seed=3))
        b = sdeint(drift, diffusion, y0, t, solver=Milstein, options=_opts(seed=3, pipeline="sync"))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), _oracle(y0[None], t.numpy(), 3, torch.float32, dev)[0])


# ----------------------------------------------------------------------------------------------
# strong order
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
def test_strong_order_one_on_geometric_brownian_motion(dev, direction):
    """dX = lam X dt + mu X dW, X0 = 1, lam = 2, mu = 1, fp64, 2^16 paths, seed 11, h = 2^-3 .. 2^-8 on [0, 1] (and on the decreasing
    grid [0, -1]): W_T from sdeint(0, 1) with the same seed and grid, the exact solution exp(lam T - mu^2 |T| / 2 + mu W_T) with
    T = +-1; the slope of log E|X_Milstein - X| against log h lies in [0.85, 1.15], and at h = 2^-8 the error is below half of
    Euler-Maruyama's on the same paths.  The numpy statement of the scheme on the oracle's noise gives slope 0.957 (errors 2.04, 1.15,
    0.600, 0.306, 0.151, 0.0760; Euler 0.553, Euler / Milstein at h = 2^-8 3.46) on the increasing grid and 1.021 (Euler 0.674;
    3.61) on the decreasing one."""
    lam, mu, M, seed = 2.0, 1.0, 1 << 16, 11
    hs, errs = [], []
    ones = torch.ones(1, M, dtype=torch.float64, device=dev)
    o = {"norm": None, "seed": seed}
    with torch.no_grad():
        for p in range(3, 9):
            N = 2**p
            t = direction * torch.arange(N + 1, dtype=torch.float64) / N
            W = sdeint(lambda t_, y: torch.zeros_like(y), lambda t_, y: torch.ones_like(y), torch.zeros_like(ones), t, solver=Euler,
                       options=o)[-1]
            X = sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, ones, t, solver=Milstein, options=o)[-1]
            exact = torch.exp((lam * direction - 0.5 * mu * mu) * 1.0 + mu * W)
            hs.append(1.0 / N)
            errs.append(float((X - exact).abs().mean()))
        euler = float((sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, ones, t, solver=Euler, options=o)[-1] - exact).abs().mean())
    slope = float(np.polyfit(np.log(hs), np.log(errs), 1)[0])
    print("direction", direction, "slope", slope, "errors", errs, "euler at the finest h", euler)
    assert 0.85 <= slope <= 1.15, (slope, errs)
    assert errs[-1] < 0.5 * euler, (errs[-1], euler)


# ----------------------------------------------------------------------------------------------
# gradients
# ----------------------------------------------------------------------------------------------
def test_gradients_equal_the_autograd_twin(dev):
    """d(sum of the last row)/d(y0, lam, mu) through sdeint(Milstein), fp64, 8 steps, 64 paths, against the same recursion in plain
    torch ops on the same Z, differentiated by autograd: two float64 statements of one sum in different orders.  Measured on the numpy
    double: the values agree bit for bit; the largest gradient discrepancy is 6.678e-17 (0.30 * 2^-52) of the largest gradient
    magnitude, GRAD_MEASURED = 6.7e-17.  The bar is 16 times that, 1.07e-15 (the margin covers the change of summation order between
    numpy and the device)."""
    dtype, T = torch.float64, np.float64
    t_np = np.linspace(0.0, 1.0, 9)
    y0 = (0.5 + torch.rand((1, 64), generator=torch.Generator().manual_seed(7), dtype=dtype)).to(dev).requires_grad_(True)
    lam = torch.tensor(-0.6, dtype=dtype, device=dev, requires_grad=True)
    mu = torch.tensor(0.4, dtype=dtype, device=dev, requires_grad=True)
    params = [y0, lam, mu]
    sol = sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, y0, torch.as_tensor(t_np), solver=Milstein, options=_opts(seed=9))
    got = torch.autograd.grad(sol[-1:].sum(), params)
    y = y0
    for k in range(len(t_np) - 1):
        dt = T(t_np[k + 1] - t_np[k])
        s, c, a = float(SO.s_of(dt, T)), float(MO.c_of(dt, T)), float(abs(dt))
        z = torch.as_tensor(backend_noise((1, 64), 9, k, dtype, dev)).to(dev)
        f, g = lam * y, mu * y
        gb = mu * ((y + f * float(dt)) + g * s)
        w = s * z
        q = c * (w * w - a)
        y = ((y + f * float(dt)) + g * w) + (gb - g) * q
    assert torch.equal(sol[-1:].detach(), y.detach())
    want = torch.autograd.grad(y.sum(), params)
    scale = max(float(b.abs().max()) for b in want)
    worst = max(float((a_ - b).abs().max()) for a_, b in zip(got, want)) / scale
    print("largest gradient discrepancy / largest gradient magnitude:", worst, "=", worst / 2.0**-52, "* 2^-52")
    assert worst <= GRAD_BAR, worst
    assert all(float(x.abs().max()) > 0 for x in got)


def test_gradients_reach_mlp_parameters_through_the_support_point(dev):
    """The parameters of a diffusion network get gradient through both of its evaluations (at y0 and at the support point)."""
    dtype = torch.float64
    torch.manual_seed(0)
    gnet = torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Tanh(), torch.nn.Linear(8, 5)).to(dev, dtype)
    fnet = torch.nn.Linear(5, 5).to(dev, dtype)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    t = torch.tensor([0.0, 0.1, 0.3, 0.3, 0.45], dtype=dtype)
    sol = sdeint(lambda t_, y: fnet(y), lambda t_, y: gnet(y), y0, t, solver=Milstein, options=_opts(seed=5, step_size=0.05))
    params = [y0] + list(fnet.parameters()) + list(gnet.parameters())
    grads = torch.autograd.grad(sol.sum(), params)
    assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in grads)


def test_gradients_agree_with_finite_differences(dev):
    t = torch.tensor([0.0, 0.2, 0.35, 0.6], dtype=torch.float64)

    def fn(y0, a, c, d):
        return sdeint(lambda t_, y: y * a, lambda t_, y: y * c + d, y0, t, solver=Milstein, options=_opts(seed=4))

    g = torch.Generator().manual_seed(5)
    inputs = [(0.5 + torch.rand(2, 1, 3, generator=g, dtype=torch.float64)).to(dev).requires_grad_(True)]
    inputs += [torch.tensor(v, dtype=torch.float64, device=dev).requires_grad_(True) for v in (-0.6, 0.4, 0.3)]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-6)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_milstein_refusals(dev):
    from paddlexde_amd.functional import odeint, sdeint_adjoint
    from paddlexde_amd.solver import RK4, AdamsBashforthMoulton, Dopri5, Midpoint

    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="use Euler"):
        odeint(drift, y0, t, solver=Milstein)
    for cls in (Midpoint, RK4, AdamsBashforthMoulton):
        with pytest.raises(NotImplementedError, match="use Euler.*Milstein"):
            sdeint(drift, diffusion, y0, t, solver=cls)
    with pytest.raises(NotImplementedError, match="fixed-step solver.*Milstein"):
        sdeint(drift, diffusion, y0, t, solver=Dopri5)
    with pytest.raises(NotImplementedError, match="pipeline='graph'"):
        sdeint(drift, diffusion, y0, t, solver=Milstein, options=_opts(pipeline="graph"))
    with pytest.raises(NotImplementedError, match="interp='cubic'"):
        sdeint(drift, diffusion, y0, t, solver=Milstein, options=_opts(interp="cubic", step_size=0.1))
    for bad in (lambda t_, y: y[..., :1], lambda t_, y: y.float(), lambda t_, y: 0.5):
        with pytest.raises(ValueError, match="diagonal noise"):
            sdeint(drift, bad, y0, t, solver=Milstein)
    # the support evaluation is checked too: a diffusion that is well-formed only on its first call of a step
    calls = []

    def second_call_is_bad(t_, y):
        calls.append(1)
        return y * MU if len(calls) % 2 else (y * MU).float()

    with pytest.raises(ValueError, match="diagonal noise"):
        sdeint(drift, second_call_is_bad, y0, t, solver=Milstein)
    with pytest.raises(NotImplementedError, match=r"sdeint\(\.\.\., solver=Euler\).*solver=Milstein"):
        sdeint_adjoint(drift, diffusion, y0, t, solver=Milstein)
