"""End-to-end cases of sdeint, run on the numpy double (tests/test_sde_host.py) and on the GPU (tests/test_gpu_sde.py) through the
``dev`` fixture of each module.  Every walk is compared with tests/_sde_oracle.py fed the backend's own normals (``_sde_noise``): on the
double those are the oracle's, on the GPU the kernel's."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import odeint, sdeint, sdeint_adjoint
from paddlexde_amd.solver import RK4, AdamsBashforthMoulton, Dopri5, Euler, Midpoint
from paddlexde_amd.utils import _rms_norm

from . import _sde_oracle as SO

_NPT = {torch.float32: np.float32, torch.float64: np.float64}

# elementwise coefficients with exactly representable constants: the same bits in numpy and in torch on either device
A, B, C, D = -0.75, 0.125, 0.5, 0.25


def drift(t, y):
    return y * A + (y * y) * B


def diffusion(t, y):
    return y * C + D


def backend_noise(shape, seed, k, dtype, dev):
    out = torch.empty(shape, dtype=dtype, device=dev)
    _hip.get_backend()._sde_noise(out, seed, k)
    return out.cpu().numpy()


def _y0(dtype, dev, shape=(3, 2, 5), seed=0):
    return (0.5 + 0.5 * torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).to(dev, dtype)


def _opts(**kw):
    return dict({"norm": _rms_norm}, **kw)


def _oracle(y0, t_np, seed, dtype, dev, grid=None):
    grid = t_np if grid is None else grid
    T = _NPT[dtype]
    states = SO.em_walk(drift, diffusion, y0.cpu().numpy(), grid, seed, T,
                        noise=lambda k: backend_noise(tuple(y0.shape), seed, k, dtype, dev))
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states)


# ----------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------
def test_output_has_the_layout_of_odeint_with_euler(dev):
    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 7, dtype=torch.float64)
    sol = sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(seed=1))
    ref = odeint(drift, y0, t, solver=Euler)
    assert sol.shape == ref.shape == (3, 7 * 2, 5) and sol.dtype == ref.dtype and sol.device == ref.device
    assert torch.equal(sol[:, :2], y0)
    zero = sdeint(drift, lambda t_, y: torch.zeros_like(y), y0, t, solver=Euler, options=_opts(seed=1))
    assert torch.equal(zero, ref)  # (no diffusion: g * (s * Z) adds exact zeros to Euler's (y0 + f*dt))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["increasing", "decreasing", "repeated"])
def test_walk_equals_the_oracle_bit_for_bit(dev, dtype, times):
    T = _NPT[dtype]
    t_np = {"increasing": np.array([0.0, 0.1, 0.25, 0.3, 0.7, 1.0]), "decreasing": np.array([1.0, 0.8, 0.55, 0.5, 0.0]),
            "repeated": np.array([0.0, 0.2, 0.2, 0.2, 0.5, 0.5, 0.9])}[times].astype(T)
    y0 = _y0(dtype, dev, shape=(4, 1, 7))  # (28 elements: a tail of the fp32 vector and fp64 pair at the end)
    seed = 0x1234_5678_9ABC_DEF0
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=seed))
    ref = _oracle(y0, t_np, seed, dtype, dev)
    assert np.array_equal(sol.cpu().numpy(), ref)
    if times == "repeated":
        s = sol.cpu().numpy()  # a zero-length step leaves the state unchanged (dt = 0, dW = 0) ...
        assert np.array_equal(s[:, 1], s[:, 2]) and np.array_equal(s[:, 2], s[:, 3]) and np.array_equal(s[:, 4], s[:, 5])
        # ... and still advances k: the step 0.2 -> 0.5 is grid step 3, not 1
        y2 = s[:, 3:4]
        z1 = backend_noise((4, 1, 7), seed, 1, dtype, dev)
        wrong = SO.em_step(y2, drift(0, y2), diffusion(0, y2), T(0.5) - T(0.2), z1, T)
        assert np.array_equal(s[:, 4:5], SO.em_step(y2, drift(0, y2), diffusion(0, y2), T(0.5) - T(0.2),
                                                    backend_noise((4, 1, 7), seed, 3, dtype, dev), T))
        assert not np.array_equal(s[:, 4:5], wrong)


def test_the_seed_fixes_the_path(dev):
    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    run = lambda **o: sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(**o))  # noqa: E731
    a, b, c = run(seed=5), run(seed=5), run(seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(run(seed=5 + (1 << 32)), a)  # (the seed's high word is the key's second word)
    torch.manual_seed(123)
    d1, d2 = run(), run()
    torch.manual_seed(123)
    e1, e2 = run(), run()
    assert torch.equal(d1, e1) and torch.equal(d2, e2) and not torch.equal(d1, d2)
    opts = _opts(seed=5)
    sdeint(drift, diffusion, y0, t, solver=Euler, options=opts)
    assert opts == _opts(seed=5)  # (the caller's dict is not consumed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("option", ["step_size", "grid_constructor", "step_size_decreasing"])
def test_substep_rows_equal_the_oracle(dev, dtype, option):
    T = _NPT[dtype]
    t_np = np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0], dtype=T)
    grid = np.array([0.0, 0.1, 0.2, 0.4, 0.5, 0.6, 0.8, 1.0], dtype=T)
    if option == "step_size":
        o = {"step_size": 0.1}
        from paddlexde_amd.solver.base_fixed_solver import step_size_grid

        grid = step_size_grid(t_np, 0.1)
    elif option == "step_size_decreasing":
        t_np = t_np[::-1].copy()
        o = {"step_size": 0.15}
        from paddlexde_amd.solver.base_fixed_solver import step_size_grid

        grid = step_size_grid(t_np, 0.15)
    else:
        o = {"grid_constructor": lambda y0, t: torch.as_tensor(grid)}
    y0 = _y0(dtype, dev, shape=(2, 3, 3))
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=77, **o))
    assert np.array_equal(sol.cpu().numpy(), _oracle(y0, t_np, 77, dtype, dev, grid=grid))


# ----------------------------------------------------------------------------------------------
# gradients
# ----------------------------------------------------------------------------------------------
class _Mlp(torch.nn.Module):
    def __init__(self, d, last=None, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.net = torch.nn.Sequential(torch.nn.Linear(d, 16), torch.nn.Tanh(), torch.nn.Linear(16, d))
        self.last = last

    def forward(self, t, y):
        h = self.net(y)
        return self.last(h) if self.last is not None else h


def _twin(f, g, y0, t_np, seed, dtype, dev):
    """The walk in torch ops, fed the backend's Z: what autograd differentiates without the kernels."""
    T = _NPT[dtype]
    y, out = y0, [y0]
    for k in range(len(t_np) - 1):
        dt = T(t_np[k + 1] - t_np[k])
        zs = torch.as_tensor(SO.s_of(dt, T) * backend_noise(tuple(y0.shape), seed, k, dtype, dev)).to(dev)
        y = (y + f(None, y) * float(dt)) + g(None, y) * zs
        out.append(y)
    return torch.cat(out, dim=-2)


def test_gradients_equal_the_autograd_twin(dev):
    dtype = torch.float64
    t_np = np.array([0.0, 0.1, 0.3, 0.3, 0.45, 0.7])
    f = _Mlp(5, seed=1).to(dev, dtype)
    g = _Mlp(5, last=torch.sigmoid, seed=2).to(dev, dtype)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    w = torch.randn(6, len(t_np), 5, generator=torch.Generator().manual_seed(3), dtype=dtype).to(dev)
    params = [y0] + list(f.parameters()) + list(g.parameters())
    sol = sdeint(f, g, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=9))
    got = torch.autograd.grad((sol * w).sum(), params)
    ref_sol = _twin(f, g, y0, t_np, 9, dtype, dev)
    assert torch.equal(sol.detach(), ref_sol.detach())
    want = torch.autograd.grad((ref_sol * w).sum(), params)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), float((a - b).abs().max())
    assert all(float(x.abs().max()) > 0 for x in got)


def test_gradients_agree_with_finite_differences(dev):
    t = torch.tensor([0.0, 0.2, 0.35, 0.6], dtype=torch.float64)

    def fn(y0, a, b, c, d):
        return sdeint(lambda t_, y: y * a + (y * y) * b, lambda t_, y: y * c + d, y0, t, solver=Euler, options=_opts(seed=4))

    g = torch.Generator().manual_seed(5)
    inputs = [(0.5 + torch.rand(2, 1, 3, generator=g, dtype=torch.float64)).to(dev).requires_grad_(True)]
    inputs += [torch.tensor(v, dtype=torch.float64, device=dev).requires_grad_(True) for v in (-0.6, 0.2, 0.4, 0.3)]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-6)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_refusals(dev):
    y0 = _y0(torch.float64, dev)
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="tuple"):
        sdeint(drift, diffusion, (y0, y0), t, solver=Euler)
    with pytest.raises(NotImplementedError, match="fixed-step solver"):
        sdeint(drift, diffusion, y0, t, solver=Dopri5)
    for cls in (Midpoint, RK4, AdamsBashforthMoulton):
        with pytest.raises(NotImplementedError, match="use Euler"):
            sdeint(drift, diffusion, y0, t, solver=cls)
    with pytest.raises(NotImplementedError, match="pipeline='graph'"):
        sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(pipeline="graph"))
    with pytest.raises(NotImplementedError, match="interp='cubic'"):
        sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(interp="cubic", step_size=0.1))
    for bad in (lambda t_, y: y[..., :1], lambda t_, y: y.float(), lambda t_, y: 0.5):
        with pytest.raises(ValueError, match="diagonal noise"):
            sdeint(drift, bad, y0, t, solver=Euler)
    with pytest.raises(NotImplementedError, match="respect to t"):
        sdeint(drift, diffusion, y0, t.clone().requires_grad_(True), solver=Euler)
    for seed in (-1, 1 << 64, 0.5, True):
        with pytest.raises((ValueError, TypeError), match="seed"):
            sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(seed=seed))
    with pytest.raises(NotImplementedError, match=r"sdeint\(\.\.\., solver=Euler\)"):
        sdeint_adjoint(drift, diffusion, y0, t, solver=Euler)


def test_auto_pipeline_keeps_the_eager_loop(dev):
    """pipeline="auto" would capture a long run of small steps; an SDE step cannot be replayed (k must advance), so it stays eager and
    gives the "sync" bits."""
    y0 = _y0(torch.float32, dev, shape=(1, 2))
    t = torch.linspace(0.0, 1.0, 40)
    with torch.no_grad():
        a = sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(seed=3))
        b = sdeint(drift, diffusion, y0, t, solver=Euler, options=_opts(seed=3, pipeline="sync"))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), _oracle(y0[None], t.numpy(), 3, torch.float32, dev)[0])
