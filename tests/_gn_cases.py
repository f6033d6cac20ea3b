"""End-to-end cases of ``sdeint(..., solver=Euler, options={"noise_type": "general" | "scalar"})``, run on the numpy double
(tests/test_gn_host.py) and on the GPU (tests/test_gpu_gn.py) through the ``dev`` fixture of each module.  The references are
tests/_gn_oracle.py fed the backend's own normals (``_sde_noise`` on a ``[..., M]`` buffer: on the double the oracle's, on the GPU the
kernel's), the diagonal call on the same seed, and the same recursion written in framework ops."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _gn_oracle as GN
from . import _sde_cases as SC
from . import _sde_oracle as SO
from ._sde_cases import _NPT, _opts, _y0, backend_noise

# the gradients of tests/test_gradients_equal_the_framework_recursion, relative to the largest gradient magnitude of each leaf, measured
# on the numpy double (the test prints its figure): 4.378e-16, the worse of the two noise types over the seven leaves (general:
# 2.738e-16, scalar: 4.378e-16); the bar on both backends is 16 times that, 7.005e-15 (DESIGN sections 10 and 16)
GRAD_MEASURED_ON_THE_DOUBLE = 4.378e-16
GRAD_BAR = 16 * GRAD_MEASURED_ON_THE_DOUBLE


def _tables(D, M):
    """Two [D, M] tables of exactly representable constants (multiples of 1/16 in [-1, 1]): the same bits in numpy and in torch."""
    i = np.arange(D * M).reshape(D, M)
    return ((i * 7) % 17 - 8) / 16.0, ((i * 5) % 13 - 6) / 16.0


class Coeffs:
    """Coefficients that are single multiplies and adds: ``drift`` of tests/_sde_cases.py and the diffusion
    ``g[.., d, m] = y[.., d]*P[d, m] + Q[d, m]``, as torch functions on ``dev`` and as numpy functions on the same bits."""

    def __init__(self, D, M, dtype, dev):
        self.M = M
        p, q = _tables(D, M)
        self.p_np, self.q_np = p.astype(_NPT[dtype]), q.astype(_NPT[dtype])
        self.p, self.q = torch.as_tensor(self.p_np).to(dev), torch.as_tensor(self.q_np).to(dev)

    def diffusion(self, t, y):
        return y.unsqueeze(-1) * self.p + self.q

    def diffusion_np(self, t, y):
        return y[..., None] * self.p_np + self.q_np


def gn_noise(state_shape, M, seed, k, dtype, dev):
    """The backend's normals of a state of ``state_shape`` under an M-dimensional Brownian motion: ``[..., M]``, numpy."""
    return backend_noise(GN.noise_shape(state_shape, M), seed, k, dtype, dev)


def _oracle(co, y0, t_np, seed, dtype, dev, grid=None):
    grid = t_np if grid is None else grid
    states = GN.gn_walk(SC.drift, co.diffusion_np, y0.cpu().numpy(), grid, _NPT[dtype],
                        lambda k: gn_noise(tuple(y0.shape), co.M, seed, k, dtype, dev))
    return SO.layout(SO.rows_at(states, grid, t_np) if grid is not t_np else states)


TIMES = {"increasing": [0.0, 0.1, 0.25, 0.3, 0.7, 1.0], "decreasing": [1.0, 0.8, 0.55, 0.5, 0.0],
         "repeated": [0.0, 0.2, 0.2, 0.2, 0.5, 0.5, 0.9]}


# ----------------------------------------------------------------------------------------------
# the walk
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("times", ["increasing", "decreasing", "repeated", "step_size"])
@pytest.mark.parametrize("noise_type, M", [("general", 3), ("scalar", 1)])
def test_walk_equals_the_oracle_bit_for_bit(dev, dtype, times, noise_type, M):
    T = _NPT[dtype]
    o, grid = {}, None
    if times == "step_size":
        t_np = np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0], dtype=T)
        o, grid = {"step_size": 0.1, "interp": "linear"}, step_size_grid(t_np, 0.1)
    else:
        t_np = np.array(TIMES[times]).astype(T)
    y0 = _y0(dtype, dev, shape=(4, 1, 7))
    co = Coeffs(7, M, dtype, dev)
    seed = 0x1234_5678_9ABC_DEF0
    sol = sdeint(SC.drift, co.diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=seed, noise_type=noise_type, **o))
    assert sol.shape == (4, len(t_np), 7) and sol.dtype == dtype
    assert np.array_equal(sol.cpu().numpy(), _oracle(co, y0, t_np, seed, dtype, dev, grid=grid))
    if times == "repeated":  # a zero-length step leaves the state unchanged and still advances k
        s = sol.cpu().numpy()
        assert np.array_equal(s[:, 1], s[:, 2]) and np.array_equal(s[:, 4], s[:, 5]) and not np.array_equal(s[:, 3], s[:, 4])


def test_general_noise_that_embeds_a_diagonal_is_the_diagonal_call(dev):
    """M == D and ``g[.., d, m] = (d == m) * b[.., d]``: the flat ``[rows, M]`` normals are the state's, the other terms of the sum are
    zeros, so the path is the diagonal call's on the same seed."""
    t = torch.linspace(0.0, 1.0, 6, dtype=torch.float64)
    for dtype in (torch.float32, torch.float64):
        y0 = _y0(dtype, dev, shape=(3, 2, 5))
        with torch.no_grad():
            diag = sdeint(SC.drift, SC.diffusion, y0, t, solver=Euler, options=_opts(seed=21))
            full = sdeint(SC.drift, lambda t_, y: torch.diag_embed(SC.diffusion(t_, y)), y0, t, solver=Euler,
                          options=_opts(seed=21, noise_type="general"))
        assert torch.equal(full, diag)


def test_diagonal_and_absent_noise_type_give_the_parents_tensor(dev):
    for dtype in (torch.float32, torch.float64):
        T = _NPT[dtype]
        t_np = np.array(TIMES["increasing"]).astype(T)
        y0 = _y0(dtype, dev, shape=(4, 1, 7))
        with torch.no_grad():
            absent = sdeint(SC.drift, SC.diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=33))
            diagonal = sdeint(SC.drift, SC.diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=33, noise_type="diagonal"))
        assert torch.equal(absent, diagonal)
        assert np.array_equal(absent.cpu().numpy(), SC._oracle(y0, t_np, 33, dtype, dev))


# ----------------------------------------------------------------------------------------------
# gradients against the same recursion in framework ops
# ----------------------------------------------------------------------------------------------
class _Net:
    """A drift ``tanh(y A + a) B`` and a general diffusion ``sigmoid(y C + c)`` reshaped to ``[.., D, M]`` plus a scalar offset."""

    def __init__(self, D, M, dtype, dev):
        g = torch.Generator().manual_seed(17)
        mk = lambda *s: (0.5 * torch.randn(*s, generator=g, dtype=torch.float64)).to(dev, dtype).requires_grad_(True)  # noqa: E731
        self.D, self.M = D, M
        self.fp = [mk(D, 8), mk(8), mk(8, D)]
        self.gp = [mk(D, D * M), mk(D * M), mk(())]

    def drift(self, t, y):
        A, a, B = self.fp
        return torch.tanh(y @ A + a) @ B

    def diffusion(self, t, y):
        C, c, off = self.gp
        return torch.sigmoid(y @ C + c).reshape(y.shape + (self.M,)) * 0.5 + off

    def params(self):
        return self.fp + self.gp


def _twin(net, y0, t_np, seed, dtype, dev):
    """The recursion in framework ops on the backend's normals (``BaseSDE.fuse``'s general statement), in sdeint's layout."""
    T = _NPT[dtype]
    y, out = y0, [y0]
    for k in range(len(t_np) - 1):
        dt = T(t_np[k + 1] - t_np[k])
        w = torch.as_tensor(SO.s_of(dt, T) * gn_noise(tuple(y0.shape), net.M, seed, k, dtype, dev)).to(dev)
        f, g = net.drift(None, y), net.diffusion(None, y)
        a = g[..., 0] * w[..., 0:1]
        for m in range(1, net.M):
            a = a + g[..., m] * w[..., m : m + 1]
        y = (y + f * float(dt)) + a
        out.append(y)
    return torch.cat(out, dim=-2)


@pytest.mark.parametrize("noise_type, M", [("general", 3), ("scalar", 1)])
def test_gradients_equal_the_framework_recursion(dev, noise_type, M):
    """fp64, ``y0`` 6 x 1 x 5, five steps (one of zero length): the gradients of a weighted sum of the path (fixed random weights) with
    respect to ``y0`` and every parameter of drift and diffusion against the same recursion in framework ops on the same normals.  The
    bar is 16 times the discrepancy measured on the numpy double (GRAD_BAR above), relative to each leaf's largest gradient."""
    dtype = torch.float64
    t_np = np.array([0.0, 0.1, 0.3, 0.3, 0.45, 0.7])
    net = _Net(5, M, dtype, dev)
    y0 = _y0(dtype, dev, shape=(6, 1, 5)).requires_grad_(True)
    w = torch.randn(6, len(t_np), 5, generator=torch.Generator().manual_seed(3), dtype=dtype).to(dev)
    leaves = [y0] + net.params()
    sol = sdeint(net.drift, net.diffusion, y0, torch.as_tensor(t_np), solver=Euler, options=_opts(seed=9, noise_type=noise_type))
    got = torch.autograd.grad((sol * w).sum(), leaves)
    ref_sol = _twin(net, y0, t_np, 9, dtype, dev)
    assert torch.equal(sol.detach(), ref_sol.detach())
    want = torch.autograd.grad((ref_sol * w).sum(), leaves)
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
    print("gradients[{}]: product against the framework recursion {:.3e}, bar {:.3e}".format(noise_type, worst, GRAD_BAR))
    assert all(float(b.abs().max()) > 0 for b in want)  # (every leaf is reached)
    assert worst <= GRAD_BAR, (worst, GRAD_BAR)


def test_an_unwanted_cotangent_is_not_computed(dev):
    """Only the diffusion's parameters take a gradient: the backward launches still run (one per step) and the drift's and y0's
    gradients stay absent."""
    dtype = torch.float64
    net = _Net(5, 2, dtype, dev)
    for p in net.fp:
        p.requires_grad_(False)
    y0 = _y0(dtype, dev, shape=(2, 1, 5))
    sol = sdeint(net.drift, net.diffusion, y0, torch.linspace(0.0, 1.0, 4, dtype=dtype), solver=Euler, options=_opts(seed=2, noise_type="general"))
    grads = torch.autograd.grad(sol.sum(), net.gp)
    assert all(float(g.abs().max()) > 0 for g in grads)
    assert not y0.requires_grad and _hip.get_backend() is not None
