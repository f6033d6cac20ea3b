"""General and scalar noise without a GPU: the C ABI of include/xde_hip_gn.h (every call below is refused on the host before anything
is enqueued, or has nothing to do), the bind, the double against the oracle, the end-to-end cases of tests/_gn_cases.py on the numpy
double, the launches of a walk, gradcheck, and what sdeint refuses."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint, sdeint_adjoint
from paddlexde_amd.solver import SRK, Euler, Milstein, ReversibleHeun
from paddlexde_amd.solver._autograd import SdeGnEulerFn
from paddlexde_amd.xde.base_sde import BaseSDE

from . import _gn_oracle as GN
from . import _sde_cases as SC
from . import _sde_oracle as SO
from ._gn_cases import *  # noqa: F401,F403
from ._gn_cases import Coeffs, _Net
from ._sde_cases import _opts, _y0


@pytest.fixture
def dev():
    from ._gn_double import GnDoubleBackend

    _hip._set_backend_for_testing(GnDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_gn.h
# ----------------------------------------------------------------------------------------------
def test_the_gn_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("gn" in m.split("_") or "sde" in m for m in pub)
    for m in ("_sde_gn_step", "_sde_gn_backward"):
        assert callable(getattr(_hip.HipBackend, m))


def test_gn_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    Y1, Y0, F, G, GG = (0x100000 * (i + 1) for i in range(5))  # (never dereferenced: every call is refused first)

    def step(y1=Y1, y0=Y0, f=F, g=G, rows=2, D=4, M=3, k=0, dtype=0):
        return lib.xde_sde_gn_step(y1, y0, f, g, rows, D, M, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    def bwd(gf=Y1, gg=GG, gy=Y0, rows=2, D=4, M=3, k=0, dtype=0):
        return lib.xde_sde_gn_backward(gf, gg, gy, rows, D, M, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    n = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32); g holds 3 times as many
    shape = [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3), dict(M=0), dict(M=-1), dict(D=(1 << 30) + 1), dict(M=(1 << 30) + 1),
             dict(rows=1 << 40, D=1 << 9), dict(rows=1 << 20, D=1 << 20, M=1 << 9),  # the product past 2^48
             dict(k=-1), dict(k=1 << 32), dict(dtype=2), dict(dtype=-1)]
    cases = [(step, "xde_sde_gn_step", [dict(y1=None), dict(y0=None), dict(f=None), dict(g=None)] + shape + [
        dict(f=F + 2), dict(g=G + 4, dtype=1), dict(y1=Y1 + 1),  # alignment to the element type
        dict(y1=F), dict(y1=G + 3 * n - 4), dict(y1=G - n + 4), dict(y1=Y0 + 4), dict(y1=Y0 - 4), dict(y1=F - 4)]),  # an output over another operand
             (bwd, "xde_sde_gn_backward", [dict(gy=None)] + shape + [
                 dict(gf=Y1 + 2), dict(gg=GG + 4, dtype=1), dict(gy=Y0 + 1),
                 dict(gf=Y0), dict(gg=Y0 - 3 * n + 4), dict(gg=Y0 + n - 4), dict(gf=GG + 3 * n - 4), dict(gf=Y0 + 4)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)
    assert bwd(gf=None, gg=None)[0] == _hip.XDE_OK  # no output wanted: nothing to do
    assert bwd(gf=None, gg=None, rows=0)[0] == _hip.XDE_EBADARG  # (after the checks)


# ----------------------------------------------------------------------------------------------
# the double states the header
# ----------------------------------------------------------------------------------------------
def test_the_double_states_the_header(dev):
    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        gen = torch.Generator().manual_seed(3)
        y0, f, gy = (torch.randn(3, 2, 7, generator=gen, dtype=dtype) for _ in range(3))
        g = torch.randn(3, 2, 7, 5, generator=gen, dtype=dtype)
        dt = T(-0.0123)
        s = SO.s_of(dt, T)
        z = SO.normals(3 * 2 * 5, 5, 17, T).astype(T).reshape(3, 2, 5)  # the flat [rows, M] array
        y1 = torch.empty_like(y0)
        be._sde_gn_step(y1, y0, f, g, float(dt), float(s), 5, 17)
        w = s * z
        a = g.numpy()[..., 0] * w[..., None, 0]
        for m in range(1, 5):
            a = a + g.numpy()[..., m] * w[..., None, m]
        assert a.dtype == T and np.array_equal(y1.numpy(), (y0.numpy() + f.numpy() * dt) + a)
        assert np.allclose(y1.numpy(), y0.numpy() + f.numpy() * dt + np.einsum("...dm,...m->...d", g.numpy(), w), rtol=1e-4, atol=1e-5)
        gf, gg = torch.empty_like(gy), torch.empty_like(g)
        be._sde_gn_backward(gf, gg, gy, 5, float(dt), float(s), 5, 17)
        assert np.array_equal(gf.numpy(), gy.numpy() * dt) and np.array_equal(gg.numpy(), gy.numpy()[..., None] * w[..., None, :])
        only = torch.full_like(g, 7.0)
        be._sde_gn_backward(None, only, gy, 5, float(dt), float(s), 5, 17)
        assert torch.equal(only, gg)
        # with M == D the normals are the diagonal step's
        assert np.array_equal(SO.state_normals(GN.noise_shape((3, 2, 7), 7), 5, 17, T), SO.state_normals((3, 2, 7), 5, 17, T))
    assert be.launches == ["sde_gn_step", "sde_gn_backward", "sde_gn_backward"] * 2


# ----------------------------------------------------------------------------------------------
# the launches of a walk
# ----------------------------------------------------------------------------------------------
def test_launches_of_a_walk(dev):
    """Four steps: exactly four sde_gn_step launches and no sde_em_step; the backward four sde_gn_backward launches.  Sub-stepped: one
    per grid step.  ``nfe`` counts steps as under diagonal noise."""
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    for noise_type, M in (("general", 2), ("scalar", 1)):
        co = Coeffs(3, M, torch.float64, dev)
        del be.launches[:]
        with torch.no_grad():
            sdeint(SC.drift, co.diffusion, y0, t, solver=Euler, options=_opts(seed=1, noise_type=noise_type))
        assert be.launches == ["sde_gn_step"] * 4
        del be.launches[:]
        with torch.no_grad():
            sdeint(SC.drift, co.diffusion, y0, t, solver=Euler, options=_opts(seed=1, noise_type=noise_type, step_size=0.125, interp="linear"))
        assert [x for x in be.launches if x != "interp_rows"] == ["sde_gn_step"] * 8
        net = _Net(3, M, torch.float64, dev)
        del be.launches[:]
        ys = sdeint(net.drift, net.diffusion, y0.clone().requires_grad_(True), t, solver=Euler, options=_opts(seed=1, noise_type=noise_type))
        assert be.launches == ["sde_gn_step"] * 4
        del be.launches[:]
        ys.sum().backward()
        assert be.launches == ["sde_gn_backward"] * 4
    xde = BaseSDE(SC.drift, Coeffs(3, 2, torch.float64, dev).diffusion, y0, t, seed=1, noise_type="general")
    solver = Euler(xde=xde, y0=y0, rtol=1e-7, atol=1e-9, norm=None)
    with torch.no_grad():
        solver.integrate(t)
    assert solver.nfe == 4 and xde.noise_dim == 2


# ----------------------------------------------------------------------------------------------
# gradcheck
# ----------------------------------------------------------------------------------------------
def test_gradcheck_through_three_steps(dev):
    """float64, (rows, D, M) = (2, 3, 2), three steps, the tool's default tolerances: with respect to y0 and a parameter of each
    coefficient."""
    t = torch.tensor([0.0, 0.2, 0.35, 0.6], dtype=torch.float64)
    gen = torch.Generator().manual_seed(5)
    P = torch.randn(3, 2, generator=gen, dtype=torch.float64)

    def fn(y0, a, c):
        return sdeint(lambda t_, y: y * a + (y * y) * 0.125, lambda t_, y: torch.tanh(y.unsqueeze(-1) * P) * c + 0.25, y0, t, solver=Euler,
                      options=_opts(seed=4, noise_type="general"))

    inputs = [(0.5 + torch.rand(2, 3, generator=gen, dtype=torch.float64)).requires_grad_(True)]
    inputs += [torch.tensor(v, dtype=torch.float64).requires_grad_(True) for v in (-0.6, 0.4)]
    assert torch.autograd.gradcheck(fn, inputs)
    assert "sde_gn_backward" in _hip.get_backend().launches


def test_gradcheck_of_the_step_node(dev):
    be = _hip.get_backend()
    gen = torch.Generator().manual_seed(4)
    y0, f = (torch.randn(2, 3, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    g = torch.randn(2, 3, 2, generator=gen, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda *xs: SdeGnEulerFn.apply(be, -0.0625, 0.25, 12345, 3, *xs), (y0, f, g))
    # an absent cotangent stays absent, and without any the backward launches nothing
    del be.launches[:]
    y1 = SdeGnEulerFn.apply(be, 0.0625, 0.25, 12345, 3, y0, f.detach(), g.detach())
    (gy,) = torch.autograd.grad(y1.sum(), (y0,))
    assert torch.equal(gy, torch.ones_like(y0)) and be.launches == ["sde_gn_step"]


# ----------------------------------------------------------------------------------------------
# what is refused, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals_say_that_euler_steps_general_noise(dev):
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 3, dtype=torch.float64)
    co = Coeffs(3, 2, torch.float64, dev)
    one = Coeffs(3, 1, torch.float64, dev)
    for noise_type, g in (("general", co.diffusion), ("scalar", one.diffusion)):
        for solver, why in ((Milstein, "Levy areas"), (SRK, "Levy areas"), (ReversibleHeun, "diagonal")):
            with pytest.raises(NotImplementedError, match=why) as e:
                sdeint(SC.drift, g, y0, t, solver=solver, options=_opts(seed=1, noise_type=noise_type))
            assert "solver=Euler" in str(e.value) and noise_type in str(e.value)
        with pytest.raises(NotImplementedError, match="solver=Euler") as e:
            sdeint_adjoint(SC.drift, g, y0, t, solver=ReversibleHeun, options=_opts(seed=1, noise_type=noise_type), adjoint_params=())
        assert "noise_type" in str(e.value)
        with pytest.raises(NotImplementedError, match="linear solve") as e:
            sdeint(SC.drift, g, y0, t, solver=Euler, options=_opts(seed=1, noise_type=noise_type, logqp=True, prior_drift=SC.drift))
        assert "solver=Euler" in str(e.value)
    for bad in ("additive", "Diagonal", None, 3):
        with pytest.raises(ValueError, match="'diagonal', 'general' or 'scalar'"):
            sdeint(SC.drift, co.diffusion, y0, t, solver=Euler, options=_opts(seed=1, noise_type=bad))
        with pytest.raises(ValueError, match="'diagonal', 'general' or 'scalar'"):
            sdeint_adjoint(SC.drift, co.diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=1, noise_type=bad), adjoint_params=())
    # the diffusion's shape, per noise type
    for noise_type, bad in (("general", SC.diffusion), ("general", lambda t_, y: co.diffusion(t_, y).float()), ("general", lambda t_, y: 0.5),
                            ("general", lambda t_, y: y.unsqueeze(-1)[..., :0]), ("scalar", co.diffusion), ("scalar", SC.diffusion)):
        with pytest.raises(ValueError, match=noise_type + " noise"):
            sdeint(SC.drift, bad, y0, t, solver=Euler, options=_opts(seed=1, noise_type=noise_type))
    with pytest.raises(ValueError, match="diagonal noise"):  # (the parent's check and message)
        sdeint(SC.drift, co.diffusion, y0, t, solver=Euler, options=_opts(seed=1))
    with pytest.raises(ValueError, match="diagonal noise"):
        sdeint(SC.drift, co.diffusion, y0, t, solver=Euler, options=_opts(seed=1, noise_type="diagonal"))
    assert be.launches == []
    # M is fixed by the first evaluation
    width = {"M": 2}
    xde = BaseSDE(SC.drift, lambda t_, y: y.unsqueeze(-1).expand(y.shape + (width["M"],)), y0, t, seed=1, noise_type="general")
    assert xde.noise_dim is None and xde.diffusion(None, y0).shape == (2, 3, 2) and xde.noise_dim == 2
    width["M"] = 3
    with pytest.raises(ValueError, match=r"\(2,\)"):
        xde.diffusion(None, y0)
    # sdeint_adjoint with the key at its default value is the parent's call
    with torch.no_grad():
        a = sdeint_adjoint(SC.drift, SC.diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=1, noise_type="diagonal"), adjoint_params=())
        b = sdeint_adjoint(SC.drift, SC.diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=1), adjoint_params=())
    assert torch.equal(a, b)


def test_fuse_states_the_general_step(dev):
    """``BaseSDE.fuse`` under general noise is the kernel's statement in framework ops: the same bits as the double's launch."""
    be = _hip.get_backend()
    gen = torch.Generator().manual_seed(8)
    y0, f = (torch.randn(4, 3, generator=gen, dtype=torch.float64) for _ in range(2))
    g = torch.randn(4, 3, 5, generator=gen, dtype=torch.float64)
    z = torch.empty(4, 5, dtype=torch.float64)
    be._sde_noise(z, 7, 2)
    y1 = torch.empty_like(y0)
    be._sde_gn_step(y1, y0, f, g, 0.125, 0.25, 7, 2)
    t = torch.linspace(0.0, 1.0, 3, dtype=torch.float64)
    xde = BaseSDE(SC.drift, SC.diffusion, y0, t, seed=7, noise_type="general")
    assert torch.equal(xde.fuse((f, g, 0.25 * z), 0.125, y0), y1)
    diag = BaseSDE(SC.drift, SC.diffusion, y0, t, seed=7)
    assert torch.equal(diag.fuse((f, f, z[:, :3]), 0.125, y0), (y0 + f * 0.125) + f * z[:, :3])
