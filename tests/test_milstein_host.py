"""sdeint's Milstein steps without a GPU: the end-to-end cases of tests/_milstein_cases.py on the numpy double, the launches of a step,
and the C ABI of the new entry points of include/xde_hip_sde.h (every call below is refused on the host before anything is enqueued,
or has nothing to do)."""
import functools

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.xde.base_sde import BaseSDE

from . import _sde_oracle as SO
from ._milstein_cases import *  # noqa: F401,F403
from ._milstein_cases import _opts, _y0, diffusion, drift


@pytest.fixture
def dev(monkeypatch):
    from ._milstein_double import MilsteinDoubleBackend

    # (the Z of (seed, k) is the same array for every walk of a test: drawn once.  The strong-order case walks 2^16 paths over up to 256
    # steps three times per grid; its 256 arrays are dropped with the fixture)
    monkeypatch.setattr(SO, "state_normals", functools.lru_cache(maxsize=512)(SO.state_normals))
    _hip._set_backend_for_testing(MilsteinDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def test_launches_of_a_step(dev):
    """Without gradients a step is one support launch and one step launch, and nothing else of the library's; with gradients the two
    backward launches appear once per step."""
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    n_steps = len(t) - 1
    with torch.no_grad():
        sdeint(drift, diffusion, y0, t, solver=Milstein, options=_opts(seed=1))
    assert be.launches == ["sde_milstein_support", "sde_milstein_step"] * n_steps
    del be.launches[:]
    mu = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    sol = sdeint(drift, lambda t_, y: y * mu, y0.clone().requires_grad_(True), t, solver=Milstein, options=_opts(seed=1))
    assert be.launches == ["sde_milstein_support", "sde_milstein_step"] * n_steps
    del be.launches[:]
    sol.sum().backward()
    assert be.launches == ["sde_milstein_backward", "sde_milstein_support_backward"] * n_steps


def test_a_step_counts_one_nfe_and_evaluates_drift_once_and_diffusion_twice(dev):
    from paddlexde_amd.solver import Milstein as M

    nf, ng = [], []
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    xde = BaseSDE(lambda t_, y: nf.append(1) or y * 0.5, lambda t_, y: ng.append(1) or y * 0.25, y0, t, seed=3)
    s = M(xde=xde, y0=y0, rtol=1e-7, atol=1e-9, norm=None)
    with torch.no_grad():
        s.integrate(t)
    assert (s.nfe, len(nf), len(ng)) == (3, 3, 6)


def test_diffusion_method_carries_the_check():
    y = torch.ones(2, 3, dtype=torch.float64)
    xde = BaseSDE(lambda t_, y_: y_, lambda t_, y_: y_ * 2.0, y, torch.tensor([0.0, 1.0]), seed=1)
    assert torch.equal(xde.diffusion(None, y), y * 2.0)
    f, g = xde.move(None, None, y)
    assert torch.equal(f, y) and torch.equal(g, y * 2.0)
    bad = BaseSDE(lambda t_, y_: y_, lambda t_, y_: y_.float(), y, torch.tensor([0.0, 1.0]), seed=1)
    for call in (lambda: bad.diffusion(None, y), lambda: bad.move(None, None, y)):
        with pytest.raises(ValueError, match="diagonal noise"):
            call()


# ----------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------
def test_milstein_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    A, B, Cc, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # (never dereferenced: every call is refused first)

    def support(yb=A, y0=B, f=Cc, g=D, n=8, dtype=0):
        return lib.xde_sde_milstein_support(yb, y0, f, g, n, 0.1, 0.3, dtype, None), lib.xde_last_error().decode()

    def support_bwd(gf=A, gg=B, gy=Cc, n=8, dtype=0):
        return lib.xde_sde_milstein_support_backward(gf, gg, gy, n, 0.1, 0.3, dtype, None), lib.xde_last_error().decode()

    def step(y1=A, y0=B, f=Cc, g=D, gb=E, n=8, k=0, dtype=0):
        return lib.xde_sde_milstein_step(y1, y0, f, g, gb, n, 0.1, 0.3, 1.5, 1, k, dtype, None), lib.xde_last_error().decode()

    def bwd(gf=A, gg=B, ggb=Cc, gy=D, n=8, k=0, dtype=0):
        return lib.xde_sde_milstein_backward(gf, gg, ggb, gy, n, 0.1, 0.3, 1.5, 1, k, dtype, None), lib.xde_last_error().decode()

    cases = [(support, "xde_sde_milstein_support", [dict(yb=None), dict(y0=None), dict(f=None), dict(g=None), dict(n=-1), dict(dtype=2),
                                                    dict(dtype=-1), dict(y0=B + 2), dict(g=D + 4, dtype=1)]),
             (support_bwd, "xde_sde_milstein_support_backward", [dict(gy=None), dict(n=-1), dict(dtype=2), dict(gf=A + 2),
                                                                 dict(gg=B + 4, dtype=1)]),
             (step, "xde_sde_milstein_step", [dict(y1=None), dict(y0=None), dict(f=None), dict(g=None), dict(gb=None), dict(n=-1),
                                              dict(dtype=2), dict(dtype=-1), dict(k=-1), dict(k=1 << 32), dict(y0=B + 2),
                                              dict(gb=E + 4, dtype=1)]),
             (bwd, "xde_sde_milstein_backward", [dict(gy=None), dict(n=-1), dict(dtype=2), dict(k=-1), dict(k=1 << 32), dict(gf=A + 2),
                                                 dict(ggb=Cc + 4, dtype=1)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)
        assert fn(n=0)[0] == _hip.XDE_OK  # n == 0: nothing to launch
    assert support_bwd(gf=None, gg=None)[0] == _hip.XDE_OK  # no output wanted
    assert bwd(gf=None, gg=None, ggb=None)[0] == _hip.XDE_OK


def test_the_library_exports_the_milstein_entry_points():
    lib = _hip.load_library()
    for sym in ("xde_sde_milstein_support", "xde_sde_milstein_support_backward", "xde_sde_milstein_step", "xde_sde_milstein_backward"):
        assert sym in _hip.HEADERS["xde_hip_sde.h"] and hasattr(lib, sym)


def test_the_milstein_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("sde" in m or "milstein" in m for m in pub)
    for m in ("_sde_milstein_support", "_sde_milstein_support_backward", "_sde_milstein_step", "_sde_milstein_backward"):
        assert callable(getattr(_hip.HipBackend, m))


def test_milstein_is_importable_from_both_solver_packages():
    import paddlexde_amd
    from paddlexde_amd.solver import FixedSolver, Milstein as A
    from paddlexde_amd.solver.fixed_solver import Milstein as B

    assert A is B and issubclass(A, FixedSolver) and A.steps_sde
    assert not hasattr(paddlexde_amd, "sdeint")  # (the top level keeps the reference's ODE / DDE names)


def test_the_double_states_the_kernels_op_order(dev):
    """The double's four methods against tests/_milstein_oracle.py on one step (the GPU test holds the kernels to the same statement)."""
    from . import _milstein_oracle as MO

    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        g = torch.Generator().manual_seed(1)
        y0, f, gd, gb, gy = (torch.randn(3, 7, generator=g, dtype=dtype) for _ in range(5))
        for dt in (T(-0.0123), T(0.0)):
            s, c = SO.s_of(dt, T), MO.c_of(dt, T)
            z = SO.state_normals((3, 7), 5, 17, T)
            yb, y1 = torch.empty_like(y0), torch.empty_like(y0)
            be._sde_milstein_support(yb, y0, f, gd, float(dt), float(s))
            assert np.array_equal(yb.numpy(), MO.support(y0.numpy(), f.numpy(), gd.numpy(), dt, T))
            be._sde_milstein_step(y1, y0, f, gd, gb, float(dt), float(s), float(c), 5, 17)
            assert np.array_equal(y1.numpy(), MO.milstein_step(y0.numpy(), f.numpy(), gd.numpy(), gb.numpy(), dt, z, T))
            if dt == 0:
                assert np.array_equal(y1.numpy(), y0.numpy()) and np.array_equal(yb.numpy(), y0.numpy())
            w, q = MO.correction(dt, z, T)
            gf, gg, ggb = (torch.empty_like(gy) for _ in range(3))
            be._sde_milstein_backward(gf, gg, ggb, gy, float(dt), float(s), float(c), 5, 17)
            assert np.array_equal(gf.numpy(), gy.numpy() * dt) and np.array_equal(gg.numpy(), gy.numpy() * (w - q))
            assert np.array_equal(ggb.numpy(), gy.numpy() * q)
            be._sde_milstein_support_backward(gf, gg, gy, float(dt), float(s))
            assert np.array_equal(gf.numpy(), gy.numpy() * dt) and np.array_equal(gg.numpy(), gy.numpy() * s)
