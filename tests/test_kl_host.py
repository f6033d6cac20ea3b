"""The KL term of a latent SDE without a GPU: the C ABI of include/xde_hip_kl.h (every call below is refused on the host before anything
is enqueued, or has nothing to do), the end-to-end cases of tests/_kl_cases.py on the numpy double, the launches of a step, the refusals
of sdeint, the sub-stepped blend, and gradcheck on the two autograd nodes."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint, sdeint_adjoint
from paddlexde_amd.solver import SRK, ReversibleHeun
from paddlexde_amd.solver._autograd import SdeKlAccFn, SdeKlEulerFn
from paddlexde_amd.xde.base_sde import BaseSDE

from . import _kl_oracle as KL
from . import _sde_oracle as SO
from ._kl_cases import *  # noqa: F401,F403
from ._kl_cases import H_EXACT, T_EXACT, Triple, _opts, _y0, diffusion, drift_cg, prior_zero


@pytest.fixture
def dev():
    from ._kl_double import KlDoubleBackend

    _hip._set_backend_for_testing(KlDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_kl.h
# ----------------------------------------------------------------------------------------------
def test_the_kl_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("kl" in m or "sde" in m for m in pub)
    for m in ("_sde_kl_step", "_sde_kl_backward"):
        assert callable(getattr(_hip.HipBackend, m))


def test_kl_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    Y1, A1, Y0, F, G, H, A0, X = (0x10000 * (i + 1) for i in range(8))  # (never dereferenced: every call is refused first)

    def step(y1=Y1, acc1=A1, y0=Y0, f=F, g=G, h=H, acc0=A0, rows=2, D=4, k=0, dtype=0):
        return lib.xde_sde_kl_step(y1, acc1, y0, f, g, h, acc0, rows, D, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    def bwd(gf=Y1, gg=A1, gh=X, gy=Y0, gacc=A0, f=F, g=G, h=H, rows=2, D=4, k=0, dtype=0):
        return lib.xde_sde_kl_backward(gf, gg, gh, gy, gacc, f, g, h, rows, D, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    n = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32)
    cases = [(step, "xde_sde_kl_step", [
        dict(acc1=None), dict(f=None), dict(g=None), dict(h=None),  # a null operand
        dict(y1=None), dict(y0=None),  # one of y1 / y0 null alone
        dict(rows=-1), dict(D=0), dict(D=-3), dict(dtype=2), dict(dtype=-1), dict(k=-1), dict(k=1 << 32),
        dict(f=F + 2), dict(g=G + 4, dtype=1), dict(acc1=A1 + 4), dict(acc0=A0 + 4),  # alignment to the element type / a double
        dict(y1=F), dict(y1=G + 16), dict(y1=H - 16), dict(y1=Y0 + 16), dict(y1=A0), dict(y1=A1),  # an output over another operand
        dict(acc1=F + n - 8), dict(acc1=Y0), dict(acc1=A0 + 8), dict(acc1=A0 - 8)]),
             (bwd, "xde_sde_kl_backward", [
                 dict(gacc=None), dict(f=None), dict(g=None), dict(h=None), dict(rows=-1), dict(D=0), dict(dtype=2), dict(k=-1),
                 dict(k=1 << 32), dict(gf=Y1 + 2), dict(gh=X + 4, dtype=1), dict(gacc=A0 + 4),
                 dict(gf=F), dict(gg=Y0 + 16), dict(gh=A0), dict(gf=A1), dict(gg=H - 16)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)
        assert fn(rows=0)[0] == _hip.XDE_OK  # no rows: nothing to launch
    assert step(rows=0, y1=Y0)[0] == _hip.XDE_OK and step(rows=0, acc1=A0)[0] == _hip.XDE_OK  # the two allowed aliases
    assert step(rows=0, acc0=None)[0] == _hip.XDE_OK and step(rows=0, y1=None, y0=None, k=-1)[0] == _hip.XDE_OK  # (k is ignored there)
    assert step(y1=None, y0=None, k=1 << 32, rows=0)[0] == _hip.XDE_OK
    assert bwd(gf=None, gg=None, gh=None)[0] == _hip.XDE_OK  # no output wanted
    assert bwd(gf=None, gg=None, gh=None, gy=None, k=-1)[0] == _hip.XDE_OK


# ----------------------------------------------------------------------------------------------
# the double states the header
# ----------------------------------------------------------------------------------------------
def test_the_double_states_the_header(dev):
    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        gen = torch.Generator().manual_seed(3)
        y0, f, h, gy = (torch.randn(3, 2, 7, generator=gen, dtype=dtype) for _ in range(4))
        g = 0.5 + torch.rand(3, 2, 7, generator=gen, dtype=dtype)
        acc0, gacc = torch.rand(3, 2, generator=gen, dtype=torch.float64), torch.randn(3, 2, generator=gen, dtype=torch.float64)
        dt = T(-0.0123)
        s = SO.s_of(dt, T)
        z = SO.state_normals((3, 2, 7), 5, 17, T)
        y1, acc1 = torch.empty_like(y0), torch.empty_like(acc0)
        be._sde_kl_step(y1, acc1, y0, f, g, h, acc0, float(dt), float(s), 5, 17)
        want_y, want_acc = KL.kl_step(y0.numpy(), f.numpy(), g.numpy(), h.numpy(), acc0.numpy(), dt, z, T)
        assert np.array_equal(y1.numpy(), want_y) and np.array_equal(acc1.numpy(), want_acc)
        u = ((f.numpy() - h.numpy()) / g.numpy())
        assert np.allclose(acc1.numpy(), acc0.numpy() + (u.astype(np.float64) ** 2).sum(-1) * 0.5 * float(dt), rtol=1e-5)
        only = torch.empty_like(acc0)
        be._sde_kl_step(None, only, None, f, g, h, acc0, float(dt), 0.0, 0, 0)
        assert torch.equal(only, acc1)
        be._sde_kl_step(None, only, None, f, g, h, None, float(dt), 0.0, 0, 0)
        assert np.array_equal(only.numpy(), KL.accumulate(None, f.numpy(), g.numpy(), h.numpy(), dt, T)[0])
        outs = [torch.empty_like(f) for _ in range(3)]
        be._sde_kl_backward(*outs, gy, gacc, f, g, h, float(dt), float(s), 5, 17)
        for o, want in zip(outs, KL.kl_backward(gy.numpy(), gacc.numpy(), f.numpy(), g.numpy(), h.numpy(), dt, s, z, T)):
            assert np.array_equal(o.numpy(), want)
    assert be.launches == ["sde_kl_step"] * 3 + ["sde_kl_backward"] + ["sde_kl_step"] * 3 + ["sde_kl_backward"]


# ----------------------------------------------------------------------------------------------
# the launches of a step
# ----------------------------------------------------------------------------------------------
def test_launches_of_a_step(dev):
    """Euler: exactly one sde_kl_step per step and no sde_em_step; Milstein: support, sde_milstein_step, sde_kl_step.  Without logqp
    the launches are what they were."""
    from paddlexde_amd.solver import Euler, Milstein

    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    kl = dict(logqp=True, prior_drift=prior_zero)
    for o, n_steps in (({}, 4), ({"step_size": 0.125, "interp": "linear"}, 8)):
        for solver, plain, fused in ((Euler, ["sde_em_step"], ["sde_kl_step"]),
                                     (Milstein, ["sde_milstein_support", "sde_milstein_step"],
                                      ["sde_milstein_support", "sde_milstein_step", "sde_kl_step"])):
            for opts, per_step in ((o, plain), (dict(o, **kl), fused)):
                del be.launches[:]
                with torch.no_grad():
                    sdeint(drift_cg, diffusion, y0, t, solver=solver, options=_opts(seed=1, **opts))
                assert [x for x in be.launches if x != "interp_rows"] == per_step * n_steps, (solver, opts)
    # with gradients: the same forward launches, and one sde_kl_backward per step in the place of sde_em_backward
    tr = Triple(torch.float64, dev, D=3)
    del be.launches[:]
    ys, logqp = sdeint(tr.drift, tr.diffusion, y0.clone().requires_grad_(True), t, solver=Euler,
                       options=_opts(seed=1, logqp=True, prior_drift=tr.prior))
    assert be.launches == ["sde_kl_step"] * 4
    del be.launches[:]
    (ys.sum() + logqp.sum()).backward()
    assert be.launches == ["sde_kl_backward"] * 4
    del be.launches[:]
    ys, logqp = sdeint(tr.drift, tr.diffusion, y0.clone().requires_grad_(True), t, solver=Milstein,
                       options=_opts(seed=1, logqp=True, prior_drift=tr.prior))
    assert be.launches == ["sde_milstein_support", "sde_milstein_step", "sde_kl_step"] * 4
    del be.launches[:]
    (ys.sum() + logqp.sum()).backward()
    assert sorted(set(be.launches)) == ["sde_kl_backward", "sde_milstein_backward", "sde_milstein_support_backward"]
    assert be.launches.count("sde_kl_backward") == 4


# ----------------------------------------------------------------------------------------------
# what sdeint refuses, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals_say_what_works(dev):
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 3, dtype=torch.float64)
    from paddlexde_amd.solver import Euler, Milstein

    with pytest.raises(ValueError, match="prior_drift"):
        sdeint(drift_cg, diffusion, y0, t, solver=Euler, options=_opts(seed=1, logqp=True))
    with pytest.raises(ValueError, match="logqp"):
        sdeint(drift_cg, diffusion, y0, t, solver=Euler, options=_opts(seed=1, prior_drift=prior_zero))
    for solver, why in ((SRK, "two-stage mean"), (ReversibleHeun, "two evaluations")):
        with pytest.raises(NotImplementedError, match=why) as e:
            sdeint(drift_cg, diffusion, y0, t, solver=solver, options=_opts(seed=1, logqp=True, prior_drift=prior_zero))
        assert "solver=Euler" in str(e.value) and "Milstein" in str(e.value)
    for key, value in (("logqp", True), ("prior_drift", prior_zero)):
        with pytest.raises(NotImplementedError, match="solver=Euler") as e:
            sdeint_adjoint(drift_cg, diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=1, **{key: value}), adjoint_params=())
        assert key in str(e.value)
    assert be.launches == []
    # logqp false or absent: the plain call, a tensor
    for o in ({}, {"logqp": False}):
        assert torch.is_tensor(sdeint(drift_cg, diffusion, y0, t, solver=Milstein, options=_opts(seed=1, **o)))
    # the prior is checked the way the diffusion is
    xde = BaseSDE(drift_cg, diffusion, y0, t, seed=1, prior=lambda t_, y: y.float())
    with pytest.raises(ValueError, match="prior drift"):
        xde.prior(None, y0)
    assert torch.equal(BaseSDE(drift_cg, diffusion, y0, t, seed=1, prior=drift_cg).prior(None, y0), drift_cg(None, y0))
    assert BaseSDE(drift_cg, diffusion, y0, t, seed=1).h is None
    with pytest.raises(ValueError, match="shape"):
        sdeint(drift_cg, diffusion, y0, t, solver=Euler, options=_opts(seed=1, logqp=True, prior_drift=lambda t_, y: y[..., :1]))


# ----------------------------------------------------------------------------------------------
# sub-stepping
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_substep_outputs_blend_the_cumulative_sums(dev, dtype):
    """On the double the sums are the oracle's own, so the rows are too: an output inside a grid step is ``L_a + w*(L_b - L_a)`` of the
    two cumulative sums, one on a grid point the copy — bit for bit."""
    from paddlexde_amd.solver import Euler
    from paddlexde_amd.solver.base_fixed_solver import step_size_grid

    from ._kl_cases import oracle_logqp

    T = np.dtype(str(dtype).split(".")[1]).type
    t_np = T_EXACT.astype(T)
    grid = step_size_grid(t_np, H_EXACT)
    tr = Triple(dtype, dev)
    y0 = _y0(dtype, dev, shape=(3, 2, 5))
    with torch.no_grad():
        _, logqp = sdeint(tr.drift, tr.diffusion, y0, torch.as_tensor(t_np), solver=Euler,
                          options=_opts(seed=9, logqp=True, prior_drift=tr.prior, step_size=H_EXACT, interp="linear"))
        _, on_grid = sdeint(tr.drift, tr.diffusion, y0, torch.as_tensor(grid), solver=Euler,
                            options=_opts(seed=9, logqp=True, prior_drift=tr.prior))
    _, want, _ = oracle_logqp(tr, y0, t_np, grid, 9, dtype, dev, "euler")
    assert np.array_equal(logqp.numpy(), want)
    # t[1] = 0.125 and t[3] = t[4] = 0.5 are grid points: the first interval is the sum of the first two grid steps
    cum = np.concatenate([np.zeros(on_grid.shape[:-1] + (1,)), np.cumsum(on_grid.numpy().astype(np.float64), -1)], -1)
    if dtype == torch.float64:
        assert np.allclose(logqp.numpy()[..., 0], cum[..., 2], rtol=1e-14, atol=0)
        w = (T_EXACT[2] - 0.375) / H_EXACT  # 0.390625 lies a quarter into the grid step from 0.375 to 0.4375: the two ends differ
        assert w == 0.25
        assert np.allclose(logqp.numpy()[..., 1], cum[..., 6] + w * (cum[..., 7] - cum[..., 6]) - cum[..., 2], rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------------------------
# gradcheck on the two nodes
# ----------------------------------------------------------------------------------------------
def _gradcheck_inputs(shape=(2, 3), with_acc=True):
    gen = torch.Generator().manual_seed(4)
    mk = lambda: torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_(True)  # noqa: E731
    y0, f, h = mk(), mk(), mk()
    g = (0.75 + torch.rand(*shape, generator=gen, dtype=torch.float64)).requires_grad_(True)
    acc0 = torch.rand(*shape[:-1], generator=gen, dtype=torch.float64).requires_grad_(True) if with_acc else None
    return y0, f, g, h, acc0


@pytest.mark.parametrize("outputs", ["y1", "acc1", "both"])
def test_gradcheck_of_the_fused_step_node(dev, outputs):
    """float64, the tool's default tolerances, with respect to y0, f, g, h and acc0; the cotangent of y1 alone, of acc1 alone, and both."""
    be = _hip.get_backend()
    y0, f, g, h, acc0 = _gradcheck_inputs()
    pick = {"y1": lambda o: o[0], "acc1": lambda o: o[1], "both": lambda o: o}[outputs]
    fn = lambda *xs: pick(SdeKlEulerFn.apply(be, 0.0625, 0.25, 12345, 3, *xs))  # noqa: E731
    assert torch.autograd.gradcheck(fn, (y0, f, g, h, acc0))
    assert torch.autograd.gradcheck(lambda *xs: pick(SdeKlEulerFn.apply(be, -0.0625, 0.25, 12345, 3, *xs, None)), (y0, f, g, h))
    assert "sde_kl_backward" in be.launches or outputs == "y1"
    if outputs == "y1":  # (without the cotangent of acc1 the backward is the plain step's)
        assert "sde_em_backward" in be.launches and "sde_kl_backward" not in be.launches


def test_gradcheck_of_the_accumulate_node(dev):
    be = _hip.get_backend()
    _, f, g, h, acc0 = _gradcheck_inputs()
    assert torch.autograd.gradcheck(lambda *xs: SdeKlAccFn.apply(be, 0.0625, *xs), (f, g, h, acc0))
    assert torch.autograd.gradcheck(lambda *xs: SdeKlAccFn.apply(be, 0.0625, *xs, None), (f, g, h))
    assert set(be.launches) == {"sde_kl_step", "sde_kl_backward"}
