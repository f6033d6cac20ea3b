"""Delay-equation cases (collected by test_gpu_odeint.py on the GPU and test_host_logic.py on the CPU double)."""
import numpy as np
import pytest
import torch

from oracle import xde_oracle as O
from paddlexde_amd import RK4, AdamsBashforthMoulton, Euler, Midpoint, ddeint, ddeint_adjoint
from paddlexde_amd.xde import BaseDDE, HistoryIndex

from . import problems as P

def _blocks(n):
    """Number of seeded blocks of a randomised sweep; XDE_SWEEP_SCALE=k runs k times as many (a soak, not the default)."""
    import os

    return n * int(os.environ.get("XDE_SWEEP_SCALE", "1"))


SOLVERS = {"euler": Euler, "midpoint": Midpoint, "rk4": RK4, "adams": AdamsBashforthMoulton}


def _history(shape, T, uniform, seed=0, dtype=np.float32):
    rng = np.random.RandomState(seed)
    t = np.arange(T, dtype=np.float64) if uniform else np.cumsum(rng.uniform(0.3, 1.7, size=T))
    base = np.sin(0.37 * t)[:, None] * np.linspace(0.5, 1.5, shape[-1])[None, :]
    his = base + 0.1 * rng.randn(*shape[:-1], T, shape[-1])
    return his.astype(dtype), t.astype(dtype)


@pytest.mark.parametrize("lead", [(3,), (2, 5), ()])
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [7, 8])  # 7: scalar kernel; 8: the 16-byte-vector kernel with the per-lag table in LDS
@pytest.mark.parametrize("method", ["cubic", "linear", "bez"])
def test_history_gather_vs_oracle(dev, lead, uniform, dtype, D, method):
    """HistoryIndex (xde/base_dde.py:82-127) for its three `interp_method`s against the oracle's restatements of
    CubicHermiteSpline / LinearInterpolation / BezierSpline `.evaluate` and `.derivative` (interpolation/interpolate.py), and its
    backward — one reduction launch — against `sum(grad_y * derivative)` over every axis but the lag axis."""
    T = 24
    his, t = _history(lead + (D,), T, uniform, dtype=dtype)
    lags = np.array([t[0] - 0.4, t[0], 0.5 * (t[0] + t[1]), t[5], t[5] + 1e-3, t[11] + 0.77 * (t[12] - t[11]), t[-4] + 0.1, t[-3], t[-2], t[-1],
                     t[-1] + 0.9], dtype=dtype)
    y_ref, _ = O.history_index(lags, his, t, dtype=dtype, interp_method=method)
    d_ref = O.HISTORY_SPLINES[method](his, t, dtype=dtype).derivative(lags)
    lg = torch.from_numpy(lags).to(dev).requires_grad_(True)
    y = HistoryIndex.apply(lg, torch.from_numpy(his).to(dev), torch.from_numpy(t).to(dev), method)
    assert y.shape == lead + (len(lags), D)
    tol = 2e-5 if dtype == np.float32 else 1e-12
    assert P.rel_err(y.detach().cpu().numpy(), y_ref) <= tol
    # the gradient w.r.t. the lags is the derivative, reduced over every axis but the lag axis
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=y.dtype).to(dev)
    (y * w).sum().backward()
    axes = tuple(a for a in range(w.dim()) if a != w.dim() - 2)
    g_ref = (w.cpu().numpy().astype(np.float64) * d_ref.astype(np.float64)).sum(axis=axes)
    assert lg.grad.shape == lg.shape and lg.grad.dtype == lg.dtype
    assert P.rel_err(lg.grad.cpu().numpy(), g_ref) <= (5e-5 if dtype == np.float32 else 1e-11)


@pytest.mark.parametrize("name", ["LinearInterpolation", "CubicHermiteSpline", "BezierSpline"])
@pytest.mark.parametrize("kind", ["ramp", "sine"])
def test_reference_interpolation_tests_as_written(dev, kind, name):
    """tests/interpolation/test_interpolation.py:34-47,74-85, line for line on the product's spline classes (`paddlexde_amd.interpolation`,
    the reference's `paddlexde.interpolation`): `interp = Cls(series, t); allclose(val_tgt, interp.evaluate(t_eval), rtol=...);
    allclose(tgt_deri, interp.derivative(t_eval), rtol=...)` — and the objects agree with `HistoryIndex` bit for bit (same launch)."""
    import paddlexde_amd.interpolation as I

    series, t, t_eval, val_tgt, der_tgt = P.interpolation_fixture(kind)
    method = {"LinearInterpolation": "linear", "CubicHermiteSpline": "cubic", "BezierSpline": "bez"}[name]
    rtol_val, rtol_der = P.INTERPOLATION_TOLERANCES[kind][method]
    interp = getattr(I, name)(torch.from_numpy(series).to(dev), torch.from_numpy(t).to(dev))
    val, der = interp.evaluate(torch.from_numpy(t_eval).to(dev)), interp.derivative(torch.from_numpy(t_eval).to(dev))
    assert val.shape == der.shape == (1, 1, 2)
    assert P.paddle_allclose(val_tgt, val.cpu().numpy(), rtol=rtol_val)
    assert P.paddle_allclose(der_tgt, der.cpu().numpy(), rtol=rtol_der)
    y = HistoryIndex.apply(torch.from_numpy(t_eval).to(dev), torch.from_numpy(series).to(dev), torch.from_numpy(t).to(dev), method)
    assert torch.equal(y, val)
    assert torch.equal(interp.grid_points.cpu(), torch.from_numpy(t)) and interp.interval.shape == (2,)
    # the default grid (t=None) is the unit grid: on the ramp series that is the fixture's own grid
    if kind == "ramp":
        assert torch.equal(getattr(I, name)(torch.from_numpy(series).to(dev)).evaluate(torch.from_numpy(t_eval).to(dev)), val)


@pytest.mark.parametrize("method", ["linear", "cubic", "bez"])
@pytest.mark.parametrize("kind", ["ramp", "sine"])
def test_reference_interpolation_fixtures_on_the_history_kernels(dev, kind, method):
    """The reference's own spline fixtures (tests/interpolation/test_interpolation.py:13-85: ramp series at t = 21.12, sine series at
    t = 16.5; value + derivative tolerances per class) through the PRODUCT: `HistoryIndex.apply` (xde_history_gather /
    xde_hermite_gather) gives the value, its backward (xde_lag_grad) the derivative — one component at a time, so that each is held
    to the reference's tolerance — and both are compared with the oracle's classes on the same inputs in ulps."""
    series, t, t_eval, val_tgt, der_tgt = P.interpolation_fixture(kind)
    rtol_val, rtol_der = P.INTERPOLATION_TOLERANCES[kind][method]
    his, ts = torch.from_numpy(series).to(dev), torch.from_numpy(t).to(dev)
    der = np.zeros((1, 1, 2), dtype=np.float32)
    for d in range(2):
        lg = torch.from_numpy(t_eval).to(dev).requires_grad_(True)
        y = HistoryIndex.apply(lg, his, ts, method)
        assert y.shape == (1, 1, 2) and y.dtype == torch.float32
        y[0, 0, d].backward()  # d y_d / d lag = the spline's time derivative of component d
        der[0, 0, d] = float(lg.grad[0])
    val = y.detach().cpu().numpy()
    assert P.paddle_allclose(val_tgt, val, rtol=rtol_val), (val_tgt, val)
    assert P.paddle_allclose(der_tgt, der, rtol=rtol_der), (der_tgt, der)
    interp = O.HISTORY_SPLINES[method](series, t)
    # The derivative is a DIFFERENCE of history rows divided by the knot spacing: the magnitude its rounding errors live at is that of
    # the summed terms, max|row| / spacing (ramp: 10.5 / 1 against a result of 0.5), not that of the result.
    i = int(np.clip(np.searchsorted(t, t_eval[0], side="left") - 1, 0, len(t) - 1))
    term = np.float32(np.abs(series[..., i : i + 4, :]).max() / (t[i + 1] - t[i]))
    d_ref = interp.derivative(t_eval)
    rec = {"kind": kind, "method": method, "value_ulps": P.ulps_apart(val, interp.evaluate(t_eval)),
           "derivative_ulps_of_terms": float(np.abs(der.astype(np.float64) - d_ref).max() / float(np.spacing(term)))}
    P.report("reference_interpolation_fixture", rec)
    # same formulas, same association; the oracle's numpy matmul may contract / reorder its 2-4 products, so "a few ulps", stated:
    assert rec["value_ulps"] <= 4 and rec["derivative_ulps_of_terms"] <= 4, rec


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lag_gradient_reduction_at_odd_sizes(dev, dtype):
    """xde_lag_grad alone: [outer, L, D] products reduced to [L] in one launch, for row lengths that are / are not a multiple of
    the vector width, a single row, many rows, an empty batch."""
    from paddlexde_amd import _hip

    be = _hip.get_backend()
    rng = np.random.RandomState(3)
    # (the last rows: ADVICE r04 — rows longer than a workgroup's reach, D > 1024 for fp32 / > 512 for fp64, were refused by the C entry
    # point while the Python gate let them through; an [L, D] plane of exactly 256 vectors; more lags than one workgroup has lanes)
    for outer, L, D in [(1, 1, 1), (5, 3, 7), (64, 12, 64), (1000, 5, 16), (17, 128, 4), (3, 2, 250), (0, 4, 8), (9, 3, 2048), (7, 2, 1031),
                        (40, 4, 256), (33, 64, 16), (3, 300, 8), (2, 1, 4100)]:
        gy, de = rng.randn(outer, L, D).astype(dtype), rng.randn(outer, L, D).astype(dtype)
        got = be.lag_grad(torch.from_numpy(gy).to(dev), torch.from_numpy(de).to(dev)).cpu().numpy()
        want = (gy * de).astype(np.float64).sum(axis=(0, 2))
        assert got.shape == (L,) and got.dtype == dtype
        assert np.allclose(got, want, rtol=3e-6 if dtype == np.float32 else 1e-13, atol=1e-6 if dtype == np.float32 else 1e-13), (outer, L, D)
    # the same launch twice: the workspace is left re-armed
    gy, de = torch.from_numpy(rng.randn(300, 12, 64).astype(dtype)).to(dev), torch.from_numpy(rng.randn(300, 12, 64).astype(dtype)).to(dev)
    assert torch.equal(be.lag_grad(gy, de), be.lag_grad(gy, de))
    # an unaligned view of a long row (element-wise path), and the autograd entry on a row of 2048 columns
    big = torch.from_numpy(rng.randn(2 * 5 * 3 * 700 + 1).astype(dtype)).to(dev)
    gy_u, de_u = big[1 : 1 + 5 * 3 * 700].view(5, 3, 700), big[1 + 5 * 3 * 700 :].view(5, 3, 700)
    want = (gy_u.cpu().numpy() * de_u.cpu().numpy()).astype(np.float64).sum(axis=(0, 2))
    assert np.allclose(be.lag_grad(gy_u, de_u).cpu().numpy(), want, rtol=3e-6 if dtype == np.float32 else 1e-13, atol=1e-5 if dtype == np.float32 else 1e-12)
    T = 8
    his, ts = _history((3, 2048), T, True, dtype=dtype)
    lg = torch.tensor([1.5, 4.25], dtype=torch.from_numpy(ts).dtype).to(dev).requires_grad_(True)
    y = HistoryIndex.apply(lg, torch.from_numpy(his).to(dev), torch.from_numpy(ts).to(dev), "linear")
    y.sum().backward()  # (raised XdeError inside backward before round 5)
    d_ref = O.HISTORY_SPLINES["linear"](his, ts, dtype=dtype).derivative(lg.detach().cpu().numpy())
    assert P.rel_err(lg.grad.cpu().numpy(), d_ref.astype(np.float64).sum(axis=(0, 2))) <= (5e-5 if dtype == np.float32 else 1e-11)


def test_history_spline_properties(dev):
    """Independent of the oracle: nodes are reproduced, a linear history is reproduced exactly between nodes and its
    derivative is the slope (uniform grid)."""
    T, D = 16, 3
    t = np.arange(T, dtype=np.float64)
    his = (2.5 * t[:, None] + np.array([0.0, 1.0, -3.0])[None, :])[None]
    lags = np.array([0.25, 3.0, 7.5, 14.9], dtype=np.float64)
    y = HistoryIndex.apply(torch.from_numpy(lags).to(dev), torch.from_numpy(his).to(dev), torch.from_numpy(t).to(dev))
    assert np.allclose(y.cpu().numpy()[0], 2.5 * lags[:, None] + np.array([0.0, 1.0, -3.0])[None, :], rtol=1e-12, atol=1e-12)
    rng = np.random.RandomState(0)
    his2 = rng.randn(2, T, D)
    nodes = t[1:-1].copy()
    y2 = HistoryIndex.apply(torch.from_numpy(nodes).to(dev), torch.from_numpy(his2).to(dev), torch.from_numpy(t).to(dev))
    assert np.allclose(y2.cpu().numpy(), his2[:, 1:-1, :], rtol=1e-12, atol=1e-12)


# only +, -, * and indexing, so numpy and torch agree to the last bit
def _dde_func_np(y_lags, y):
    return -0.5 * y + 0.25 * (y_lags[..., 0, :] * y_lags[..., -1, :]) - 0.1 * y * y * y + 0.125 * y_lags[..., 1, :]


def _dde_func_t(y_lags, y):
    return -0.5 * y + 0.25 * (y_lags[..., 0, :] * y_lags[..., -1, :]) - 0.1 * y * y * y + 0.125 * y_lags[..., 1, :]


@pytest.mark.parametrize("solver", list(SOLVERS))
def test_ddeint_vs_oracle_bit_exact_with_processed_history(dev, solver):
    """his_processed=True feeds both sides the same delayed states: the damped fuse (xde/base_dde.py:55-58) and the whole
    fixed-step trajectory are then bit-exact."""
    rng = np.random.RandomState(2)
    B, L, D = 6, 5, 4
    y0 = rng.randn(B, D).astype(np.float32)
    y_lags = rng.randn(B, L, D).astype(np.float32)
    t = np.linspace(0.0, 1.0, 21).astype(np.float32)
    ref, yl = O.ddeint(_dde_func_np, y0, t, None, y_lags, None, solver, his_processed=True)
    got, gl = ddeint(_dde_func_t, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), None, torch.from_numpy(y_lags).to(dev), None,
                     SOLVERS[solver], his_processed=True)
    assert got.shape == ref.shape == (21 * B, D)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(gl.cpu().numpy(), yl)
    # the damping really is applied: an undamped RK4 run of the same dynamics differs
    from paddlexde_amd import odeint

    yl_t = torch.from_numpy(y_lags).to(dev)
    plain = odeint(lambda t_, y: _dde_func_t(yl_t, y), torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), solver=SOLVERS[solver])
    assert not torch.equal(plain, got)


def test_ddeint_full_path_vs_oracle(dev):
    his, ht = _history((4, 3), 20, uniform=True)
    lags = np.array([1.5, 4.0, 7.25, 12.8, 18.0], dtype=np.float32)
    y0 = his[:, -1, :].copy()
    t = np.linspace(0.0, 2.0, 17).astype(np.float32)
    ref, yl = O.ddeint(_dde_func_np, y0, t, lags, his, ht, "rk4")
    got, gl = ddeint(_dde_func_t, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(lags).to(dev),
                     torch.from_numpy(his).to(dev), torch.from_numpy(ht).to(dev), RK4)
    assert P.rel_err(gl.cpu().numpy(), yl) <= 2e-5
    assert P.rel_err(got.cpu().numpy(), ref) <= 1e-5


def test_ddeint_backprop_to_params_and_lags(dev):
    """The reference trains through ddeint (example/dde_demo.py, D3STN): gradients reach func's parameters through the
    damped combine nodes and the lags through HistoryIndex.backward — checked against the same scheme in eager ops."""
    dtype = torch.float64
    his, ht = _history((3, 2), 18, uniform=True, dtype=np.float64)
    his_t, ht_t = torch.from_numpy(his).to(dev), torch.from_numpy(ht).to(dev)
    lin = torch.nn.Linear(2, 2).to(dtype).to(dev)

    def func(y_lags, y):
        return lin(torch.tanh(y)) + 0.3 * y_lags.mean(dim=-2)

    y0 = torch.from_numpy(his[:, -1, :].copy()).to(dev)
    t = torch.linspace(0.0, 1.0, 6, dtype=dtype).to(dev)
    lags = torch.tensor([2.25, 6.5, 11.0], dtype=dtype, device=dev, requires_grad=True)
    sol, y_lags = ddeint(func, y0, t, lags, his_t, ht_t, RK4)
    (sol * sol).mean().backward()
    got = [lags.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()]
    lags.grad = None
    lin.zero_grad()

    # eager restatement: differentiable cubic Hermite on the uniform grid + the damped RK4 variant
    i = torch.clamp(torch.bucketize(lags.detach(), ht_t) - 1, 0, len(ht) - 1)
    s = (lags - ht_t[i]).unsqueeze(-1)  # h = 1

    def ser(j):
        return his_t[:, torch.clamp(j, max=len(ht) - 1), :]

    def drv(j):
        jj = torch.clamp(j, max=len(ht) - 2)
        return ser(jj + 1) - ser(jj)

    p0, p1, d0, d1 = ser(i), ser(i + 1), drv(i), drv(i + 1)
    yl = (2 * s**3 - 3 * s**2 + 1) * p0 + (-2 * s**3 + 3 * s**2) * p1 + (s**3 - 2 * s**2 + s) * d0 + (s**3 - s**2) * d1
    assert torch.allclose(yl, y_lags, rtol=1e-12, atol=1e-12)

    def fuse(dy, dt, y):
        yy = dy * dt + y
        return (dy - 0.001 * yy) * dt + y

    y, ys = y0, [y0]
    for k in range(1, len(t)):
        dt = t[k] - t[k - 1]
        k1 = func(yl, y)
        k2 = func(yl, fuse(k1, dt / 3, y))
        k3 = func(yl, fuse(k1 - k2 / 3, dt, y))
        k4 = func(yl, fuse(k1 - k2 + k3, dt, y))
        y = (fuse(k1, dt, y) + 3 * fuse(k2, dt, y) + 3 * fuse(k3, dt, y) + fuse(k4, dt, y)) * 0.125
        ys.append(y)
    ref_sol = torch.cat(ys, dim=-2)
    assert torch.allclose(sol, ref_sol, rtol=1e-11, atol=1e-13)
    (ref_sol * ref_sol).mean().backward()
    for a, b in zip(got, [lags.grad, lin.weight.grad, lin.bias.grad]):
        assert torch.allclose(a, b, rtol=1e-8, atol=1e-12), float((a - b).abs().max())


def test_dde_api_conventions(dev):
    with pytest.raises(NotImplementedError):
        ddeint_adjoint(func=None)
    his, ht = _history((2, 3), 8, uniform=True)
    x = BaseDDE(lambda yl, y: y, y0=torch.zeros(2, 3, device=dev), t_span=torch.tensor([0.0, 1.0]), lags=None,
                his=torch.from_numpy(his).to(dev), his_span=torch.from_numpy(ht).to(dev), his_processed=True)
    dy, y0 = torch.ones(2, 3, device=dev), torch.full((2, 3), 2.0, device=dev)
    assert torch.allclose(x.fuse(dy, 0.5, y0), (dy - 0.001 * (dy * 0.5 + y0)) * 0.5 + y0)
    with pytest.raises(NotImplementedError):  # (the reference's own refusal of an unknown method, base_dde.py:110-111)
        HistoryIndex.apply(torch.zeros(1, device=dev), torch.from_numpy(his).to(dev), torch.from_numpy(ht).to(dev), "spline")
    with pytest.raises(ValueError, match="at least 4"):
        HistoryIndex.apply(torch.zeros(1, device=dev), torch.from_numpy(his[:, :3]).to(dev), torch.from_numpy(ht[:3]).to(dev), "bez")


@pytest.mark.parametrize("block", range(_blocks(3)))
def test_randomised_ddeint_sweep_vs_oracle(dev, block):
    """8 random configurations per block: solver, dtype, leading axes, history length and grid (uniform or not), number of
    lags (some outside the history span: clamped / extrapolated as the reference does), output grid.  The gathered delayed
    states to the spline bar; with the delayed states handed over (``his_processed``) the trajectory is bit-exact."""
    rng = np.random.RandomState(555 + block)
    for case in range(8):
        solver = list(SOLVERS)[rng.randint(len(SOLVERS))]
        dtype = (np.float32, np.float64)[rng.randint(2)]
        lead = tuple(int(x) for x in rng.randint(1, 5, size=rng.randint(1, 3)))
        D = int(rng.choice([1, 2, 3, 4, 8, 12]))
        Th = int(rng.randint(4, 40))
        uniform = bool(rng.rand() < 0.5)
        his, ht = _history(lead + (D,), Th, uniform, seed=int(rng.randint(1000)), dtype=dtype)
        nl = int(rng.randint(1, 9))
        lags = rng.uniform(ht[0] - 0.5, ht[-1] + 0.5, size=nl).astype(dtype)
        if rng.rand() < 0.5:
            lags[rng.randint(nl)] = ht[rng.randint(Th)]  # exactly on a node
        y0 = his[..., -1, :].copy()
        T = int(rng.randint(2, 12))
        t = np.cumsum(rng.uniform(0.01, 0.1, size=T)).astype(dtype)
        tag = (block, case, solver, dtype.__name__, lead, D, Th, uniform, nl, T)

        def f_np(y_lags, y):
            return -0.5 * y + 0.25 * (y_lags[..., 0, :] * y_lags[..., -1, :]) - 0.1 * y * y * y

        ref, yl = O.ddeint(f_np, y0, t, lags, his, ht, solver)
        tt = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        got, gl = ddeint(f_np, tt(y0), tt(t), tt(lags), tt(his), tt(ht), SOLVERS[solver])
        assert tuple(gl.shape) == yl.shape == lead + (nl, D), tag
        assert P.rel_err(gl.cpu().numpy(), yl) <= (5e-5 if dtype == np.float32 else 1e-11), (tag, P.rel_err(gl.cpu().numpy(), yl))
        assert tuple(got.shape) == ref.shape, tag
        assert P.rel_err(got.cpu().numpy(), ref) <= (5e-5 if dtype == np.float32 else 1e-10), (tag, P.rel_err(got.cpu().numpy(), ref))
        # same delayed states on both sides -> bit-exact trajectory
        ref2, _ = O.ddeint(f_np, y0, t, None, yl, None, solver, his_processed=True)
        got2, _ = ddeint(f_np, tt(y0), tt(t), None, tt(yl), None, SOLVERS[solver], his_processed=True)
        assert np.array_equal(got2.cpu().numpy(), ref2), tag


def test_ddeint_graph_pipeline_is_bitwise_equal_to_eager(dev):
    """The D3STN-style caller with options["pipeline"] = "graph": damped fuse, delayed states fixed during the solve."""
    rng = np.random.RandomState(4)
    y0 = rng.randn(6, 4).astype(np.float32)
    y_lags = rng.randn(6, 5, 4).astype(np.float32)
    t = np.linspace(0.0, 1.0, 25).astype(np.float32)
    from paddlexde_amd.utils import _rms_norm

    with torch.no_grad():
        a, _ = ddeint(_dde_func_t, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), None, torch.from_numpy(y_lags).to(dev), None, RK4,
                      his_processed=True)
        b, _ = ddeint(_dde_func_t, torch.from_numpy(y0).to(dev), torch.from_numpy(t).to(dev), None, torch.from_numpy(y_lags).to(dev), None, RK4,
                      his_processed=True, options={"norm": _rms_norm, "pipeline": "graph"})
    assert torch.equal(a, b)
