"""The gradient with respect to the control path of cdeint on the GPU: the control-gradient kernel against the numpy double
(tests/_cdegrad_double.py) bit for bit — all three controls, both dtypes, over the grid and the table of tests/_cdegrad_plans.py (each
table row held to its plan, the union held to full coverage), with every form of time and on the scalar path — the coefficient and the
gather transposes bit for bit over the patterns of missing values, every output pre-filled with a sentinel (so an element the launch
skips, or a zero of the wrong sign, shows), refused calls leaving their outputs standing, CdeControlContractFn on torch's allocations,
the end-to-end cases of tests/_cdegrad_e2e.py on the HIP backend, and the demo's --encoder flag."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.interpolation import NaturalCubicSpline

from . import _cdegrad_double as GD
from . import _cdegrad_plans as P
from . import _spline_cases as SC
from . import _spline_double as SD
from ._cdegrad_e2e import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
_DT = {torch.float32: "f32", torch.float64: "f64"}
SENTINEL = 7.0
th = torch.from_numpy


@pytest.fixture
def dev():
    return DEV


@pytest.fixture(autouse=True, scope="module")
def _collect_the_modules_cycles():
    yield
    gc.collect()


def _placed(x, misalign=False):
    """``x`` (numpy) on the device, contiguous, 16-byte aligned or one element off it."""
    flat = torch.empty(x.size + 1, dtype=th(x).dtype, device=DEV)
    view = (flat[1:] if misalign else flat[:-1]).view(x.shape)
    view.copy_(th(x))
    assert (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


def _same_bits(got, want):
    """Equal values and equal signs of zero."""
    got = got.cpu().numpy()
    return np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def _times(knots, Tn):
    """inside the first, a middle and the last interval; on the first, an interior (the first where there is none) and the last knot"""
    m = (Tn - 1) // 2
    return [float(knots[0] + 0.25 * (knots[1] - knots[0])), float(knots[m] + 0.5 * (knots[m + 1] - knots[m])),
            float(knots[-1] - 0.25 * (knots[-1] - knots[-2])), float(knots[0]), float(knots[1 if Tn > 2 else 0]), float(knots[-1])]


def _query(dt, B, H, C, misalign):
    big = torch.empty(8, dtype=torch.float32 if dt == "f32" else torch.float64, device=DEV)[1 if misalign else 0:]
    assert (big.data_ptr() % 16 != 0) == bool(misalign)
    return _hip.get_backend()._cde_control_grad_plan(big, B, H, C)


def _check(double, dtype, B, H, C, Tn, t, form, misalign=False, controls=("linear", "cubic", "natural")):
    """Launch (a) for ``controls`` against the double, bit for bit, on sentinel-filled outputs; returns the branches the launch took."""
    be, T = _hip.get_backend(), _NPT[dtype]
    rs = np.random.RandomState(1000 * C + 10 * H + B)
    F, gout = rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    F_d, g_d = _placed(F, misalign), _placed(gout, misalign)
    where = (dtype, B, H, C, Tn, t, form, misalign)
    for control in controls:
        kn = SC.knots(rs, Tn, T) if control == "natural" else np.arange(Tn, dtype=T)
        tv = _times(kn, Tn)[t]
        # the time as a float64 device scalar (also with a float32 series), as a [1] device tensor of the series dtype, as a host number
        cpu_t = [torch.tensor(tv, dtype=torch.float64), torch.tensor([tv], dtype=dtype), tv][form]
        dev_t = cpu_t.to(DEV) if torch.is_tensor(cpu_t) else cpu_t
        full = lambda: _placed(np.full((B, Tn, C), SENTINEL, dtype=T), misalign)  # noqa: E731
        if control == "natural":
            wy, wm = torch.empty(B, Tn, C, dtype=dtype), torch.empty(B, Tn, C, dtype=dtype)
            double._cde_control_grad_natural(wy, wm, th(gout), th(F), th(kn), cpu_t)
            gy, gm = full(), full()
            be._cde_control_grad_natural(gy, gm, g_d, F_d, _placed(kn), dev_t)
            assert _same_bits(gy, wy.numpy()) and _same_bits(gm, wm.numpy()), (control,) + where
        else:
            want = torch.empty(B, Tn, C, dtype=dtype)
            double._cde_control_grad(want, th(gout), th(F), th(kn), cpu_t, control)
            got = full()
            be._cde_control_grad(got, g_d, F_d, _placed(kn), dev_t, control)
            assert _same_bits(got, want.numpy()), (control,) + where
    plan = be._cde_control_grad_plan(F_d, B, H, C)
    assert plan == double._cde_control_grad_plan(F_d, B, H, C), where
    return P.features(plan, B, H, C, _DT[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_control_gradient_equals_the_double_bit_for_bit(dtype):
    """The grid of tests/_cdegrad_plans.py: C below one vector, unaligned, one vector, many, more than one chunk; H with no tree, a
    short tree, the row loop; B 1 and 3; aligned and one element off 16 bytes (the scalar path); Tn 2, 3, 8, the six kinds of time and
    the three forms of time in rotation; all three controls."""
    double = GD.CdeGradDoubleBackend()
    for n, (B, H, C, mis) in enumerate(P.GRID_SHAPES):
        _check(double, dtype, B, H, C, (2, 3, 8)[(n // 2) % 3], t=n % 6, form=n % 3, misalign=mis)
    assert double.launches.count("cde_control_grad") == 2 * len(P.GRID_SHAPES)
    assert double.launches.count("cde_control_grad_natural") == len(P.GRID_SHAPES)


@pytest.mark.parametrize("row", P.TABLE, ids=P.ROW_IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_every_launch_plan_of_the_control_gradient_equals_the_double_bit_for_bit(dtype, row):
    """tests/_cdegrad_plans.py's table (B up to 2101: more batch rows than workgroups; C = 2050: beyond any on-chip table): the shape
    takes the branches the row is there for — asserted from the plan before anything is launched and again from the operands launched
    — and the kernel gives the double's bits."""
    B, H, C = row.shape
    got = P.features(_query(_DT[dtype], B, H, C, row.misalign), B, H, C, _DT[dtype])
    assert row.features <= got, (row.label, "not taken:", sorted(row.features - got))
    n = P.TABLE.index(row)
    took = _check(GD.CdeGradDoubleBackend(), dtype, B, H, C, Tn=(3, 2, 8)[n % 3], t=n % 6, form=n % 3, misalign=row.misalign,
                  controls=("cubic", "natural") if n % 2 else ("linear", "natural"))
    assert row.features <= took, (row.label, took)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_shapes_launched_reach_every_branch_of_the_plan(dtype):
    assert P.coverage_gaps(_query, _DT[dtype]) == []


@pytest.mark.parametrize("Tn", SC.TNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_coefficient_and_gather_transposes_equal_the_double_bit_for_bit(dtype, Tn):
    """1, 15 and 4100 columns (below, and beyond, one workgroup; more than one workgroup), column e carrying pattern e mod n of
    tests/_spline_cases.py so that neighbouring lanes branch differently; L = 1, 3 and 130 query times (two tiles of the table), on,
    inside and outside the knots; either cotangent alone; outputs pre-filled with a sentinel, zeros compared with their sign."""
    be, T = _hip.get_backend(), _NPT[dtype]
    for (B, C), L in zip(((1, 1), (3, 5), (82, 50)), (1, 3, 130)):
        rs = np.random.RandomState(1000 * Tn + B)
        kn, x = SC.knots(rs, Tn, T), SC.series(rs, B, Tn, C, T)
        gY, gM = rs.randn(B, Tn, C).astype(T), rs.randn(B, Tn, C).astype(T)
        want = GD.natural_coeffs_backward(gY, gM, x, kn)
        assert not want[np.isnan(x)].any()
        out = _placed(np.full(x.shape, SENTINEL, dtype=T), misalign=bool(B & 2))
        be._spline_natural_coeffs_backward(out, _placed(gY), _placed(gM), _placed(x), _placed(kn))
        assert _same_bits(out, want), ("coeffs", dtype, B, Tn, C)
        tq = np.concatenate([kn[:1], rs.uniform(kn[0] - 1.0, kn[-1] + 1.0, L - 1)]).astype(T)[:L] if L > 1 else kn[-1:]
        gval, gder = rs.randn(B, L, C).astype(T), rs.randn(B, L, C).astype(T)
        for gv, gd in ((gval, gder), (gval, None), (None, gder)):
            wy, wm = GD.natural_gather_backward(gv, gd, kn, tq, Tn)
            oy, om = (_placed(np.full(x.shape, SENTINEL, dtype=T)) for _ in range(2))
            be._spline_natural_gather_backward(oy, om, None if gv is None else _placed(gv), None if gd is None else _placed(gd),
                                               _placed(kn), _placed(tq))
            assert _same_bits(oy, wy) and _same_bits(om, wm), ("gather", dtype, B, Tn, C, L, gv is None, gd is None)


def test_a_refused_call_leaves_the_output_standing():
    be = _hip.get_backend()
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)  # noqa: E731
    F, g, kn = torch.randn(2, 3, 4, device=DEV), torch.randn(2, 3, device=DEV), torch.arange(5.0, device=DEV)
    x, gy, gm = torch.randn(2, 5, 4, device=DEV), torch.randn(2, 5, 4, device=DEV), torch.randn(2, 5, 4, device=DEV)
    gv, tq = torch.randn(2, 3, 4, device=DEV), torch.tensor([0.5, 1.5, 3.0], device=DEV)
    ws = torch.empty(2 * 2 * 5 * 4, device=DEV)
    gS, gY, gM, gS2, hY, hM = (full(2, 5, 4) for _ in range(6))
    st = be._stream(F)
    p = lambda t: t.data_ptr()  # noqa: E731
    calls = (("xde_cde_control_grad", (gS,), [p(gS), p(g), p(F), p(kn), None, 1.5, 1, 2, 3, 4, 5, 1, 0, st],
              ((1, None), (2, None), (3, None), (7, 0), (8, 0), (9, 0), (10, 1), (11, 2), (11, 3), (12, 2), (6, 2))),
             ("xde_cde_control_grad_natural", (gY, gM), [p(gY), p(gM), p(g), p(F), p(kn), None, 1.5, 1, 2, 3, 4, 5, 0, st],
              ((1, None), (2, None), (3, None), (4, None), (8, 0), (9, 0), (10, 0), (11, 1), (12, 2), (7, 2))),
             ("xde_spline_natural_coeffs_backward", (gS2,), [p(gS2), p(gy), p(gm), p(x), p(kn), p(ws), 2, 5, 4, 0, st],
              ((1, None), (2, None), (3, None), (4, None), (5, None), (6, 0), (7, 1), (8, 0), (9, 2))),
             ("xde_spline_natural_gather_backward", (hY, hM), [p(hY), p(hM), p(gv), p(gv), p(kn), p(tq), 2, 5, 3, 4, 0, st],
              ((4, None), (5, None), (6, 0), (7, 1), (8, 0), (9, 0), (10, 2))))
    for sym, dsts, good, bad in calls:
        fn = getattr(be.lib, sym)
        for i, v in bad:
            args = list(good)
            args[i] = v
            assert fn(*args) == _hip.XDE_EBADARG, (sym, i, v)
            assert be.lib.xde_last_error().decode().startswith(sym + ":")
        torch.cuda.synchronize()
        assert all(bool((d == SENTINEL).all()) for d in dsts), sym
        assert fn(*good) == _hip.XDE_OK
        torch.cuda.synchronize()
        assert not any(bool((d == SENTINEL).any()) for d in dsts), sym


@pytest.mark.parametrize("control", ["natural", "cubic", "linear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_autograd_wrapper_gives_the_control_its_gradient(dtype, control):
    """CdeControlContractFn.apply and its backward on torch's allocations: out and gF are CdeContractFn's bits (the existing
    launches), the series / (Y, M) gradient is the double's; without requires_grad on the control no control-gradient launch runs
    (the gradient stays None)."""
    from paddlexde_amd.xde.base_cde import CdeContractFn, CdeControlContractFn

    double, T = GD.CdeGradDoubleBackend(), _NPT[dtype]
    B, H, C, Tn = 70, 33, 8, 9
    rs = np.random.RandomState(B)
    kn = SC.knots(rs, Tn, T) if control == "natural" else np.arange(Tn, dtype=T)
    Y, M = SD.natural_coeffs(SC.series(rs, B, Tn, C, T), kn)
    F, gout = rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    tv = float(kn[3] + 0.5 * (kn[4] - kn[3]))
    t_d = torch.tensor(tv, dtype=torch.float64, device=DEV)
    coef = (lambda: th(M).to(DEV)) if control == "natural" else (lambda: None)

    F0 = th(F).to(DEV).requires_grad_(True)
    out0 = CdeContractFn.apply(F0, th(Y).to(DEV), th(kn).to(DEV), t_d, control, coef())
    out0.backward(th(gout).to(DEV))

    F1, Y1, M1 = th(F).to(DEV).requires_grad_(True), th(Y).to(DEV).requires_grad_(True), coef()
    if M1 is not None:
        M1.requires_grad_(True)
    out1 = CdeControlContractFn.apply(F1, Y1, th(kn).to(DEV), t_d, control, M1)
    out1.backward(th(gout).to(DEV))
    assert torch.equal(out1.detach(), out0.detach()) and torch.equal(F1.grad, F0.grad)
    if control == "natural":
        wy, wm = torch.empty(B, Tn, C, dtype=dtype), torch.empty(B, Tn, C, dtype=dtype)
        double._cde_control_grad_natural(wy, wm, th(gout), th(F), th(kn), tv)
        assert _same_bits(Y1.grad, wy.numpy()) and _same_bits(M1.grad, wm.numpy())
    else:
        want = torch.empty(B, Tn, C, dtype=dtype)
        double._cde_control_grad(want, th(gout), th(F), th(kn), tv, control)
        assert _same_bits(Y1.grad, want.numpy())

    F2, Y2 = th(F).to(DEV).requires_grad_(True), th(Y).to(DEV)
    CdeControlContractFn.apply(F2, Y2, th(kn).to(DEV), t_d, control, coef()).backward(th(gout).to(DEV))
    assert torch.equal(F2.grad, F0.grad) and Y2.grad is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_differentiable_spline_on_torchs_allocations(dtype):
    """NaturalCubicSpline(differentiable=True): Y, M and evaluate / derivative are the bits of the default spline; the series
    gradient through evaluate and derivative is the double's (gather transpose, then coefficient transpose)."""
    T = _NPT[dtype]
    rs = np.random.RandomState(11)
    kn, x = SC.knots(rs, 9, T), SC.series(rs, 3, 9, 5, T)
    tq = np.asarray([kn[0], 0.5 * (kn[2] + kn[3]), kn[-1]], dtype=T)
    series = th(x).to(DEV).requires_grad_(True)
    X0, X1 = NaturalCubicSpline(th(x).to(DEV), th(kn).to(DEV)), NaturalCubicSpline(series, th(kn).to(DEV), differentiable=True)
    assert torch.equal(X0._series, X1._series.detach()) and torch.equal(X0._coef, X1._coef.detach())
    val, der = X1.evaluate(th(tq)), X1.derivative(th(tq))
    assert torch.equal(val.detach(), X0.evaluate(th(tq))) and torch.equal(der.detach(), X0.derivative(th(tq)))
    gval, gder = rs.randn(*val.shape).astype(T), rs.randn(*val.shape).astype(T)
    (val * th(gval).to(DEV)).sum().backward(retain_graph=True)
    gy, gm = GD.natural_gather_backward(gval, None, kn, tq, 9)
    assert _same_bits(series.grad, GD.natural_coeffs_backward(gy, gm, x, kn))
    series.grad = None
    (der * th(gder).to(DEV)).sum().backward()
    gy, gm = GD.natural_gather_backward(None, gder, kn, tq, 9)
    assert _same_bits(series.grad, GD.natural_coeffs_backward(gy, gm, x, kn))


@pytest.mark.parametrize("adjoint", [False, True])
def test_cde_demo_trains_an_encoder_through_the_control(adjoint):
    """examples/cde_demo.py --control natural --irregular --missing 0.3 --encoder for 8 iterations, through the steps and through the
    adjoint: the loss falls and the encoder's parameters have moved (they get their gradient through the control alone)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=8, n=32, length=16, adjoint=adjoint, log_every=0, control="natural", irregular=True, missing=0.3,
                            encoder=True)
    assert len(losses) == 8 and all(np.isfinite(losses)) and sum(losses[-3:]) < sum(losses[:3]), losses


def test_cde_demo_encoder_gets_a_gradient_on_the_cubic_control():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=4, n=16, length=8, log_every=0, control="cubic", encoder=True)
    assert len(losses) == 4 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
