"""NaturalCubicSpline on the GPU: the coefficient build, the gather and both natural contraction kernels against the numpy double
(tests/_spline_double.py) bit for bit — the coefficients over B x Tn x C with the patterns of missing values mixed across the columns
of one launch; the gather on, inside and outside the knots, vector and scalar, with and without `der`, beyond one table tile; the
contractions over every shape of tests/_cde_plans.py (each table row held to its plan, the union held to full coverage), with every
form of time and on the scalar path — then the identity field against X.derivative(t), refused calls leaving their outputs standing,
the end-to-end cases of tests/_spline_e2e.py on the HIP backend, the captured adjoint dynamics against the eager one, and the demo."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.interpolation import NaturalCubicSpline
from paddlexde_amd.xde.base_cde import CdeContractFn

from . import _cde_plans as P
from . import _spline_cases as SC
from . import _spline_double as SD
from ._cde_cases import _field, _grads
from ._spline_e2e import *  # noqa: F401,F403
from ._spline_e2e import Dopri5, cdeint_adjoint

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
    """The captured adjoint dynamics and the demo's models die in reference cycles that own captured HIP graphs.  They are collected
    here, outside any recording (utils/graphed.py parks an owner that dies inside one until the recording ends), so that a later
    test's collection does not come upon them."""
    yield
    gc.collect()


def _placed(x, misalign=False):
    """``x`` (numpy) on the device, contiguous, 16-byte aligned or one element off it."""
    flat = torch.empty(x.size + 1, dtype=th(x).dtype, device=DEV)
    view = (flat[1:] if misalign else flat[:-1]).view(x.shape)
    view.copy_(th(x))
    assert (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


# ----------------------------------------------------------------------------------------------
# the coefficient build
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn", SC.TNS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_coefficients_equal_the_double_bit_for_bit(dtype, Tn):
    """B in {1, 3, 70} x C in {1, 3, 4, 5, 64, 260}: below, at and beyond one workgroup of columns (70 x 260 = 72 of them); column
    e = b C + c carries pattern e mod n of tests/_spline_cases.py, so neighbouring lanes take different branches of every sweep."""
    be, T = _hip.get_backend(), _NPT[dtype]
    for B in (1, 3, 70):
        for C in (1, 3, 4, 5, 64, 260):
            rs = np.random.RandomState(1000 * Tn + 10 * C + B)
            kn, x = SC.knots(rs, Tn, T), SC.series(rs, B, Tn, C, T)
            Yw, Mw = SD.natural_coeffs(x, kn)
            assert not np.isnan(Yw).any() and not np.isnan(Mw).any()
            Y, M = _placed(np.full(x.shape, SENTINEL, dtype=T)), _placed(np.full(x.shape, SENTINEL, dtype=T), misalign=bool(B & 2))
            be._spline_natural_coeffs(Y, M, _placed(x), _placed(kn))
            assert np.array_equal(Y.cpu().numpy(), Yw) and np.array_equal(M.cpu().numpy(), Mw), (dtype, B, Tn, C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_column_with_nothing_observed_is_all_nan_and_its_neighbours_are_not(dtype):
    """What the header defines for the C entry point (the Python class refuses such a series before it launches)."""
    be, T = _hip.get_backend(), _NPT[dtype]
    rs = np.random.RandomState(2)
    kn, x = SC.knots(rs, 9, T), SC.series(rs, 3, 9, 5, T)
    x[1, :, 2] = np.nan
    Yw, Mw = SD.natural_coeffs(x, kn)
    Y, M = _placed(np.zeros(x.shape, dtype=T)), _placed(np.zeros(x.shape, dtype=T))
    be._spline_natural_coeffs(Y, M, _placed(x), _placed(kn))
    Y, M = Y.cpu().numpy(), M.cpu().numpy()
    assert np.isnan(Y[1, :, 2]).all() and np.isnan(M[1, :, 2]).all() and np.isnan(Y).sum() == np.isnan(M).sum() == 9
    assert np.array_equal(Y, Yw, equal_nan=True) and np.array_equal(M, Mw, equal_nan=True)
    with pytest.raises(ValueError, match="no observed"):
        NaturalCubicSpline(th(x).to(DEV), th(kn).to(DEV))


# ----------------------------------------------------------------------------------------------
# the gather
# ----------------------------------------------------------------------------------------------
def _times(kn):
    """the first knot, an interior knot (the first where there is none), the last knot; inside the first and the last interval;
    before the first and beyond the last knot"""
    Tn = len(kn)
    k = kn.astype(np.float64)
    return np.asarray([k[0], k[(Tn - 1) // 2], k[-1], k[0] + 0.3 * (k[1] - k[0]), k[-1] - 0.25 * (k[-1] - k[-2]),
                       k[0] - 0.75 * (k[1] - k[0]), k[-1] + 1.5 * (k[-1] - k[-2])]).astype(kn.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_gather_equals_the_double_bit_for_bit(dtype):
    """D below one vector, unaligned, one vector, many; the scalar kernel on operands one element off 16 bytes; `der` absent; 130 query
    times (two tiles of the on-chip table)."""
    be, T = _hip.get_backend(), _NPT[dtype]
    n = 0
    for outer, Tn, D in ((1, 2, 1), (3, 3, 3), (3, 4, 4), (2, 9, 5), (3, 33, 64), (2, 9, 260), (70, 4, 8)):
        rs = np.random.RandomState(100 * Tn + D)
        kn, x = SC.knots(rs, Tn, T), SC.series(rs, outer, Tn, D, T)
        Yw, Mw = SD.natural_coeffs(x, kn)
        tq = _times(kn)
        if D == 5:
            tq = np.concatenate([tq, np.linspace(kn[0] - 1, kn[-1] + 1, 123).astype(T)])
        vw, dw = SD.natural_gather(Yw, Mw, kn, tq)
        for mis, with_der in ((False, True), (True, True), (False, False)):
            val = _placed(np.full(vw.shape, SENTINEL, dtype=T), mis)
            der = _placed(np.full(vw.shape, SENTINEL, dtype=T), mis) if with_der else None
            be._spline_natural_gather(val, der, _placed(Yw, mis), _placed(Mw, mis), _placed(kn), _placed(tq))
            assert np.array_equal(val.cpu().numpy(), vw), (dtype, outer, Tn, D, mis)
            assert der is None or np.array_equal(der.cpu().numpy(), dw), (dtype, outer, Tn, D, mis)
            n += 1
        # the class: the same launches on torch's allocations
        X = NaturalCubicSpline(th(x).to(DEV), th(kn).to(DEV))
        assert np.array_equal(X._series.cpu().numpy(), Yw) and np.array_equal(X._coef.cpu().numpy(), Mw)
        assert np.array_equal(X.evaluate(th(tq)).cpu().numpy(), vw) and np.array_equal(X.derivative(th(tq)).cpu().numpy(), dw)
    assert n == 21


# ----------------------------------------------------------------------------------------------
# the contraction kernels
# ----------------------------------------------------------------------------------------------
def _cde_times(knots, Tn):
    """tests/test_gpu_cde.py's eight kinds of time"""
    m = (Tn - 1) // 2
    return [float(knots[0]), float(knots[1 if Tn > 2 else 0]), float(knots[-1] - 0.25 * (knots[-1] - knots[-2])), float(knots[-1]),
            float(knots[0] + 0.25 * (knots[1] - knots[0])), float(knots[m] + 0.5 * (knots[m + 1] - knots[m])),
            float(knots[0] - 0.75 * (knots[1] - knots[0])), float(knots[-1] + 1.5 * (knots[-1] - knots[-2]))]


def _query(backward, dt, B, H, C, misalign):
    big = torch.empty(8, dtype=torch.float32 if dt == "f32" else torch.float64, device=DEV)[1 if misalign else 0:]
    assert (big.data_ptr() % 16 != 0) == bool(misalign)
    return _hip.get_backend()._cde_plan(backward, big, B, H, C)


def _check(double, dtype, B, H, C, Tn, t, form, misalign=False, seed=0):
    """Both natural kernels against the double, bit for bit; returns the branches (tests/_cde_plans.py: ``features``) the two launches
    took.  Small controls are real coefficients (a series with missing values through the double's build); beyond 2^16 columns Y and M
    are random rows — the contraction reads four rows and does not care where they came from."""
    be, T = _hip.get_backend(), _NPT[dtype]
    rs = np.random.RandomState(seed + 1000 * C + 10 * H + B)
    kn = SC.knots(rs, Tn, T)
    if B * C <= 1 << 16:
        Y, M = SD.natural_coeffs(SC.series(rs, B, Tn, C, T), kn)
    else:
        Y, M = rs.randn(B, Tn, C).astype(T), rs.randn(B, Tn, C).astype(T)
    F, gout = rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    tv = _cde_times(kn, Tn)[t]
    want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
    cpu_t = [torch.tensor(tv, dtype=torch.float64), torch.tensor([tv], dtype=dtype), tv][form]
    double._cde_contract_natural(want, th(F), th(Y), th(M), th(kn), cpu_t)
    double._cde_contract_natural_backward(gwant, th(gout), th(Y), th(M), th(kn), cpu_t)
    Y_d, M_d, kn_d = _placed(Y), _placed(M), _placed(kn)
    out = _placed(np.full((B, H), SENTINEL, dtype=T), misalign)
    gF = _placed(np.full((B, H, C), SENTINEL, dtype=T), misalign)
    # the time as a float64 device scalar (also with a float32 series), as a [1] device tensor of the series dtype, as a host number
    td = [torch.tensor(tv, dtype=torch.float64, device=DEV), torch.tensor([tv], dtype=dtype, device=DEV), tv][form]
    F_d = _placed(F, misalign)
    be._cde_contract_natural(out, F_d, Y_d, M_d, kn_d, td)
    be._cde_contract_natural_backward(gF, _placed(gout, misalign), Y_d, M_d, kn_d, td)
    where = (dtype, B, H, C, Tn, tv, form, misalign)
    assert np.array_equal(out.cpu().numpy(), want.numpy()), where
    assert np.array_equal(gF.cpu().numpy(), gwant.numpy()), where
    return P.features(be._cde_plan(False, F_d, B, H, C), B, H, C, False), P.features(be._cde_plan(True, gF, B, H, C), B, H, C, True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_natural_kernels_equal_the_double_bit_for_bit(dtype):
    """The grid of tests/_cde_plans.py (C below one vector, unaligned, one vector, many, more than one team pass; H and B around a
    workgroup's teams; aligned and one element off 16 bytes: the scalar path), Tn 2, 3, 9, all eight kinds of time and the three forms
    of time in rotation; then its grouped shapes and the rows longer than the on-chip table."""
    double = SD.SplineDoubleBackend()
    for n, (B, H, C, mis) in enumerate(P.GRID_SHAPES):
        Tn = (2, 3, 9)[(n // 2) % 3]
        for k in range(2):
            _check(double, dtype, B, H, C, Tn, t=(n + 4 * k) % 8, form=(n + k) % 3, misalign=mis)
    for n, (B, H, C, mis) in enumerate(P.ITEM_SHAPES + P.TABLE_SHAPES):
        _check(double, dtype, B, H, C, (9, 3, 2, 3, 4)[n], t=(2, 5, 1, 4, 7)[n], form=n % 3, misalign=mis)
    n = 2 * len(P.GRID_SHAPES) + len(P.ITEM_SHAPES) + len(P.TABLE_SHAPES)
    assert double.launches.count("cde_contract_natural") == double.launches.count("cde_contract_natural_backward") == n


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_three_forms_of_time_give_the_same_bits_on_the_natural_control(dtype, C):
    """One shape and one time under all three forms of time (the test above rotates the forms over its shapes): B, H, Tn = 2, 3, 4 on
    the unit grid, C = 5 (the scalar tail) and C = 8 (the vector path), at 1.375 (inside an interval, exact in float32) and 2.0 (on a
    knot).  Both natural launches give identical bits whether the time is a float64 device element, an element of the series dtype or a
    Python number, and they are the double's."""
    be, double, T = _hip.get_backend(), SD.SplineDoubleBackend(), _NPT[dtype]
    B, H, Tn = 2, 3, 4
    rs = np.random.RandomState(40 + C)
    kn = np.arange(Tn).astype(T)
    Y, M = SD.natural_coeffs(rs.randn(B, Tn, C).astype(T), kn)
    F, gout = rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    Y_d, M_d, kn_d, F_d, gout_d = (_placed(x) for x in (Y, M, kn, F, gout))
    assert be._cde_plan(False, F_d, B, H, C)["vec"] == be._cde_plan(True, F_d, B, H, C)["vec"] == int(C == 8)
    for tv in (1.375, 2.0):
        got = []
        for form in range(3):
            cpu_t = [torch.tensor(tv, dtype=torch.float64), torch.tensor([tv], dtype=dtype), tv][form]
            want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
            double._cde_contract_natural(want, th(F), th(Y), th(M), th(kn), cpu_t)
            double._cde_contract_natural_backward(gwant, th(gout), th(Y), th(M), th(kn), cpu_t)
            out, gF = _placed(np.full((B, H), SENTINEL, dtype=T)), _placed(np.full((B, H, C), SENTINEL, dtype=T))
            td = [torch.tensor(tv, dtype=torch.float64, device=DEV), torch.tensor([tv], dtype=dtype, device=DEV), tv][form]
            be._cde_contract_natural(out, F_d, Y_d, M_d, kn_d, td)
            be._cde_contract_natural_backward(gF, gout_d, Y_d, M_d, kn_d, td)
            got.append((out.cpu().numpy(), gF.cpu().numpy()))
            where = (dtype, C, tv, form)
            assert np.array_equal(got[-1][0], want.numpy()) and np.array_equal(got[-1][1], gwant.numpy()), where
            assert np.array_equal(got[-1][0], got[0][0]) and np.array_equal(got[-1][1], got[0][1]), where


@pytest.mark.parametrize("row", P.TABLE, ids=P.ROW_IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_every_launch_plan_equals_the_double_bit_for_bit_on_the_natural_control(dtype, row):
    """tests/_cde_plans.py's table: the shape takes the branches the row is there for (the plan does not depend on the control) —
    asserted from the launch plan before anything is launched and again from the operands launched — and both natural kernels give
    the double's bits."""
    (B, H, C), fwd, bwd = P.row_case(row, _DT[dtype])
    for backward, want in ((False, fwd), (True, bwd)):
        got = P.features(_query(backward, _DT[dtype], B, H, C, row.misalign), B, H, C, backward)
        assert want <= got, (row.label, "backward" if backward else "forward", "not taken:", sorted(want - got))
    n = P.TABLE.index(row)
    took = _check(SD.SplineDoubleBackend(), dtype, B, H, C, Tn=(3, 2, 9)[n % 3] if C < 2048 else 3, t=n % 8, form=n % 3, misalign=row.misalign)
    assert fwd <= took[0] and bwd <= took[1], (row.label, took)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_shapes_launched_on_the_natural_control_reach_every_reachable_plan(dtype):
    """The two tests above launch every shape of ``P.suite_shapes``: per direction all six instantiations, a second work item in each
    family, a second row pass in each path, a short last slice, a short last group and the streaming loads."""
    assert P.coverage_gaps(_query, _DT[dtype]) == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_autograd_wrapper_on_the_natural_control(dtype):
    """CdeContractFn.apply with the coefficient operand and its backward, on torch's allocations, at a grouped shape: the double's
    bits, and gradient to F only."""
    double, T = SD.SplineDoubleBackend(), _NPT[dtype]
    B, H, C, Tn = 2049, 3, 8, 9
    rs = np.random.RandomState(B)
    kn = SC.knots(rs, Tn, T)
    Y, M = SD.natural_coeffs(SC.series(rs, B, Tn, C, T), kn)
    F, gout = rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    tv = float(kn[3] + 0.5 * (kn[4] - kn[3]))
    want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
    double._cde_contract_natural(want, th(F), th(Y), th(M), th(kn), tv)
    double._cde_contract_natural_backward(gwant, th(gout), th(Y), th(M), th(kn), tv)
    F_d = th(F).to(DEV).requires_grad_(True)
    Y_d, M_d = th(Y).to(DEV).requires_grad_(True), th(M).to(DEV).requires_grad_(True)
    out = CdeContractFn.apply(F_d, Y_d, th(kn).to(DEV), torch.tensor(tv, dtype=torch.float64, device=DEV), "natural", M_d)
    out.backward(th(gout).to(DEV))
    assert np.array_equal(out.detach().cpu().numpy(), want.numpy()) and np.array_equal(F_d.grad.cpu().numpy(), gwant.numpy())
    assert Y_d.grad is None and M_d.grad is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_identity_field_returns_the_natural_splines_derivative(dtype):
    """H = C and F[b] = I: the output is X.derivative(t), the `der` of xde_spline_natural_gather, bit for bit (not through the double)
    — at every kind of time, so the convention outside the knots is held to the spline's too."""
    be, T = _hip.get_backend(), _NPT[dtype]
    for C, Tn in ((1, 2), (3, 3), (5, 9), (64, 9), (260, 33)):
        rs = np.random.RandomState(5 + C)
        X = NaturalCubicSpline(th(SC.series(rs, 3, Tn, C, T)).to(DEV), th(SC.knots(rs, Tn, T)).to(DEV))
        F = torch.eye(C, dtype=dtype, device=DEV).expand(3, C, C).contiguous()
        for tv in _cde_times(X._t.cpu().numpy(), Tn):
            t = torch.tensor([tv], dtype=dtype, device=DEV)
            out = torch.full((3, C), SENTINEL, dtype=dtype, device=DEV)
            be._cde_contract_natural(out, F, X._series, X._coef, X._t, t)
            assert torch.equal(out, X.derivative(t)[:, 0, :]), (C, Tn, tv)


def test_a_refused_call_leaves_the_output_standing():
    be = _hip.get_backend()
    Y, M, kn = torch.randn(2, 5, 4, device=DEV), torch.randn(2, 5, 4, device=DEV), torch.arange(5.0, device=DEV)
    F, g, tq = torch.randn(2, 3, 4, device=DEV), torch.randn(2, 3, device=DEV), torch.tensor([0.5, 1.5, 3.0], device=DEV)
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)  # noqa: E731
    out, gF, Yo, Mo, val, der = full(2, 3), full(2, 3, 4), full(2, 5, 4), full(2, 5, 4), full(2, 3, 4), full(2, 3, 4)
    st = be._stream(out)
    p = lambda x: x.data_ptr()  # noqa: E731
    calls = (("xde_cde_contract_natural", (out,), [p(out), p(F), p(Y), p(M), p(kn), None, 1.5, 1, 2, 3, 4, 5, 0, st],
              ((1, None), (2, None), (3, None), (4, None), (8, 0), (9, 0), (10, 0), (11, 1), (12, 2), (7, 2))),
             ("xde_cde_contract_natural_backward", (gF,), [p(gF), p(g), p(Y), p(M), p(kn), None, 1.5, 1, 2, 3, 4, 5, 0, st],
              ((1, None), (2, None), (3, None), (4, None), (8, 0), (9, 0), (10, 0), (11, 1), (12, 2), (7, 2))),
             ("xde_spline_natural_coeffs", (Yo, Mo), [p(Yo), p(Mo), p(Y), p(kn), 2, 5, 4, 0, st],
              ((2, None), (3, None), (4, 0), (5, 1), (6, 0), (7, 2))),
             ("xde_spline_natural_gather", (val, der), [p(val), p(der), p(Y), p(M), p(kn), p(tq), 2, 5, 3, 4, 0, st],
              ((2, None), (3, None), (4, None), (5, None), (6, 0), (7, 1), (8, 0), (9, 0), (10, 2))))
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


def test_the_captured_adjoint_dynamics_give_the_eager_gradients_bit_for_bit(dev):
    """cdeint_adjoint with adjoint_options["graph_func"] = True (the natural contraction and its cotangent inside a captured HIP graph,
    the time read from device memory at every replay) against graph_func = False."""
    series, kn, _, z0 = (th(x).to(dev) for x in SC.cde_problem(torch.float64))
    X = NaturalCubicSpline(series, kn)
    ts = kn[[0, 2, 5, 7]]
    field = _field(dev)

    def grads(captured):
        loss = lambda z: cdeint_adjoint(field, X, z, ts, solver=Dopri5, adjoint_options={"graph_func": captured}).square().sum()  # noqa: E731
        return _grads(loss, field, z0)

    eager, captured = grads(False), grads(True)
    for a, b in zip(eager, captured):
        assert np.abs(a).max() > 0 and np.array_equal(a, b)


@pytest.mark.parametrize("adjoint", [False, True])
def test_cde_demo_loss_falls_on_irregular_partly_observed_spirals(adjoint):
    """examples/cde_demo.py --control natural --irregular --missing 0.3 for 8 iterations, through the steps and through the adjoint."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=8, n=32, length=16, adjoint=adjoint, log_every=0, control="natural", irregular=True, missing=0.3)
    assert all(np.isfinite(losses)) and sum(losses[-3:]) < 0.9 * sum(losses[:3]), losses
