"""The gradient with respect to the control path of cdeint, without a GPU: the numpy double of include/xde_hip_cdegrad.h against the
float64 Jacobian oracle (tests/_cdegrad_oracle.py), the structure of the outputs (exact zeros, the end rule, full overwrite), the
end-to-end gradients on the double (tests/_cdegrad_e2e.py), the default path untouched, every refusal by message, the C ABI of the
header, and the plan table."""
import types

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import AdjointProblem, cdeint, cdeint_adjoint
from paddlexde_amd.interpolation import BezierSpline, CubicHermiteSpline, LinearInterpolation, NaturalCubicSpline
from paddlexde_amd.solver import RK4, Dopri5
from paddlexde_amd.utils.ode_utils import _rms_norm
from paddlexde_amd.xde import base_cde
from paddlexde_amd.xde.base_cde import CDEField, CdeContractFn

from . import _cde_oracle as CO
from . import _cdegrad_double as GD
from . import _cdegrad_oracle as GO
from . import _cdegrad_plans as GP
from . import _spline_cases as SC
from ._cde_cases import B, C, H, T, _field, inputs
from ._cdegrad_e2e import *  # noqa: F401,F403
from .test_srk_host import _entry

_U = {np.float32: 2.0**-24, np.float64: 2.0**-53}
CS, HS = (1, 3, 5, 64), (1, 7, 33, 512)

# The double against the oracle.  Every output element is a short sum of terms (Jacobian entry x cotangent); its error is measured in
# units of u x (the sum of the absolute values of its terms), u = the dtype's unit roundoff.  Phase 1 of (a) is a length-H sum of
# products in SOME order: the standard bound gamma_H = H u / (1 - H u) holds and is asserted as derived.  For the rest — (a)'s scatter
# ("a": the weights are a handful of ops on the knots and the time), (b) and (c) — MEASURED is the worst figure over this module's inputs
# (every Tn of SC.TNS x every pattern of SC.PATTERNS that fits, knot spacings 0.25 .. 4, times on every knot and at 0.25 / 0.5 / 0.9 of
# every interval) with the committed double on the CPU, and the test asserts 4 x that, as tests/test_spline_host.py does.  For (a) the
# figure is in units of (gamma_H + u) x (the largest row weight of the time) x sum_h |gout F|: the sum's own bound, plus one u for the
# weight (see _widest).
MEASURED = {np.float32: {"a": 12.9, "b": 3.58, "c": 21.1}, np.float64: {"a": 5.37, "b": 10.0, "c": 31.0}}
BOUND = {T_: {k: 4.0 * v for k, v in m.items()} for T_, m in MEASURED.items()}


@pytest.fixture
def dev():
    _hip._set_backend_for_testing(GD.CdeGradDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def _times(kn):
    k64 = kn.astype(np.float64)
    return np.concatenate([k64] + [k64[:-1] + f * np.diff(k64) for f in (0.25, 0.5, 0.9)]).astype(kn.dtype)


def _rel(got, want, scale):
    """max |got - want| / scale over the elements with a non-zero scale; elements with scale 0 must be exactly zero."""
    assert not got[scale == 0].any()
    live = scale > 0
    return float((np.abs(got.astype(np.float64) - want)[live] / scale[live]).max()) if live.any() else 0.0


def _widest(scale):
    """The scale of the row with the largest weight, for every row of a time's gradient [B, Tn, C]: the row weights of one time are
    sums and differences of a few shared entries (a0 - b0 - b1, ...), so a row's rounding error is a multiple of u x the largest of
    them, not of the row's own — possibly cancelled — weight."""
    return scale.max(axis=1, keepdims=True) * np.ones_like(scale)


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_phase_one_of_the_double_is_within_the_bound_of_a_length_h_sum(T_):
    rs = np.random.RandomState(5)
    for H_ in HS:
        for C_ in CS:
            gout, F = rs.randn(3, H_).astype(T_), rs.randn(3, H_, C_).astype(T_)
            want, scale = GO.gdx(gout, F)
            got = GD.gdx_in_header_order(gout, F)
            assert np.abs(got - want).max() <= (CO.gamma(H_, T_) * scale).max() and (np.abs(got - want) <= CO.gamma(H_, T_) * scale).all()


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_the_control_gradient_of_the_double_against_the_oracle(T_):
    """(a), the three controls: every Tn, every time of ``_times`` (the linear / cubic controls on the unit grid — their scale
    conventions are exact there — and on the irregular knots, where the oracle's classes carry the same conventions)."""
    u, worst_a = _U[T_], 0.0
    rs = np.random.RandomState(6)
    n = 0
    for Tn in SC.TNS:
        for kn in (SC.knots(rs, Tn, T_), np.arange(Tn, dtype=T_)):
            H_, C_ = HS[n % 4], CS[(n // 2) % 4]
            gout, F = rs.randn(2, H_).astype(T_), rs.randn(2, H_, C_).astype(T_)
            for tau in _times(kn):
                n += 1
                unit = CO.gamma(H_, T_) + u
                for method in ("linear", "cubic"):
                    want, scale = GO.control_grad(gout, F, kn, float(tau), method)
                    worst_a = max(worst_a, _rel(GD.control_grad(gout, F, kn, tau, method), want, _widest(scale) * unit))
                wy, wm, sy, sm = GO.control_grad_natural(gout, F, kn, float(tau))
                gy, gm = GD.control_grad_natural(gout, F, kn, tau)
                worst_a = max(worst_a, _rel(gy, wy, _widest(sy) * unit), _rel(gm, wm, _widest(sm) * unit))
    print("{}: (a) worst = {:.3g} in units of (gamma_H + u) x sum|terms|; asserted {}".format(T_.__name__, worst_a, BOUND[T_]["a"]))
    assert n > 100 and worst_a <= BOUND[T_]["a"]


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_the_coefficient_and_gather_transposes_of_the_double_against_the_oracle(T_):
    u, worst_b, worst_c, n = _U[T_], 0.0, 0.0, 0
    for Tn in SC.TNS:
        for pattern in SC.PATTERNS:
            if SC.missing(pattern, Tn) is None:
                continue
            n += 1
            rs = np.random.RandomState(100 * Tn + SC.PATTERNS.index(pattern))
            kn = SC.knots(rs, Tn, T_)
            x = SC.series(rs, 3, Tn, 5, T_, patterns=(pattern,))
            gY, gM = rs.randn(*x.shape).astype(T_), rs.randn(*x.shape).astype(T_)
            want, scale = GO.coeffs_backward(gY, gM, x, kn)
            got = GD.natural_coeffs_backward(gY, gM, x, kn)
            assert not got[np.isnan(x)].any() and not np.signbit(got[np.isnan(x)]).any()
            worst_b = max(worst_b, _rel(got, want, scale * u))
            tq = _times(kn)
            gval, gder = rs.randn(3, len(tq), 5).astype(T_), rs.randn(3, len(tq), 5).astype(T_)
            for gv, gd in ((gval, gder), (gval, None), (None, gder)):
                wy, wm, sy, sm = GO.gather_backward(gv, gd, kn, tq)
                gy, gm = GD.natural_gather_backward(gv, gd, kn, tq, Tn)
                worst_c = max(worst_c, _rel(gy, wy, sy * u), _rel(gm, wm, sm * u))
    print("{}: {} cases, worst in units of u x sum|terms|: (b) {:.3g}, (c) {:.3g}; asserted {}".format(
        T_.__name__, n, worst_b, worst_c, BOUND[T_]))
    assert n == 30 and worst_b <= BOUND[T_]["b"] and worst_c <= BOUND[T_]["c"]


# ----------------------------------------------------------------------------------------------
# structure
# ----------------------------------------------------------------------------------------------
def _plus_zero(a):
    return not a.any() and not np.signbit(a).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_outputs_are_fully_overwritten_and_zero_outside_the_rows_read(dev, dtype):
    be = _hip.get_backend()
    T_ = np.float32 if dtype == torch.float32 else np.float64
    rs = np.random.RandomState(2)
    Tn = 9
    kn = torch.from_numpy(SC.knots(rs, Tn, T_))
    gout, F = torch.from_numpy(rs.randn(3, 7).astype(T_)), torch.from_numpy(rs.randn(3, 7, 5).astype(T_))
    tv = 0.5 * float(kn[3] + kn[4])  # inside interval 3: the linear control reads rows 3, 4; the cubic 3, 4, 5; the natural 3, 4
    for method, rows in (("linear", (3, 4)), ("cubic", (3, 4, 5))):
        out = torch.full((3, Tn, 5), float("nan"), dtype=dtype)
        be._cde_control_grad(out, gout, F, kn, tv, method)
        o = out.numpy()
        idle = [k for k in range(Tn) if k not in rows]
        assert _plus_zero(o[:, idle]) and np.isfinite(o).all() and all(o[:, k].any() for k in rows)
    gY, gM = (torch.full((3, Tn, 5), float("nan"), dtype=dtype) for _ in range(2))
    be._cde_control_grad_natural(gY, gM, gout, F, kn, torch.tensor(tv, dtype=torch.float64))
    idle = [k for k in range(Tn) if k not in (3, 4)]
    for o in (gY.numpy(), gM.numpy()):
        assert _plus_zero(o[:, idle]) and np.isfinite(o).all() and o[:, 3].any() and o[:, 4].any()
    # (b): unobserved entries exactly +0; a leading-NaN column sends its first row's cotangent to its first observed entry
    x = SC.series(rs, 2, Tn, 7, T_)
    gy, gm = rs.randn(2, Tn, 7).astype(T_), rs.randn(2, Tn, 7).astype(T_)
    out = torch.full((2, Tn, 7), float("nan"), dtype=dtype)
    be._spline_natural_coeffs_backward(out, torch.from_numpy(gy), torch.from_numpy(gm), torch.from_numpy(x), kn)
    o = out.numpy()
    assert np.isfinite(o).all() and _plus_zero(o[np.isnan(x)])
    lead = np.full((1, Tn, 1), 1.0, dtype=T_)
    lead[0, :2, 0] = np.nan
    only_first = np.zeros((1, Tn, 1), dtype=T_)
    only_first[0, 0, 0] = 3.0  # dL/dY_0 = 3, nothing else: Y_0 = y_2 by the end rule, and rows 0, 1 are flat
    out = torch.full((1, Tn, 1), float("nan"), dtype=dtype)
    be._spline_natural_coeffs_backward(out, torch.from_numpy(only_first), torch.zeros(1, Tn, 1, dtype=dtype), torch.from_numpy(lead), kn)
    want = np.zeros(Tn, dtype=T_)
    want[2] = 3.0
    assert np.array_equal(out.numpy()[0, :, 0], want)
    # (c): rows outside the queries' intervals +0, outputs fully overwritten, either cotangent alone
    tq = torch.from_numpy(np.asarray([0.5 * float(kn[5] + kn[6])], dtype=T_))
    g = torch.from_numpy(rs.randn(2, 1, 3).astype(T_))
    for gv, gd in ((g, g), (g, None), (None, g)):
        gY, gM = (torch.full((2, Tn, 3), float("nan"), dtype=dtype) for _ in range(2))
        be._spline_natural_gather_backward(gY, gM, gv, gd, kn, tq)
        for o in (gY.numpy(), gM.numpy()):
            assert _plus_zero(o[:, [k for k in range(Tn) if k not in (5, 6)]]) and np.isfinite(o).all() and o[:, 5].any()


def test_the_gather_transpose_of_an_identity_contraction_is_the_control_gradient(dev):
    """H = C, F = I: gdX = gout, and (a) for the natural control is then (c) for the cotangent of ``der`` alone: the same bits (one
    statement of the weights)."""
    be = _hip.get_backend()
    rs = np.random.RandomState(3)
    kn = torch.from_numpy(SC.knots(rs, 8, np.float64))
    gout = torch.from_numpy(rs.randn(B, C))
    F = torch.eye(C, dtype=torch.float64).expand(B, C, C).contiguous()
    for tv in (float(kn[0]), float(kn[3]), 0.5 * float(kn[3] + kn[4]), float(kn[-1])):
        gY, gM, hY, hM = (torch.empty(B, 8, C, dtype=torch.float64) for _ in range(4))
        be._cde_control_grad_natural(gY, gM, gout, F, kn, tv)
        be._spline_natural_gather_backward(hY, hM, None, gout[:, None, :].contiguous(), kn, torch.tensor([tv], dtype=torch.float64))
        assert torch.equal(gY, hY) and torch.equal(gM, hM)


# ----------------------------------------------------------------------------------------------
# the default path is untouched
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["natural", "cubic", "linear"])
def test_without_differentiable_nothing_changes(dev, kind):
    """differentiable=False and the default: CdeContractFn serves the field, the launches and the bits are those of a control built
    from the detached series, no control-gradient launch runs, and the series gets no gradient."""
    be = _hip.get_backend()
    x, kn, _, z0 = (torch.from_numpy(a) for a in SC.cde_problem(torch.float64))
    if kind != "natural":
        x, kn = torch.from_numpy(inputs(torch.float64)[0]), None
    make = {"natural": NaturalCubicSpline, "cubic": CubicHermiteSpline, "linear": LinearInterpolation}[kind]
    ts = torch.arange(T, dtype=torch.float64) if kn is None else kn
    runs = []
    for kw in ({}, {"differentiable": False}):
        series = x.clone().requires_grad_(True)
        field = _field(dev)
        X = make(series, kn, **kw)
        assert X.differentiable is False and not X._series.requires_grad
        f = CDEField(field, X)
        assert f._contract is CdeContractFn and f.control_tensors() == ()
        del be.launches[:]
        sol = cdeint(field, X, z0.clone().requires_grad_(True), ts, RK4)
        sol.sum().backward()
        assert series.grad is None
        assert not any("control_grad" in name or name.endswith("coeffs_backward") or name.endswith("gather_backward") for name in be.launches)
        runs.append((sol.detach().clone(), list(be.launches), [p.grad.clone() for p in field.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    # the differentiable control gives the same solution bits and the same parameter gradients through the same launches + its own
    series = x.clone().requires_grad_(True)
    field = _field(dev)
    X = make(series, kn, differentiable=True)
    assert CDEField(field, X)._contract is base_cde.CdeControlContractFn
    del be.launches[:]
    sol = cdeint(field, X, z0.clone().requires_grad_(True), ts, RK4)
    sol.sum().backward()
    assert torch.equal(sol.detach(), runs[0][0]) and all(torch.equal(p.grad, g) for p, g in zip(field.parameters(), runs[0][2]))
    own = "cde_control_grad_natural" if kind == "natural" else "cde_control_grad"
    assert [n for n in be.launches if n != own and not n.startswith("spline_natural_coeffs")] == [
        n for n in runs[0][1] if not n.startswith("spline_natural_coeffs")]
    assert be.launches.count(own) == 4 * (len(ts) - 1) and series.grad is not None


def test_a_control_whose_series_asks_for_nothing_launches_no_control_gradient(dev):
    be = _hip.get_backend()
    x, kn, _, z0 = (torch.from_numpy(a) for a in SC.cde_problem(torch.float64))
    X = NaturalCubicSpline(x, kn, differentiable=True)
    field = _field(dev)
    del be.launches[:]
    cdeint(field, X, z0, kn, RK4).sum().backward()
    assert "cde_control_grad_natural" not in be.launches and be.launches.count("cde_contract_natural_backward") == 4 * (T - 1)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_refusals_by_message(dev):
    x, kn, _, z0 = (torch.from_numpy(a) for a in SC.cde_problem(torch.float64))
    series = x.clone().requires_grad_(True)
    field = _field(dev)
    with pytest.raises(NotImplementedError, match=r"BezierSpline\(differentiable=True\).*NaturalCubicSpline take differentiable=True"):
        BezierSpline(torch.zeros(2, 5, 3), differentiable=True)
    plain = torch.from_numpy(inputs(torch.float64)[0]).requires_grad_(True)
    for cls in (LinearInterpolation, CubicHermiteSpline):
        Xl = cls(plain, differentiable=True)
        for call in (Xl.evaluate, Xl.derivative):
            with pytest.raises(NotImplementedError, match="the values at the knots are the series rows themselves \\(index the series"):
                call(torch.tensor([0.0]))
    X = NaturalCubicSpline(series, kn, differentiable=True)
    with pytest.raises(NotImplementedError, match="differentiable control with process_group.*differentiable=False"):
        cdeint(field, X, z0, kn, RK4, options={"norm": _rms_norm, "process_group": True})
    with pytest.raises(NotImplementedError, match="differentiable control with process_group"):
        cdeint_adjoint(field, X, z0, kn, solver=Dopri5, adjoint_options={"process_group": True})
    with pytest.raises(NotImplementedError, match=r"differentiable control with options\['backprop'\] = 'steps'.*fixed-step solver"):
        cdeint(field, X, z0, kn, Dopri5, options={"norm": _rms_norm, "backprop": "steps"})
    hook = lambda t, y, g: (y, None, g)  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"differentiable control with adjoint_options\['vjp'\] / AdjointProblem.*drop the key"):
        cdeint_adjoint(field, X, z0, kn, solver=Dopri5, adjoint_options={"vjp": hook}, adjoint_params=())
    with pytest.raises(NotImplementedError, match=r"differentiable control with adjoint_options\['vjp'\] / AdjointProblem.*use cdeint_adjoint"):
        AdjointProblem(CDEField(field, X), vjp=hook, adjoint_params=(), solver=Dopri5)
    for forced in (True, {}):
        with pytest.raises(NotImplementedError, match=r"adjoint_options\['graph_func'\] = True.*\"auto\""):
            cdeint_adjoint(field, X, z0, kn, solver=Dopri5, adjoint_options={"graph_func": forced})
    # none of these is refused for a control that asks for no gradient
    AdjointProblem(CDEField(field, NaturalCubicSpline(x, kn)), vjp=hook, adjoint_params=(), solver=Dopri5)
    with torch.no_grad():
        assert cdeint(field, X, z0, kn[[0, -1]], Dopri5, options={"norm": _rms_norm, "backprop": "steps"}).shape == (2, B, H)


def test_an_adaptive_cdeint_under_grad_gives_the_series_its_gradient_through_the_adjoint(dev):
    """cdeint(Dopri5) with nothing else requiring grad: served by the adjoint with the control's tensors as its parameters (after
    func's); explicit adjoint_params keep their place in front."""
    x, kn, a, z0 = (torch.from_numpy(v) for v in SC.cde_problem(torch.float64))
    series = x.clone().requires_grad_(True)
    X = NaturalCubicSpline(series, kn, differentiable=True)
    f = lambda t, z: z[..., None] * a  # noqa: E731
    cdeint(f, X, z0, kn[[0, 3]], Dopri5).sum().backward()
    g = series.grad.clone()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and not g[torch.isnan(x)].any()
    series.grad = None
    scale = torch.ones((), dtype=torch.float64, requires_grad=True)
    X = NaturalCubicSpline(series, kn, differentiable=True)
    cdeint_adjoint(lambda t, z: z[..., None] * (a * scale), X, z0, kn[[0, 3]], solver=Dopri5, adjoint_params=(scale,)).sum().backward()
    assert scale.grad is not None and float(scale.grad.abs()) > 0
    # (two adjoint solves at rtol 1e-7 whose error norms see different parameter sets, hence other step sequences: 100 x rtol of the
    # largest entry)
    assert float((series.grad - g).abs().max()) <= 1e-5 * float(g.abs().max())


def test_exports():
    import paddlexde_amd
    import paddlexde_amd.xde as Xd

    assert Xd.CdeControlContractFn is base_cde.CdeControlContractFn
    assert not hasattr(paddlexde_amd, "CdeControlContractFn")


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_cdegrad.h
# ----------------------------------------------------------------------------------------------
def test_the_cdegrad_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("control_grad" in m or "backward" in m and "spline" in m for m in pub)
    for m in ("_cde_control_grad", "_cde_control_grad_natural", "_spline_natural_coeffs_backward", "_spline_natural_gather_backward",
              "_cde_control_grad_plan"):
        assert callable(getattr(_hip.HipBackend, m)) and callable(getattr(GD.CdeGradDoubleBackend, m))


A = 0x10000
_TIME = [("t_host", 0.5), ("time_dtype", 1), ("B", 2), ("H", 3), ("C", 4), ("Tn", 5)]
_GRAD = ("xde_cde_control_grad", 5, _TIME + [("method", 1), ("dtype", 0)])
_GRADN = ("xde_cde_control_grad_natural", 6, _TIME + [("dtype", 0)])
_COEFFS = ("xde_spline_natural_coeffs_backward", 6, [("B", 2), ("Tn", 5), ("C", 4), ("dtype", 0)])
_GATHER = ("xde_spline_natural_gather_backward", 6, [("outer", 2), ("Tn", 5), ("L", 3), ("D", 4), ("dtype", 0)])


def test_cdegrad_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    common = [({}, dict(Tn=1)), ({}, dict(Tn=0)), ({}, dict(dtype=2)), ({}, dict(dtype=-1)), ({0: A + 2}, {}), ({2: 3 * A + 4}, dict(dtype=1))]
    timed = [({}, dict(B=0)), ({}, dict(H=0)), ({}, dict(C=-1)), ({}, dict(time_dtype=2)), ({}, dict(time_dtype=-1))]
    cases = [(_GRAD, [({i: None}, {}) for i in range(4)] + timed + [({}, dict(method=2)), ({}, dict(method=3)), ({}, dict(method=-1)),
                                                                  ({4: 5 * A + 2}, dict(time_dtype=0)), ({4: 5 * A + 4}, {})]),
             (_GRADN, [({i: None}, {}) for i in range(5)] + timed + [({5: 6 * A + 2}, dict(time_dtype=0)), ({5: 6 * A + 4}, {})]),
             (_COEFFS, [({i: None}, {}) for i in range(6)] + [({}, dict(B=0)), ({}, dict(B=-1)), ({}, dict(C=0)), ({5: 6 * A + 2}, {})]),
             (_GATHER, [({i: None}, {}) for i in (0, 1, 4, 5)]
              + [({2: None, 3: None}, {}), ({}, dict(outer=0)), ({}, dict(L=0)), ({}, dict(D=0)), ({3: 4 * A + 2}, {})])]
    for (name, nptr, scalars), bad in cases:
        fn = _entry(lib, name, nptr, scalars)
        t_at = {"xde_cde_control_grad": 4, "xde_cde_control_grad_natural": 5}.get(name)
        for ptrs, kw in bad + common:
            for extra in ({}, {t_at: None}) if t_at is not None and t_at not in ptrs else ({},):  # (device time, host time)
                rc, msg = fn({**extra, **ptrs}, **kw)
                assert rc == _hip.XDE_EBADARG, (name, ptrs, kw, rc, msg)
                assert msg.startswith(name + ":"), (ptrs, kw, msg)
        assert fn({0: None}, Tn=1)[1] == name + ": null pointer"
        assert fn(Tn=1)[1] == name + ": bad sizes (need Tn >= 2)"
        assert fn(dtype=3)[1] == name + ": bad dtype"
        assert fn({0: A + 1})[1] == name + ": operand not aligned to its element type"
    assert "XDE_HISTORY_BEZIER is not a control path" in _entry(lib, *_GRAD)(method=2)[1]
    # the plan query and the workspace query
    plan = _hip.XdeCdeGradPlan()
    import ctypes

    for args in ((A, 2, 3, 4, 0, None), (A, 0, 3, 4, 0, ctypes.byref(plan)), (A, 2, 0, 4, 0, ctypes.byref(plan)), (A, 2, 3, 0, 0, ctypes.byref(plan)),
                 (A, 2, 3, 4, 2, ctypes.byref(plan)), (A + 2, 2, 3, 4, 0, ctypes.byref(plan)), (A + 4, 2, 3, 4, 1, ctypes.byref(plan))):
        assert lib.xde_cde_control_grad_plan(*args) == _hip.XDE_EBADARG
        assert lib.xde_last_error().decode().startswith("xde_cde_control_grad_plan:")
    ws = lib.xde_spline_natural_coeffs_backward_workspace_bytes
    assert ws(2, 5, 4, 0) == 2 * 2 * 5 * 4 * 4 and ws(2, 5, 4, 1) == 2 * 2 * 5 * 4 * 8
    assert ws(0, 5, 4, 0) == ws(2, 1, 4, 0) == ws(2, 5, 0, 0) == ws(2, 5, 4, 2) == -1


def test_cdegrad_host_halves_run_up_to_the_launch_without_a_gpu():
    """With well-formed (fake, never dereferenced on the host) device addresses on a box without a GPU, each entry point runs its host
    half — checks, the plan, the argument block — and the launch fails: XDE_EHIP."""
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the launches would run on the fake addresses")
    lib = _hip.load_library()
    for name, nptr, scalars in (_GRAD, _GRADN, _COEFFS, _GATHER):
        fn = _entry(lib, name, nptr, scalars)
        variants = [{}, dict(dtype=1)]
        variants += {"xde_cde_control_grad": [{4: None}, dict(method=0)], "xde_cde_control_grad_natural": [{5: None}],
                     "xde_spline_natural_gather_backward": [{2: None}, {3: None}]}.get(name, [])
        for v in variants:
            ptrs = {k: val for k, val in v.items() if isinstance(k, int)}
            rc, msg = fn(ptrs, **{k: val for k, val in v.items() if not isinstance(k, int)})
            assert rc == _hip.XDE_EHIP and msg, (name, v, rc, msg)


# ----------------------------------------------------------------------------------------------
# the plan table
# ----------------------------------------------------------------------------------------------
def _library_plan(dt, B_, H_, C_, misalign):
    import ctypes

    plan = _hip.XdeCdeGradPlan()
    es = 4 if dt == "f32" else 8
    rc = _hip.load_library().xde_cde_control_grad_plan(A + (es if misalign else 0), B_, H_, C_, 0 if dt == "f32" else 1, ctypes.byref(plan))
    assert rc == 0
    return {name: int(getattr(plan, name)) for name, _ in _hip.XdeCdeGradPlan._fields_}


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_every_row_of_the_plan_table_runs_the_branch_it_names_and_the_suite_reaches_them_all(dt):
    """Host arithmetic only: the library's plan of every row of tests/_cdegrad_plans.py has the features the row is there for, the
    double states the same plan, and the union of the GPU suite's shapes reaches every branch."""
    for row in GP.TABLE:
        B_, H_, C_ = row.shape
        p = _library_plan(dt, B_, H_, C_, row.misalign)
        assert row.features <= GP.features(p, B_, H_, C_, dt), (row.label, p, GP.features(p, B_, H_, C_, dt))
        fake = types.SimpleNamespace(dtype=torch.float32 if dt == "f32" else torch.float64,
                                     data_ptr=lambda: A + ((4 if dt == "f32" else 8) if row.misalign else 0))
        assert GD.CdeGradDoubleBackend._cde_control_grad_plan(None, fake, B_, H_, C_) == p, row.label
    assert GP.coverage_gaps(lambda *a: _library_plan(*a), dt) == []
