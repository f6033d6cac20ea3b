"""NaturalCubicSpline without a GPU: the numpy double of include/xde_hip_spline.h against the float64 dense-solve oracle
(tests/_spline_oracle.py), the exact cases (two knots, data on a straight line), the observed data back at the knots, whole missing
rows against the shorter series, every refusal by message, the C ABI of the header (every call is refused on the host, or — on a box
without a GPU — runs its host half up to the launch), the launches of a cdeint walk on the natural control, and the exports."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import cdeint, cdeint_adjoint
from paddlexde_amd.interpolation import NaturalCubicSpline
from paddlexde_amd.solver import RK4, Dopri5

from . import _spline_cases as SC
from . import _spline_double as SD
from . import _spline_oracle as SO
from ._cde_cases import B, C, H, T, _field
from ._spline_e2e import *  # noqa: F401,F403
from .test_srk_host import _entry

_U = {np.float32: 2.0**-24, np.float64: 2.0**-53}

# The double against the oracle, in units of u = the dtype's unit roundoff:
#   M    |M - M_o|     / (u max|M_o|)                       on the whole knot grid (both are zero where the oracle's is)
#   val  |val - val_o| / (u max|val_o|)
#   der  |der - der_o| / (u (max|der_o| + max|y| / min h))  (the derivative is a difference of values over a knot spacing)
# MEASURED is the worst of each over this module's inputs (every Tn of SC.TNS x every pattern of SC.PATTERNS that fits, knot spacing
# ratio 16, queries on every knot and at 0.25, 0.5, 0.9 of every interval) with the committed double on the CPU; the test asserts
# 4 x that (the system is strictly diagonally dominant, so the error is a small multiple of u; 4 x covers another libm / numpy).
MEASURED = {np.float32: {"M": 2.22, "val": 7.17, "der": 0.916}, np.float64: {"M": 3.17, "val": 6.71, "der": 1.20}}
BOUND = {T_: {k: 4.0 * v for k, v in m.items()} for T_, m in MEASURED.items()}


@pytest.fixture
def dev():
    _hip._set_backend_for_testing(SD.SplineDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def _queries(kn):
    k64 = kn.astype(np.float64)
    return np.concatenate([k64] + [k64[:-1] + f * np.diff(k64) for f in (0.25, 0.5, 0.9)]).astype(kn.dtype)


def _errors(T_, Tn, pattern):
    """(M, val, der) errors of the double against the oracle in the units above, for three series of five columns with ``pattern``."""
    u = _U[T_]
    rs = np.random.RandomState(100 * Tn + SC.PATTERNS.index(pattern))
    kn = SC.knots(rs, Tn, T_)
    x = SC.series(rs, 3, Tn, 5, T_, patterns=(pattern,))
    Y, M = SD.natural_coeffs(x, kn)
    tq = _queries(kn)
    val, der = SD.natural_gather(Y, M, kn, tq)
    oval, oder, oM = SO.spline(x.astype(np.float64), kn.astype(np.float64), tq.astype(np.float64))
    if np.abs(oM).max() == 0.0:
        assert not M.any(), (Tn, pattern)  # (a constant or a straight line: exactly zero in the double too)
        eM = 0.0
    else:
        eM = np.abs(M - oM).max() / (u * np.abs(oM).max())
    ev = np.abs(val - oval).max() / (u * np.abs(oval).max())
    hmin = np.diff(kn.astype(np.float64)).min()
    ed = np.abs(der - oder).max() / (u * (np.abs(oder).max() + np.nanmax(np.abs(x)) / hmin))
    return eM, ev, ed


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_the_double_against_the_dense_solve_oracle(T_):
    worst = {"M": 0.0, "val": 0.0, "der": 0.0}
    n = 0
    for Tn in SC.TNS:
        for pattern in SC.PATTERNS:
            if SC.missing(pattern, Tn) is None:
                continue
            n += 1
            for key, e in zip(("M", "val", "der"), _errors(T_, Tn, pattern)):
                worst[key] = max(worst[key], float(e))
    print("{}: {} cases, worst in units of u: {}; asserted: {}".format(T_.__name__, n, worst, BOUND[T_]))
    assert n == 30
    for key in worst:
        assert worst[key] <= BOUND[T_][key], (key, worst[key], BOUND[T_][key])


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_two_knots_and_straight_lines_have_no_curvature_exactly(T_):
    """Tn = 2 is the chord; data on a line whose slopes divide exactly (knots on multiples of 1/4, slope a power of two) gives equal
    one-sided slopes at every node, so rhs = 0 and M == 0 exactly at any spacing — with NaNs too — and der is the slope at any time."""
    rs = np.random.RandomState(1)
    x = rs.randn(2, 2, 3).astype(T_)
    Y, M = SD.natural_coeffs(x, np.asarray([0.5, 2.25], dtype=T_))
    assert np.array_equal(Y, x) and not M.any()
    kn = np.asarray([0.0, 0.25, 1.0, 1.5, 4.5, 4.75, 8.0], dtype=T_)
    line = np.stack([3.0 + 2.0 * kn, -1.0 - 0.5 * kn], axis=-1)[None].astype(T_)  # [1, 7, 2]
    holes = line.copy()
    holes[0, [0, 2, 3], 0] = np.nan  # (a NaN first row: the end rule makes the path flat up to the first observed knot ...)
    holes[0, [2, 3, 4], 1] = np.nan
    Y, M = SD.natural_coeffs(line, kn)
    assert np.array_equal(Y, line) and not M.any()
    Yh, Mh = SD.natural_coeffs(holes, kn)
    assert not Mh[:, :, 1].any() and np.array_equal(Yh[:, :, 1], line[:, :, 1])  # (... so only the interior holes keep the line)
    tq = np.asarray([-1.0, 0.0, 0.1, 1.0, 3.3, 8.0, 9.5], dtype=T_)
    val, der = SD.natural_gather(Y, M, kn, tq)
    assert np.array_equal(der[0, :, 0], np.full(7, 2.0, dtype=T_)) and np.array_equal(der[0, :, 1], np.full(7, -0.5, dtype=T_))
    assert np.array_equal(SD.natural_gather(Yh, Mh, kn, tq)[1][0, :, 1], np.full(7, -0.5, dtype=T_))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_evaluate_at_the_knots_returns_the_observed_data(dev, dtype):
    """s = 0 at a left knot, so the value there is Y_i exactly; the last knot is reached from the left (s = h) and is held to the
    `val` bound.  Missing entries are compared where they were observed only."""
    T_ = np.float32 if dtype == torch.float32 else np.float64
    for Tn in SC.TNS:
        rs = np.random.RandomState(Tn)
        kn = SC.knots(rs, Tn, T_)
        x = SC.series(rs, 2, Tn, 7, T_)
        X = NaturalCubicSpline(torch.from_numpy(x), torch.from_numpy(kn))
        assert X.method == "natural" and X.min_times == 2 and X._series.shape == X._coef.shape == x.shape
        assert torch.equal(X.grid_points, torch.from_numpy(kn)) and X.interval.tolist() == [kn[0], kn[-1]]
        got = X.evaluate(kn).numpy()
        assert got.shape == x.shape and X.derivative(kn[:1]).shape == (2, 1, 7)
        obs = ~np.isnan(x)
        assert np.array_equal(got[:, :-1][obs[:, :-1]], x[:, :-1][obs[:, :-1]])
        err = np.abs(got[:, -1][obs[:, -1]].astype(np.float64) - x[:, -1][obs[:, -1]])
        assert (err <= BOUND[T_]["val"] * _U[T_] * np.nanmax(np.abs(x))).all()
        assert not np.isnan(X._series.numpy()).any() and not np.isnan(X._coef.numpy()).any()


@pytest.mark.parametrize("T_", [np.float32, np.float64])
def test_rows_missing_in_every_column_equal_the_series_without_them(T_):
    """Interior rows j that are NaN in every column are no nodes: the nodes, hence the Thomas sweeps, are those of the series with the
    rows (and their knots) removed — Y and M at the kept rows are the same bits, and val / der agree within twice the oracle bounds
    (the filled rows split an interval in two; each side is within the bound of the one exact spline)."""
    rs = np.random.RandomState(9)
    Tn, gone = 9, [2, 3, 6]
    keep = [k for k in range(Tn) if k not in gone]
    kn = SC.knots(rs, Tn, T_)
    x = np.cumsum(0.5 * rs.randn(3, Tn, 4), axis=1).astype(T_)
    holes = x.copy()
    holes[:, gone, :] = np.nan
    Y, M = SD.natural_coeffs(holes, kn)
    Ys, Ms = SD.natural_coeffs(np.ascontiguousarray(x[:, keep, :]), kn[keep])
    assert np.array_equal(Y[:, keep, :], Ys) and np.array_equal(M[:, keep, :], Ms)
    tq = _queries(kn)
    (v, d), (vs, ds) = SD.natural_gather(Y, M, kn, tq), SD.natural_gather(Ys, Ms, kn[keep], tq)
    u, hmin = _U[T_], np.diff(kn.astype(np.float64)).min()
    assert np.abs(v.astype(np.float64) - vs).max() <= 2 * BOUND[T_]["val"] * u * np.abs(vs).max()
    assert np.abs(d.astype(np.float64) - ds).max() <= 2 * BOUND[T_]["der"] * u * (np.abs(ds).max() + np.abs(x).max() / hmin)


def _problem(dtype=torch.float64):
    return tuple(torch.from_numpy(x) for x in SC.cde_problem(dtype))


def test_refusals_by_message(dev):
    series, kn, a, z0 = _problem()
    f = lambda t, z: z[..., None] * a  # noqa: E731
    bad_t = kn.clone()
    bad_t[3] = bad_t[2]
    with pytest.raises(ValueError, match="NaturalCubicSpline: t must be strictly increasing"):
        NaturalCubicSpline(series, bad_t)
    with pytest.raises(ValueError, match="NaturalCubicSpline: t must be strictly increasing"):
        NaturalCubicSpline(series, kn.flip(0))
    empty = series.clone()
    empty[1, :, 2] = float("nan")
    with pytest.raises(ValueError, match="a column of the series has no observed"):
        NaturalCubicSpline(empty, kn)
    with pytest.raises(ValueError, match="NaturalCubicSpline needs at least 2 time points"):
        NaturalCubicSpline(series[:, :1], kn[:1])
    with pytest.raises(ValueError, match="t must have one entry per time row"):
        NaturalCubicSpline(series, kn[:-1])
    X = NaturalCubicSpline(series, kn)
    with pytest.raises(ValueError, match="series is torch.float32 and z0 is torch.float64"):
        cdeint(f, NaturalCubicSpline(series.float(), kn.float()), z0, kn, RK4)
    lo, hi = float(kn[0]), float(kn[-1])
    for span in (torch.tensor([lo, hi + 0.5]), torch.tensor([lo - 0.5, hi])):
        with pytest.raises(ValueError, match=r"leaves the control's interval X.interval = \[0.0, "):
            cdeint(f, X, z0, span.double(), RK4)
        with pytest.raises(ValueError, match="leaves the control's interval"):
            cdeint_adjoint(f, X, z0, span.double(), solver=Dopri5, adjoint_params=())
    with pytest.raises(ValueError, match="leading dimensions"):
        cdeint(f, X, z0[:1], kn, RK4)
    with pytest.raises(TypeError, match="X must be a paddlexde_amd.interpolation CubicHermiteSpline or LinearInterpolation.*NaturalCubicSpline"):
        cdeint(f, object(), z0, kn, RK4)
    # the natural control is served by fixed and adaptive solvers alike
    with torch.no_grad():
        assert cdeint(f, X, z0, kn, RK4).shape == (T * B, H)
        assert cdeint(f, X, z0, kn[[0, -1]], Dopri5).shape == (2, B, H)


def test_launches_of_a_walk_on_the_natural_control_and_of_its_backward(dev):
    """The constructor is one coefficient launch; cdeint(RK4) over n steps is one natural contraction per stage and no gather (and no
    launch of the other controls' contraction); its backward launches the natural cotangent as often."""
    be = _hip.get_backend()
    series, kn, _, z0 = _problem()
    del be.launches[:]
    X = NaturalCubicSpline(series, kn)
    assert be.launches == ["spline_natural_coeffs"]
    field = _field(dev)
    ts = kn[[0, 2, 3, 5, 7]]
    n_steps = len(ts) - 1
    del be.launches[:]
    sol = cdeint(field, X, z0.clone().requires_grad_(True), ts, RK4)
    assert be.launches.count("cde_contract_natural") == 4 * n_steps and "cde_contract" not in be.launches
    assert not any(name.startswith(("history", "spline")) or name == "hermite" for name in be.launches)
    del be.launches[:]
    sol.sum().backward()
    assert be.launches.count("cde_contract_natural_backward") == 4 * n_steps
    assert not {"cde_contract_natural", "cde_contract", "cde_contract_backward"} & set(be.launches)
    assert not any(name.startswith(("history", "spline")) or name == "hermite" for name in be.launches)
    for p in field.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def test_the_contraction_of_the_double_is_the_gathers_derivative(dev):
    """H = C, F = I: the double's natural contraction returns the double's X.derivative(t) bit for bit (one statement of dX)."""
    be = _hip.get_backend()
    series, kn, _, _ = _problem()
    X = NaturalCubicSpline(series, kn)
    F = torch.eye(C, dtype=torch.float64).expand(B, C, C).contiguous()
    for tv in (float(kn[0]), float(kn[3]), 0.5 * float(kn[3] + kn[4]), float(kn[-1])):
        out = torch.empty(B, C, dtype=torch.float64)
        be._cde_contract_natural(out, F, X._series, X._coef, X._t, tv)
        assert torch.equal(out, X.derivative(torch.tensor([tv], dtype=torch.float64))[:, 0, :])


def test_exports():
    import paddlexde_amd
    import paddlexde_amd.interpolation as I

    assert "NaturalCubicSpline" in I.__all__ and I.NaturalCubicSpline is NaturalCubicSpline
    assert issubclass(NaturalCubicSpline, I.InterpolationBase)
    for name in ("evaluate", "derivative", "grid_points", "interval"):
        assert hasattr(NaturalCubicSpline, name)
    assert not hasattr(paddlexde_amd, "NaturalCubicSpline")  # (the top level keeps its names)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_spline.h
# ----------------------------------------------------------------------------------------------
def test_the_spline_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("spline" in m or "natural" in m for m in pub)
    for m in ("_spline_natural_coeffs", "_spline_natural_gather", "_cde_contract_natural", "_cde_contract_natural_backward"):
        assert callable(getattr(_hip.HipBackend, m)) and callable(getattr(SD.SplineDoubleBackend, m))


A = 0x10000
_COEFFS = ("xde_spline_natural_coeffs", 4, [("B", 2), ("Tn", 5), ("C", 4), ("dtype", 0)])
_GATHER = ("xde_spline_natural_gather", 6, [("outer", 2), ("Tn", 5), ("L", 3), ("D", 4), ("dtype", 0)])
_CONTRACT = [(name, 6, [("t_host", 0.5), ("time_dtype", 1), ("B", 2), ("H", 3), ("C", 4), ("Tn", 5), ("dtype", 0)])
             for name in ("xde_cde_contract_natural", "xde_cde_contract_natural_backward")]


def test_spline_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    common = [({}, dict(Tn=1)), ({}, dict(Tn=0)), ({}, dict(dtype=2)), ({}, dict(dtype=-1)), ({0: A + 2}, {}), ({2: 3 * A + 4}, dict(dtype=1))]
    cases = [(_COEFFS, [({i: None}, {}) for i in range(4)] + [({}, dict(B=0)), ({}, dict(B=-1)), ({}, dict(C=0)), ({3: 4 * A + 2}, {})]),
             (_GATHER, [({i: None}, {}) for i in (0, 2, 3, 4, 5)]
              + [({}, dict(outer=0)), ({}, dict(L=0)), ({}, dict(D=0)), ({1: 2 * A + 2}, {}), ({5: 6 * A + 4}, dict(dtype=1))])]
    cases += [(c, [({i: None}, {}) for i in range(5)]
               + [({}, dict(B=0)), ({}, dict(H=0)), ({}, dict(C=-1)), ({}, dict(time_dtype=2)), ({}, dict(time_dtype=-1)),
                  ({3: 4 * A + 2}, {}), ({5: 6 * A + 2}, dict(time_dtype=0)), ({5: 6 * A + 4}, {})]) for c in _CONTRACT]
    for (name, nptr, scalars), bad in cases:
        fn = _entry(lib, name, nptr, scalars)
        for ptrs, kw in bad + common:
            for extra in ({}, {5: None}) if name.startswith("xde_cde") and 5 not in ptrs else ({},):  # (device time, host time)
                rc, msg = fn({**extra, **ptrs}, **kw)
                assert rc == _hip.XDE_EBADARG, (name, ptrs, kw, rc, msg)
                assert msg.startswith(name + ":"), (ptrs, kw, msg)
        assert fn({0: None}, Tn=1)[1] == name + ": null pointer"
        assert fn(Tn=1)[1] == name + ": bad sizes (need Tn >= 2)"
        assert fn(dtype=3)[1] == name + ": bad dtype"
        assert fn({0: A + 1})[1] == name + ": operand not aligned to its element type"


def test_the_public_contraction_still_refuses_every_method_code_but_its_two():
    """The natural control has entry points of its own: no method code of xde_cde_contract reaches it."""
    lib = _hip.load_library()
    scalars = [("t_host", 0.5), ("time_dtype", 1), ("B", 2), ("H", 3), ("C", 4), ("Tn", 5), ("method", 1), ("dtype", 0)]
    for name in ("xde_cde_contract", "xde_cde_contract_backward"):
        fn = _entry(lib, name, 5, scalars)
        for method in (3, 4, -1):
            assert fn(method=method) == (_hip.XDE_EBADARG, name + ": unknown method")


def test_spline_host_halves_run_up_to_the_launch_without_a_gpu():
    """With well-formed (fake, never dereferenced on the host) device addresses on a box without a GPU, each entry point runs its host
    half — checks, the vector decision, the plan, the argument block — and the launch fails: XDE_EHIP."""
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the launches would run on the fake addresses")
    lib = _hip.load_library()
    for name, nptr, scalars in [_COEFFS, _GATHER] + _CONTRACT:
        fn = _entry(lib, name, nptr, scalars)
        variants = [{}, dict(dtype=1)] + ([{5: None}] if name.startswith("xde_cde") else [{1: None}] if name == _GATHER[0] else [])
        for v in variants:
            ptrs = {k: val for k, val in v.items() if isinstance(k, int)}
            rc, msg = fn(ptrs, **{k: val for k, val in v.items() if not isinstance(k, int)})
            assert rc == _hip.XDE_EHIP and msg, (name, v, rc, msg)
