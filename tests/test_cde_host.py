"""cdeint without a GPU: the end-to-end cases of tests/_cde_cases.py on the numpy double, the launches of a walk and of its backward,
the double against tests/_cde_oracle.py, every refusal by message, and the C ABI of include/xde_hip_cde.h (every call below is refused
on the host before anything is enqueued)."""
import ctypes

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _cde_oracle as CO
from ._cde_cases import *  # noqa: F401,F403
from ._cde_cases import B, C, H, T, Field, _field, cdeint, cdeint_adjoint, inputs, CubicHermiteSpline, LinearInterpolation, RK4, Dopri5
from . import _cde_plans as P
from ._cde_double import CdeDoubleBackend, contract_in_header_order, team_lanes
from .test_srk_host import _entry

LAUNCHES = ("xde_cde_contract", "xde_cde_contract_backward")  # (the entry points that enqueue: one signature)


@pytest.fixture
def dev():
    _hip._set_backend_for_testing(CdeDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def test_launches_of_a_walk_and_of_its_backward(dev):
    """cdeint(RK4) over n steps: one cde_contract per stage and no history gather; its backward launches cde_contract_backward as
    often."""
    be = _hip.get_backend()
    series, _, z0 = (torch.from_numpy(x) for x in inputs(torch.float64))
    X = CubicHermiteSpline(series)
    field = _field(dev)
    ts = torch.linspace(0.0, 7.0, 6, dtype=torch.float64)
    n_steps = len(ts) - 1
    del be.launches[:]
    sol = cdeint(field, X, z0.clone().requires_grad_(True), ts, RK4)
    assert be.launches.count("cde_contract") == 4 * n_steps
    assert not any(name.startswith("history") or name == "hermite" for name in be.launches)
    del be.launches[:]
    sol.sum().backward()
    assert be.launches.count("cde_contract_backward") == 4 * n_steps and "cde_contract" not in be.launches
    assert not any(name.startswith("history") or name == "hermite" for name in be.launches)


def test_team_lanes_follow_the_header():
    assert team_lanes(1, np.float32) == (4, 1, 1) and team_lanes(5, np.float32) == (4, 2, 2) and team_lanes(64, np.float32) == (4, 16, 16)
    assert team_lanes(260, np.float32) == (4, 65, 64) and team_lanes(3, np.float64) == (2, 2, 2) and team_lanes(260, np.float64) == (2, 130, 64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_the_double_against_the_oracle(dev, dtype, method):
    """The double's contraction and cotangent against the float64 contraction with the oracle spline's derivative, at every kind of
    time (first knot, an interior knot, inside the last interval, the last knot) and at C on both sides of a team pass.  The two
    derivatives are the same four-term sum in two op orders (the oracle's is a matrix product): on the unit grid every term is a basis
    weight (at most 1.5 in size) times a row or a row difference (at most 2 max|series|), each carrying under ten roundings, so the
    derivatives differ by at most E = 128 u max|series|.  The contraction then differs by at most gamma_C sum|F dX| + 2 E sum|F|, the
    cotangent by at most |gout| (E + 2 u |dX|)."""
    be = _hip.get_backend()
    T_ = np.float32 if dtype == torch.float32 else np.float64
    rs = np.random.RandomState(3)
    for Cc, Tn in ((1, 2), (5, 3), (64, 8), (260, 8)):
        series = rs.randn(3, Tn, Cc).astype(T_)
        knots = np.arange(Tn).astype(T_)
        F = rs.randn(3, 7, Cc).astype(T_)
        gout = rs.randn(3, 7).astype(T_)
        for t in (0.0, float(Tn // 2), Tn - 1.25, float(Tn - 1)):
            out = torch.empty(3, 7, dtype=dtype)
            be._cde_contract(out, torch.from_numpy(F), torch.from_numpy(series), torch.from_numpy(knots), t, method)
            u = 2.0**-24 if T_ == np.float32 else 2.0**-53
            E = 128 * u * np.abs(series).max()
            dX = np.abs(CO.dX(series, knots, t, method, T_)).astype(np.float64)
            absF = np.abs(F).astype(np.float64)
            bound = CO.gamma(Cc, T_) * np.einsum("bhc,bc->bh", absF, dX) + 2 * E * absF.sum(axis=-1)
            err = np.abs(out.numpy().astype(np.float64) - CO.contract(F, series, knots, t, method, T_))
            assert (err <= bound).all(), (Cc, Tn, t, float((err / bound).max()))
            gF = torch.empty(3, 7, Cc, dtype=dtype)
            tt = torch.tensor(t, dtype=torch.float64)  # (a float64 time with a float32 series)
            be._cde_contract_backward(gF, torch.from_numpy(gout), torch.from_numpy(series), torch.from_numpy(knots), tt, method)
            err = np.abs(gF.numpy() - CO.contract_backward(gout, series, knots, t, method, T_))
            bound = np.abs(gout)[:, :, None].astype(np.float64) * (E + 2 * u * dX[:, None, :])
            assert (err <= bound).all(), (Cc, Tn, t, float((err / bound).max()))
    # the order is the header's: C = 5 in fp32 is two lanes, ((f0 d0 + f1 d1) + f2 d2) + f3 d3 on lane 0 and f4 d4 on lane 1
    f, d = rs.randn(1, 1, 5).astype(np.float32), rs.randn(1, 5).astype(np.float32)
    p = f[0, 0] * d[0]
    assert contract_in_header_order(f, d)[0, 0] == (((np.float32(0) + p[0]) + p[1]) + p[2]) + p[3] + (np.float32(0) + p[4])


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_refusals_say_what_works(dev):
    from paddlexde_amd.interpolation import BezierSpline
    from paddlexde_amd.xde import BaseCDE, CDEField

    series, a, z0 = (torch.from_numpy(x) for x in inputs(torch.float64))
    X = CubicHermiteSpline(series)
    ts = torch.linspace(0.0, 7.0, 5, dtype=torch.float64)
    f = lambda t, z: z[..., None] * a  # noqa: E731
    with pytest.raises(NotImplementedError, match="BezierSpline is not a control path.*use CubicHermiteSpline"):
        cdeint(f, BezierSpline(series), z0, ts, RK4)
    with pytest.raises(NotImplementedError, match="BezierSpline is not a control path"):
        CDEField(f, BezierSpline(series))
    for call in (lambda: cdeint(f, LinearInterpolation(series), z0, ts, Dopri5),
                 lambda: cdeint_adjoint(f, LinearInterpolation(series), z0, ts, solver=Dopri5, adjoint_params=()),
                 lambda: cdeint_adjoint(f, LinearInterpolation(series), z0, ts, solver=RK4, adjoint_solver=Dopri5, adjoint_params=())):
        with pytest.raises(NotImplementedError, match="derivative jumps at every knot.*jump_t.*CubicHermiteSpline.*fixed-step solver"):
            call()
    with torch.no_grad():
        assert cdeint(f, LinearInterpolation(series), z0, torch.arange(8.0, dtype=torch.float64), RK4).shape == (8 * B, H)
    bad = {"not [..., H, C]": lambda t, z: z, "wrong C": lambda t, z: z[..., None] * a[:, :2],
           "wrong H": lambda t, z: (z[..., None] * a)[:, :3]}
    for g in bad.values():
        with pytest.raises(ValueError, match=r"func\(t, z\) must return \[\.\.\., H, C\]"):
            cdeint(g, X, z0, ts, RK4)
    with pytest.raises(ValueError, match="must return z's dtype on z's device"):
        cdeint(lambda t, z: (z[..., None] * a).float(), X, z0, ts, RK4)
    with pytest.raises(ValueError, match="series is torch.float32 and z0 is torch.float64"):
        cdeint(f, CubicHermiteSpline(series.float()), z0, ts, RK4)
    with pytest.raises(ValueError, match="leading dimensions"):
        cdeint(f, X, z0[:1], ts, RK4)
    for span in (torch.tensor([0.0, 7.5]), torch.tensor([-0.5, 3.0])):
        with pytest.raises(ValueError, match=r"leaves the control's interval X.interval = \[0.0, 7.0\]"):
            cdeint(f, X, z0, span.double(), RK4)
    with pytest.raises(NotImplementedError, match="no gradient with respect to t_span"):
        cdeint(f, X, z0, ts.clone().requires_grad_(True), RK4)
    with pytest.raises(NotImplementedError, match="tensor z0, not a tuple"):
        cdeint(f, X, (z0, z0), ts, RK4)
    # the wrapper
    xde = BaseCDE(f, X, z0, ts)
    assert xde.name == "CDE" and type(xde).fuse is type(xde).__mro__[1].fuse and isinstance(xde.func, CDEField)
    field = Field()
    assert [id(p) for p in CDEField(field, X).parameters()] == [id(p) for p in field.parameters()]


def test_exports():
    import paddlexde_amd
    import paddlexde_amd.functional as Fn
    import paddlexde_amd.xde as Xd

    assert callable(Fn.cdeint) and callable(Fn.cdeint_adjoint) and Xd.BaseCDE and Xd.CDEField
    for name in ("BaseCDE", "CDEField", "cdeint", "cdeint_adjoint"):
        assert not hasattr(paddlexde_amd, name)  # (the top level keeps its names)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_cde.h
# ----------------------------------------------------------------------------------------------
def test_cde_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    A = 0x10000
    scalars = [("t_host", 0.5), ("time_dtype", 1), ("B", 2), ("H", 3), ("C", 4), ("Tn", 5), ("method", 1), ("dtype", 0)]
    bad = ([({i: None}, {}) for i in range(4)]
           + [({}, dict(B=0)), ({}, dict(B=-1)), ({}, dict(H=0)), ({}, dict(C=0)), ({}, dict(Tn=1)), ({}, dict(Tn=0)),
              ({}, dict(dtype=2)), ({}, dict(dtype=-1)), ({}, dict(time_dtype=2)), ({}, dict(time_dtype=-1)),
              ({}, dict(method=2)), ({}, dict(method=3)), ({}, dict(method=-1)),
              ({0: A + 2}, {}), ({1: 2 * A + 4}, dict(dtype=1)), ({4: 5 * A + 2}, dict(time_dtype=0)), ({4: 5 * A + 4}, {})])
    assert set(_hip.HEADERS["xde_hip_cde.h"]) == set(LAUNCHES) | {"xde_cde_plan"}  # (the plan query has its own test below)
    for name in LAUNCHES:
        fn = _entry(lib, name, 5, scalars)
        for ptrs, kw in bad:
            for extra in ({}, {4: None}) if 4 not in ptrs else ({},):  # (with the time in device memory, and as a host number)
                rc, msg = fn({**extra, **ptrs}, **kw)
                assert rc == _hip.XDE_EBADARG, (name, ptrs, kw, rc, msg)
                assert msg.startswith(name + ":"), (ptrs, kw, msg)
        assert fn({0: None}, B=0)[1] == name + ": null pointer"
        assert fn(Tn=1)[1] == name + ": bad sizes (need Tn >= 2)"
        assert "XDE_HISTORY_BEZIER is not a control path" in fn(method=2)[1]
        assert fn(method=7)[1] == name + ": unknown method"


def test_the_cde_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("cde" in m for m in pub)
    for m in ("_cde_contract", "_cde_contract_backward"):
        assert callable(getattr(_hip.HipBackend, m)) and callable(getattr(CdeDoubleBackend, m))
    assert callable(_hip.HipBackend._cde_plan)


# ----------------------------------------------------------------------------------------------
# the launch plan (host arithmetic: no device)
# ----------------------------------------------------------------------------------------------
def host_plan(backward, dt, B, H, C, misalign):
    """xde_cde_plan for a big operand that is 16-byte aligned or one element off it (the pointer is never dereferenced)."""
    plan = _hip.XdeCdePlan()
    at = 0x10000 + (0 if not misalign else 4 if dt == "f32" else 8)
    rc = _hip.load_library().xde_cde_plan(int(backward), at, B, H, C, _hip.XDE_F32 if dt == "f32" else _hip.XDE_F64, ctypes.byref(plan))
    assert rc == _hip.XDE_OK, _hip.load_library().xde_last_error()
    return {name: int(getattr(plan, name)) for name, _ in _hip.XdeCdePlan._fields_}


def test_the_plan_query_validates_its_arguments():
    lib = _hip.load_library()
    plan = _hip.XdeCdePlan()
    good = dict(backward=0, big=0x10000, B=2, H=3, C=4, dtype=0)
    sizes, align = "bad sizes (need B, H, C >= 1)", "operand not aligned to its element type"
    for kw, msg in ((dict(B=0), sizes), (dict(H=0), sizes), (dict(C=-1), sizes), (dict(dtype=2), "bad dtype"),
                    (dict(big=0x10002), align), (dict(big=0x10004, dtype=1), align)):
        a = dict(good, **kw)
        assert lib.xde_cde_plan(a["backward"], a["big"], a["B"], a["H"], a["C"], a["dtype"], ctypes.byref(plan)) == _hip.XDE_EBADARG, kw
        assert lib.xde_last_error().decode() == "xde_cde_plan: " + msg
    assert lib.xde_cde_plan(0, 0x10000, 2, 3, 4, 0, None) == _hip.XDE_EBADARG and lib.xde_last_error().decode() == "xde_cde_plan: null pointer"
    assert lib.xde_cde_plan(0, None, 2, 3, 4, 0, ctypes.byref(plan)) == _hip.XDE_OK  # (only the alignment of `big` is used)


def test_the_plan_of_the_plainest_launch():
    """B, H, C = 2, 4, 3 (tests/_cde_cases.py): what the fields mean, on the one shape whose plan follows from the header alone —
    C = 3 is one fp32 vector (R = 1) and two fp64 ones (R = 2), no whole vector, so scalar loads; C fits the on-chip table; two
    batch rows are two items on two workgroups, far from the grid cap, and F is far from the streaming threshold."""
    for dt, R in (("f32", 1), ("f64", 2)):
        for backward in (False, True):
            p = host_plan(backward, dt, B, H, C, False)
            assert (p["vec"], p["lds"], p["grouped"], p["Gb"], p["nt"]) == (0, 1, 0, 1, 0)
            assert p["items"] == p["blocks"] == B * p["S"] and p["S"] * p["Hc"] >= H > (p["S"] - 1) * p["Hc"] and p["rows_per_pass"] >= 1
            assert (p["R"], p["single"]) == ((1, 0) if backward else (R, 1))
    # alignment decides vec where C is whole vectors, and only there
    assert host_plan(False, "f32", 2, 4, 8, False)["vec"] == 1 and host_plan(False, "f32", 2, 4, 8, True)["vec"] == 0
    assert host_plan(True, "f64", 2, 4, 6, False)["vec"] == 1 and host_plan(True, "f64", 2, 4, 5, False)["vec"] == 0


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_every_row_of_the_plan_table_takes_its_branches(dt):
    """tests/_cde_plans.py: each row's shape takes the branches the row is there for (the GPU test launches them and asserts this again
    on the pointers it launches with)."""
    missed = []
    for row in P.TABLE:
        (B_, H_, C_), fwd, bwd = P.row_case(row, dt)
        for backward, want in ((False, fwd), (True, bwd)):
            got = P.features(host_plan(backward, dt, B_, H_, C_, row.misalign), B_, H_, C_, backward)
            if not want <= got:
                missed.append((row.label, "backward" if backward else "forward", "not taken:", sorted(want - got)))
    assert missed == []


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_suites_shapes_reach_every_reachable_plan(dt):
    """Over every shape tests/test_gpu_cde.py launches: all six instantiations, a second item in each family, a second row pass in
    each path, a short last slice, a short last group and the streaming loads — forward and backward."""
    assert P.coverage_gaps(host_plan, dt) == []


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_double_is_within_the_standard_bound_at_the_plan_tables_row_lengths(dtype):
    """contract_in_header_order against the float64 einsum of the same rounded operands at C = 8, 256, 2052 (the row lengths the plan
    table adds): |err| <= gamma_C sum|F dX|, the bound of a length-C inner product in any order — so the bits the kernels are held to
    at those lengths do not rest on the double alone."""
    rs = np.random.RandomState(8)
    for Cc in (8, 256, 2052):
        F, dX = rs.randn(3, 5, Cc).astype(dtype), rs.randn(3, Cc).astype(dtype)
        got = contract_in_header_order(F, dX)
        assert got.dtype == dtype and got.shape == (3, 5)
        Fd, dXd = F.astype(np.float64), dX.astype(np.float64)
        err = np.abs(got.astype(np.float64) - np.einsum("bhc,bc->bh", Fd, dXd))
        bound = CO.gamma(Cc, dtype) * np.einsum("bhc,bc->bh", np.abs(Fd), np.abs(dXd))
        assert (err <= bound).all(), (Cc, float((err / bound).max()))
