"""cdeint on the GPU: xde_cde_contract / xde_cde_contract_backward against the numpy double bit for bit (below one vector, unaligned,
one vector, more than one team pass, the scalar path, every kind of time, inside and outside the knots; and a table of shapes,
tests/_cde_plans.py, that reaches every launch plan the default settings can reach — each row held to its plan through xde_cde_plan,
the union held to full coverage — with the one plan they cannot reach, a sliced launch beyond the grid, in a child process), the
autograd wrapper at two of those shapes, two checks that do not go through the double (the identity field returns X.derivative(t); the
standard summation bound against a float64 dot), a refused call leaving its output standing, the end-to-end cases of
tests/_cde_cases.py on the HIP backend, the captured adjoint dynamics against the eager one, and the demo."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.interpolation import CubicHermiteSpline, LinearInterpolation

from paddlexde_amd.xde.base_cde import CdeContractFn

from . import _cde_oracle as CO
from . import _cde_plans as P
from ._cde_cases import *  # noqa: F401,F403
from ._cde_cases import Field, _field, _grads, cdeint_adjoint, inputs, Dopri5
from ._cde_double import CdeDoubleBackend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
SPLINE = {"linear": LinearInterpolation, "cubic": CubicHermiteSpline}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DT = {torch.float32: "f32", torch.float64: "f64"}


@pytest.fixture
def dev():
    return DEV


def _placed(x, misalign):
    """``x`` (numpy) on the device, contiguous, 16-byte aligned or one element off it."""
    flat = torch.empty(x.size + 1, dtype=torch.from_numpy(x).dtype, device=DEV)
    view = (flat[1:] if misalign else flat[:-1]).view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


def _times(knots, Tn):
    """0-3: first knot, exactly on an interior knot (the first one where there is none), inside the last interval, the last knot;
    4-7: strictly inside the first interval, strictly inside a middle one (Tn = 8: the fourth of seven), before the first knot,
    beyond the last knot (the header defines dX for any tau: the interval index is clipped)"""
    m = (Tn - 1) // 2
    return [float(knots[0]), float(knots[1 if Tn > 2 else 0]), float(knots[-1] - 0.25 * (knots[-1] - knots[-2])), float(knots[-1]),
            float(knots[0] + 0.25 * (knots[1] - knots[0])), float(knots[m] + 0.5 * (knots[m + 1] - knots[m])),
            float(knots[0] - 0.75 * (knots[1] - knots[0])), float(knots[-1] + 1.5 * (knots[-1] - knots[-2]))]


def _time_forms(t, dtype):
    """the time as a float64 device scalar (also with a float32 series), as a [1] device tensor of the series dtype, as a host number"""
    return [torch.tensor(t, dtype=torch.float64, device=DEV), torch.tensor([t], dtype=dtype, device=DEV), t]


def _query(backward, dt, B, H, C, misalign):
    """The launch plan for a big operand placed as ``_placed`` places it (only its alignment enters the plan)."""
    big = torch.empty(8, dtype=torch.float32 if dt == "f32" else torch.float64, device=DEV)[1 if misalign else 0:]
    assert (big.data_ptr() % 16 != 0) == bool(misalign)
    return _hip.get_backend()._cde_plan(backward, big, B, H, C)


def _check(double, dtype, method, B, H, C, Tn, t, form, misalign=False, seed=0):
    """Both kernels against the double, bit for bit.  Returns the branches (tests/_cde_plans.py: ``features``) the two launches took,
    from the plans of the operands they were launched with."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    rs = np.random.RandomState(seed + 1000 * C + 10 * H + B)
    series, F, gout = rs.randn(B, Tn, C).astype(T), rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    knots = np.cumsum(0.5 + rs.rand(Tn)).astype(T)  # (an irregular grid: the scale conventions as written)
    tv = _times(knots, Tn)[t]
    th = torch.from_numpy
    want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
    cpu_t = [torch.tensor(tv, dtype=torch.float64), torch.tensor([tv], dtype=dtype), tv][form]
    double._cde_contract(want, th(F), th(series), th(knots), cpu_t, method)
    double._cde_contract_backward(gwant, th(gout), th(series), th(knots), cpu_t, method)
    ser_d, kn_d = _placed(series, False), _placed(knots, False)
    out = _placed(np.full((B, H), SENTINEL, dtype=T), misalign)
    gF = _placed(np.full((B, H, C), SENTINEL, dtype=T), misalign)
    td = _time_forms(tv, dtype)[form]
    F_d = _placed(F, misalign)
    be._cde_contract(out, F_d, ser_d, kn_d, td, method)
    be._cde_contract_backward(gF, _placed(gout, misalign), ser_d, kn_d, td, method)
    where = (dtype, method, B, H, C, Tn, tv, form, misalign)
    assert np.array_equal(out.cpu().numpy(), want.numpy()), where
    assert np.array_equal(gF.cpu().numpy(), gwant.numpy()), where
    return P.features(be._cde_plan(False, F_d, B, H, C), B, H, C, False), P.features(be._cde_plan(True, gF, B, H, C), B, H, C, True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_the_kernels_equal_the_double_bit_for_bit(dtype, method):
    """C below one vector, unaligned, one vector, many, more than one team pass (260 > 64 W in both dtypes); H and B around a
    workgroup's teams; Tn 2, 3, 8; every kind and form of time; the scalar path (operands one element off 16 bytes) gives the aligned
    bits — both equal the double's."""
    double = CdeDoubleBackend()
    n = 0
    for C in (1, 3, 4, 5, 64, 260):
        for H in (1, 7, 33):
            for B in (1, 3):
                Tn = (2, 3, 8)[n % 3]
                for t in range(4):
                    _check(double, dtype, method, B, H, C, Tn, t, form=(n + t) % 3)
                _check(double, dtype, method, B, H, C, Tn, t=2, form=0, misalign=True)
                n += 1
    assert double.launches.count("cde_contract") == double.launches.count("cde_contract_backward") == 36 * 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_more_work_items_than_the_grid(dtype):
    """Short rows of consecutive batch rows share a work item where B is large.  B = 2100, H = 1, C = 3 is grouped (scalar kernel: C
    is no whole vector), every item a full group, and the items stay within the grid; B = 2101: the last item holds fewer batch rows
    than the others; B = 4200, H = 512, C = 1: the grouped items still exceed the grid, so a workgroup takes a second one, and the
    backward kernel walks each item in more than one pass.  (The ungrouped and no-LDS kernels beyond the grid: the plan table below.)"""
    double = CdeDoubleBackend()
    for method in ("linear", "cubic"):
        fwd, bwd = _check(double, dtype, method, 2100, 1, 3, 8, t=2, form=0)
        for took in (fwd, bwd):
            assert "kernel:scalar-grouped" in took and not took & {"second-item:grouped", "short-last-group"}, took
        fwd, bwd = _check(double, dtype, method, 2101, 1, 3, 3, t=1, form=1)
        for took in (fwd, bwd):
            assert {"kernel:scalar-grouped", "short-last-group"} <= took and "second-item:grouped" not in took, took
        fwd, bwd = _check(double, dtype, method, 4200, 512, 1, 2, t=2, form=2)
        assert {"kernel:scalar-grouped", "second-item:grouped"} <= fwd and "second-pass:single" not in fwd, fwd
        assert {"kernel:scalar-grouped", "second-item:grouped", "second-pass:backward"} <= bwd, bwd


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_three_forms_of_time_give_the_same_bits(dtype, C):
    """One shape and one time under all three forms of time (the other tests rotate the forms over their shapes): B, H, Tn = 2, 3, 4
    on the unit grid, C = 5 (the scalar tail) and C = 8 (the vector path), at 1.375 (inside an interval, exact in float32) and 2.0 (on
    a knot).  Both launches give identical bits whether the time is a float64 device element, an element of the series dtype or a
    Python number, and they are the double's."""
    be, double, T, th = _hip.get_backend(), CdeDoubleBackend(), _NPT[dtype], torch.from_numpy
    B, H, Tn = 2, 3, 4
    rs = np.random.RandomState(40 + C)
    series, F, gout = rs.randn(B, Tn, C).astype(T), rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
    knots = np.arange(Tn).astype(T)
    ser_d, kn_d, F_d, gout_d = (_placed(x, False) for x in (series, knots, F, gout))
    assert be._cde_plan(False, F_d, B, H, C)["vec"] == be._cde_plan(True, F_d, B, H, C)["vec"] == int(C == 8)
    for method in ("linear", "cubic"):
        for tv in (1.375, 2.0):
            got = []
            for form in range(3):
                cpu_t = [torch.tensor(tv, dtype=torch.float64), torch.tensor([tv], dtype=dtype), tv][form]
                want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
                double._cde_contract(want, th(F), th(series), th(knots), cpu_t, method)
                double._cde_contract_backward(gwant, th(gout), th(series), th(knots), cpu_t, method)
                out, gF = _placed(np.full((B, H), SENTINEL, dtype=T), False), _placed(np.full((B, H, C), SENTINEL, dtype=T), False)
                td = _time_forms(tv, dtype)[form]
                be._cde_contract(out, F_d, ser_d, kn_d, td, method)
                be._cde_contract_backward(gF, gout_d, ser_d, kn_d, td, method)
                got.append((out.cpu().numpy(), gF.cpu().numpy()))
                where = (dtype, method, C, tv, form)
                assert np.array_equal(got[-1][0], want.numpy()) and np.array_equal(got[-1][1], gwant.numpy()), where
                assert np.array_equal(got[-1][0], got[0][0]) and np.array_equal(got[-1][1], got[0][1]), where


@pytest.mark.parametrize("row", P.TABLE, ids=P.ROW_IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_every_launch_plan_equals_the_double_bit_for_bit(dtype, row):
    """tests/_cde_plans.py's table: the shape takes the branches the row is there for — asserted from the launch plan before anything
    is launched, forward and backward, and again from the operands launched — and both kernels give the double's bits with both
    methods.  (The bits do not depend on the plan: the double is the one of the small shapes.)"""
    (B, H, C), fwd, bwd = P.row_case(row, _DT[dtype])
    for backward, want in ((False, fwd), (True, bwd)):
        got = P.features(_query(backward, _DT[dtype], B, H, C, row.misalign), B, H, C, backward)
        assert want <= got, (row.label, "backward" if backward else "forward", "not taken:", sorted(want - got))
    double = CdeDoubleBackend()
    n = P.TABLE.index(row)
    for k, method in enumerate(("linear", "cubic")):
        took = _check(double, dtype, method, B, H, C, Tn=(3, 2, 8)[n % 3] if C < 2048 else 3, t=(n + 3 * k) % 8, form=(n + k) % 3,
                      misalign=row.misalign)
        assert fwd <= took[0] and bwd <= took[1], (row.label, took)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_suites_shapes_reach_every_reachable_plan(dtype):
    """Over every shape this module launches at the default settings (the grid of the first test, the three grouped shapes, C = 2050
    and the plan table), per direction: all six instantiations, a second work item in the LDS, grouped and no-LDS families, a second
    row pass in the single path, the long path and the backward kernel, a short last slice, a short last group, the streaming loads.
    A condition, not a measurement: after a retune that moves a shape off its branch this names the branch."""
    assert P.coverage_gaps(_query, _DT[dtype]) == []


def test_a_sliced_launch_beyond_the_grid_in_a_child_process():
    """The one plan the default settings cannot reach (the slicing keeps B * S within the grid): an 8-workgroup grid and a 4 KiB
    streaming threshold, read once per process, so in a fresh child (tests/_cde_grid_child.py) — small sliced shapes take second and
    third work items and the streaming loads; the child asserts that from the plan and compares with the double."""
    env = dict(os.environ, XDE_GRID_BLOCKS="8", XDE_NT_BYTES="4096")
    r = subprocess.run([sys.executable, "-m", "tests._cde_grid_child"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "CHILD DONE" in r.stdout, r.stdout[-2000:]
    assert [line for line in r.stdout.splitlines() if line.startswith("FAIL ")] == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_times_inside_the_first_and_a_middle_interval_and_outside_the_knots(dtype, method):
    """The four kinds of time the first test does not ask for (``_times`` 4-7), through all three forms of time, at C below one
    vector, unaligned, one team and more than one team pass; Tn = 8 (a middle interval), 3 and 2."""
    double = CdeDoubleBackend()
    for B, H, C, Tn in ((3, 7, 5, 8), (1, 33, 64, 8), (3, 7, 260, 8), (3, 1, 1, 2), (1, 7, 3, 3), (3, 33, 4, 8)):
        for t in range(4, 8):
            for form in range(3):
                _check(double, dtype, method, B, H, C, Tn, t, form)
        _check(double, dtype, method, B, H, C, Tn, t=6, form=0, misalign=True)
        _check(double, dtype, method, B, H, C, Tn, t=7, form=1, misalign=True)
    assert double.launches.count("cde_contract") == double.launches.count("cde_contract_backward") == 6 * 14


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_autograd_wrapper_at_a_grouped_and_a_two_pass_shape(dtype):
    """CdeContractFn.apply and its backward (the operands torch's allocator hands out) at the plan table's short-last-group shape and
    its two-pass shape: the output and the gradient of F are the double's _cde_contract / _cde_contract_backward bit for bit."""
    be, double, T = _hip.get_backend(), CdeDoubleBackend(), _NPT[dtype]
    th = torch.from_numpy
    for (B, H, C), method, fwd, bwd in (((2049, 3, 8), "cubic", "kernel:vec-grouped", "kernel:vec-grouped"),
                                        ((1024, 70, 64), "linear", "second-pass:single", "second-pass:backward")):
        rs = np.random.RandomState(B)
        series, F, gout = rs.randn(B, 8, C).astype(T), rs.randn(B, H, C).astype(T), rs.randn(B, H).astype(T)
        knots = np.cumsum(0.5 + rs.rand(8)).astype(T)
        tv = float(knots[3] + 0.5 * (knots[4] - knots[3]))
        want, gwant = torch.empty(B, H, dtype=dtype), torch.empty(B, H, C, dtype=dtype)
        double._cde_contract(want, th(F), th(series), th(knots), tv, method)
        double._cde_contract_backward(gwant, th(gout), th(series), th(knots), tv, method)
        F_d = th(F).to(DEV).requires_grad_(True)
        assert fwd in P.features(be._cde_plan(False, F_d, B, H, C), B, H, C, False)
        out = CdeContractFn.apply(F_d, th(series).to(DEV), th(knots).to(DEV), torch.tensor(tv, dtype=torch.float64, device=DEV), method)
        out.backward(th(gout).to(DEV))
        assert bwd in P.features(be._cde_plan(True, F_d.grad, B, H, C), B, H, C, True)
        assert np.array_equal(out.detach().cpu().numpy(), want.numpy()), (B, H, C)
        assert np.array_equal(F_d.grad.cpu().numpy(), gwant.numpy()), (B, H, C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_row_longer_than_the_on_chip_table(dtype):
    """C = 2050 > the 2048 channels of dX a workgroup keeps in LDS: the derivative is recomputed per use, same bits."""
    double = CdeDoubleBackend()
    for method in ("linear", "cubic"):
        _check(double, dtype, method, 2, 3, 2050, 3, t=2, form=1)
        _check(double, dtype, method, 2, 3, 2050, 3, t=1, form=2, misalign=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_the_identity_field_returns_the_spline_derivative(dtype, method):
    """H = C and F[b] = I: the output is X.derivative(t), the `der` of xde_history_gather, bit for bit (not through the double) — at
    every kind of time of ``_times``, so the convention outside the knots is held to the spline's too."""
    be = _hip.get_backend()
    rs = np.random.RandomState(5)
    for C, Tn in ((1, 2), (3, 3), (5, 8), (64, 8), (260, 8)):
        series = torch.from_numpy(rs.randn(3, Tn, C).astype(_NPT[dtype])).to(DEV)
        knots = torch.from_numpy(np.cumsum(0.5 + rs.rand(Tn)).astype(_NPT[dtype])).to(DEV)
        X = SPLINE[method](series, knots)
        F = torch.eye(C, dtype=dtype, device=DEV).expand(3, C, C).contiguous()
        for tv in _times(knots.cpu().numpy(), Tn):
            t = torch.tensor([tv], dtype=dtype, device=DEV)
            out = torch.full((3, C), SENTINEL, dtype=dtype, device=DEV)
            be._cde_contract(out, F, X._series, X._t, t, method)
            assert torch.equal(out, X.derivative(t)[:, 0, :]), (C, Tn, tv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_sum_is_within_the_standard_bound_of_the_float64_dot(dtype):
    """Against the float64 dot of the same rounded operands (F and the X.derivative(t) the device wrote): |err| <= gamma_C sum|F dX|,
    gamma_C = C u / (1 - C u), valid for any summation order (not through the double)."""
    be = _hip.get_backend()
    rs = np.random.RandomState(6)
    for C in (1, 5, 64, 260):
        series = torch.from_numpy(rs.randn(3, 8, C).astype(_NPT[dtype])).to(DEV)
        X = CubicHermiteSpline(series)
        F = torch.from_numpy(rs.randn(3, 33, C).astype(_NPT[dtype])).to(DEV)
        t = torch.tensor(3.6, dtype=torch.float64, device=DEV)
        out = torch.empty(3, 33, dtype=dtype, device=DEV)
        be._cde_contract(out, F, X._series, X._t, t, "cubic")
        dX = X.derivative(t)[:, 0, :].double().cpu().numpy()
        Fd = F.double().cpu().numpy()
        err = np.abs(out.double().cpu().numpy() - np.einsum("bhc,bc->bh", Fd, dX))
        bound = CO.gamma(C, _NPT[dtype]) * np.einsum("bhc,bc->bh", np.abs(Fd), np.abs(dX))
        print("C = {}, {}: worst err / bound = {:.3g}".format(C, dtype, float((err / bound).max())))
        assert (err <= bound).all()


def test_a_refused_call_leaves_the_output_standing():
    be = _hip.get_backend()
    series, knots = torch.randn(2, 5, 4, device=DEV), torch.arange(5.0, device=DEV)
    F, g = torch.randn(2, 3, 4, device=DEV), torch.randn(2, 3, device=DEV)
    out, gF = torch.full((2, 3), SENTINEL, device=DEV), torch.full((2, 3, 4), SENTINEL, device=DEV)
    st = be._stream(out)
    for sym, dst, src in (("xde_cde_contract", out, F), ("xde_cde_contract_backward", gF, g)):
        fn = getattr(be.lib, sym)
        good = [dst.data_ptr(), src.data_ptr(), series.data_ptr(), knots.data_ptr(), None, 1.5, 1, 2, 3, 4, 5, 0, 0, st]
        for i, v in ((1, None), (2, None), (3, None), (7, 0), (8, 0), (9, 0), (10, 1), (11, 2), (11, 9), (12, 2), (6, 2)):
            args = list(good)
            args[i] = v
            assert fn(*args) == _hip.XDE_EBADARG, (sym, i, v)
        with pytest.raises(_hip.XdeError, match="XDE_HISTORY_BEZIER is not a control path"):
            (be._cde_contract if dst is out else be._cde_contract_backward)(dst, src, series, knots, 1.5, "bez")
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all())
        assert fn(*good) == _hip.XDE_OK
        torch.cuda.synchronize()
        assert not bool((dst == SENTINEL).any())


def test_the_captured_adjoint_dynamics_give_the_eager_gradients_bit_for_bit(dev):
    """cdeint_adjoint with adjoint_options["graph_func"] = True (the contraction and its cotangent inside a captured HIP graph, the
    time read from device memory at every replay) against graph_func = False."""
    series, _, z0 = inputs(torch.float64)
    X = CubicHermiteSpline(torch.from_numpy(series).to(dev))
    z0 = torch.from_numpy(z0).to(dev)
    ts = torch.linspace(0.0, 7.0, 4, dtype=torch.float64).to(dev)
    field = _field(dev)

    def grads(captured):
        loss = lambda z: cdeint_adjoint(field, X, z, ts, solver=Dopri5, adjoint_options={"graph_func": captured}).square().sum()  # noqa: E731
        return _grads(loss, field, z0)

    eager, captured = grads(False), grads(True)
    for a, b in zip(eager, captured):
        assert np.abs(a).max() > 0 and np.array_equal(a, b)


@pytest.mark.parametrize("adjoint", [False, True])
def test_cde_demo_loss_falls(adjoint):
    """examples/cde_demo.py for a few iterations, through the steps and through the adjoint."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=8, n=32, length=16, adjoint=adjoint, log_every=0)
    assert all(np.isfinite(losses)) and sum(losses[-3:]) < 0.9 * sum(losses[:3]), losses
