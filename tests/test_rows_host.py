"""Per-sample adaptive stepping without a GPU: the C ABI of include/xde_hip_rows.h (every call below is refused on the host before
anything is enqueued), the bind, the launches of an attempt, what ``per_sample`` refuses, and the end-to-end cases of
tests/_rows_cases.py on the numpy double against the rows solved alone by the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from paddlexde_amd import RK4, AdaptiveHeun, Bosh3, Dopri5, Dopri8, Fehlberg2, _hip, odeint
from paddlexde_amd.utils import _rms_norm

from . import _rows_cases as RC
from . import _rows_oracle as RO

ATTEMPT = ["rows_stage_combine"] * 6 + ["rows_norm_control", "rows_dense_commit"]  # Dopri5: six stages, FSAL
FIRST_STEP = ["rows_scaled_norm", "rows_scaled_norm", "rows_stage_combine", "rows_scaled_norm"]


@pytest.fixture
def be():
    from ._rows_double import RowsDoubleBackend

    b = RowsDoubleBackend()
    _hip._set_backend_for_testing(b)
    try:
        yield b
    finally:
        _hip._set_backend_for_testing(None)


def _solve(lam, dtype, t=None, func=None, solver=Dopri5, tdtype=None, **opt):
    st = {}
    tdtype = dtype if tdtype is None else tdtype  # the time dtype: the state's unless said
    t = RC.t_of(tdtype) if t is None else t
    func = RC.func_of(lam, dtype) if func is None else func
    with torch.no_grad():
        sol = odeint(func, RC.y0_of(lam, dtype), t, solver, rtol=RC.RTOL, atol=RC.ATOL, options=dict(opt, per_sample=True, dtype=tdtype, stats_out=st))
    return sol, st


def _counts(st):
    return tuple(zip(st["n_accept"].tolist(), st["n_reject"].tolist()))


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_rows.h
# ----------------------------------------------------------------------------------------------
def test_the_rows_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("rows" in m.split("_") for m in pub - {"interp_rows"})
    for m in ("_rows_stage_combine", "_rows_norm_control", "_rows_dense_commit", "_rows_scaled_norm"):
        assert callable(getattr(_hip.HipBackend, m))


def test_rows_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    P = [0x100000 * (i + 1) for i in range(24)]  # (never dereferenced: every call is refused first)
    OUT, OUT2, Y0, Y1, F1, EP, TS, A, B = P[:9]
    KS = P[9:16]

    def ctl(**kw):
        c = _hip.XdeRowsCtl()
        for i, (name, _) in enumerate(_hip.XdeRowsCtl._fields_[2:]):
            setattr(c, name, 0x4000000 + 0x1000 * i)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def params(**kw):
        p = _hip.XdeCtrlParams()
        p.rtol, p.atol, p.max_step, p.safety, p.ifactor, p.dfactor, p.order = 1e-5, 1e-7, float("inf"), 0.9, 10.0, 0.2, 5.0
        p.max_num_steps, p.direction, p.n_stage, p.n_seg, p.norm_kind = 100, 1, 6, 1, _hip.NORM_RMS
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def ks(n, **at):
        arr = (C.c_void_p * 7)(*KS)
        for i, v in at.items():
            arr[int(i[1:])] = v
        return arr

    coef = (C.c_double * 7)(*([0.5] * 7))

    def combine(out=OUT, out2=None, y0=Y0, k=None, c=coef, c2=None, nk=3, ct=None, rows=2, D=4, dtype=0, null_ctl=False, f0=None):
        rc = lib.xde_rows_stage_combine(out, out2, y0, ks(nk) if k is None else k, c, c2, nk, None if null_ctl else C.byref(ct or ctl()),
                                        rows, D, dtype, None)
        return rc, lib.xde_last_error().decode()

    def control(k=None, c=coef, nk=1, ep=None, y0=Y0, y1=Y1, ct=None, p=None, ts=TS, n_out=3, rows=2, D=4, dtype=0, null_ctl=False, null_p=False,
                f0=None):
        rc = lib.xde_rows_norm_control(ks(nk) if k is None else k, c, nk, ep, y0, y1, None if null_ctl else C.byref(ct or ctl()),
                                       None if null_p else C.byref(p or params(state_dtype=dtype)), ts, n_out, rows, D, dtype, None)
        return rc, lib.xde_last_error().decode()

    def dense(out=OUT, k=None, c=coef, nk=2, y0=Y0, y1=Y1, f0=KS[0], f1=F1, ct=None, p=None, ts=TS, n_out=3, rows=2, D=4, dtype=0,
              null_ctl=False, null_p=False):
        rc = lib.xde_rows_dense_commit(out, ks(nk) if k is None else k, c, nk, y0, y1, f0, f1, None if null_ctl else C.byref(ct or ctl()),
                                       None if null_p else C.byref(p or params(state_dtype=dtype)), ts, n_out, rows, D, dtype, None)
        return rc, lib.xde_last_error().decode()

    def scaled(out=OUT, a=A, b=B, y0=Y0, rows=2, D=4, dtype=0):
        return lib.xde_rows_scaled_norm(out, a, b, y0, 1e-5, 1e-7, rows, D, dtype, None), lib.xde_last_error().decode()

    shape = [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3), dict(rows=1 << 21, D=(1 << 19) + 1), dict(dtype=2), dict(dtype=-1)]
    ctls = [dict(null_ctl=True), dict(ct=ctl(struct_size=8)), dict(ct=ctl(h=None)), dict(ct=ctl(done=None)), dict(ct=ctl(t=0x4000004)),
            dict(ct=ctl(accept=0x4000002)), dict(ct=ctl(t_stage=0x4000001))]
    nks = [dict(nk=0), dict(nk=8), dict(k=ks(3, k1=None), nk=3), dict(k=ks(3, k0=KS[0] + 2), f0=KS[0] + 2), dict(c=None)]
    outs = [dict(n_out=0), dict(n_out=-1), dict(n_out=1 << 30, rows=1 << 10, D=1 << 10)]
    pars = [dict(null_p=True), dict(p=params(struct_size=8)), dict(p=params(abi_version=5)), dict(p=params(direction=0)),
            dict(p=params(time_dtype=3)), dict(p=params(state_dtype=1)), dict(p=params(order=0.0)), dict(p=params(n_step_t=1)),
            dict(p=params(pi_controller=1)), dict(p=params(replay=0x100)), dict(p=params(norm_kind=_hip.NORM_LINF)), dict(p=params(n_stage=0))]
    n = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32)
    cases = [
        (combine, "xde_rows_stage_combine", shape + ctls + nks + [
            dict(out=None), dict(y0=None), dict(out2=OUT2), dict(c2=coef), dict(out=OUT + 2), dict(y0=Y0 + 4, dtype=1), dict(out2=OUT2 + 1, c2=coef),
            dict(out=Y0), dict(out=Y0 + n - 4), dict(out=KS[1] - n + 4), dict(out2=KS[2], c2=coef), dict(out2=OUT + 4, c2=coef)]),
        (control, "xde_rows_norm_control", shape + ctls + nks + outs + pars + [
            dict(y0=None), dict(y1=None), dict(ts=None), dict(ts=TS + 4), dict(ep=EP, nk=2), dict(ep=EP + 2), dict(y1=Y1 + 4, dtype=1),
            dict(D=(1 << 31) + 1, rows=1), dict(ct=ctl(t_stage=None))]),
        (dense, "xde_rows_dense_commit", shape + ctls + nks + outs + pars[:7] + [
            dict(out=None), dict(y0=None), dict(y1=None), dict(f0=None), dict(f1=None), dict(ts=None), dict(f0=KS[1]), dict(out=OUT + 1),
            dict(f1=F1 + 4, dtype=1), dict(y1=Y0 + 4), dict(f1=KS[0] + n - 4), dict(k=ks(2, k1=Y0)), dict(D=(1 << 31) + 1, rows=1)]),
        (scaled, "xde_rows_scaled_norm", shape + [dict(out=None), dict(a=None), dict(y0=None), dict(out=OUT + 4), dict(a=A + 2),
                                                  dict(b=B + 4, dtype=1), dict(D=(1 << 31) + 1, rows=1)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)


# ----------------------------------------------------------------------------------------------
# the double states the header's row sum
# ----------------------------------------------------------------------------------------------
def test_the_row_sum_is_a_function_of_the_row_alone(be):
    """The scaled norm of a row through the backend's launch does not depend on the rows beside it, at every lane count the header's
    row sum takes; and the double's launch is the header's statement (the sum's order included)."""
    gen = torch.Generator().manual_seed(0)
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        for D in (1, 3, 5, 64, 257, 1027, 3 * 4096 + 5):
            a, b, y0 = (torch.randn(3, D, generator=gen, dtype=torch.float64).to(dtype) for _ in range(3))
            whole = torch.empty(3, dtype=torch.float64)
            be._rows_scaled_norm(whole, a, b, y0, 1e-3, 1e-6)
            for r in range(3):
                one = torch.empty(1, dtype=torch.float64)
                be._rows_scaled_norm(one, a[r:r + 1].clone(), b[r:r + 1].clone(), y0[r:r + 1].clone(), 1e-3, 1e-6)
                assert one[0] == whole[r], (D, r)
            q = ((a - b).numpy() / (T(1e-6) + np.abs(y0.numpy()) * T(1e-3))).astype(np.float64)
            assert np.array_equal(whole.numpy(), RO.norm_of(RO.row_sum(q * q, T), D, T))
            assert np.allclose(whole.numpy(), np.sqrt((q * q).mean(axis=1)), rtol=1e-6)
    assert RO.lanes_of(1, np.float32) == (4, 1, 1) and RO.lanes_of(5, np.float32) == (4, 2, 2) and RO.lanes_of(257, np.float64) == (2, 129, 256)
    assert RO.lanes_of(3 * 4096 + 5, np.float32)[2] == 256
    assert be.launches == ["rows_scaled_norm"] * (2 * 7 * 4)


# ----------------------------------------------------------------------------------------------
# the launches of a solve
# ----------------------------------------------------------------------------------------------
def test_one_attempt_of_dopri5_is_exactly_the_expected_launch_list(be):
    lam = RC.LAM[:2]
    _, st = _solve(lam, torch.float64, first_step=0.01, check_every=1)
    attempts = max(a + r for a, r in _counts(st))
    assert be.launches == ATTEMPT * attempts  # a given first step: nothing but attempts, as many as the slowest row needs
    assert st["nfe"] == 1 + 6 * attempts
    del be.launches[:]
    _, st = _solve(lam, torch.float64)
    attempts = max(a + r for a, r in _counts(st))
    n = -(-attempts // 4) * 4  # the host looks every fourth attempt (the default): a late look costs attempts, never bits
    assert be.launches == FIRST_STEP + ATTEMPT * n and st["nfe"] == 2 + 6 * n
    del be.launches[:]
    _solve(lam, torch.float64, solver=Fehlberg2, first_step=0.01, check_every=64)  # not FSAL: two stages, the solution, norm, commit
    assert be.launches[:5] == ["rows_stage_combine"] * 3 + ["rows_norm_control", "rows_dense_commit"] and len(be.launches) % (5 * 64) == 0


def test_without_the_key_every_launch_is_the_parents(be):
    lam, dtype = RC.LAM[:2], torch.float64
    logs = []
    for opt in ({}, {"per_sample": False}):
        del be.launches[:]
        with torch.no_grad():
            sol = odeint(lambda t, y: -y, RC.y0_of(lam, dtype), RC.t_of(dtype), Dopri5, rtol=RC.RTOL, atol=RC.ATOL,
                         options=dict(opt, norm=_rms_norm, dtype=dtype))
        logs.append((list(be.launches), sol))
    assert logs[0][0] == logs[1][0] and torch.equal(logs[0][1], logs[1][1])
    assert not any(x.startswith("rows_") for x in logs[0][0])


# ----------------------------------------------------------------------------------------------
# what is refused, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals_say_what_works(be):
    dtype = torch.float64
    lam = RC.LAM[:2]
    y0, t, f = RC.y0_of(lam, dtype), RC.t_of(dtype), RC.func_of(lam, dtype)

    def call(solver=Dopri5, y0=y0, t=t, f=f, grad=False, **opt):
        with torch.enable_grad() if grad else torch.no_grad():
            return odeint(f, y0, t, solver, rtol=RC.RTOL, atol=RC.ATOL, options=dict(opt, per_sample=True))

    with pytest.raises(NotImplementedError, match="13 stages") as e:
        call(Dopri8)
    assert "follow-up" in str(e.value) and "Dopri5" in str(e.value)
    with pytest.raises(NotImplementedError, match="fixed-step") as e:
        call(RK4)
    assert "Dopri5, Bosh3, Fehlberg2 and AdaptiveHeun" in str(e.value)
    net = torch.nn.Linear(3, 3).double()
    for kw in (dict(y0=y0.clone().requires_grad_(True)), dict(t=t.clone().requires_grad_(True)), dict(f=_Net(net))):
        with pytest.raises(NotImplementedError, match="no_grad") as e:
            call(grad=True, **kw)
        assert "drop per_sample" in str(e.value) and "follow-up" in str(e.value)
    w = torch.tensor(0.5, dtype=dtype, requires_grad=True)  # a plain callable over a tensor that requires grad: seen in what it returns
    with pytest.raises(NotImplementedError, match="no_grad") as e:
        call(grad=True, f=lambda t_, y_: -w * y_)
    assert "closes over" in str(e.value) and be.launches == []
    call(f=lambda t_, y_: -w * y_, first_step=0.5, check_every=64)  # (under no_grad it is served)
    call(f=_Net(net), check_every=64, first_step=0.5, max_num_steps=1000)  # (the same module under no_grad is served)
    del be.launches[:]
    with pytest.raises(NotImplementedError, match="no_grad"):
        call(backprop="steps")
    with pytest.raises(NotImplementedError, match="tuple"):
        call(y0=(y0, y0))
    for key, val in (("step_t", [0.5]), ("jump_t", [0.5]), ("callback_step", print), ("callback_accept_step", print),
                     ("callback_reject_step", print), ("callback_accept", print), ("callback_reject", print)):
        with pytest.raises(NotImplementedError, match=key):
            call(**{key: val})
    cb = _Net(net)
    cb.callback_step = lambda t0, y0_, dt: None
    with pytest.raises(NotImplementedError, match="callback_step"):
        call(f=cb)
    with pytest.raises(NotImplementedError, match="controller='I'"):
        call(controller="PI")
    with pytest.raises(NotImplementedError, match="_rms_norm"):
        call(norm=lambda x: x.abs().max())
    with pytest.raises(NotImplementedError, match="process_group"):
        call(process_group=object())
    for pipeline in ("lag", "graph"):
        with pytest.raises(NotImplementedError, match="'auto' or 'sync'"):
            call(pipeline=pipeline)
    with pytest.raises(NotImplementedError, match="seam='auto' or 'launches'"):
        call(seam="resident")
    with pytest.raises(NotImplementedError, match="_replay"):
        call(_replay=[(0.1, True)])
    with pytest.raises(ValueError, match=r"y0\[None\]"):
        call(y0=y0[0].clone())
    with pytest.raises(ValueError, match="contiguous"):
        call(y0=RC.y0_of(lam, dtype).T.contiguous().T)
    with pytest.raises(NotImplementedError, match="record_trace"):
        call(record_trace=True)
    assert be.launches == []
    call(norm=_rms_norm, pipeline="sync", seam="launches", controller="I", first_step=0.5)  # (the defaults, spelled out, are served)
    assert be.launches


class _Net(torch.nn.Module):
    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, t, y):
        return -y + 0.01 * self.lin(y)


# ----------------------------------------------------------------------------------------------
# end to end on the double, against the rows solved alone by the oracle
# ----------------------------------------------------------------------------------------------
def test_the_five_row_problem_in_fp64_steps_every_row_as_if_alone(be):
    """Counts per row equal the row-alone oracle's, attempt for attempt; the solution within 16 x the deviation measured on the double
    (1.4e-14: the oracle's norms are numpy's pairwise sums, the kernels' THE ROW SUM).  The counts spelled out below are those of
    tests/_rows_cases.py's initial state (1, 0.5, -0.25) in every row."""
    dtype = torch.float64
    sol, st = _solve(RC.LAM, dtype)
    ref, counts = RC.reference(RC.LAM, dtype)
    assert _counts(st) == counts == ((5, 1), (11, 0), (26, 1), (66, 2), (157, 2))
    dev = np.abs(sol.numpy() - ref).max()
    print("fp64 deviation from the rows solved alone:", dev)
    assert dev <= RC.BAR[dtype]
    # the joint solve takes one step size for all: every row pays the stiffest row's attempts, and that row misses its tolerance
    joint_st = {}
    with torch.no_grad():
        joint = odeint(RC.func_of(RC.LAM, dtype), RC.y0_of(RC.LAM, dtype), RC.t_of(dtype), Dopri5, rtol=RC.RTOL, atol=RC.ATOL,
                       options={"norm": _rms_norm, "dtype": dtype, "stats_out": joint_st})
    assert joint_st["n_accept"] + joint_st["n_reject"] > 140
    assert np.abs(joint.numpy() - ref)[:, 4].max() > 1e3 * np.abs(sol.numpy() - ref)[:, 4].max()


def test_the_five_row_problem_in_fp32_holds_the_bar(be):
    dtype = torch.float32
    sol, st = _solve(RC.LAM, dtype)
    ref, counts = RC.reference(RC.LAM, dtype)
    dev = np.abs(sol.numpy() - ref).max()
    print("fp32 counts", _counts(st), "oracle", counts, "deviation", dev)  # (free-running fp32 decisions part by an ulp of h: DESIGN 2)
    assert dev <= RC.BAR[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_independence_bit_for_bit(be, dtype):
    a, b, c = 2.0, 50.0, 200.0
    two, _ = _solve((a, b), dtype)
    three, st = _solve((a, c, b), dtype)
    alone, _ = _solve((a,), dtype)
    assert torch.equal(two[:, 0], three[:, 0]) and torch.equal(two[:, 1], three[:, 2]) and torch.equal(alone[:, 0], two[:, 0])
    looked_late, _ = _solve((a, c, b), dtype, check_every=7)
    assert torch.equal(looked_late, three)


def test_equal_rows_give_equal_rows(be):
    sol, st = _solve((10.0,) * 4, torch.float32)
    assert all(torch.equal(sol[:, 0], sol[:, r]) for r in range(1, 4)) and len(set(_counts(st))) == 1


def test_a_decreasing_t_span(be):
    dtype = torch.float64
    fwd = RC.func_of(RC.LAM, dtype)
    sol, st = _solve(RC.LAM, dtype, t=-RC.t_of(dtype), func=lambda t, y: -fwd(t, y))
    ref, counts = RC.reference(RC.LAM, dtype, reverse=True)
    assert _counts(st) == counts and np.abs(sol.numpy() - ref).max() <= RC.BAR[dtype]
    assert bool((st["t"] <= -2.0).all()) and bool((st["dt_next"] < 0).all())  # native signed steps


def test_time_dtype_other_than_the_state_dtype(be):
    """fp64 state under fp32 times: counts equal the oracle's, the fp64 bar holds.  fp32 state under fp64 times (the heuristic's probe
    time and every stage time rounded from fp64 to the state dtype): its own bar, 16 x the 7.0e-6 measured on the double; counts
    recorded, as for every fp32 state."""
    sol, st = _solve(RC.LAM, torch.float64, tdtype=torch.float32)
    ref, counts = RC.reference(RC.LAM, torch.float64, tdtype=torch.float32)
    assert _counts(st) == counts and np.abs(sol.numpy() - ref).max() <= RC.BAR[torch.float64]
    assert st["t"].dtype == torch.float64 and bool((st["t"] == st["t"].float().double()).all())  # doubles holding fp32 values
    sol, st = _solve(RC.LAM, torch.float32, tdtype=torch.float64)
    ref, counts = RC.reference(RC.LAM, torch.float32, tdtype=torch.float64)
    dev = np.abs(sol.numpy() - ref).max()
    print("fp32 state, fp64 time: counts", _counts(st), "oracle", counts, "deviation", dev)
    assert sol.dtype == torch.float32 and dev <= RC.BAR_F32_STATE_F64_TIME


@pytest.mark.parametrize("opt", [dict(first_step=0.01), dict(max_step=0.05), dict(first_step=0.3, max_step=0.25, min_step=0.001)], ids=str)
def test_first_step_and_max_step(be, opt):
    dtype = torch.float64
    sol, st = _solve(RC.LAM, dtype, **opt)
    ref, counts = RC.reference(RC.LAM, dtype, **opt)
    assert _counts(st) == counts and np.abs(sol.numpy() - ref).max() <= RC.BAR[dtype]
    if "first_step" not in opt:
        assert "rows_scaled_norm" in be.launches
    else:
        assert "rows_scaled_norm" not in be.launches


@pytest.mark.parametrize("solver, name", [(Bosh3, "bosh3"), (Fehlberg2, "fehlberg2"), (AdaptiveHeun, "adaptive_heun")])
def test_the_other_served_solvers(be, solver, name):
    dtype, lam = torch.float64, RC.LAM[:3]
    sol, st = _solve(lam, dtype, solver=solver)
    ref, counts = RC.reference(lam, dtype, solver=name)
    assert _counts(st) == counts and np.abs(sol.numpy() - ref).max() <= RC.BAR[dtype]


def test_a_step_covering_three_outputs(be):
    dtype = torch.float64
    sol, st = _solve(RC.LAM, dtype, t=RC.t_of(dtype, n=21))
    ref, counts = RC.reference(RC.LAM, dtype, n=21)
    assert _counts(st) == counts and np.abs(sol.numpy() - ref).max() <= RC.BAR[dtype]
    assert counts[0][0] * 3 < 20  # row 0 takes 5 accepted steps over 20 output intervals: a step holds 3 outputs or more


def test_a_row_that_finishes_early_stays_frozen_bit_for_bit(be):
    dtype, lam = torch.float64, (0.5, 200.0)
    inner = RC.func_of(lam, dtype)
    seen = []

    def func(t, y):
        seen.append((t[0].clone(), y[0].clone()))
        return inner(t, y)

    sol, st = _solve(lam, dtype, func=func)
    (a0, r0), (a1, r1) = _counts(st)
    assert (a1 + r1) - (a0 + r0) > 100
    alone, _ = _solve(lam[:1], dtype)
    assert torch.equal(sol[:, 0], alone[:, 0])
    after = seen[2 + 6 * (a0 + r0):]  # the evaluations of the attempts after row 0's last one
    assert len(after) > 600
    assert all(torch.equal(t, after[0][0]) and torch.equal(y, after[0][1]) for t, y in after)
    assert float(after[0][0]) == float(st["t"][0]) >= 2.0


def test_max_num_steps_names_the_row(be):
    dtype, lam = torch.float64, (0.5, 200.0, 2.0)
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(20>=20\) \(row 1 of the batch\)"):
        _solve(lam, dtype, t=torch.tensor([0.0, 2.0], dtype=dtype), max_num_steps=20)
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(20>=20\)"):  # the reference's message for that row alone
        RO.solve_alone(lambda r: RC.np_func_of(lam, np.float64)(1), RC.y0_of(lam, dtype).numpy()[1:2], np.array([0.0, 2.0]), "dopri5",
                       rtol=RC.RTOL, atol=RC.ATOL, options={"dtype": np.float64, "max_num_steps": 20})
    sol, _ = _solve(lam, dtype, t=torch.tensor([0.0, 2.0], dtype=dtype), max_num_steps=20, func=RC.func_of((0.5, 1.0, 2.0), dtype))
    assert sol.shape == (2, 3, 3)  # (rows that stay under the budget are served)


def test_the_other_two_status_messages_name_the_row(be):
    dtype, lam = torch.float64, (0.5, 2.0)
    y_bad = RC.y0_of(lam, dtype)
    y_bad[1, 2] = float("nan")
    with torch.no_grad(), pytest.raises(AssertionError, match=r"non-finite values in state `y`: 1 non-finite element\(s\) \(row 1 of the batch\)"):
        odeint(RC.func_of(lam, dtype), y_bad, RC.t_of(dtype), Dopri5, rtol=RC.RTOL, atol=RC.ATOL, options={"per_sample": True, "dtype": dtype,
                                                                                                        "first_step": 0.1})
    with pytest.raises(AssertionError, match=r"underflow in dt .* \(row 0 of the batch\)"):
        _solve(lam, dtype, t=torch.tensor([1e30, 2e30], dtype=dtype), first_step=1.0)
