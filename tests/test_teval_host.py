"""Per-sample output times (``options["t_eval"]``) without a GPU: the C ABI of include/xde_hip_teval.h (every call below is refused on
the host before anything is enqueued), what ``t_eval`` refuses, and the end-to-end cases of tests/_teval_cases.py on the numpy double:
the forward bit for bit against the existing ``odeint`` on the union of the times, the gradients against the eager twin."""
import ctypes as C
import gc
import weakref

import numpy as np
import pytest
import torch

from paddlexde_amd import RK4, AdaptiveHeun, Bosh3, Dopri5, Dopri8, Fehlberg2, _hip, odeint
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _teval_cases as TC
from ._backprop_twin import twin_odeint

SOLVERS = [(Dopri5, "dopri5"), (Dopri8, "dopri8"), (Bosh3, "bosh3"), (Fehlberg2, "fehlberg2"), (AdaptiveHeun, "adaptive_heun")]


@pytest.fixture
def be():
    from ._teval_double import TevalDoubleBackend

    b = TevalDoubleBackend()
    _hip._set_backend_for_testing(b)
    try:
        yield b
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_teval.h
# ----------------------------------------------------------------------------------------------
def test_the_teval_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("teval" in m for m in pub)
    for m in ("_teval_dense", "_teval_cotangent"):
        assert callable(getattr(_hip.HipBackend, m))


def test_teval_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    P = [0x100000 * (i + 1) for i in range(32)]  # (never dereferenced: every call is refused first)
    OUT, TQ, CNT, Y0, Y1, F0, F1, G = P[:8]
    KS = P[8:22]
    OS = P[22:27]
    mid = (C.c_double * 14)(*([0.5] * 14))

    def ks(**at):
        arr = (C.c_void_p * 14)(*KS)
        for i, v in at.items():
            arr[int(i[1:])] = v
        return arr

    def outs(**at):
        arr = (C.c_void_p * 5)(*OS)
        for i, v in at.items():
            arr[int(i[1:])] = v
        return arr

    def dense(out=OUT, tq=TQ, cnt=CNT, k=None, c=mid, nk=3, y0=Y0, y1=Y1, f0=F0, f1=F1, t0=0.0, t1=0.5, dt=0.5, direction=1, time_dtype=0,
              rows=2, D=4, Q=3, dtype=0, null_k=False, **_):
        rc = lib.xde_teval_dense(out, tq, cnt, None if null_k else (ks() if k is None else k), c, nk, y0, y1, f0, f1, t0, t1, dt, direction,
                                 time_dtype, rows, D, Q, dtype, None)
        return rc, lib.xde_last_error().decode()

    def cot(o=None, g=G, tq=TQ, cnt=CNT, t0=0.0, t1=0.5, dt=0.5, direction=1, time_dtype=0, acc=0, rows=2, D=4, Q=3, dtype=0, null_o=False,
            **_):
        rc = lib.xde_teval_cotangent(None if null_o else (outs() if o is None else o), g, tq, cnt, t0, t1, dt, direction, time_dtype, acc,
                                     rows, D, Q, dtype, None)
        return rc, lib.xde_last_error().decode()

    inf, nan = float("inf"), float("nan")
    shared = [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3), dict(rows=1 << 21, D=(1 << 19) + 1), dict(D=(1 << 31) + 1, rows=1),
              dict(Q=0), dict(Q=-1), dict(Q=1 << 31), dict(Q=1 << 30, rows=1 << 10, D=1 << 10), dict(dtype=2), dict(dtype=-1),
              dict(time_dtype=2), dict(time_dtype=-1), dict(direction=0), dict(direction=2), dict(t0=nan), dict(t1=inf), dict(dt=nan),
              dict(t1=0.0), dict(t0=0.5, t1=0.0), dict(t0=0.0, t1=-0.5), dict(t0=-0.5, t1=0.0, direction=-1),
              dict(tq=None), dict(cnt=None), dict(tq=TQ + 4), dict(cnt=CNT + 2)]
    n = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32)
    cases = [
        (dense, "xde_teval_dense", shared + [
            dict(out=None), dict(y0=None), dict(y1=None), dict(f0=None), dict(f1=None), dict(null_k=True), dict(c=None), dict(nk=0), dict(nk=15),
            dict(k=ks(k1=None)), dict(k=ks(k0=KS[0] + 2)), dict(out=OUT + 2), dict(y0=Y0 + 1), dict(f1=F1 + 4, dtype=1), dict(out=Y0),
            dict(out=Y0 - 3 * n + 4), dict(out=F1 + n - 4), dict(k=ks(k2=OUT + 2 * n))]),
        (cot, "xde_teval_cotangent", shared + [
            dict(null_o=True), dict(g=None), dict(o=outs(o0=None, o1=None, o2=None, o3=None, o4=None)), dict(acc=32), dict(acc=0x80),
            dict(g=G + 2), dict(o=outs(o1=OS[1] + 1)), dict(o=outs(o3=OS[3] + 4), dtype=1), dict(o=outs(o0=G)), dict(o=outs(o4=G + 3 * n - 4)),
            dict(o=outs(o2=OS[1])), dict(o=outs(o2=OS[1] + n - 4))])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)


# ----------------------------------------------------------------------------------------------
# what is refused, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals_say_what_works(be):
    dtype = torch.float64
    func, y0, ends = TC.five_row_problem(dtype)
    tq = TC.five_row_times(dtype)
    t = torch.tensor(ends, dtype=dtype)

    def call(solver=Dopri5, y0=y0, t=t, f=func, tq=tq, grad=False, **opt):
        with torch.enable_grad() if grad else torch.no_grad():
            return odeint(f, y0, t, solver, rtol=1e-5, atol=1e-7, options=dict(opt, t_eval=tq, norm=_rms_norm, dtype=dtype))

    def with_(r, q, v):
        x = tq.clone()
        x[r, q] = v
        return x

    with pytest.raises(NotImplementedError, match="fixed-step") as e:
        call(RK4)
    assert "union" in str(e.value)
    with pytest.raises(NotImplementedError, match="tuple"):
        call(y0=(y0, y0))
    with pytest.raises(ValueError, match=r"y0\[None\]"):
        call(y0=y0[0].clone())
    with pytest.raises(ValueError, match="contiguous"):
        call(y0=y0.T.contiguous().T)
    for bad_t in (torch.tensor([0.0, 1.0, 2.0], dtype=dtype), torch.tensor([0.0], dtype=dtype)):
        with pytest.raises(ValueError, match="exactly two times"):
            call(t=bad_t)
    with pytest.raises(TypeError, match="torch tensor"):
        call(tq=tq.tolist())
    for bad_q in (tq[0], tq[:4], tq[:, :0], tq[:, :, None]):
        with pytest.raises(ValueError, match=r"\[rows, Q\]"):
            call(tq=bad_q)
    with pytest.raises(TypeError, match="float32 or float64"):
        call(tq=torch.zeros(5, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match="t_eval.to"):
        call(tq=tq.to("meta"))
    with pytest.raises(ValueError, match=r"row 2, column 3: the time 0\.01 lies behind"):
        call(tq=with_(2, 3, 0.01))
    with pytest.raises(ValueError, match=r"row 0, column 6: the time 2\.5 lies outside the interval"):
        call(tq=with_(0, 6, 2.5))
    with pytest.raises(ValueError, match=r"row 1, column 0: the time -0\.5 lies outside"):
        call(tq=with_(1, 0, -0.5))
    with pytest.raises(ValueError, match=r"row 0, column 6: the time inf lies outside"):
        call(tq=with_(0, 6, float("inf")))
    with pytest.raises(ValueError, match=r"row 3 has the time 1\.9 in column 6 after a NaN"):
        call(tq=with_(3, 6, 1.9))
    with pytest.raises(NotImplementedError, match="detach"):
        call(tq=tq.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="jump at every distinct time"):
        call(backprop="adjoint")
    with pytest.raises(ValueError, match="'steps' or 'adjoint'"):
        call(backprop="through")
    with pytest.raises(NotImplementedError, match="process_group"):
        call(process_group=object())
    for pipeline in ("lag", "graph"):
        with pytest.raises(NotImplementedError, match="'auto' or 'sync'"):
            call(pipeline=pipeline)
    for key in ("step_t", "jump_t"):
        with pytest.raises(NotImplementedError, match=key):
            call(**{key: [0.5]})
    with pytest.raises(NotImplementedError, match="t_span"):
        call(t=t.clone().requires_grad_(), grad=True)
    with pytest.raises(NotImplementedError, match=r"does not take the option\(s\) \['t_eval'\]"):  # per_sample's own message
        call(per_sample=True)
    assert be.launches == []
    call(pipeline="sync", backprop="steps")  # (the defaults, spelled out, are served)
    assert "teval_dense" in be.launches


def test_without_the_key_every_launch_is_the_parents(be):
    dtype = torch.float64
    func, y0, ends = TC.five_row_problem(dtype)
    with torch.no_grad():
        odeint(func, y0, torch.tensor(ends, dtype=dtype), Dopri5, rtol=1e-5, atol=1e-7, options={"norm": _rms_norm, "dtype": dtype})
    assert be.launches and not any(x.startswith("teval") for x in be.launches)


# ----------------------------------------------------------------------------------------------
# end to end on the double: the forward, bit for bit against the union solve
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["rising", "falling"])
@pytest.mark.parametrize("dtype, tdtype", [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float32, torch.float64)],
                         ids=["fp32", "fp64", "fp32-state-fp64-time"])
def test_forward_equals_the_union_solve_bit_for_bit(be, dtype, tdtype, reverse):
    func, y0, ends = TC.five_row_problem(dtype, reverse)
    tq = TC.five_row_times(tdtype, reverse)
    with torch.no_grad():
        sol, steps = TC.solve_teval(func, y0, ends, tq, Dopri5, tdtype)
        launches = list(be.launches)
        union, idx = TC.solve_union(func, y0, ends, tq, Dopri5, tdtype)
    assert sol.shape == (7, 5, 3) and sol.dtype == dtype
    assert torch.equal(sol, TC.gather(union, idx))
    assert bool((sol[4:, 3] == 0).all()) and bool((sol[2:, 4] == 0).all()) and torch.equal(sol[0, 1], y0[1])
    held = TC.held_per_step(steps, tq, ends, tdtype)
    assert any(max(h) >= 2 for h in held), "some step holds two queries of one row"
    assert any(0 < sum(1 for x in h if x) < 5 for h in held), "some step holds queries of some rows only"
    assert any(sum(h) == 0 for h in held), "some step holds none"
    assert sum(sum(h) for h in held) == int((~torch.isnan(tq)).sum()) - 1  # every query but the one at the start, exactly once
    # one launch per accepted step that holds a query and none otherwise (the joint solve's own dense launch is the one of its end time)
    assert launches.count("teval_dense") == sum(1 for h in held if sum(h)) and launches.count("dense") == 1


@pytest.mark.parametrize("solver, name", SOLVERS[1:], ids=[n for _, n in SOLVERS[1:]])
def test_forward_with_the_other_solvers(be, solver, name):
    dtype = torch.float64
    func, y0, ends = TC.five_row_problem(dtype)
    tq = TC.five_row_times(dtype)
    with torch.no_grad():
        sol, _ = TC.solve_teval(func, y0, ends, tq, solver, dtype, rtol=1e-4, atol=1e-6)
        union, idx = TC.solve_union(func, y0, ends, tq, solver, dtype, rtol=1e-4, atol=1e-6)
    assert torch.equal(sol, TC.gather(union, idx))


def test_the_default_options_are_served(be):
    """``options={"t_eval": tq}`` alone: the RMS norm and fp32 times, as ``odeint``'s own defaults."""
    func, y0, ends = TC.five_row_problem(torch.float32)
    tq = TC.five_row_times(torch.float32)
    with torch.no_grad():
        sol = odeint(func, y0, torch.tensor(ends), Dopri5, rtol=1e-4, atol=1e-6, options={"t_eval": tq})
        ref, _ = TC.solve_teval(func, y0, ends, tq, Dopri5, torch.float32, rtol=1e-4, atol=1e-6)
    assert torch.equal(sol, ref)


# ----------------------------------------------------------------------------------------------
# gradients on the double against the eager twin
# ----------------------------------------------------------------------------------------------
def _teval_grads(f, y0, tq, solver, **opt):
    y0 = y0.clone().requires_grad_()
    sol, steps = TC.solve_teval(f, y0, TC.MLP_ENDS, tq, solver, y0.dtype, **opt)
    w = TC.loss_weights(sol)
    return sol.detach(), torch.autograd.grad(TC.loss_of(sol, w), [y0] + list(f.parameters())), steps, w


def _twin_grads(f, y0, tq, name, steps, w):
    times, idx = TC.union_of(tq, TC.MLP_ENDS)
    y0 = y0.clone().requires_grad_()
    sol = TC.gather(twin_odeint(f, y0, times, name, steps), idx)
    return sol.detach(), torch.autograd.grad(TC.loss_of(sol, w), [y0] + list(f.parameters()))


@pytest.mark.parametrize("solver, name", SOLVERS, ids=[n for _, n in SOLVERS])
def test_gradients_match_the_twin_fp64(be, solver, name):
    f, y0 = TC.MLP(), TC.mlp_y0(torch.float64)
    tq = torch.tensor(TC.MLP_TIMES, dtype=torch.float64)
    sol, grads, steps, w = _teval_grads(f, y0, tq, solver)
    held = TC.held_per_step(steps, tq, TC.MLP_ENDS, torch.float64)
    assert any(max(h) >= 2 for h in held) and any(sum(h) == 0 for h in held[:-1])
    assert be.launches.count("teval_cotangent") == be.launches.count("teval_dense") == sum(1 for h in held if sum(h))
    assert "dense_cotangent" not in be.launches
    tsol, tgrads = _twin_grads(f, y0, tq, name, steps, w)
    assert TC.rel(sol, tsol) <= 1e-12
    for a, b in zip(grads, tgrads):
        print(name, "gradient, normwise relative to the twin:", TC.rel(a, b))
        assert TC.rel(a, b) <= 1e-10


def test_gradients_in_falling_time_fp64(be):
    f, y0 = TC.MLP(), TC.mlp_y0(torch.float64)
    tq = 1.6 - 0.3 * torch.tensor(TC.MLP_TIMES, dtype=torch.float64)  # on [1.6, 0.1]
    ends = [1.6, 0.1]
    y0g = y0.clone().requires_grad_()
    sol, steps = TC.solve_teval(f, y0g, ends, tq, Dopri5, torch.float64)
    w = TC.loss_weights(sol)
    grads = torch.autograd.grad(TC.loss_of(sol, w), [y0g] + list(f.parameters()))
    times, idx = TC.union_of(tq, ends)
    y0t = y0.clone().requires_grad_()
    tsol = TC.gather(twin_odeint(f, y0t, times, "dopri5", steps), idx)
    tgrads = torch.autograd.grad(TC.loss_of(tsol, w), [y0t] + list(f.parameters()))
    for a, b in zip(grads, tgrads):
        assert TC.rel(a, b) <= 1e-10


def test_the_backprop_key_and_the_padding_change_nothing(be):
    """``backprop="steps"`` spelled out gives the same bits; what the loss puts on padded entries and on an all-NaN row reaches nothing."""
    f, y0 = TC.MLP(), TC.mlp_y0(torch.float64)
    tq = torch.tensor(TC.MLP_TIMES, dtype=torch.float64)
    sol, grads, _, w = _teval_grads(f, y0, tq, Dopri5)
    sol2, grads2, _, _ = _teval_grads(f, y0, tq, Dopri5, backprop="steps")
    assert torch.equal(sol, sol2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    pad = torch.isnan(tq).t()  # [Q, rows]
    assert bool((sol[pad] == 0).all())
    y0g = y0.clone().requires_grad_()
    out, _ = TC.solve_teval(f, y0g, TC.MLP_ENDS, tq, Dopri5, torch.float64)
    noise = torch.where(pad[:, :, None], torch.full_like(w, 1e6), torch.zeros_like(w))
    g3 = torch.autograd.grad(TC.loss_of(out, w) + (out * noise).sum(), [y0g] + list(f.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(grads, g3))
    assert bool((grads[0][2] == 0).all())  # the row without an observation


def test_nothing_requires_grad_is_a_plain_solve(be):
    f, y0 = TC.MLP().requires_grad_(False), TC.mlp_y0(torch.float64)
    tq = torch.tensor(TC.MLP_TIMES, dtype=torch.float64)
    sol, _ = TC.solve_teval(f, y0, TC.MLP_ENDS, tq, Dopri5, torch.float64)
    assert sol.grad_fn is None and "teval_cotangent" not in be.launches
    f.requires_grad_(True)
    with torch.no_grad():
        sol2, _ = TC.solve_teval(f, y0.clone().requires_grad_(), TC.MLP_ENDS, tq, Dopri5, torch.float64)
    assert sol2.grad_fn is None and torch.equal(sol, sol2)


def test_nothing_of_the_solve_outlives_backward_without_the_cycle_collector(be):
    f = TC.MLP()
    refs = []

    def hook(i, y0_, y1, ks, c):
        refs.extend(weakref.ref(x) for x in [y1] + list(ks[1:]))

    gc.collect()
    gc.disable()
    try:
        y0 = TC.mlp_y0(torch.float64).requires_grad_()
        tq = torch.tensor(TC.MLP_TIMES, dtype=torch.float64)
        sol = odeint(f, y0, torch.tensor(TC.MLP_ENDS, dtype=torch.float64), Dopri5,
                     options={"norm": _rms_norm, "dtype": torch.float64, "t_eval": tq, "_step_hook": hook})
        sol.square().sum().backward()
        del sol
        assert refs and not [r for r in refs if r() is not None]
    finally:
        gc.enable()


# ----------------------------------------------------------------------------------------------
# the oracle's membership is the kernels' binary search
# ----------------------------------------------------------------------------------------------
def test_membership_puts_every_later_query_in_exactly_one_step():
    from . import _teval_oracle as TO

    for TT in (np.float32, np.float64):
        row = np.array([0.0, 0.25, 0.25, 0.5, 1.0, np.nan], dtype=np.float64)
        edges = [0.0, 0.25, 0.3, 1.0]
        got = [TO.members(row, 5, a, b, 1, TT) for a, b in zip(edges[:-1], edges[1:])]
        assert got == [[1, 2], [], [3, 4]]  # the query at t0 = 0 is in none; one equal to t1 closes its step
        got = [TO.members(-row, 5, -a, -b, -1, TT) for a, b in zip(edges[:-1], edges[1:])]
        assert got == [[1, 2], [], [3, 4]]
