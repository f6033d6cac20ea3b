"""``ddeint_steps`` without a GPU: the C ABI of include/xde_hip_dde.h (every call below is refused on the host before anything is
enqueued), the bind, the double against an independent numpy expression, the Hermite weights and the interval rule case by case, the
launches of a walk, what is refused, the tape's memory under ``no_grad``, and the end-to-end cases of tests/_dde_tape_cases.py on the
numpy double."""
import ctypes as C

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import ddeint, ddeint_steps, odeint
from paddlexde_amd.functional.ddeint_steps import _problem
from paddlexde_amd.solver import RK4, AdamsBashforthMoulton, Dopri5, Euler, Midpoint
from paddlexde_amd.solver._autograd import DdeTapeGatherFn
from paddlexde_amd.xde.base_ode import BaseODE
from paddlexde_amd.xde.steps_dde import StepsDDE, hermite_weights, pick_interval

from oracle import xde_oracle as O

from . import _dde_tape_oracle as DO
from ._dde_cases import _dde_func_np, _dde_func_t
from ._dde_tape_cases import *  # noqa: F401,F403
from ._dde_tape_cases import _history

MAXL = _hip.XDE_DDE_MAX_LAGS


@pytest.fixture
def dev():
    from ._dde_tape_double import DdeTapeDoubleBackend

    _hip._set_backend_for_testing(DdeTapeDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_dde.h
# ----------------------------------------------------------------------------------------------
def test_the_header_sits_between_gn_and_rows_and_the_methods_are_private():
    order = list(_hip.HEADERS)
    assert order.index("xde_hip_gn.h") + 1 == order.index("xde_hip_dde.h") == order.index("xde_hip_rows.h") - 1
    assert list(_hip.HEADERS["xde_hip_dde.h"]) == ["xde_dde_tape_gather", "xde_dde_tape_gather_backward"]
    assert _hip.XDE_DDE_MAX_LAGS == 16 and _hip.ABI_VERSION == 6
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("dde" in m.split("_") or "tape" in m for m in pub)
    for m in ("_dde_tape_gather", "_dde_tape_gather_backward"):
        assert callable(getattr(_hip.HipBackend, m))
    from paddlexde_amd import functional
    import paddlexde_amd

    assert functional.ddeint_steps is ddeint_steps and not hasattr(paddlexde_amd, "ddeint_steps")
    assert issubclass(StepsDDE, BaseODE) and StepsDDE.fuse is BaseODE.fuse


def _arr(ctype, xs):
    return (ctype * len(xs))(*xs)


def test_dde_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    OUT, DT, G = 0x100000, 0x200000, 0x300000  # (never dereferenced: every call is refused first)
    SRC = [0x400000 + 0x10000 * i for i in range(4 * MAXL)]
    GS = [0x800000 + 0x10000 * i for i in range(4 * MAXL)]

    def gather(out=OUT, dtau=DT, src=SRC, stride=None, w=True, wd=True, rows=2, D=4, L=2, j0=0, Ltot=2, dtype=0, null_src=False, null_stride=False):
        stride = [D] * len(src) if stride is None else stride
        ws = _arr(C.c_double, [0.25] * len(src))
        rc = lib.xde_dde_tape_gather(out, dtau, None if null_src else _arr(C.c_void_p, src), None if null_stride else _arr(C.c_int64, stride),
                                     ws if w else None, ws if wd else None, rows, D, L, j0, Ltot, dtype, None)
        return rc, lib.xde_last_error().decode()

    def bwd(gsrc=GS[:2], first=(0, 2, 3), lag=(0, 1, 1), wt=(0.5, 0.25, 1.0), nq=2, g=G, rows=2, D=4, j0=0, Ltot=2, dtype=0, null=()):
        args = dict(gsrc=_arr(C.c_void_p, list(gsrc)), first=_arr(C.c_int32, list(first)), lag=_arr(C.c_int32, list(lag)), wt=_arr(C.c_double, list(wt)))
        for name in null:
            args[name] = None
        rc = lib.xde_dde_tape_gather_backward(args["gsrc"], args["first"], args["lag"], args["wt"], nq, g, rows, D, j0, Ltot, dtype, None)
        return rc, lib.xde_last_error().decode()

    n = 2 * 4 * 4  # bytes of a rows x D operand at the default shape (fp32); an output of the gather holds Ltot = 2 times as many
    shape = [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3), dict(D=(1 << 30) + 1), dict(rows=1 << 40, D=1 << 9),
             dict(rows=1 << 20, D=1 << 20, Ltot=1 << 9), dict(j0=-1), dict(dtype=2), dict(dtype=-1)]
    one_off = lambda i, v: SRC[:i] + [v] + SRC[i + 1:]  # noqa: E731
    cases = [(gather, "xde_dde_tape_gather", [dict(out=None), dict(null_src=True), dict(null_stride=True), dict(w=False), dict(src=one_off(5, None))]
              + shape + [dict(L=0), dict(L=MAXL + 1, Ltot=MAXL + 1), dict(j0=1), dict(L=2, Ltot=1), dict(j0=3, Ltot=4, L=2),
                         dict(stride=[4] * 3 + [3] + [4] * 60), dict(stride=[4] * 7 + [0] + [4] * 56),  # a stride below D
                         dict(dtau=None), dict(wd=False),  # dtau / wd given singly
                         dict(out=OUT + 2), dict(dtau=DT + 1), dict(src=one_off(2, SRC[2] + 2)), dict(src=one_off(0, SRC[0] + 4), dtype=1),  # alignment
                         dict(out=SRC[3]), dict(out=SRC[3] - 2 * n + 4), dict(out=SRC[3] + n - 4), dict(dtau=SRC[6] + 4),  # an output over an operand
                         dict(dtau=OUT + 2 * n - 4), dict(dtau=OUT),  # ... and over the other output
                         dict(src=one_off(1, OUT + 16), stride=[4, 1 << 10] + [4] * 62)]),  # (an operand's extent follows its stride)
             (bwd, "xde_dde_tape_gather_backward", [dict(null=("gsrc",)), dict(null=("first",)), dict(null=("lag",)), dict(null=("wt",)), dict(g=None),
                                                    dict(gsrc=[GS[0], None])] + shape + [
                 dict(nq=0), dict(nq=4 * MAXL + 1), dict(first=(1, 2, 3)),
                 dict(first=(0, 0, 3)), dict(first=(0, 3, 3)),  # a term list with an empty output
                 dict(first=(0, 2, 4 * MAXL + 1)), dict(lag=(0, 2, 1)), dict(lag=(0, -1, 1)), dict(j0=1), dict(Ltot=1),
                 dict(g=G + 2), dict(gsrc=[GS[0] + 1, GS[1]]), dict(gsrc=[GS[0] + 4, GS[1]], dtype=1),
                 dict(gsrc=[G, GS[1]]), dict(gsrc=[GS[0], G + 2 * n - 4]), dict(gsrc=[GS[0], G - n + 4]), dict(gsrc=[GS[0], GS[0] + n - 4]),
                 dict(gsrc=[GS[0], GS[0]])])]
    for fn, name, bad in cases:
        for kw in bad:  # (the well-formed default call itself is never sent: its pointers are made up)
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert msg.startswith(name + ":"), (kw, msg)


# ----------------------------------------------------------------------------------------------
# the double states the header
# ----------------------------------------------------------------------------------------------
def test_the_double_states_the_header(dev):
    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        gen = torch.Generator().manual_seed(3)
        rows, D, L, Th = 3, 7, 3, 4
        his = torch.randn(rows, Th, D, generator=gen, dtype=dtype)
        nodes = [torch.randn(rows, D, generator=gen, dtype=dtype) for _ in range(4)]
        # delay 0: a history interval (strided rows); delays 1 and 2: one tape interval, twice
        srcs = [his[:, 1, :], his[:, 2, :], his[:, 2, :], nodes[0]] + nodes * 2
        w = [float(x) for x in np.linspace(-1.0, 2.0, 12)]
        wd = [float(x) for x in np.linspace(3.0, -2.0, 12)]
        out, dtau = torch.empty(rows, L, D, dtype=dtype), torch.empty(rows, L, D, dtype=dtype)
        be._dde_tape_gather(out, dtau, srcs, w, wd)
        for j in range(L):
            ya, fa, yb, fb = (x.numpy() for x in srcs[4 * j : 4 * j + 4])
            for dst, c in ((out, w), (dtau, wd)):
                c0, c1, c2, c3 = (T(x) for x in c[4 * j : 4 * j + 4])
                want = (ya * c0 + fa * c1) + (yb * c2 + fb * c3)
                assert want.dtype == T and np.array_equal(dst.numpy()[:, j, :], want)
        only = torch.empty(rows, L, D, dtype=dtype)
        be._dde_tape_gather(only, None, srcs, w)
        assert torch.equal(only, out)
        # the cotangent: node 0 is read by delay 0 (as fb) and by delays 1 and 2 (as ya): one output, three terms
        g = torch.randn(rows, L, D, generator=gen, dtype=dtype)
        terms = [[(0, w[3]), (1, w[4]), (2, w[8])], [(1, w[5]), (2, w[9])]]
        gouts = [torch.empty(rows, D, dtype=dtype) for _ in terms]
        be._dde_tape_gather_backward(gouts, terms, g)
        gn = g.numpy()
        want0 = (gn[:, 0] * T(w[3]) + gn[:, 1] * T(w[4])) + gn[:, 2] * T(w[8])
        want1 = gn[:, 1] * T(w[5]) + gn[:, 2] * T(w[9])
        assert np.array_equal(gouts[0].numpy(), want0) and np.array_equal(gouts[1].numpy(), want1)
        # a tile that starts at j0 = 1 reads the same rows of g
        again = [torch.empty(rows, D, dtype=dtype)]
        be._dde_tape_gather_backward(again, [[(0, w[5]), (1, w[9])]], g, 1)
        assert torch.equal(again[0], gouts[1])
    assert be.launches == ["dde_tape_gather", "dde_tape_gather", "dde_tape_gather_backward", "dde_tape_gather_backward"] * 2


def test_the_weights_at_the_ends_of_an_interval_are_exact():
    for h in (0.25, 0.1, 3.0):
        a, b = hermite_weights(0.0, h)
        assert a == (1.0, 0.0, 0.0, 0.0) and b == (0.0, -1.0, 0.0, 0.0)
        a, b = hermite_weights(1.0, h)
        assert a == (0.0, 0.0, 1.0, 0.0) and b == (0.0, 0.0, 0.0, -1.0)
        for sigma in (0.0, 0.3, 0.5, 1.0):
            assert hermite_weights(sigma, h) == DO.weights(sigma, h)
    # dtau is -H'(theta): against a central difference of the value weights in theta
    h, sigma, e = 0.25, 0.37, 1e-6
    up, dn = hermite_weights(sigma + e / h, h)[0], hermite_weights(sigma - e / h, h)[0]
    assert np.allclose(hermite_weights(sigma, h)[1], [-(u - d) / (2 * e) for u, d in zip(up, dn)], rtol=1e-7, atol=1e-8)


def test_the_interval_rule_case_by_case(dev):
    his_t = np.linspace(-1.0, 0.0, 5)
    grid = np.arange(9) * 0.25
    for pick in (pick_interval, DO.pick):
        # theta on a history node: that node's interval at sigma = 0
        assert pick(-0.5, his_t, grid, 0, 0) == ("his", 2, -0.5, -0.25)
        # theta before the history: nothing
        assert pick(-1.0 - 1e-9, his_t, grid, 3, 1) is None
        # theta = t0: the history's last interval (sigma = 1) until tape interval 0 is complete — f_1 is known from the second stage
        # of step 1 on
        assert pick(0.0, his_t, grid, 0, 0) == pick(0.0, his_t, grid, 0, 3) == ("his", 3, -0.25, 0.0)
        assert pick(0.0, his_t, grid, 1, 0) == ("his", 3, -0.25, 0.0)
        assert pick(0.0, his_t, grid, 1, 1) == pick(0.0, his_t, grid, 2, 0) == ("tape", 0, 0.0, 0.25)
        # theta on a tape node: its own interval once complete, else the one before at sigma = 1
        assert pick(0.5, his_t, grid, 4, 0) == ("tape", 2, 0.5, 0.75)
        assert pick(0.5, his_t, grid, 3, 0) == ("tape", 1, 0.25, 0.5)
        assert pick(0.5, his_t, grid, 3, 1) == ("tape", 2, 0.5, 0.75)
        # tau equal to the step: the first stage of step k wants grid[k - 1] and falls back one interval; the later stages do not
        assert pick(grid[5] - 0.25, his_t, grid, 5, 0) == ("tape", 3, 0.75, 1.0)
        assert pick(grid[5] + 0.25 / 3 - 0.25, his_t, grid, 5, 1) == ("tape", 4, 1.0, 1.25)
        # inside an interval
        assert pick(0.3, his_t, grid, 6, 0) == ("tape", 1, 0.25, 0.5)
    # ... and what the plan makes of the fall-back: sigma = 1 exactly, the weights (0, 0, 1, 0)
    his, ht = _history((1,), 5, 2, torch.float64)
    xde, _, _ = _problem(lambda t, y, yl: -yl, his, torch.as_tensor(ht), torch.as_tensor(grid), torch.tensor([0.25]), RK4, None, None)
    sp = xde._plans[5][0]
    assert sp.w == [0.0, 0.0, 1.0, 0.0] and sp.keys == [(3, 0), (3, 1), (4, 0), (4, 1)] and sp.src == [0, 1, 2, 3]
    sp = xde._plans[0][0]  # the history's last interval at sigma = 0: its end state is tape node 0
    assert sp.w == [1.0, 0.0, 0.0, 0.0] and sp.keys == [(0, 0)] and sp.src[2] == 0 and torch.is_tensor(sp.src[0]) and torch.is_tensor(sp.src[3])


# ----------------------------------------------------------------------------------------------
# the launches of a walk
# ----------------------------------------------------------------------------------------------
def _small(dtype=torch.float64, Th=2):
    his = (0.5 * torch.randn(3, Th, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).to(dtype)
    return his, torch.linspace(-0.5, 0.0, Th, dtype=torch.float64), torch.linspace(0.0, 1.0, 5, dtype=torch.float64)


def test_launches_of_a_walk(dev):
    """Four RK4 steps, L = 2: one gather per stage and nothing of ddeint's history kernels; the backward one cotangent launch per stage
    (every stage reads a node with a gradient: the history here is one interval, whose end state is tape node 0) and one delay-gradient
    launch per stage when the delays require grad, none otherwise."""
    be = _hip.get_backend()
    his, his_t, t = _small()
    a = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    func = lambda t_, y, yl: (y * a + yl[..., 0:1, :]) - yl[..., 1:2, :] * 0.5  # noqa: E731
    with torch.no_grad():
        ddeint_steps(func, his, his_t, t, torch.tensor([0.3, 0.4]))
    assert be.launches.count("dde_tape_gather") == 16 and not [x for x in be.launches if x.startswith(("hermite", "history"))]
    assert set(be.launches) == {"dde_tape_gather", "combine"}
    for grad_lags, n_lag in ((True, 16), (False, 0)):
        lags = torch.tensor([0.3, 0.4], dtype=torch.float64, requires_grad=grad_lags)
        y0 = his[..., -1:, :].clone().requires_grad_(True)
        del be.launches[:]
        sol = ddeint_steps(func, torch.cat([his[..., :-1, :], y0], dim=-2), his_t, t, lags)
        assert be.launches.count("dde_tape_gather") == 16 and "dde_tape_gather_backward" not in be.launches
        del be.launches[:]
        sol.sum().backward()
        assert be.launches.count("dde_tape_gather_backward") == 16 and be.launches.count("lag_grad") == n_lag
        assert y0.grad is not None and (lags.grad is not None) == grad_lags
    # nfe counts as under odeint: four per RK4 step
    xde, s, args = _problem(func, his, his_t, t, torch.tensor([0.3, 0.4]), RK4, None, None)
    with torch.no_grad():
        s._walk(*args)
    assert s.nfe == 16


def test_more_delays_than_a_launch_takes_are_two_launches_per_stage(dev):
    be = _hip.get_backend()
    his, his_t, t = _small()
    L = MAXL + 1
    lags = torch.linspace(0.25, 0.5, L, dtype=torch.float64, requires_grad=True)
    y0 = his[..., -1:, :].clone().requires_grad_(True)
    sol = ddeint_steps(lambda t_, y, yl: -yl.sum(-2, keepdim=True) * 0.0625, torch.cat([his[..., :-1, :], y0], dim=-2), his_t, t, lags, solver=Euler)
    assert be.launches.count("dde_tape_gather") == 2 * 4
    del be.launches[:]
    sol.sum().backward()
    assert be.launches.count("dde_tape_gather_backward") == 2 * 4 and be.launches.count("lag_grad") == 4
    assert lags.grad.shape == (L,) and float(y0.grad.abs().max()) > 0


@pytest.mark.parametrize("solver, method", [(Euler, "euler"), (Midpoint, "midpoint"), (RK4, "rk4")])
def test_a_func_that_ignores_the_delays_gives_odeint_s_solution(dev, solver, method):
    for dtype in (torch.float32, torch.float64):
        his, his_t, _ = _small(dtype)
        t = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5], dtype=dtype)
        f = lambda t_, y: y * -0.5 + (y * y) * 0.125  # noqa: E731
        for o in ({}, {"step_size": 0.25, "interp": "linear"}):
            with torch.no_grad():
                a = ddeint_steps(lambda t_, y, yl: f(t_, y), his, his_t, t, torch.tensor([0.5]), solver=solver, options=dict(o))
                b = odeint(f, his[..., -1:, :], t, solver=solver, options=dict(o, norm=None))
            assert torch.equal(a, b)


def test_ddeint_is_what_it_was(dev):
    """The parent's case (tests/_dde_cases.py): the same bits against the oracle and the same launches — one history gather, then the
    combines."""
    be = _hip.get_backend()
    rng = np.random.RandomState(2)
    B, L, D = 6, 5, 4
    y0 = rng.randn(B, D).astype(np.float32)
    y_lags = rng.randn(B, L, D).astype(np.float32)
    t = np.linspace(0.0, 1.0, 21).astype(np.float32)
    ref, _ = O.ddeint(_dde_func_np, y0, t, None, y_lags, None, "rk4", his_processed=True)
    got, _ = ddeint(_dde_func_t, torch.from_numpy(y0), torch.from_numpy(t), None, torch.from_numpy(y_lags), None, RK4, his_processed=True)
    assert np.array_equal(got.numpy(), ref)
    assert be.launches == ["combine"] * 80
    del be.launches[:]
    his = rng.randn(4, 20, 3).astype(np.float32)
    ddeint(_dde_func_t, torch.from_numpy(his[:, -1, :].copy()), torch.from_numpy(t[:5]), torch.tensor([1.5, 4.0, 7.25]), torch.from_numpy(his),
           torch.arange(20, dtype=torch.float32), RK4)
    assert be.launches == ["hermite"] + ["combine"] * 16


# ----------------------------------------------------------------------------------------------
# what is refused, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals_name_the_value_and_say_what_works(dev):
    be = _hip.get_backend()
    his, his_t, t = _small(Th=3)
    f = lambda t_, y, yl: -yl[..., 0:1, :]  # noqa: E731
    lags = torch.tensor([0.3, 0.4], dtype=torch.float64)

    def refused(exc, match, *says, **kw):
        args = dict(func=f, his=his, his_span=his_t, t_span=t, lags=lags, solver=RK4, his_derivative=None, options=None)
        args.update(kw)
        with pytest.raises(exc, match=match) as e:
            ddeint_steps(**args)
        for word in says:
            assert word in str(e.value), (word, str(e.value))

    refused(ValueError, "smaller than the largest grid step", "lags[0] = 0.2", "0.25", "step_size", lags=torch.tensor([0.2, 0.4]))
    refused(ValueError, "before his_span", "lags[1]", "-0.6", "-0.5", lags=torch.tensor([0.3, 0.6]))
    refused(ValueError, "must equal t_span", "-0.1", "0.0", his_span=torch.tensor([-0.6, -0.35, -0.1], dtype=torch.float64))
    refused(ValueError, "strictly increasing", "t_span[2] = 0.5", "forwards", t_span=torch.tensor([0.0, 0.25, 0.5, 0.4]))
    refused(ValueError, "strictly increasing", "t_span[0]", t_span=torch.tensor([0.0, -0.25, -0.5]))
    refused(ValueError, "1-D tensor", "(1, 2)", lags=torch.tensor([[0.3, 0.4]]))
    refused(ValueError, "1-D tensor", "(0,)", lags=torch.zeros(0))
    refused(ValueError, "1-D tensor", "1 to 2048", "(2049,)", lags=torch.full((2049,), 0.3))
    refused(ValueError, "not a positive delay", "lags[1] = -0.3", "tau > 0", lags=torch.tensor([0.3, -0.3]))
    refused(ValueError, "not a positive delay", "lags[0] = 0.0", lags=torch.tensor([0.0, 0.3]))
    refused(NotImplementedError, "not a tuple", "stack", his=(his, his))
    refused(ValueError, "his_derivative must have", "(3, 3, 4)", "(3, 2, 4)", his_derivative=his[:, :2])
    refused(ValueError, "his_derivative must have", "float64", "float32", his_derivative=his.float())
    for solver in (AdamsBashforthMoulton, Dopri5):
        refused(NotImplementedError, solver.__name__, "Euler, Midpoint or RK4", solver=solver)
    refused(NotImplementedError, "interp='cubic'", "interp='linear'", options={"interp": "cubic", "step_size": 0.125})
    refused(NotImplementedError, "pipeline='graph'", "pipeline='sync'", options={"pipeline": "graph"})
    refused(ValueError, "at least 2", his=his[:, -1:], his_span=his_t[-1:])
    # a grid whose steps the delays cover, but a stage that would still reach past the last complete interval: none exists by the
    # rule above — the plan's own check stands behind it (here it is met through a grid_constructor's uneven grid)
    refused(ValueError, "smaller than the largest grid step", "0.5", lags=torch.tensor([0.3, 0.4]),
            options={"grid_constructor": lambda y0, t_: torch.tensor([0.0, 0.5, 0.75, 1.0], dtype=torch.float64)})
    assert be.launches == []
    # "auto" never captures, whatever the number of steps
    with torch.no_grad():
        ddeint_steps(f, his, his_t, torch.linspace(0.0, 8.0, 33, dtype=torch.float64), lags, options={"pipeline": "auto"})
    assert be.launches.count("dde_tape_gather") == 4 * 32


def test_the_tape_is_bounded_under_no_grad(dev):
    """64 steps with max(lags) = 2h.  A node is dropped once it is older than t - max(lags) by more than one interval: at the start of
    step k the stages still read from t_k - 2h - h on, nodes k - 3 .. k, and the step adds its own: at most 5 nodes at any time (with
    grad mode on the tape keeps all 65 for the backward)."""
    his, his_t, _ = _small(Th=3)
    t = torch.as_tensor(np.arange(65) * 0.25)
    f = lambda t_, y, yl: -yl[..., 0:1, :] * 0.5 + yl[..., 1:2, :] * 0.25  # noqa: E731
    xde, s, args = _problem(f, his, his_t, t, torch.tensor([0.5, 0.3]), RK4, None, None)
    with torch.no_grad():
        sol = s._walk(*args)
    assert sol.shape == (3, 65, 4) and xde.tape_high_water <= 5 and len(xde._tape) <= 5
    xde, s, args = _problem(f, his, his_t, t, torch.tensor([0.5, 0.3]), RK4, None, None)
    again = s._walk(*args)
    assert torch.equal(again, sol) and len(xde._tape) == 64


def test_gradcheck_of_the_gather_node(dev):
    be = _hip.get_backend()
    gen = torch.Generator().manual_seed(4)
    his, his_t, t = _small(Th=3)
    lags = torch.tensor([0.3, 0.45], dtype=torch.float64, requires_grad=True)
    xde, _, _ = _problem(lambda t_, y, yl: -yl, his, his_t, t, lags, RK4, None, None)
    sp = xde._plans[3][1]
    nodes = [torch.randn(3, 1, 4, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in sp.keys]
    assert len(nodes) >= 2
    # (lags enters through the saved dtau only: the plan's weights are constants of the node, so lags is checked by ddeint_steps' own
    # gradcheck in tests/_dde_tape_cases.py)
    assert torch.autograd.gradcheck(lambda *xs: DdeTapeGatherFn.apply(be, sp, None, *xs), nodes)
    # an absent cotangent stays absent
    del be.launches[:]
    out = DdeTapeGatherFn.apply(be, sp, None, nodes[0], *[x.detach() for x in nodes[1:]])
    (g0,) = torch.autograd.grad(out.sum(), (nodes[0],))
    assert g0.shape == nodes[0].shape and be.launches == ["dde_tape_gather", "dde_tape_gather_backward"]
