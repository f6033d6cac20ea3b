"""Per-sample adaptive stepping on the GPU: the four kernels of include/xde_hip_rows.h against tests/_rows_oracle.py bit for bit
(aligned and one element off, h of mixed sign with zero on done rows, accepted, rejected, done and non-finite rows in one launch, steps
holding 0, 1 and 3 outputs, guard elements around every output), xde_rows_stage_combine at equal h against xde_stage_combine itself,
and the end-to-end cases of tests/_rows_cases.py with the HIP backend.

The controller's step factor goes through ``pow``, the one operation whose result differs between the device's and the host's libm
(tests/_controller_scripts.py, RATIO POLICY): the kernel-level cases keep every error ratio where the factor is clamped to ifactor or
dfactor, so the comparison is exact; the end-to-end cases run free."""
import numpy as np
import pytest
import torch

from paddlexde_amd import Dopri5, _hip, odeint

from . import _rows_cases as RC
from . import _rows_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
# (rows, D): the smallest case; one lane per row; rows that straddle vectors; whole vectors; one past a wave of lanes (fp32) and past
# a workgroup of lanes (fp64); a loop inside the workgroup; D beyond one workgroup's stride three times over; many rows per workgroup
SHAPES = [(1, 1), (3, 1), (5, 3), (7, 64), (2, 257), (3, 1027), (1, 3 * 4096 + 5), (300, 5)]
N_OUT = 8
T_SPAN = np.arange(N_OUT) * 0.125  # exact in both time dtypes


class Guarded:
    """A ``shape`` view into a sentinel-filled buffer with whole 16-byte vectors of guard on both sides, its base 16-byte aligned or
    (``misalign``) one element past."""

    def __init__(self, shape, dtype, misalign, fill=None):
        n = int(np.prod(shape))
        W = 16 // torch.empty((), dtype=dtype).element_size()
        self.off, self.n = W + (1 if misalign else 0), n
        self.full = torch.full((n + 2 * W + 1,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.full[self.off : self.off + n].view(shape)
        if fill is not None:
            self.view.copy_(torch.as_tensor(fill))

    def guards_intact(self):
        g = torch.cat([self.full[: self.off], self.full[self.off + self.n :]])
        return bool((g == SENTINEL).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _to_device(c, dtype):
    """A numpy control block of the oracle as a ``_hip.RowsCtl`` on the device."""
    d = _hip.RowsCtl(len(c.t), c.t_stage.shape[0], dtype, torch.device(DEV))
    for n in RO.F64 + RO.I32:
        getattr(d, n).copy_(torch.from_numpy(getattr(c, n)))
    d.t_stage.copy_(torch.from_numpy(c.t_stage))
    return d


def _planes_equal(d, c):
    bad = [n for n in RO.F64 + RO.I32 + ("t_stage",) if not np.array_equal(getattr(d, n).cpu().numpy(), getattr(c, n), equal_nan=True)]
    return bad == [], bad


def _params(dtype, tdtype, n_stage, direction=1):
    p = _hip.XdeCtrlParams()
    p.rtol, p.atol, p.min_step, p.max_step = 1e-3, 1e-6, 0.0, float("inf")
    p.safety, p.ifactor, p.dfactor, p.order, p.max_num_steps = 0.9, 10.0, 0.2, 5.0, 5
    p.time_dtype, p.state_dtype, p.direction, p.norm_kind, p.n_stage, p.n_seg = _hip.dtype_code(tdtype), _hip.dtype_code(dtype), direction, 0, n_stage, 1
    for i, a in enumerate((0.2, 0.3, 0.8, 8.0 / 9.0, 1.0, 1.0)[:n_stage]):
        p.alpha[i] = float(_NPT[dtype](a))
    return p


def _randn(gen, rows, D, dtype, scale=1.0):
    return (torch.randn(rows, D, generator=gen, dtype=torch.float64) * scale).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_stage_combine_equals_the_oracle_bit_for_bit(dtype, rows, D, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    gen = torch.Generator().manual_seed(rows * 1031 + D)
    coef = [0.2, -0.3, 0.8, 8.0 / 9.0, -1.0, 0.1, 0.7]
    coef2 = [0.01, 0.3, -0.02, 1.5, 0.25, -0.125, 3.0]
    c = RO.new_ctl(rows, 1, T)
    c.h[:] = np.random.RandomState(rows + D).randn(rows) * 0.1  # mixed sign
    c.done[:] = (np.arange(rows) % 3) == 1  # (rows 1, 4, ...: frozen, h = 0)
    c.h[c.done != 0] = 0.0
    ctl = _to_device(c, dtype)
    y0 = Guarded((rows, D), dtype, misalign, fill=_randn(gen, rows, D, dtype)).view
    ks = [Guarded((rows, D), dtype, misalign, fill=_randn(gen, rows, D, dtype)).view for _ in range(7)]
    Y0, KS = y0.cpu().numpy(), [k.cpu().numpy() for k in ks]
    for nk, two in ((1, False), (3, True), (5, False), (6, True), (7, False), (7, True)):
        want, want2 = RO.stage_combine(Y0, KS[:nk], coef[:nk], c, coef2[:nk] if two else None)
        out, out2 = Guarded((rows, D), dtype, misalign), Guarded((rows, D), dtype, misalign)
        be._rows_stage_combine(out.view, y0, ks[:nk], coef[:nk], ctl, out2=out2.view if two else None, coef2=coef2[:nk] if two else None)
        assert np.array_equal(out.numpy(), want) and out.guards_intact(), (nk, two)
        assert np.array_equal(out.numpy()[c.done != 0], Y0[c.done != 0])
        if two:
            assert np.array_equal(out2.numpy(), want2) and out2.guards_intact(), nk
        else:
            assert bool((out2.full == SENTINEL).all())
    # operands of different phases (an output one element off its inputs) take the element-wise instantiation: the same bits
    want, _ = RO.stage_combine(Y0, KS[:3], coef[:3], c)
    other = Guarded((rows, D), dtype, not misalign)
    be._rows_stage_combine(other.view, y0, ks[:3], coef[:3], ctl)
    assert np.array_equal(other.numpy(), want) and other.guards_intact()
    # at equal h (no row done) the output is xde_stage_combine's
    c.done[:] = 0
    c.h[:] = -0.0371
    ctl = _to_device(c, dtype)
    mine, mine2, theirs, theirs2 = (Guarded((rows, D), dtype, misalign) for _ in range(4))
    be._rows_stage_combine(mine.view, y0, ks[:5], coef[:5], ctl, out2=mine2.view, coef2=coef2[:5])
    be.stage_combine(theirs.view, y0, ks[:5], coef[:5], _hip.COMBINE_RK, dt_host=float(T(-0.0371)), out2=theirs2.view, coef2=coef2[:5])
    assert torch.equal(mine.full, theirs.full) and torch.equal(mine2.full, theirs2.full)


def _attempt_state(rows, D, T, phase):
    """A control block and operands in which one launch meets accepted, rejected, done and (``phase`` 1) non-finite rows, and steps
    that hold 0, 1 and 3 outputs and the last one.  Accepted rows have tiny errors and rejected rows huge ones (pow-free factors)."""
    rng = np.random.RandomState(rows * 131 + D + phase)
    c = RO.new_ctl(rows, 6, T)
    kind = (np.arange(rows) + phase) % 4
    c.t[:] = np.where(kind == 3, 0.8125, 0.0625)
    c.next_out[:] = np.where(kind == 3, 7, 1)
    c.h[:] = np.choose(kind, [0.03125, 0.09375, 0.34375, 0.125])  # reaches no output, one, three, the last one
    c.steps_in_interval[:] = rng.randint(0, 5, rows)  # (max_num_steps = 5: a rejected row at 4 runs out of budget)
    c.n_accept[:] = rng.randint(0, 9, rows)
    c.n_reject[:] = rng.randint(0, 9, rows)
    reject = (np.arange(rows) + phase) % 5 == 4
    done = (np.arange(rows) + phase) % 7 == 5
    c.done[done] = 1
    c.h[done] = 0.0
    if phase == 2 and rows >= 2:
        c.status[rows - 1] = RO.STATUS_MAX_STEPS  # a failed row is judged no more
    y0 = rng.randn(rows, D).astype(T)
    y1 = (y0 + 0.01 * rng.randn(rows, D)).astype(T)
    ks = [(rng.randn(rows, D) * np.where(reject, 1e9, 1e-12)[:, None]).astype(T) for _ in range(4)]
    e_pre = (rng.randn(rows, D) * np.where(reject, 1e9, 1e-13)[:, None]).astype(T)
    if phase == 1 and rows >= 3:
        y0[2, D // 2] = np.nan
    return c, y0, y1, ks, e_pre


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_norm_control_and_dense_commit_equal_the_oracle_bit_for_bit(dtype, rows, D, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    c_err = [0.0012, -0.0042, 0.05, -1.0 / 60.0]
    mid = [0.1, 0.39, -0.03, 0.06]
    ts_dev = torch.from_numpy(T_SPAN.astype(np.float64)).to(DEV)
    for phase in range(4):
        tdtype = torch.float32 if phase % 2 else torch.float64
        p = _params(dtype, tdtype, 6)
        c, Y0, Y1, KS, EP = _attempt_state(rows, D, T, phase)
        pre = phase >= 2  # the e_pre form, and the full sum
        G = lambda a: Guarded((rows, D), dtype, misalign, fill=a)  # noqa: E731
        y0, y1, ep = G(Y0), G(Y1), G(EP)
        ks = [G(k) for k in KS]
        ctl = _to_device(c, dtype)
        live = (c.done == 0) & (c.status == 0)
        if pre:
            be._rows_norm_control([ks[3].view], c_err[3:], y0.view, y1.view, ctl, p, ts_dev, e_pre=ep.view)
            RO.norm_control(KS[3:], c_err[3:], EP, Y0, Y1, c, p, T_SPAN, N_OUT)
        else:
            be._rows_norm_control([k.view for k in ks], c_err, y0.view, y1.view, ctl, p, ts_dev)
            RO.norm_control(KS, c_err, None, Y0, Y1, c, p, T_SPAN, N_OUT)
        ok, bad = _planes_equal(ctl, c)
        assert ok, (phase, bad)
        if rows >= 5:
            assert set(c.accept[live]) == {0, 1}  # accepted and rejected rows in one launch
        if phase == 1 and rows >= 3:
            assert c.status[2] == RO.STATUS_NONFINITE and c.nonfinite[2] == 1.0
        # kernel 3 on what kernel 2 left
        out = Guarded((N_OUT, rows, D), dtype, misalign)
        want = np.full((N_OUT, rows, D), SENTINEL, T)
        before = c.next_out.copy()
        be._rows_dense_commit(out.view, [k.view for k in ks], mid, y0.view, y1.view, ks[3].view, ctl, p, ts_dev)
        F1 = KS[3].copy()
        RO.dense_commit(want, KS, mid, Y0, Y1, F1, c, p, T_SPAN, N_OUT)
        assert np.array_equal(out.numpy(), want, equal_nan=True) and out.guards_intact(), phase
        assert np.array_equal(y0.numpy(), Y0, equal_nan=True) and np.array_equal(ks[0].numpy(), KS[0]) and y0.guards_intact() and ks[0].guards_intact()
        ok, bad = _planes_equal(ctl, c)
        assert ok, (phase, bad)
        if rows >= 4:
            assert {0, 1, 3} <= set((c.next_out - before)[c.accept != 0]) | {0}  # steps that hold no output, one and three
        assert all(x.guards_intact() for x in [y1, ep] + ks[1:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_scaled_norm_equals_the_oracle_bit_for_bit(dtype, rows, D, misalign):
    be = _hip.get_backend()
    gen = torch.Generator().manual_seed(rows * 7 + D)
    a, b, y0 = (Guarded((rows, D), dtype, misalign, fill=_randn(gen, rows, D, dtype)) for _ in range(3))
    for other in (None, b):
        out = Guarded((rows,), torch.float64, False)
        be._rows_scaled_norm(out.view, a.view, None if other is None else other.view, y0.view, 1e-3, 1e-6)
        want = RO.scaled_norm(a.numpy(), None if other is None else other.numpy(), y0.numpy(), 1e-3, 1e-6)
        assert np.array_equal(out.numpy(), want) and out.guards_intact()


# ----------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------
def _solve(lam, dtype, **opt):
    st = {}
    with torch.no_grad():
        sol = odeint(RC.func_of(lam, dtype, DEV), RC.y0_of(lam, dtype, DEV), RC.t_of(dtype, dev=DEV), Dopri5, rtol=RC.RTOL, atol=RC.ATOL,
                     options=dict(opt, per_sample=True, dtype=dtype, stats_out=st))
    return sol, tuple(zip(st["n_accept"].tolist(), st["n_reject"].tolist()))


def test_the_five_row_problem_in_fp64_on_the_device():
    """Counts per row equal the row-alone oracle's; the solution within 16 x the deviation measured on the numpy double."""
    assert _hip.get_backend().name == "hip"
    sol, counts = _solve(RC.LAM, torch.float64)
    ref, want = RC.reference(RC.LAM, torch.float64)
    dev = np.abs(sol.cpu().numpy() - ref).max()
    print("fp64 deviation from the rows solved alone:", dev, "counts", counts)
    assert counts == want
    assert dev <= RC.BAR[torch.float64]


def test_the_five_row_problem_in_fp32_on_the_device():
    """The solution within the bar measured on the numpy double; the counts are recorded, not asserted (free-running fp32 decisions
    part by an ulp of h: DESIGN section 2)."""
    sol, counts = _solve(RC.LAM, torch.float32)
    ref, want = RC.reference(RC.LAM, torch.float32)
    dev = np.abs(sol.cpu().numpy() - ref).max()
    print("fp32 deviation from the rows solved alone:", dev, "counts", counts, "oracle", want)
    assert dev <= RC.BAR[torch.float32]


def test_a_decreasing_t_span_on_the_device():
    """Kernels 2 and 3 with direction -1 end to end: native negative steps, counts equal to the row-alone oracle's, the fp64 bar."""
    dtype = torch.float64
    fwd = RC.func_of(RC.LAM, dtype, DEV)
    st = {}
    with torch.no_grad():
        sol = odeint(lambda t, y: -fwd(t, y), RC.y0_of(RC.LAM, dtype, DEV), -RC.t_of(dtype, dev=DEV), Dopri5, rtol=RC.RTOL, atol=RC.ATOL,
                     options={"per_sample": True, "dtype": dtype, "stats_out": st})
    ref, want = RC.reference(RC.LAM, dtype, reverse=True)
    dev = np.abs(sol.cpu().numpy() - ref).max()
    print("decreasing t_span, fp64 deviation:", dev)
    assert tuple(zip(st["n_accept"].tolist(), st["n_reject"].tolist())) == want and dev <= RC.BAR[dtype]
    assert bool((st["t"] <= -2.0).all()) and bool((st["dt_next"] < 0).all())


def test_an_fp32_state_under_fp64_times_on_the_device():
    st = {}
    dtype, tdtype = torch.float32, torch.float64
    with torch.no_grad():
        sol = odeint(RC.func_of(RC.LAM, dtype, DEV), RC.y0_of(RC.LAM, dtype, DEV), RC.t_of(tdtype, dev=DEV), Dopri5, rtol=RC.RTOL, atol=RC.ATOL,
                     options={"per_sample": True, "dtype": tdtype, "stats_out": st})
    ref, want = RC.reference(RC.LAM, dtype, tdtype=tdtype)
    dev = np.abs(sol.cpu().numpy() - ref).max()
    print("fp32 state, fp64 time: deviation", dev, "counts", st["n_accept"].tolist(), st["n_reject"].tolist(), "oracle", want)
    assert dev <= RC.BAR_F32_STATE_F64_TIME


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_independence_bit_for_bit_on_the_device(dtype):
    a, b, c = 2.0, 50.0, 200.0
    two, _ = _solve((a, b), dtype)
    three, _ = _solve((a, c, b), dtype)
    assert torch.equal(two[:, 0], three[:, 0]) and torch.equal(two[:, 1], three[:, 2])
    late, _ = _solve((a, c, b), dtype, check_every=7)
    assert torch.equal(late, three)
