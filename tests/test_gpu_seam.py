"""The resident seam launch on the GPU (options["seam"] = "resident", include/xde_hip_seam.h): error norm + controller + the next attempt's
first stage combine in ONE launch, against the three launches it replaces IN THE SAME BUILD — solution rows, every attempt's
(t0, dt, ratio, accept), the control block on the device and in the host mirror, bit for bit — and, attempt by attempt, against the
oracle's own functions to the bars of tests/_kernel_oracle_cases.py.

The three launches are xde_error_norm_partial -> xde_rk_control -> xde_stage_combine.  States of <= SINGLE_MAX_ELEMS elements take
another path by default (xde_error_norm_control: ONE workgroup of 1024 lanes, whose partition of the sum is not the multi-workgroup
pass's), so the comparison solver sets SINGLE_MAX_ELEMS = 0 — the three launches at every size; the sizes at which both partitions give
the same sums by construction (one workgroup's worth of vectors: every other term is an exact zero) are compared with the default path too.

Shapes (fp32 lanes hold 4 elements, fp64 lanes 2): 1 and 7 elements — scalar tail only; 1027 — vector body + tail, fewer lanes than one
workgroup (fp32); 256*4*3 + 5 — several workgroups, uneven; 1 200 003 — every lane of the 512-workgroup grid carries 3 (fp32) or 5 (fp64)
vectors per array.

test_solver_variants: what else a solve hands to the launch — NORM_LINF, Bosh3's pair (a21 = 1/2, another last error coefficient, order
3), reverse time, `step_t`, `max_step` / `min_step`, the PI controller — on 1027 and 3077 elements, against the three launches as above;
a state that leaves the finite range ends in the three launches' exception.  tests/test_gpu_seam_kernel.py calls the launch directly."""
import numpy as np
import pytest
import torch

from oracle import xde_oracle as O
from paddlexde_amd import Bosh3, Dopri5, _hip
from paddlexde_amd.utils import _linf_norm, _rms_norm
from paddlexde_amd.xde import BaseODE

from . import problems as P

pytestmark = pytest.mark.gpu

SHAPES = {"n1": (1, 1), "n7": (1, 7), "n1027": (79, 13), "n3077": (181, 17), "carry": (400001, 3)}
FIELDS = [f for f, _ in _hip.XdeCtrl._fields_ if f not in ("seq", "chk", "reserved", "ratio_seg")]  # (seq: the block's launches since it was allocated)


class Dopri5ThreeLaunches(Dopri5):
    SINGLE_MAX_ELEMS = 0  # no one-workgroup error-norm + controller kernel: the three launches the seam replaces, at every size


class Bosh3ThreeLaunches(Bosh3):
    SINGLE_MAX_ELEMS = 0


@pytest.fixture
def dev():
    return torch.device("cuda")


def _block(c):
    return tuple(getattr(c, f) for f in FIELDS) + tuple(c.ratio_seg)


def _solve(dev, cls, seam, pipeline, dtype, shape, t_end=12.0, count=None, norm=_rms_norm, t_start=0.0, **kw):
    prob = P.Linear(dim=shape[1], seed=3)
    y0 = torch.randn(*shape, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    t = torch.linspace(t_start, t_end, 5, dtype=dtype)
    s = cls(xde=BaseODE(prob.f_torch(dev), y0=y0, t_span=t), y0=y0, rtol=1e-6, atol=1e-8, norm=norm, dtype=dtype, pipeline=pipeline,
            record_trace=True, seam=seam, **kw)
    be = s.backend
    if count is not None:
        real = be._seam_attempt
        be._seam_attempt = lambda *a, **k: (count.append(1), real(*a, **k))[1]
    try:
        sol = s.integrate(t)
        torch.cuda.synchronize()
        on_device = _hip.XdeCtrl.from_buffer_copy(s._ctrl.cpu().numpy().tobytes())
        assert be._seam_expired(s._ctrl) == 0
    finally:
        if count is not None:
            del be._seam_attempt
    return sol.cpu().numpy(), list(s.trace), _block(s._last), _block(on_device), dict(s.stats)


def _same(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True), "solution rows"
    assert a[1] == b[1], "trace"
    assert a[2] == b[2], "host mirror"
    assert a[3] == b[3], "device block"
    assert a[4] == b[4], "stats"


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_accept_path_with_interior_output_times(dev, shape, dtype, pipeline):
    """The linear problem, first step from the heuristic, t_span with three interior output times."""
    n = []
    got = _solve(dev, Dopri5ThreeLaunches, "resident", pipeline, dtype, SHAPES[shape], count=n)
    want = _solve(dev, Dopri5ThreeLaunches, "launches", pipeline, dtype, SHAPES[shape])
    assert len(n) >= 3 and got[4]["n_steps"] > len(n)  # (the seam ran; the last attempts of the solve took the launches)
    _same(got, want)
    numel = SHAPES[shape][0] * SHAPES[shape][1]
    vectors = numel // (4 if dtype == torch.float32 else 2)
    if vectors <= 256 or numel > Dopri5.SINGLE_MAX_ELEMS:  # the default path's sums are these sums (module docstring)
        _same(got, _solve(dev, Dopri5, "launches", pipeline, dtype, SHAPES[shape]))


# what the host hands to the seam launch beyond the default solve: (solver, options of _solve)
VARIANTS = {
    "linf": (Dopri5ThreeLaunches, dict(norm=_linf_norm, first_step=0.5)),
    "bosh3_rms": (Bosh3ThreeLaunches, dict(t_end=2.0)),  # a21 = 1/2, another c_last, order 3
    "bosh3_linf": (Bosh3ThreeLaunches, dict(t_end=2.0, norm=_linf_norm)),
    "reverse_time": (Dopri5ThreeLaunches, dict(t_start=12.0, t_end=0.0)),
    "step_t": (Dopri5ThreeLaunches, dict(step_t=[1.7, 5.1])),
    "max_step": (Dopri5ThreeLaunches, dict(max_step=0.3)),
    "min_step": (Dopri5ThreeLaunches, dict(min_step=0.2)),
    "pi_rms": (Dopri5ThreeLaunches, dict(controller="PI")),
    "pi_linf": (Dopri5ThreeLaunches, dict(controller="PI", norm=_linf_norm)),
}


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ["n1027", "n3077"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_solver_variants(dev, variant, shape, dtype, pipeline):
    """The other instantiations and operands a solve hands over — NORM_LINF, Bosh3's pair, reverse time, `step_t`, the step clamps, the
    PI controller: rows, trace, mirror, device block and stats of the three launches, and the seam did run."""
    cls, kw = VARIANTS[variant]
    n = []
    got = _solve(dev, cls, "resident", pipeline, dtype, SHAPES[shape], count=n, **kw)
    want = _solve(dev, cls, "launches", pipeline, dtype, SHAPES[shape], **kw)
    assert len(n) >= 3, len(n)
    _same(got, want)


class _Square(torch.nn.Module):
    def forward(self, t, y):
        return y * y


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
def test_a_state_that_leaves_the_finite_range_ends_as_under_the_launches(dev, pipeline):
    """y' = y^2 from 1 has its pole at t = 1: the solve to t = 2 ends in the exception (type and message, the step included) it ends in
    under the three launches, after seam launches, and nothing names the grid barrier."""
    def run(seam, count=None):
        y0 = torch.ones(*SHAPES["n1027"], dtype=torch.float64, device=dev)
        t = torch.tensor([0.0, 2.0], dtype=torch.float64)
        s = Dopri5ThreeLaunches(xde=BaseODE(_Square(), y0=y0, t_span=t), y0=y0, rtol=1e-6, atol=1e-8, norm=_rms_norm, dtype=torch.float64,
                                pipeline=pipeline, seam=seam)
        be = s.backend
        if count is not None:
            real = be._seam_attempt
            be._seam_attempt = lambda *a, **k: (count.append(1), real(*a, **k))[1]
        try:
            with pytest.raises(Exception) as e:
                s.integrate(t)
            torch.cuda.synchronize()
            assert be._seam_expired(s._ctrl) == 0
        finally:
            if count is not None:
                del be._seam_attempt
        return type(e.value), str(e.value)

    n = []
    got, want = run("resident", n), run("launches")
    assert got == want and len(n) >= 3, (got, want, len(n))
    assert got[0] is AssertionError and "grid barrier" not in got[1] and ("underflow" in got[1] or "non-finite" in got[1]), got


def _advance(dev, seam, pipeline, dtype, shape, budgets, **kw):
    """The solver driven attempt by attempt (as a benchmark drives it): advance(k) for every k of `budgets`."""
    prob = P.Linear(dim=shape[1], seed=3)
    y0 = torch.randn(*shape, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    t = np.asarray([0.0, 1.0e9], dtype=np.float32 if dtype == torch.float32 else np.float64)
    s = Dopri5ThreeLaunches(xde=BaseODE(prob.f_torch(dev), y0=y0, t_span=torch.from_numpy(t)), y0=y0, rtol=1e-6, atol=1e-8, norm=_rms_norm,
                            dtype=dtype, pipeline=pipeline, record_trace=True, seam=seam, **kw)
    s.y0 = y0
    s._before_integrate(t)
    for k in budgets:
        c = s.advance(k)
    torch.cuda.synchronize()
    assert s._seam_on == (seam == "resident") and s._carry is False and s.backend._seam_expired(s._ctrl) == 0
    on_device = _hip.XdeCtrl.from_buffer_copy(s._ctrl.cpu().numpy().tobytes())
    return _block(c), _block(on_device), list(s.trace), s._base[0].cpu().numpy(), s._base[1].cpu().numpy()


def _same_state(a, b):
    assert a[0] == b[0] and a[1] == b[1], "control block"
    assert a[2] == b[2], "trace"
    assert np.array_equal(a[3], b[3], equal_nan=True) and np.array_equal(a[4], b[4], equal_nan=True), "state"


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ["n7", "n3077", "carry"])
def test_reject_path(dev, shape, dtype, pipeline):
    """first_step far too large: the first attempts are rejected one after the other, each in a seam launch, which then writes the next
    first stage input from the attempt's own (y0, f0) — under `lag` from whichever candidate the attempt ran on.  advance(k): k - 1 seam
    launches, the separate launches last; block, trace and state as the launches leave them."""
    got = _advance(dev, "resident", pipeline, dtype, SHAPES[shape], (6, 4), first_step=200.0)
    accepts = [acc for (_, _, _, acc) in got[2]]
    assert len(accepts) == 10 and accepts[:3] == [False] * 3 and sum(accepts) >= 3, accepts
    _same_state(got, _advance(dev, "launches", pipeline, dtype, SHAPES[shape], (6, 4), first_step=200.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_solve_of_one_attempt(dev, dtype):
    n = []
    got = _solve(dev, Dopri5ThreeLaunches, "resident", "sync", dtype, SHAPES["n3077"], t_end=1e-3, count=n, first_step=1e-3)
    assert got[4]["n_steps"] == 1 and not n
    _same(got, _solve(dev, Dopri5ThreeLaunches, "launches", "sync", dtype, SHAPES["n3077"], t_end=1e-3, first_step=1e-3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ["n1027", "carry"])
def test_every_attempt_vs_the_oracle(dev, shape, dtype):
    """Every attempt of a seamed solve taken apart with the oracle's own functions, from the stage derivatives the device holds: the
    error ratio (rel 3e-6: the reduction), the verdict, and the next step from that ratio (2 ulp: the one `pow`) — the bars of
    tests/_kernel_oracle_cases.py — and with them the accepted / rejected counts."""
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    prob = P.Linear(dim=SHAPES[shape][1], seed=3)
    y0h = torch.randn(*SHAPES[shape], generator=torch.Generator().manual_seed(1)).to(tdt)
    so = O.AdaptiveRKSolver(prob.f_np, y0h.numpy(), 1e-6, 1e-8, method="dopri5", norm=O._rms_norm, dtype=dtype)
    tt = so.tt
    seen = []

    def hook(index, y0, y1, ks, c):
        k = np.stack([x.cpu().numpy() for x in ks], axis=-1)
        y0n, y1n = y0.cpu().numpy(), y1.cpu().numpy()
        dt = dtype(c.dt_last)
        with np.errstate(all="ignore"):
            err = O._sum_last(k * (dt * so.tableau.c_error)).reshape(y0n.shape)
            ratio_ref = float(O.compute_error_ratio(err, so.rtol, so.atol, y0n, y1n, O._rms_norm))
        assert c.ratio == pytest.approx(ratio_ref, rel=3e-6), (index, c.ratio, ratio_ref)
        assert bool(c.accept) == bool(ratio_ref <= 1), (index, c.ratio, ratio_ref)
        want_dt = tt(np.clip(O.optimal_step_size(tt(c.dt_last), tt(c.ratio), so.safety, so.ifactor, so.dfactor, so.order), so.min_step, so.max_step))
        assert c.dt == pytest.approx(float(want_dt), rel=2.4e-7 if dtype == np.float32 else 4.5e-16), (index, c.dt, float(want_dt))
        seen.append(bool(ratio_ref <= 1))

    y0 = y0h.to(dev)
    t = torch.linspace(0.0, 12.0, 5, dtype=tdt)
    n = []
    s = Dopri5ThreeLaunches(xde=BaseODE(prob.f_torch(dev), y0=y0, t_span=t), y0=y0, rtol=1e-6, atol=1e-8, norm=_rms_norm, dtype=tdt,
                            pipeline="sync", seam="resident", first_step=8.0, _step_hook=hook)
    real = s.backend._seam_attempt
    s.backend._seam_attempt = lambda *a, **k: (n.append(1), real(*a, **k))[1]
    try:
        s.integrate(t)
    finally:
        del s.backend._seam_attempt
    assert len(n) >= 3 and len(seen) == s.stats["n_steps"]
    assert (s.stats["n_accept"], s.stats["n_reject"]) == (sum(seen), len(seen) - sum(seen)) and s.stats["n_reject"] >= 1


def test_resident_refuses_a_state_beyond_the_register_carry(dev):
    y0 = torch.zeros(512 * 256 * 4 * 16 + 4096, device=dev)
    t = torch.tensor([0.0, 1.0])
    s = Dopri5(xde=BaseODE(lambda t_, y: -y, y0=y0, t_span=t), y0=y0, rtol=1e-5, atol=1e-7, norm=_rms_norm, seam="resident")
    with pytest.raises(ValueError, match="does not fit the resident launch .512 workgroups, 512 resident; 17 vectors per lane"):
        s.integrate(t)
    plan = s.backend._seam_plan(65536 * 128, torch.float32)
    assert plan == {"blocks": 512, "per_lane": 16, "resident": 512, "fits": 1}
