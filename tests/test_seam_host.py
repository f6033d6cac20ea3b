"""The resident seam launch (options["seam"], include/xde_hip_seam.h) without a GPU: the host logic on the numpy double of its entry
points (tests/_seam_double.py) — which attempts end in the seam launch, that the solve is the one the separate launches give, what an
expired grid barrier does — and the C ABI's refusals (every call below is refused before anything is enqueued)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from paddlexde_amd import Dopri5, _hip
from paddlexde_amd.utils import _rms_norm
from paddlexde_amd.xde import BaseODE

from . import problems as P
from ._seam_double import SeamDoubleBackend, seam_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xde_hip_seam.h")


@pytest.fixture
def seam_double():
    be = SeamDoubleBackend()
    _hip._set_backend_for_testing(be)
    try:
        yield be
    finally:
        _hip._set_backend_for_testing(None)


def _solver(seam, pipeline, dtype=torch.float64, n=(79, 13), t=None, **kw):
    prob = P.Linear(dim=n[1], seed=3)
    y0 = torch.randn(*n, generator=torch.Generator().manual_seed(1)).to(dtype)
    t = torch.linspace(0.0, 2.0, 5, dtype=dtype) if t is None else t
    s = Dopri5(xde=BaseODE(prob.f_torch("cpu"), y0=y0, t_span=t), y0=y0, rtol=1e-6, atol=1e-8, norm=_rms_norm, dtype=dtype,
               pipeline=pipeline, record_trace=True, seam=seam, **kw)
    return s, t


def _per_attempt(launches):
    """The double's launch names cut into attempts: an attempt ends with its controller (`control`, or `seam`, which holds one)."""
    out, cur = [], []
    for name in launches:
        if name == "dense":
            continue
        cur.append(name)
        if name in ("control", "seam"):
            out.append(cur)
            cur = []
    assert not cur
    return out


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_solve_is_the_separate_launches_solve(seam_double, pipeline, dtype):
    """Rows, trace and final control block of a solve with interior output times, bit for bit, and the launch list: a seamed attempt is
    followed by one of five combines; the solve's last attempt — and, under `lag`, every attempt that could be it — ends in the
    separate launches."""
    runs = {}
    for seam in ("launches", "resident"):
        # (a first step far too large: rejected; a span long enough that `lag` knows most attempts cannot end the solve)
        s, t = _solver(seam, pipeline, dtype, first_step=0.5, t=torch.linspace(0.0, 12.0, 5, dtype=dtype))
        n0 = len(seam_double.launches)
        sol = s.integrate(t)
        runs[seam] = (sol.numpy().copy(), list(s.trace), bytes(s._last), _per_attempt(seam_double.launches[n0:]), dict(s.stats))
    a, b = runs["launches"], runs["resident"]
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[4] == b[4]
    assert a[4]["n_reject"] > 0 and a[4]["n_accept"] > 3
    assert all(att == ["combine"] * 6 + ["errnorm", "control"] for att in a[3])
    seamed = [att[-1] == "seam" for att in b[3]]
    assert any(seamed) and not seamed[-1]
    for i, att in enumerate(b[3]):
        combines = 5 if (i > 0 and seamed[i - 1]) else 6
        assert att == ["combine"] * combines + (["seam"] if seamed[i] else ["errnorm", "control"]), (i, att)
    if pipeline == "sync":  # the host knows where every attempt lands: only attempts that can end the solve take the launches
        assert seamed[1:-1] == [True] * (len(seamed) - 2)


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
def test_budgeted_advance_ends_in_the_separate_launches(seam_double, pipeline):
    """advance(k): k - 1 seam launches, then the error norm and the controller; the state is the one k unseamed attempts leave."""
    blocks = {}
    for seam in ("launches", "resident"):
        s, _ = _solver(seam, pipeline, t=torch.tensor([0.0, 1.0e9], dtype=torch.float64))
        s._before_integrate(np.asarray([0.0, 1.0e9], dtype=np.float64))
        n0 = len(seam_double.launches)
        s.advance(4)
        c = s.advance(3)
        atts = _per_attempt(seam_double.launches[n0:])
        blocks[seam] = (bytes(c), list(s.trace), s._base[0].numpy().copy(), s._base[1].numpy().copy())
        if seam == "resident":
            assert [a[-1] for a in atts] == ["seam"] * 3 + ["control"] + ["seam"] * 2 + ["control"]
            assert [a.count("combine") for a in atts] == [6, 5, 5, 5, 6, 5, 5]
            assert s._carry is False
    a, b = blocks["launches"], blocks["resident"]
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_a_solve_of_one_attempt_takes_no_seam_launch(seam_double):
    s, t = _solver("resident", "sync", t=torch.tensor([0.0, 1e-3], dtype=torch.float64), first_step=1e-3)
    s.integrate(t)
    assert s.stats["n_steps"] == 1 and "seam" not in seam_double.launches


@pytest.mark.parametrize("pipeline", ["sync", "lag"])
def test_expired_barrier_stops_the_solve_and_is_named(seam_double, pipeline):
    """A workgroup whose bounded poll ran out adds one to the non-finite count its controller sees and records the launch's tag: the
    controller stops the solve (XDE_STATUS_NONFINITE) and the host reports the barrier, not the state."""
    seam_double.expire_at = 2
    s, _ = _solver("resident", pipeline, t=torch.tensor([0.0, 1.0e9], dtype=torch.float64))
    s._before_integrate(np.asarray([0.0, 1.0e9], dtype=np.float64))
    with pytest.raises(_hip.XdeError, match="grid barrier of the resident seam launch .controller launch 3. expired"):
        s.advance(8)
    c = seam_double.ctrl_read(s._ctrl)
    assert c.status == _hip.STATUS_NONFINITE and c.nonfinite == 1.0 and seam_double._expired_tag == 3
    # ... and a launch on that state after an expiry stops its solve too (the word is sticky)
    seam_double.expire_at = None
    s2, _ = _solver("resident", pipeline, t=torch.tensor([0.0, 1.0e9], dtype=torch.float64))
    s2._before_integrate(np.asarray([0.0, 1.0e9], dtype=np.float64))
    with pytest.raises(_hip.XdeError, match="expired"):
        s2.advance(3)


def test_expiry_in_the_last_seam_launch_of_an_advance_is_still_reported(seam_double):
    seam_double.expire_at = 1
    s, _ = _solver("resident", "lag", t=torch.tensor([0.0, 1.0e9], dtype=torch.float64))
    s._before_integrate(np.asarray([0.0, 1.0e9], dtype=np.float64))
    with pytest.raises(_hip.XdeError, match="expired"):
        s.advance(3)  # attempts 0 and 1 seamed, attempt 2 on the separate launches


def test_option_values_and_what_resident_refuses(seam_double):
    with pytest.raises(ValueError, match="seam must be"):
        _solver("always", "sync")
    s, t = _solver("resident", "sync", n=(4, 3))
    big = seam_double.RESIDENT * 256 * 4 * 16 + 4096  # one vector per lane more than the carry holds (fp32)
    assert seam_double._seam_plan(big, torch.float32) == {"blocks": 512, "per_lane": 17, "resident": 512, "fits": 0}
    assert seam_double._seam_plan(big - 4096, torch.float32)["fits"] == 1
    assert seam_double._seam_plan(big // 2, torch.float64)["per_lane"] == 17
    seam_double.RESIDENT = 0  # a device that holds no workgroup of the kernel: nothing fits
    with pytest.raises(ValueError, match="cannot serve a state that does not fit"):
        s.integrate(t)
    seam_double.RESIDENT = 512
    from paddlexde_amd import AdaptiveHeun

    y0 = torch.ones(4, 3, dtype=torch.float64)
    b = AdaptiveHeun(xde=BaseODE(lambda t_, y: -y, y0=y0, t_span=t), y0=y0, rtol=1e-6, atol=1e-8, norm=_rms_norm, dtype=torch.float64, seam="resident")
    with pytest.raises(ValueError, match="cannot serve a pair without FSAL and a fused error estimate"):
        b.integrate(t)


def test_auto_leaves_host_tensors_and_small_states_alone(seam_double):
    s, t = _solver("auto", "sync")
    s.integrate(t)
    assert s._seam_on is False and "seam" not in seam_double.launches


def test_geometry_is_the_error_norm_launch_s():
    assert seam_geometry(1, 4) == (1, 0) and seam_geometry(7, 4) == (1, 1) and seam_geometry(1027, 4) == (2, 1)
    assert seam_geometry(256 * 4 * 3 + 5, 4) == (4, 1) and seam_geometry(65536 * 128, 4) == (512, 16) and seam_geometry(65536 * 64, 4) == (512, 8)
    assert seam_geometry(65536 * 64, 2) == (512, 16)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_seam.h
# ----------------------------------------------------------------------------------------------
def test_header_declares_what_python_binds():
    """(The table against the header and the bind's refusals: tests/test_cabi_headers.py.)"""
    assert int(re.search(r"#define XDE_SEAM_CAP\s+(\d+)", open(HEADER).read()).group(1)) == 16


def test_seam_methods_stay_outside_the_backend_contract():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("seam" in m for m in pub)
    assert all(callable(getattr(_hip.HipBackend, m)) for m in ("_seam_plan", "_seam_attempt", "_seam_expired"))


def test_plan_geometry_and_refusals_without_a_launch():
    lib = _hip.load_library()
    assert lib.xde_seam_state_bytes() == 17 * 128
    plan = _hip.XdeSeamPlan()
    for n, dt, want in [(1, 0, (1, 0)), (7, 0, (1, 1)), (1027, 0, (2, 1)), (256 * 4 * 3 + 5, 0, (4, 1)), (65536 * 128, 0, (512, 16)),
                        (65536 * 64, 1, (512, 16)), (65536 * 128 + 4096, 0, (512, 17))]:
        assert lib.xde_seam_plan(n, dt, C.byref(plan)) == _hip.XDE_OK
        assert (plan.blocks, plan.per_lane) == want == seam_geometry(n, 4 if dt == 0 else 2)
        assert plan.fits == int(plan.blocks <= plan.resident and plan.per_lane <= 16)
        assert plan.resident >= 0 and (torch.cuda.is_available() or plan.resident == 0)
    assert lib.xde_seam_plan(0, 0, C.byref(plan)) == _hip.XDE_EBADARG and b"positive" in lib.xde_last_error()
    assert lib.xde_seam_plan(8, 5, C.byref(plan)) == _hip.XDE_EBADARG and b"dtype" in lib.xde_last_error()
    assert lib.xde_seam_plan(8, 0, None) == _hip.XDE_EBADARG
    assert lib.xde_seam_expired(None, None, None) == _hip.XDE_EBADARG and b"xde_seam_expired" in lib.xde_last_error()
    p = _hip.XdeCtrlParams()
    p.n_stage, p.n_seg, p.direction, p.order = 6, 1, 1, 5.0
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    args = lambda **kw: [kw.get("k", a), 1.0, a, a, kw.get("y0_alt"), a, kw.get("f0_alt"), a, a, 0.2, kw.get("n", 8), kw.get("dtype", 0),  # noqa: E731
                         a, a, a, C.byref(kw.get("p", p)), a, None, a, None, kw.get("spin", 1000), None]
    for kw, msg in [({"k": None}, b"null pointer"), ({"y0_alt": a}, b"must come together"), ({"n": 0}, b"positive"),
                    ({"spin": 0}, b"bounded"), ({"dtype": 1}, b"state_dtype")]:
        assert lib.xde_seam_attempt(*args(**kw)) == _hip.XDE_EBADARG
        assert msg in lib.xde_last_error(), (kw, lib.xde_last_error())
    p2 = _hip.XdeCtrlParams()
    p2.n_stage, p2.n_seg, p2.direction, p2.order = 6, 2, 1, 5.0
    assert lib.xde_seam_attempt(*args(p=p2)) == _hip.XDE_EBADARG and b"one segment" in lib.xde_last_error()
    p3 = _hip.XdeCtrlParams()
    p3.struct_size -= 8
    assert lib.xde_seam_attempt(*args(p=p3)) == _hip.XDE_EBADARG and b"layout mismatch" in lib.xde_last_error()
