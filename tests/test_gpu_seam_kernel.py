"""The resident seam launch (csrc/xde_seam.hip, `_seam_attempt`) called DIRECTLY on crafted operands: every instantiation
(float / double x NORM_RMS / NORM_LINF x non-temporal loads on / off), every depth of the register carry that takes another path, the
operand select, `out` over `e_pre`, and non-finite operands.  tests/test_gpu_seam.py reaches the kernel through whole solves.

(a) NORM_LINF as a state machine against the numpy double (tests/_seam_double.py), bit for bit: the max is an exact max, and the
    scripted ratios keep `pow` out of the next step (tests/test_gpu_controller_kernels.py (d) does the same for
    `xde_error_norm_control`).  Reverse time, `step_t`, fp32 and fp64 time, n = 1, 7 (scalar tail only), 1027, 3077.
(b) Both norms against the three launches the seam replaces, byte for byte (`chk` included), at 1, 4, 5, 8, 9, 13 and 16 vectors per
    lane: both sides of every edge of the kernel's batches of 4 and the full carry; the last batch row ends inside workgroup 37, so
    lanes take the clamped reload and later workgroups skip the batch; a scalar tail sits next to it.
(c) NORM_RMS against the numpy double to the bar of tests/_kernel_oracle_cases.py (rel 3e-6 for an fp32 state, 1e-12 for fp64), each
    attempt from the double's own block, and `out` exactly as the header states it from the kernel's own verdict and step.
(d) One non-finite operand at a time — a NaN error at vector 0, in the last workgroup, at the last real vector (the neighbour of the
    clamped lanes), in the scalar tail; an infinite `e_pre`; an infinite `y0` in the body and in the tail; a NaN in the selected
    `y0_alt`; rtol = atol = 0 with a 0 / 0 element — against the three launches byte for byte, NORM_LINF also against the double.
(e) The instantiations without non-temporal loads (XDE_NT=0 is read once per process) in a fresh child: the digests of (a) and (b).

MEASURED on an MI355X (c), worst relative deviation of the kernel's ratio from the double's over the three shapes and four attempts:
    fp32 state: 0 — every ratio equal to the double's once rounded to fp32 (bar 3e-6);  fp64 state: 2.220e-16 (bar 1e-12).

Mutation check (one change at a time in a scratch build of csrc/xde_seam.hip, arithmetic and selection only; first failing test and
what it reported):
the NORM_LINF merge reduced to `ar > acc ? ar : acc` (a NaN is lost) — test_nonfinite_operands[nan_k_vector0-n3077-f32-linf], the
block against the three launches: `ratio` finite where theirs is NaN; `on` ignored (a clamped lane is counted) —
test_carry_vs_three_launches[p16-f32-rms], attempt 0, the block: `ratio`; `c1` formed from the `dt` read before the barrier —
test_linf_state_machine_vs_double[1-f32-t64], attempt 2 (the first after the step has changed), `out`; the rejected path always on
`f0[0]` — test_carry_vs_three_launches[p16-f32-rms], attempt 1 (rejected on the selected candidates), `out` from element 0; `sel`
without `accw` — test_linf_state_machine_vs_double[7-f32-t64], attempt 3 (candidates passed after a rejected attempt), `ratio_prev` /
`ratio`; the tail element's error without `epre[tj]` — test_linf_state_machine_vs_double[1-f32-t64], attempt 0, `dt` (and `ratio`);
`nf_d` taken from every lane — test_nonfinite_operands[inf_y0_body-n3077-f32-rms], the block: `nonfinite`; slot `j` of the accepted
path on `ck[j ^ 1]` — test_linf_state_machine_vs_double[7-f64-t64], attempt 0, `out` from element 0.
"""
import os
import subprocess
import sys

import pytest
import torch

from paddlexde_amd import _hip

from . import _seam_drivers as D
from ._controller_drivers import SENTINEL, block_of, fields
from ._seam_double import SeamDoubleBackend
from .test_gpu_controller_kernels import _G, _R, _mid_solve_params, assert_blocks_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["f32", "f64"]
NORMS = ["rms", "linf"]


@pytest.fixture(scope="module")
def be():
    return _hip.get_backend()


@pytest.fixture(scope="module")
def dbl():
    return SeamDoubleBackend()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def workspaces(be, dev):
    """ONE pair of workspaces (seam side, three-launch side) for every case of (b) and (d): the records of wider grids stay behind."""
    return be.new_workspace(dev), be.new_workspace(dev)


_digests = {}  # what (a) and (b) compared, by case: computed once, read again by (e)


def _digest(key, run):
    if key not in _digests:
        _digests[key] = run()
    return _digests[key]


# ------------------------------------------------------------------------------------------------------------------------------
# (a) NORM_LINF against the numpy double
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", ["f64", "f32"], ids=["t64", "t32"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 1027, 3077])
def test_linf_state_machine_vs_double(be, dbl, dev, n, dtype, tdt):
    _digest(("a", dtype, tdt, n), lambda: D.state_machine(be, dbl, dev, dtype, tdt, n))


# ------------------------------------------------------------------------------------------------------------------------------
# (b) both norms against the three launches, across the carry
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", D.DEPTHS, ids=["p{}".format(p) for p in D.DEPTHS])
def test_carry_vs_three_launches(be, dev, workspaces, p, dtype, norm):
    _digest(("b", dtype, norm, p), lambda: D.carry_run(be, dev, dtype, norm, p, *workspaces))


# ------------------------------------------------------------------------------------------------------------------------------
# (c) NORM_RMS against the numpy double
# ------------------------------------------------------------------------------------------------------------------------------
RMS_SHAPES = {"n1027": lambda w: 1027, "n3077": lambda w: 3077, "p5": lambda w: D.carry_n(5, w)}
RMS_TARGETS = (0.5, 3.0, 0.05, 40.0)
RMS_BAR = {"f32": 3e-6, "f64": 1e-12}  # tests/_kernel_oracle_cases.py: numpy's pairwise sum vs fp32 lanes -> fp64 accumulation


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(RMS_SHAPES))
def test_rms_vs_double(be, dbl, dev, shape, dtype):
    """Four attempts (ratio 0.5, 3, 0.05, 40: the double's ratio is asserted at least 1e-3 away from 1 before the kernel is looked at),
    each from the double's own block, odd ones on (y0_alt, f0_alt) with `out` over `e_pre`: the ratio within the bar, the verdict and
    the counters the double's, and `out` byte-equal to the header's statement evaluated with the kernel's own verdict and next step."""
    dt = D.DT[dtype]
    n = RMS_SHAPES[shape](D.WIDTH[dtype])
    D.check_plan(be, n, dtype, per_lane=5 if shape == "p5" else 1)
    o = D.operands(n, dtype, 7)
    od = {name: t.to(dev) for name, t in o.items()}
    p = _mid_solve_params(dtype, _hip.NORM_RMS, [n])
    ts = torch.tensor(D.CARRY_T_SPAN, dtype=torch.float64)
    ts_d = ts.to(dev)
    cd = dbl.new_ctrl(None)
    sd = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt)
    dbl.ctrl_init(cd, p, 0.0, 0.01, 4, ts, None, sd)
    cg = torch.zeros(cd.numel(), dtype=torch.uint8, device=dev)
    sg = sd.to(dev)
    ws = be.new_workspace(dev)
    worst = 0.0
    for i, target in enumerate(RMS_TARGETS):
        tag = (shape, dtype, i, target)
        alt = alias = i % 2 == 1
        cg.copy_(cd)  # (the next step comes out of one `pow`: every attempt starts from the same block on both sides)
        before = dbl.ctrl_read(cd)
        scale = target / D.probe_ratio(dbl, cd, p, o, ts, None, sd, alt)
        ka, ea = o["k"] * scale, o["e"] * scale
        dbl._seam_attempt(ka, D.C_LAST, ea.clone(), o["y0"], o["f0"], o["y1"], torch.empty_like(ea), D.A21, None, cd, p, ts, None, sd,
                          y0_alt=o["y0a"] if alt else None, f0_alt=o["f0a"] if alt else None)
        want = dbl.ctrl_read(cd)
        assert abs(want.ratio - 1) >= 1e-3 and abs(want.ratio / target - 1) < 1e-3 and want.accept == (target < 1), tag + (want.ratio,)
        ka_d, ea_d = ka.to(dev), ea.to(dev, copy=True)
        out_d = ea_d if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        be._seam_attempt(ka_d, D.C_LAST, ea_d, od["y0"], od["f0"], od["y1"], out_d, D.A21, ws, cg, p, ts_d, None, sg,
                         y0_alt=od["y0a"] if alt else None, f0_alt=od["f0a"] if alt else None)
        got = block_of(cg)
        rel = abs(got.ratio / want.ratio - 1)
        worst = max(worst, rel)
        print("rms {} {} attempt {}: kernel {!r} double {!r} rel {:.3e}".format(shape, dtype, i, got.ratio, want.ratio, rel))
        assert got.ratio == pytest.approx(want.ratio, rel=RMS_BAR[dtype]), tag + (got.ratio, want.ratio)
        for f in ("accept", "sel_used", "status", "nonfinite", "n_steps", "n_accept", "n_reject", "t0", "t1", "dt_last", "seq"):
            assert getattr(got, f) == getattr(want, f), tag + (f, fields(got), fields(want))
        stated = D.stated_out(o, ka, dtype, got.dt, got.accept, alt and before.accept)
        assert out_d.cpu().numpy().tobytes() == stated.tobytes(), tag + ("out",)
        assert be._seam_expired(cg) == 0, tag
    print("rms {} {}: worst relative deviation {:.3e} (bar {:.0e})".format(shape, dtype, worst, RMS_BAR[dtype]))


# ------------------------------------------------------------------------------------------------------------------------------
# (d) non-finite operands
# ------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# name -> (what is poisoned, alt passed, the clean operands' ratio, tolerances zeroed, kind of outcome)
POISONS = {
    "nan_k_vector0": ("k", False, _R, False, "nan"),
    "nan_k_last_workgroup": ("k", False, _R, False, "nan"),
    "nan_k_last_vector": ("k", False, _R, False, "nan"),
    "nan_k_tail": ("k", False, _R, False, "nan"),
    "inf_epre_body": ("e", False, _G, False, "inf"),
    "inf_y0_body": ("y0", False, _G, False, "count"),
    "inf_y0_tail": ("y0", False, _R, False, "count"),
    "nan_y0alt_selected": ("y0a", True, _R, False, "count"),
    "zero_tol_zero_over_zero": ("y0", False, _R, True, "nan"),
}
POISON_SHAPES = {"n3077": lambda w: 3077, "p5": lambda w: D.carry_n(5, w)}
_clean = {}


def _clean_operands(n, dtype, dev):
    """The clean operands of (d) on the host and on the device, made once per (n, dtype) and never modified (a case poisons copies)."""
    if (n, dtype) not in _clean:
        o = D.operands(n, dtype, 13)
        _clean[(n, dtype)] = (o, {name: t.to(dev) for name, t in o.items()})
    return _clean[(n, dtype)]


def _poisoned(case, o, n, w):
    """A copy of the operand set with ONE poison, and where it sits."""
    nvec = n // w
    blocks, _ = D.geometry(n, w)
    what = POISONS[case][0]
    q = dict(o)
    q[what] = o[what].clone()
    at = {
        "nan_k_vector0": 0,
        "nan_k_last_workgroup": (blocks - 1) * D.BLOCK * w + (w - 1),
        "nan_k_last_vector": (nvec - 1) * w,
        "nan_k_tail": n - 1,
        "inf_epre_body": (nvec // 2) * w + 1,
        "inf_y0_body": (nvec // 3) * w,
        "inf_y0_tail": n - 1,
        "nan_y0alt_selected": (nvec // 2) * w,
        "zero_tol_zero_over_zero": (nvec // 2) * w + 1,
    }[case]
    assert n % w and (blocks - 1) * D.BLOCK < nvec and 0 <= at < n and (at >= nvec * w) == case.endswith("tail"), (case, n, at)
    if case == "zero_tol_zero_over_zero":
        for name in ("y0", "y1", "e", "k"):  # e = 0 + 0 * c over tol = 0 + 0 * max(0, 0)
            q[name] = o[name].clone()
            q[name][at] = 0.0
    else:
        q[what][at] = NAN if case.startswith("nan") else INF
    return q, at


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(POISON_SHAPES))
@pytest.mark.parametrize("case", list(POISONS))
def test_nonfinite_operands(be, dbl, dev, workspaces, case, shape, dtype, norm):
    """A clean accepted attempt, then the poisoned one, on a fresh mirrored block; the three launches run on a byte-identical bare copy
    of it.  Blocks (`chk` too), stage times and `out` byte-identical; NORM_LINF: every field, the stage times and `out` equal to the
    double's.  The clean operands' ratio sits in a range that keeps `pow` out of the next step.  A NaN error: ratio NaN, status 0,
    rejected, the step shrunk by dfactor.  A non-finite element of the y0 the attempt ran on: counted, XDE_STATUS_NONFINITE.  Never an
    expired barrier."""
    dt, w = D.DT[dtype], D.WIDTH[dtype]
    n = POISON_SHAPES[shape](w)
    D.check_plan(be, n, dtype, per_lane=5 if shape == "p5" else 1)
    _, alt1, target1, zero_tol, outcome = POISONS[case]
    clean, cleand = _clean_operands(n, dtype, dev)
    q, at = _poisoned(case, clean, n, w)
    qd = {name: (cleand[name] if t is clean[name] else t.to(dev)) for name, t in q.items()}
    p = _mid_solve_params(dtype, D.KIND[norm], [n])
    pz = _mid_solve_params(dtype, D.KIND[norm], [n])
    pz.rtol = pz.atol = 0.0
    segs = _hip.make_segments([(0, n)])
    ts = torch.tensor(D.CARRY_T_SPAN, dtype=torch.float64)
    ts_d = ts.to(dev)
    ca, cd = be.new_ctrl(dev), dbl.new_ctrl(None)  # (fresh: the expiry word is sticky per block)
    sa = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
    sd = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt)
    be.ctrl_init(ca, p, 0.0, 0.01, 4, ts_d, None, sa)
    dbl.ctrl_init(cd, p, 0.0, 0.01, 4, ts, None, sd)
    seq0 = block_of(ca).seq
    cb, sb = ca.clone(), sa.clone()
    ws_a, ws_b = workspaces
    for attempt in range(2):
        tag = (case, shape, dtype, norm, attempt, at)
        poisoned = attempt == 1
        alt = poisoned and alt1
        pp = pz if (poisoned and zero_tol) else p
        src, srcd = (q, qd) if poisoned else (clean, cleand)
        # the scale comes from the CLEAN operands (the double, on scratch copies of its block)
        scale = (target1 if poisoned else _G) / D.probe_ratio(dbl, cd, p, clean, ts, None, sd, alt)
        ka, ea = src["k"] * scale, src["e"] * scale
        ka_d = ka.to(dev)
        ea_a, ea_b = ea.to(dev, copy=True), ea.to(dev, copy=True)
        alias = poisoned
        oa = ea_a if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        ob = ea_b if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        oh = ea if alias else torch.full((n,), SENTINEL, dtype=dt)
        alts_d = (srcd["y0a"], srcd["f0a"]) if alt else (None, None)
        be._seam_attempt(ka_d, D.C_LAST, ea_a, srcd["y0"], srcd["f0"], srcd["y1"], oa, D.A21, ws_a, ca, pp, ts_d, None, sa,
                         y0_alt=alts_d[0], f0_alt=alts_d[1])
        D.three_launches(be, ka_d, ea_b, srcd["y0"], srcd["f0"], srcd["y1"], ob, ws_b, cb, pp, ts_d, None, sb, segs, *alts_d)
        dbl._seam_attempt(ka, D.C_LAST, ea, src["y0"], src["f0"], src["y1"], oh, D.A21, None, cd, pp, ts, None, sd,
                          y0_alt=src["y0a"] if alt else None, f0_alt=src["f0a"] if alt else None)
        read = be.ctrl_read(ca)
        ga, gb, want = block_of(ca), block_of(cb), dbl.ctrl_read(cd)
        assert bytes(read) == bytes(ga), tag
        assert bytes(ga) == bytes(gb), tag + (fields(ga), fields(gb))
        assert D.same_bytes(sa, sb), tag
        assert D.same_bytes(oa, ob), tag + ("out",)
        assert be._seam_expired(ca) == 0, tag + ("a non-finite operand was reported as an expired barrier",)
        if norm == "linf":
            assert_blocks_equal(ga, want, tag, seq0)
            assert sa.cpu().numpy().tobytes() == sd.numpy().tobytes(), tag
            assert oa.cpu().numpy().tobytes() == oh.numpy().tobytes(), tag + ("out vs the double",)
        if not poisoned:
            assert (ga.accept, ga.status, ga.nonfinite) == (1, 0, 0.0) and ga.ratio < 1e-6, tag + (fields(ga),)
    # what the double does with each kind of poison, stated once more without it
    if outcome == "nan":
        assert ga.ratio != ga.ratio and (ga.status, ga.accept, ga.nonfinite) == (0, 0, 0.0) and ga.dt == ga.dt_last * 0.2, fields(ga)
    elif outcome == "inf":
        assert ga.ratio == INF and (ga.status, ga.accept, ga.nonfinite) == (0, 0, 0.0) and ga.dt == ga.dt_last * 0.2, fields(ga)
    else:
        assert ga.nonfinite == 1.0 and ga.status == _hip.STATUS_NONFINITE and ga.ratio == ga.ratio, fields(ga)
        assert ga.accept == (1 if target1 == _G else 0), fields(ga)
    assert want.ratio != want.ratio if outcome == "nan" else want.ratio == want.ratio, fields(want)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) the instantiations without non-temporal loads
# ------------------------------------------------------------------------------------------------------------------------------
def test_nt_off_instantiations_in_a_fresh_child(be, dbl, dev, workspaces):
    """XDE_NT=0 (read once per process: a fresh child, tests/_seam_nt_child.py) selects the four instantiations with plain loads.  The
    child runs (b) at 1 and 5 vectors per lane for both dtypes and norms and (a) at n = 3077 for both state and time dtypes — with
    their own assertions — and prints a digest of everything each compared; the digests are those of the default policy."""
    from ._seam_nt_child import CASES

    assert (int(os.environ.get("XDE_NT", "7")) & 1) == 1, "this process must run the default load policy"
    mine = {}
    for key in CASES:
        if key[0] == "a":
            mine[key] = _digest(key, lambda: D.state_machine(be, dbl, dev, key[1], key[2], key[3]))
        else:
            mine[key] = _digest(key, lambda: D.carry_run(be, dev, key[1], key[2], key[3], *workspaces))
    env = dict(os.environ, XDE_NT="0")
    r = subprocess.run([sys.executable, "-m", "tests._seam_nt_child"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "CHILD OK nt=0" in r.stdout
    got = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("DIGEST "))
    assert set(got) == {"-".join(map(str, k)) for k in CASES}
    bad = [k for k in CASES if got["-".join(map(str, k))] != mine[k]]
    assert not bad, bad
