"""GPU parity, kernel level, for the device-resident step controller (csrc/xde_control_device.hpp, csrc/xde_control.hip): the four
launches that run it — `xde_rk_control` fed through `sums` and through `ws`, `xde_error_norm_control` on its one-workgroup and on its
ticketed path — and the three that construct its block (`xde_ctrl_init`, `xde_initial_step_fused`, `xde_initial_step_tail`).

(a) The state machine, EXACTLY: every script of tests/_controller_scripts.py and its reverse-time twin, launch by launch against the
    numpy double (which tests/test_controller_double_host.py holds to the oracle): all fields of `xde_ctrl_t` but `chk` / `reserved`
    bit for bit, the stage times as bytes, `chk` recomputed, the mirror's block byte-equal to device memory, sentinels past `n_stage`.
    The scripts' ratios are chosen so that no `pow` result can differ between implementations (see the case table's ratio policy).
(b) The `pow`-dependent step factor, one attempt at a time against mpmath at 200 bits on the kernel's own rounded inputs.
(c) The partials path (`ws`) against the sums path, byte for byte, over grids that shrink (stale records in the workspace).
(d) The fused launch as a state machine (NORM_LINF: the reduction is an exact max).
(e) Block construction, field by field.
(f) The other publish protocols (`XDE_CTRL_FLAGS` 0 and 7) in fresh child processes: same digests as the default.

MEASURED on an MI355X (b), fp64 time, worst error of the next step in ulp of the result, over 2 000 ratios for each of the orders 2, 3,
5 and 8 (dt = 1/64, safety 0.9, ifactor 10, dfactor 0.2, PI: beta 0.04, prev 0.5):
    I  controller: kernel 1.927 ulp, numpy statement 1.306 ulp  (bound: statement + 2 = 3.306)
    PI controller: kernel 2.271 ulp, numpy statement 1.683 ulp  (bound: statement + 4 = 5.683)
fp32 time: 8 000 ratios per controller, none skipped at a rounding midpoint, every next step equal to the statement bit for bit.

Mutation check (one change at a time in a scratch build; each caught by test_state_machine_bit_for_bit, first failing script / field):
`<=` -> `<` in the min_step accept — ratio_above_one_clipped, attempt 1 (dt == min_step, ratio > 1), `t1`; `ratio <= 1` -> `< 1` —
ratio_edges, the attempt with ratio exactly 1, `t1`; `ratio < 1` -> `<= 1` for the dfactor reset — the same attempt, `dt` (factor 1
instead of 0.9); `<=` -> `<` in the row scan — step_t_inside_reject_and_row, the row whose time equals t1; `table_at` returning slot 0
for `base + 1` — the same script, `out_end` (a step that covers one row reports two); `steps_in_interval` not reset on an emitted row —
the same script, `steps_in_interval`; `ratio_prev` updated on a rejected attempt — ratio_edges, `ratio_prev`; stage time `t0 + a * dt`
where alpha == 1 (fp32 state) — ratio_above_one_clipped in fp64 time / fp32 state, the stage times; `accept` left as it was by the no-op
after `done` — after_done, `accept`; `control_step<float>` chosen for fp64 time — ratio_above_one_clipped, `dt` after the first
attempt; the sign dropped in the magnitude clip — ratio_edges' reverse twin, `dt`.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from mpmath import mp, mpf

from paddlexde_amd import _hip

from . import _controller_scripts as S
from ._controller_drivers import SENTINEL, block_of, digest, fields, gpu_run, run_double, same
from ._cpu_double import NumpyDoubleBackend
from .test_gpu_handover_kernels import _checksum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": torch.float32, "f64": torch.float64}
NPT = S.TT
CHECKSUMMED = (int(os.environ.get("XDE_CTRL_FLAGS", "15")) & 8) != 0
SKIP = ("chk", "reserved")
N_CHUNKS = 8


@pytest.fixture(scope="module")
def be():
    return _hip.get_backend()


@pytest.fixture(scope="module")
def dbl():
    return NumpyDoubleBackend()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_double_runs = {}


def double_of(s):
    """The double's run of a script: computed once, shared by every test that needs it, never modified."""
    if s.id not in _double_runs:
        _double_runs[s.id] = run_double(s)
    return _double_runs[s.id]


def assert_blocks_equal(got, want, tag, seq0=0):
    """Every field but `chk` / `reserved`, bit for bit (`seq` counted from `seq0`)."""
    fg, fw = fields(got), fields(want)
    fg["seq"] -= seq0
    for f in fw:
        if f in SKIP:
            continue
        a = np.array(fg[f], dtype=np.float64 if isinstance(fw[f], float) or (isinstance(fw[f], tuple) and isinstance(fw[f][0], float)) else np.int64)
        b = np.array(fw[f], dtype=a.dtype)
        assert a.tobytes() == b.tobytes(), tag + (f, fg[f], fw[f])


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the state machine
# ------------------------------------------------------------------------------------------------------------------------------
ALL_SCRIPTS = [x for s in S.SCRIPTS for x in (s, s.reversed())]


@pytest.mark.parametrize("mirrored", [True, False], ids=["mirror", "bare"])
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_state_machine_bit_for_bit(be, dev, chunk, mirrored):
    """`ctrl_init`, then one `rk_control(ctrl, p, None, sums, ...)` per attempt of every script (chunk `chunk` of them), each block and
    each stage-time buffer equal to the double's; `chk` is the block's checksum under the default protocol; with a control block from
    `new_ctrl` the mirror's copy is the block in device memory (gpu_run), with a bare tensor there is no mirror at all."""
    launches = 0
    for s in ALL_SCRIPTS[chunk::N_CHUNKS]:
        blocks, stages = gpu_run(be, dev, s, mirrored)
        want_b, want_s = double_of(s)
        assert len(blocks) == len(want_b) == len(s.attempts) + 1
        if not mirrored:
            assert blocks[0].seq == 0, s.id
        n = len(s.alpha)
        for i, (g, w) in enumerate(zip(blocks, want_b)):
            tag = (s.id, "mirror" if mirrored else "bare", "init" if i == 0 else "attempt {}".format(i - 1))
            assert_blocks_equal(g, w, tag, seq0=blocks[0].seq)
            assert stages[i].tobytes() == want_s[i].tobytes(), tag + (stages[i], want_s[i])
            assert (stages[i][n:] == SENTINEL).all(), tag
            if i and CHECKSUMMED:
                assert g.chk == _checksum(g), tag
            launches += 1
    assert launches > 500


# ------------------------------------------------------------------------------------------------------------------------------
# (f) the other publish protocols
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_digests(be, dev):
    out = {}
    for s0 in S.FIXED:
        for s in (s0, s0.reversed()):
            out[s.id] = digest(s, *gpu_run(be, dev, s, True))
    return out


@pytest.mark.parametrize("flags", [0, 7])
def test_other_publish_protocols_publish_the_same_block(default_digests, flags):
    """`XDE_CTRL_FLAGS` 0 (SEQLOCK publish with system-scope fences, two-trip partials, no time prefetch) and 7 (SEQLOCK with light
    ordering, speculative partials, prefetch) in a fresh child: every fixed script and its reverse twin, through a mirrored block, leaves
    the digests of the default protocol (15); without bit 8 `chk` keeps what init left in it (checked in the child)."""
    env = dict(os.environ, XDE_CTRL_FLAGS=str(flags))
    r = subprocess.run([sys.executable, "-m", "tests._controller_flags_child"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (flags, r.stdout[-2000:], r.stderr[-4000:])
    assert "CHILD OK flags={}".format(flags) in r.stdout
    got = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("DIGEST "))
    assert set(got) == set(default_digests)
    bad = [k for k in got if got[k] != default_digests[k]]
    assert not bad, (flags, bad)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the pow-dependent factor, one attempt at a time
# ------------------------------------------------------------------------------------------------------------------------------
SWEEP_ORDERS = (2, 3, 5, 8)
SWEEP_N = 2000
SAFETY, IFACTOR, DFACTOR, PREV, DT0 = 0.9, 10.0, 0.2, 0.5, 1.0 / 64


def _sweep_ratios(order, pi):
    """2 000 log-spaced ratios across both unclamped ranges: below 1 (dfactor reset to 1: 1 < factor < ifactor) and from 1 up
    (dfactor < factor <= safety * prev**beta); 2% inside each end."""
    a = 1.0 / order - (0.75 * S.PI_BETA if pi else 0.0)
    top = SAFETY * (PREV**S.PI_BETA if pi else 1.0)
    lo1, hi1 = (top / IFACTOR) ** (1 / a), min(top ** (1 / a), 1.0)
    lo2, hi2 = 1.0, (top / DFACTOR) ** (1 / a)
    half = SWEEP_N // 2
    return np.concatenate([np.geomspace(lo1 * 1.02, hi1 / 1.02, half), np.geomspace(lo2 * 1.0001, hi2 / 1.02, SWEEP_N - half)])


def _sweep_params(tdt, order, pi):
    p = _hip.XdeCtrlParams()
    T = NPT[tdt]
    p.rtol, p.atol, p.min_step, p.max_step = 1e-3, 1e-6, 0.0, float("inf")
    p.safety, p.ifactor, p.dfactor, p.order = float(T(SAFETY)), float(T(IFACTOR)), float(T(DFACTOR)), float(order)
    p.max_num_steps = S.NO_LIMIT
    p.time_dtype = _hip.XDE_F32 if tdt == "f32" else _hip.XDE_F64
    p.state_dtype = _hip.XDE_F64
    p.direction, p.norm_kind, p.n_stage, p.n_seg = 1, _hip.NORM_LINF, 2, 1
    p.alpha[0], p.alpha[1] = 0.5, 1.0
    p.seg_count[0] = 1.0
    p.pi_controller, p.pi_beta = int(pi), S.PI_BETA
    return p


def _sweep_launch(be, dbl, dev, tdt, order, pi, ratios):
    """One controller launch per ratio, each from its own copy of ONE fixed block (t = 0, dt = 1/64, ratio_prev = 1/2, no clipping);
    returns (kernel blocks, double blocks)."""
    p = _sweep_params(tdt, order, pi)
    ts = torch.tensor([0.0, 1e9], dtype=torch.float64)
    t_stage = torch.zeros(_hip.XDE_MAX_STAGE, dtype=torch.float64)
    c0 = dbl.new_ctrl(None)
    dbl.ctrl_init(c0, p, 0.0, DT0, 2, ts, None, t_stage)
    dbl._c(c0).ratio_prev = PREV
    n = len(ratios)
    size = C.sizeof(_hip.XdeCtrl)
    ctrls = c0.repeat(n, 1).to(dev)
    sums_h = torch.zeros(n, 2 * _hip.XDE_MAX_SEG, dtype=torch.float64)
    sums_h[:, 0] = torch.from_numpy(ratios)
    sums, ts_d, stage_d = sums_h.to(dev), ts.to(dev), t_stage.to(dev)
    for i in range(n):
        be.rk_control(ctrls[i], p, None, sums[i], ts_d, None, stage_d)
    raw = ctrls.cpu().numpy()
    got = [_hip.XdeCtrl.from_buffer_copy(raw[i].tobytes()) for i in range(n)]
    want = []
    for i in range(n):
        c = c0.clone()
        dbl.rk_control(c, p, None, sums_h[i], ts, None, t_stage)
        want.append(dbl.ctrl_read(c))
    assert size == raw.shape[1]
    return got, want


EXACT_IN_SWEEP = ("accept", "sel_used", "status", "n_steps", "n_accept", "n_reject", "steps_in_interval", "out_begin", "out_end", "next_out",
                  "n_out", "done", "next_step_index", "on_step_t", "seq", "ratio", "ratio_seg", "nonfinite", "t0", "t1", "dt_last")


def _assert_decisions(got, want, tag):
    for i, (g, w) in enumerate(zip(got, want)):
        fg, fw = fields(g), fields(w)
        for f in EXACT_IN_SWEEP:
            assert same(fg[f], fw[f]), tag + (i, f, fg[f], fw[f])


def _round24(x):
    """mpf -> the nearest float32 (one rounding), and whether x lies within 2^-40 (relative) of a rounding midpoint."""
    with mp.workprec(24):
        r = +x
    with mp.workprec(200):
        ulp = mpf(2) ** (mp.floor(mp.log(abs(x), 2)) - 23)
        frac = (x / ulp) - mp.floor(x / ulp)
        near = abs(frac - mpf(0.5)) * ulp < abs(x) * mpf(2) ** -40
    return np.float32(float(r)), bool(near)


@pytest.mark.parametrize("pi", [False, True], ids=["I", "PI"])
def test_step_factor_fp32_time_equals_the_statement(be, dbl, dev, pi):
    """fp32 time: the next `dt` equals, bit for bit, `float32(dt * min(ifactor, max(safety [* float32(prev**beta)] / float32(r**e),
    dfactor)))` with the TRUE powers (mpmath, 200 bits) rounded once to float32 and every other operation in float32 as the kernel does
    it.  A ratio is skipped only when a true power lies within 2^-40 of a float32 rounding midpoint: at most 1% (expected: none)."""
    F = np.float32
    skipped = checked = 0
    for order in SWEEP_ORDERS:
        ratios = _sweep_ratios(order, pi)
        got, want = _sweep_launch(be, dbl, dev, "f32", order, pi, ratios)
        _assert_decisions(got, want, ("f32", order, pi))
        beta = F(S.PI_BETA)
        e = F(1) / F(order) - (F(0.75) * beta if pi else F(0))
        prev = F(PREV)
        with mp.workprec(200):
            pb, near_b = _round24(mp.power(mpf(float(prev)), mpf(float(beta)))) if pi else (F(1), False)
        for i, r in enumerate(ratios):
            r32 = F(r)
            with mp.workprec(200):
                pa, near_a = _round24(mp.power(mpf(float(r32)), mpf(float(e))))
            if near_a or near_b:
                skipped += 1
                continue
            x = (F(SAFETY) * pb / pa) if pi else (F(SAFETY) / pa)
            dfac = F(1) if r32 < 1.0 else F(DFACTOR)  # (state dtype fp64: the kernel compares the ratio it was given; r32 == 1 is not in the sweep)
            factor = np.fmin(F(IFACTOR), np.fmax(x, dfac))
            stated = F(DT0) * factor
            assert dfac < factor < F(IFACTOR), (order, pi, r, factor)  # (the sweep stays unclamped)
            assert F(got[i].dt).tobytes() == stated.tobytes() and got[i].dt == float(F(got[i].dt)), (order, pi, i, r, got[i].dt, float(stated))
            checked += 1
    print("fp32-time sweep ({}): {} ratios checked, {} skipped at rounding midpoints".format("PI" if pi else "I", checked, skipped))
    assert skipped <= 0.01 * (checked + skipped) and checked >= 0.99 * SWEEP_N * len(SWEEP_ORDERS)


@pytest.mark.parametrize("pi", [False, True], ids=["I", "PI"])
def test_step_factor_fp64_time_within_the_statements_error(be, dbl, dev, pi):
    """fp64 time: neither the device's `pow` nor glibc's is correctly rounded.  The kernel's next `dt` and the numpy statement's are
    both measured against `dt * min(ifactor, max(safety [* prev**beta] / r**e, dfactor))` in exact arithmetic on the rounded inputs
    (mpmath, 200 bits), in ulp of the result.  The kernel must stay within the numpy statement's own worst error plus 2 ulp per `pow`
    call of the formula (+2 for I, +4 for PI): the device's `pow` may be that much looser than libm's, and no looser."""
    worst_k = worst_n = 0.0
    for order in SWEEP_ORDERS:
        ratios = _sweep_ratios(order, pi)
        got, want = _sweep_launch(be, dbl, dev, "f64", order, pi, ratios)
        _assert_decisions(got, want, ("f64", order, pi))
        e = 1.0 / order - (0.75 * S.PI_BETA if pi else 0.0)  # (as the kernel forms it, in fp64)
        with mp.workprec(200):
            top = mpf(SAFETY) * (mp.power(mpf(PREV), mpf(S.PI_BETA)) if pi else mpf(1))
            for i, r in enumerate(ratios):
                x = top / mp.power(mpf(float(r)), mpf(e))
                dfac = mpf(1) if r < 1.0 else mpf(DFACTOR)
                ref = mpf(DT0) * min(mpf(IFACTOR), max(x, dfac))
                ulp = mpf(float(np.spacing(float(ref))))
                worst_k = max(worst_k, float(abs(mpf(got[i].dt) - ref) / ulp))
                worst_n = max(worst_n, float(abs(mpf(want[i].dt) - ref) / ulp))
    margin = 4.0 if pi else 2.0
    print("fp64-time sweep ({}): kernel worst {:.3f} ulp, numpy statement worst {:.3f} ulp, bound {:.3f}".format(
        "PI" if pi else "I", worst_k, worst_n, worst_n + margin))
    assert worst_k <= worst_n + margin, (worst_k, worst_n)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the partials path against the sums path
# ------------------------------------------------------------------------------------------------------------------------------
def _mid_solve_params(sdt, norm_kind, lens, tdt="f64", direction=1, n_step_t=0):
    p = _hip.XdeCtrlParams()
    p.rtol, p.atol, p.min_step, p.max_step = 1e-3, 1e-5, 0.0, float("inf")
    p.safety, p.ifactor, p.dfactor, p.order = 0.9, 10.0, 0.2, 5.0
    p.max_num_steps = S.NO_LIMIT
    p.time_dtype = _hip.XDE_F32 if tdt == "f32" else _hip.XDE_F64
    p.state_dtype = _hip.XDE_F32 if sdt == "f32" else _hip.XDE_F64
    p.direction, p.norm_kind, p.n_stage, p.n_seg, p.n_step_t = direction, norm_kind, 6, len(lens), n_step_t
    for i, a in enumerate(S.ALPHA["dopri5"][1]):
        p.alpha[i] = a
    for i, l in enumerate(lens):
        p.seg_count[i] = float(l)
    return p


def _padded_segments(lens, width):
    segl, off = [], 0
    for l in lens:
        segl.append((off, l))
        off += -(-l // width) * width
    return segl, off


SMALL_LENS = [1, 5, 300, 37, 1000, 2, 64, 129, 7, 513, 3, 255, 4096, 11, 90]


@pytest.mark.parametrize("norm_kind", [_hip.NORM_RMS, _hip.NORM_LINF], ids=["rms", "linf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_partials_path_equals_sums_path(be, dev, dtype, norm_kind):
    """`rk_control(ws, sums=None)` against `norm_finalize` + `rk_control(None, sums)` from two byte-identical copies of one mid-solve
    block: blocks (so `chk` too) and stage times byte-identical.  The first segment has n = 2^21 + 3, 65536 + 8, 1000, 1 elements IN
    THAT ORDER on ONE workspace (each launch's grid is smaller than the one before: the records it does not write are stale and must be
    masked by the speculative load), with 1, 5 (fp32 time) and 16 padded segments; two consecutive attempts per case."""
    dt = DT[dtype]
    width = 4 if dtype == "f32" else 2
    ws, sums = be.new_workspace(dev), be.new_sums(dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    big = (1 << 21) + 3 + sum(SMALL_LENS) + 64
    pool = [torch.randn(big, generator=gen, dtype=dt, device=dev) for _ in range(4)]
    ts = torch.tensor([0.0, 0.004, 0.03, 10.0], dtype=torch.float64, device=dev)
    c_err = [1.2e-3, -7.5e-3]
    for n in ((1 << 21) + 3, 65536 + 8, 1000, 1):
        for n_seg in (16, 5, 1):
            lens = [n] + SMALL_LENS[: n_seg - 1]
            segl, total = _padded_segments(lens, width)
            segs = _hip.make_segments(segl)
            y0, ks = pool[0][:total], [pool[2][:total], pool[3][:total]]
            y1 = y0 + 1e-3 * pool[1][:total]
            p = _mid_solve_params(dtype, norm_kind, lens, tdt="f32" if n_seg == 5 else "f64")
            a = torch.zeros(C.sizeof(_hip.XdeCtrl), dtype=torch.uint8, device=dev)
            sa = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
            be.ctrl_init(a, p, 0.0, 0.01, 4, ts, None, sa)
            b, sb = a.clone(), sa.clone()
            for attempt in range(2):
                be.error_norm_partial(ks, c_err, y0, y1, p.rtol, p.atol, segs, norm_kind, ws, ctrl=a)
                be.norm_finalize(ws, 0, sums)
                be.rk_control(a, p, ws, None, ts, None, sa)
                be.rk_control(b, p, None, sums, ts, None, sb)
                ga, gb = block_of(a), block_of(b)
                tag = (dtype, norm_kind, n, n_seg, attempt)
                assert bytes(ga) == bytes(gb), tag + (fields(ga), fields(gb))
                assert sa.cpu().numpy().tobytes() == sb.cpu().numpy().tobytes(), tag
                assert ga.n_steps == attempt + 1 and ga.ratio == ga.ratio and ga.ratio > 0, tag
                if CHECKSUMMED:
                    assert ga.chk == _checksum(ga), tag


# ------------------------------------------------------------------------------------------------------------------------------
# (d) the fused launch as a state machine
# ------------------------------------------------------------------------------------------------------------------------------
_G, _R = 1e-9, 1e9  # GROW / SHRINK of dopri5's I controller (bounds 5.9e-6 and 1.8e3), small enough to stay normal in fp32 operands
assert _G < S.ratio_ranges(5, S.TRIPLES[0], False)[1] and _R > S.ratio_ranges(5, S.TRIPLES[0], False)[2]
FUSED_TARGETS = [S.H, _G, _R, S.H, _R, S.H, S.H, 0.0, _R, S.H, _G, S.H, _R, S.H]  # crosses 1 in both directions


@pytest.mark.parametrize("tdt", ["f64", "f32"], ids=["t64", "t32"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [5, 4099, 65536, 65536 + 8])
def test_fused_launch_state_machine(be, dbl, dev, dtype, n, tdt):
    """`xde_error_norm_control` with NORM_LINF (an exact max: bit-comparable on the one-workgroup path, n <= 65536, and on the ticketed
    path) against `dbl.error_norm_control`, 14 attempts in REVERSE time with `step_t`, fp64 and fp32 time, every field and the stage times after every
    attempt.  One operand is rescaled per attempt so that the error ratio lands in the scripted pow-free range (HOLD / GROW / SHRINK /
    exactly 0) whatever `dt` has become; attempt 3 is launched with `y1` one element off a 16-byte boundary."""
    dt = DT[dtype]
    g = torch.Generator().manual_seed(5)
    y0 = torch.randn(n, generator=g, dtype=dt)
    y1 = y0 + 1e-3 * torch.randn(n, generator=g, dtype=dt)
    k0, k1 = torch.randn(n, generator=g, dtype=dt), torch.randn(n, generator=g, dtype=dt)
    c_err = [1.2e-3, -7.5e-3]
    segs = _hip.make_segments([(0, n)])
    step_t = torch.tensor([0.5, 0.0, -1 / 128, -1 / 16, -3.0], dtype=torch.float64)
    p = _mid_solve_params(dtype, _hip.NORM_LINF, [n], tdt=tdt, direction=-1, n_step_t=len(step_t))
    ts = torch.tensor([0.0, -1 / 16, -1 / 16, -1e6], dtype=torch.float64)
    ts_d, st_d = ts.to(dev), step_t.to(dev)
    cg, cd = be.new_ctrl(dev), dbl.new_ctrl(None)
    sg = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
    sd = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt)
    ws = be.new_workspace(dev)
    be.ctrl_init(cg, p, 0.0, -1 / 64, 4, ts_d, st_d, sg)
    dbl.ctrl_init(cd, p, 0.0, -1 / 64, 4, ts, step_t, sd)
    seq0 = block_of(cg).seq
    assert_blocks_equal(block_of(cg), dbl.ctrl_read(cd), (dtype, tdt, n, "init"), seq0)
    y0_d, k1_d = y0.to(dev), k1.to(dev)
    clipped = 0
    for i, target in enumerate(FUSED_TARGETS):
        # the ratio k0 -> k0 * scale gives, measured with the double on a scratch copy of its block
        probe = cd.clone()
        dbl.error_norm_partial([k0, k1 * 0], c_err, y0, y1, p.rtol, p.atol, segs, _hip.NORM_LINF, None, ctrl=probe)
        base = dbl._slots[0][0][0]
        ka = k0 * (target / base) if target else k0 * 0
        kb = k1 * 0
        y1_d = y1.to(dev)
        if i == 3:
            buf = torch.empty(n + 1, dtype=dt, device=dev)
            y1_d = buf[1:]
            y1_d.copy_(y1)
            assert y1_d.data_ptr() % 16 != 0
        be.error_norm_control([ka.to(dev), kb.to(dev)], c_err, y0_d, y1_d, segs, ws, cg, p, ts_d, st_d, sg)
        dbl.error_norm_control([ka, kb], c_err, y0, y1, segs, None, cd, p, ts, step_t, sd)
        read = be.ctrl_read(cg)
        got, want = block_of(cg), dbl.ctrl_read(cd)
        tag = (dtype, tdt, n, i, target)
        assert bytes(read) == bytes(got), tag
        assert_blocks_equal(got, want, tag, seq0)
        assert sg.cpu().numpy().tobytes() == sd.numpy().tobytes(), tag
        clipped += got.on_step_t
        if target:
            assert abs(got.ratio / target - 1) < 1e-3, tag + (got.ratio,)
    # (a rejected clipped step, an accepted one that lands on the two rows at -1/16, the index moved on to the last entry)
    assert clipped >= 2 and got.n_accept >= 5 and got.n_reject >= 4 and (got.next_out, got.next_step_index) == (3, 4), fields(got)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) block construction
# ------------------------------------------------------------------------------------------------------------------------------
def _init_cases():
    """(name, time dtype, direction, t_start, first_step, t_span, step_t, replay, first_step_dev, keep_seq, expectations)"""
    nan = float("nan")
    return [
        ("plain", "f64", 1, 0.0, 1 / 16, [0.0, 1.0], None, None, None, False, dict(next_out=1, done=0, on_step_t=0, dt=1 / 16)),
        ("rows equal to t_start", "f32", 1, 0.5, 1 / 16, [0.5, 0.5, 0.5, 1.0], None, None, None, False, dict(next_out=3, out_begin=3, out_end=3, done=0)),
        ("all rows equal to t_start", "f64", 1, 0.5, 1 / 16, [0.5, 0.5, 0.5], None, None, None, False, dict(next_out=3, done=1, status=0)),
        ("reverse time", "f64", -1, 1.0, -1 / 16, [1.0, 1.0, 0.0], None, None, None, False, dict(next_out=2, done=0, t_plan=1.0 - 1 / 16)),
        ("step_t entries at or before t_start", "f32", 1, 0.25, 1 / 16, [0.25, 1.0], [0.0, 0.125, 0.25, 0.5, 0.75], None, None, False,
         dict(next_step_index=3, on_step_t=0)),
        ("every step_t entry at or before t_start", "f64", 1, 0.25, 1 / 16, [0.25, 1.0], [0.0, 0.125, 0.25], None, None, False,
         dict(next_step_index=2, on_step_t=0)),
        ("first step clipped by step_t", "f64", 1, 0.0, 1 / 16, [0.0, 1.0], [0.0, 1 / 64, 0.5], None, None, False,
         dict(next_step_index=1, on_step_t=1, dt=1 / 64, t_plan=1 / 64)),
        ("first step clipped, reverse", "f32", -1, 0.0, -1 / 16, [0.0, -1.0], [0.5, 0.0, -1 / 64, -0.5], None, None, False,
         dict(next_step_index=2, on_step_t=1, dt=-1 / 64, t_plan=-1 / 64)),
        ("first dt from the replay table", "f64", 1, 0.0, 1 / 16, [0.0, 1.0], None, [1 / 128, 1.0, 1 / 4, 0.0], None, False, dict(dt=1 / 128, t_plan=1 / 128)),
        ("first_step_dev, negative magnitude, forward", "f64", 1, 0.0, 99.0, [0.0, 1.0], None, None, -1 / 32, False, dict(dt=1 / 32)),
        ("first_step_dev, negative magnitude, reverse", "f64", -1, 0.0, 99.0, [0.0, -1.0], None, None, -1 / 32, False, dict(dt=-1 / 32)),
        ("t_start = nan", "f64", 1, nan, 1 / 16, [0.375, 0.375, 1.0], None, None, None, False, dict(t0=0.375, t1=0.375, next_out=2)),
        ("keep_seq", "f64", 1, 0.0, 1 / 16, [0.0, 1.0], None, None, None, True, dict(seq=41, dt=1 / 16)),
        ("first step underflows", "f32", 1, 1.0, 1e-9, [1.0, 2.0], None, None, None, False, dict(status=_hip.STATUS_DT_UNDERFLOW)),
        ("max_num_steps = 0", "f64", 1, 0.0, 1 / 16, [0.0, 1.0], None, None, None, False, dict(status=_hip.STATUS_MAX_STEPS)),
    ]


@pytest.mark.parametrize("mirrored", [False, True], ids=["bare", "mirror"])
def test_ctrl_init_field_by_field(be, dbl, dev, mirrored):
    """`xde_ctrl_init` against the double, every field and the stage times, over the table above; the double's answers for the fields
    each case is about are stated once more without it.  The block starts from garbage: init must leave no field of the old block."""
    for name, tdt, direction, t_start, first, t_span, step_t, replay, first_dev, keep_seq, expect in _init_cases():
        for sdt in ("f32", "f64"):
            p = _mid_solve_params(sdt, _hip.NORM_LINF, [1], tdt=tdt, direction=direction, n_step_t=0 if step_t is None else len(step_t))
            if name == "max_num_steps = 0":
                p.max_num_steps = 0
            ts = torch.tensor(t_span, dtype=torch.float64)
            st = None if step_t is None else torch.tensor(step_t, dtype=torch.float64)
            pg, pd, keep = p, p, None
            if replay is not None:
                pg, pd = _mid_solve_params(sdt, _hip.NORM_LINF, [1], tdt=tdt), _mid_solve_params(sdt, _hip.NORM_LINF, [1], tdt=tdt)
                keep = (torch.tensor(replay, dtype=torch.float64, device=dev), (C.c_double * len(replay))(*replay))
                pg.replay, pg.n_replay = keep[0].data_ptr(), len(replay) // 2
                pd.replay, pd.n_replay = C.addressof(keep[1]), len(replay) // 2
            old = _hip.XdeCtrl()
            C.memset(C.addressof(old), 0x5A, C.sizeof(old))
            old.seq = 41
            cg = be.new_ctrl(dev) if mirrored else torch.zeros(C.sizeof(old), dtype=torch.uint8, device=dev)
            cg.copy_(torch.frombuffer(bytearray(bytes(old)), dtype=torch.uint8))
            cd = torch.frombuffer(bytearray(bytes(old)), dtype=torch.uint8)
            sg = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=DT[sdt], device=dev)
            sd = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=DT[sdt])
            fd_h = None if first_dev is None else torch.tensor([first_dev], dtype=torch.float64)
            be.ctrl_init(cg, pg, t_start, first, len(t_span), ts.to(dev), None if st is None else st.to(dev), sg,
                         first_step_dev=None if fd_h is None else fd_h.to(dev), keep_seq=keep_seq)
            dbl.ctrl_init(cd, pd, t_start, first, len(t_span), ts, st, sd, first_step_dev=fd_h, keep_seq=keep_seq)
            got, want = block_of(cg), dbl.ctrl_read(cd)
            tag = (name, tdt, sdt, mirrored)
            seq0 = 0 if keep_seq else (be._mirrors[cg.data_ptr()].seq0 if mirrored else 0)
            assert_blocks_equal(got, want, tag, seq0)
            assert got.chk == 0 and tuple(got.reserved) == (0, 0), tag  # (init publishes nothing: the block is zeroed first)
            assert sg.cpu().numpy().tobytes() == sd.numpy().tobytes(), tag
            assert (sg.cpu().numpy()[6:] == SENTINEL).all(), tag
            fg = fields(got)
            fg["seq"] -= seq0
            for f, v in expect.items():
                want_v = float(NPT[tdt](v)) if isinstance(v, float) else v
                assert fg[f] == want_v, tag + (f, fg[f], want_v)
            assert (got.n_steps, got.n_accept, got.n_reject, got.accept, got.ratio_prev, got.n_out) == (0, 0, 0, 0, 1e-4, len(t_span)), tag
            assert bytes(be.ctrl_read(cg)) == bytes(got), tag


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("which", ["fused", "tail"])
def test_initial_step_phase_1_constructs_the_block_ctrl_init_constructs(be, dev, dtype, which):
    """Phase 1 of `initial_step_fused` / `initial_step_tail` leaves the block (and stage times) that `ctrl_init(first_step_dev =
    hs[3:4])` leaves on the same inputs: repeated rows at the start, `step_t` with entries at or before the start and one inside the
    first step, forward and reverse time."""
    dt = DT[dtype]
    n = 1000
    g = torch.Generator().manual_seed(3)
    y0, f0, f1 = (torch.randn(n, generator=g, dtype=dt).to(dev) for _ in range(3))
    segs = _hip.make_segments([(0, n)])
    for direction in (1, -1):
        for tdt in ("f32", "f64"):
            d = float(direction)
            ts = torch.tensor([0.0, 0.0, d * 0.5, d * 1.0], dtype=torch.float64, device=dev)
            st = torch.tensor([-d * 0.5, 0.0, d * 1e-7, d * 0.75], dtype=torch.float64, device=dev)
            p = _mid_solve_params(dtype, _hip.NORM_RMS, [n], tdt=tdt, direction=direction, n_step_t=4)
            hs = torch.zeros(8, dtype=torch.float64, device=dev)
            probe = torch.zeros(1, dtype=dt, device=dev)
            ws = be.new_workspace(dev)
            ca = torch.zeros(C.sizeof(_hip.XdeCtrl), dtype=torch.uint8, device=dev)
            sa = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
            if which == "fused":
                be.initial_step_fused(0, f0, None, y0, segs, hs, p, 0.0, probe, ca)
                be.initial_step_fused(1, f1, f0, y0, segs, hs, p, 0.0, None, ca, n_out=4, t_span_dev=ts, step_t_dev=st, t_stage=sa)
            else:
                be.scaled_norm2_partial(f0, y0, p.rtol, p.atol, segs, _hip.NORM_RMS, ws)
                be.initial_step_tail(0, ws, hs, p, 0.0, probe, ca)
                be.scaled_norm_partial(f1, f0, y0, p.rtol, p.atol, segs, _hip.NORM_RMS, ws, 0)
                be.initial_step_tail(1, ws, hs, p, 0.0, None, ca, n_out=4, t_span_dev=ts, step_t_dev=st, t_stage=sa)
            cb = torch.zeros(C.sizeof(_hip.XdeCtrl), dtype=torch.uint8, device=dev)
            sb = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
            be.ctrl_init(cb, p, 0.0, 0.0, 4, ts, st, sb, first_step_dev=hs[3:4])
            ga, gb = block_of(ca), block_of(cb)
            tag = (which, dtype, tdt, direction)
            assert bytes(ga) == bytes(gb), tag + (fields(ga), fields(gb))
            assert sa.cpu().numpy().tobytes() == sb.cpu().numpy().tobytes(), tag
            first = hs.cpu()[3].item()
            assert first > 1e-7 and (ga.next_out, ga.next_step_index, ga.on_step_t) == (2, 2, 1), tag + (first, fields(ga))
            assert ga.dt == float(NPT[tdt](d * 1e-7)) - 0.0 and ga.t_plan == float(NPT[tdt](d * 1e-7)), tag
