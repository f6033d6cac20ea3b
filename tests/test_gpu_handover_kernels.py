"""GPU parity, kernel level, for the kernels around an accepted step that tests/test_gpu_kernels.py does not hold directly:
`xde_scale_fanout`, `xde_commit`, `xde_dense_commit`, `xde_dense_eval` beyond four rows / at 1 and 9-14 operands, `xde_ctrl_retarget`
and `xde_error_ratio` — each against the numpy statement of its contract (tests/_cpu_double.py, the kernels' op order).

Element-wise results are BIT-EXACT.  Sizes cover the empty launch, less than one 16-byte vector, vector tails, one workgroup, several
passes; every kernel is also launched once with one operand a single element off a 16-byte boundary (the scalar kernels).  Buffers a
launch must not touch hold a sentinel and are compared afterwards; operands a launch both reads and writes (`y0`, `f0 = k[0]` of the
fused commit) are checked against copies taken before it.

Mutation check (one change at a time in a scratch build, each caught by assertion): the fan-out tail multiplying `g` by the factor
before `dt` — test_scale_fanout_bit_exact at n = 1, 3, 257, 4101 with `dt_dev`; the fused commit storing `y1` over `y0` before `y0`
is loaded — the rows of both dense-commit tests; `<=` -> `<` in the retarget row scan — "a time equal to t1"; the ratio kernel's
non-finite test reading `y0` whatever the select — the count under "select, accept 1"."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from ._cpu_double import NumpyDoubleBackend

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
NPT = {"f32": np.float32, "f64": np.float64}
SIZES = [0, 1, 3, 257, 4096 + 5, 1 << 20]
SENTINEL = -777.0


@pytest.fixture(scope="module")
def be():
    return _hip.get_backend()


@pytest.fixture(scope="module")
def dbl():
    return NumpyDoubleBackend()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _rand(n, dtype, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _up(x, dev, misaligned=False):
    """`x` on the device; `misaligned`: as a view one element into a larger buffer (not 16-byte aligned)."""
    if not misaligned:
        return x.to(dev, copy=True)
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
    view = buf[1:]
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    return view


def _ctrl_pair(ch, dev):
    raw = bytes(ch)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev), torch.frombuffer(bytearray(raw), dtype=torch.uint8)


def _same(a, b):
    """Same values element for element, NaN equal to NaN (an element-wise kernel must reproduce those too)."""
    return a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------
# xde_scale_fanout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_scale_fanout_bit_exact(be, dbl, dev, dtype, n):
    """outs[j] = g * (T(factor_j) * dt): 1, 2, 7 and 15 outputs, `dt_dev` absent and a device scalar, factors of mixed signs; then `g`
    or one output misaligned.  The factor is formed BEFORE it meets g (one rounding of the product, then one of the scaling)."""
    dt = DT[dtype]
    g = _rand(n, dt, 1)
    factors_all = [0.3, -1.7, 2.0 / 3.0, -1e-3, 5.5, -0.125, 1.0, -1.0 / 7.0, 3.1, -2.9, 0.77, -0.01, 9.0, -4.4, 1e-2]
    dt_val = torch.tensor([0.0371 / 3.0], dtype=torch.float64)
    for nout in (1, 2, 7, 15):
        for use_dt in (False, True):
            for mis in ((None,) if n == 0 else (None, "g", nout - 1)):
                if mis is not None and not (nout == 7 or (nout == 1 and use_dt)):
                    continue
                gd = _up(g, dev, misaligned=mis == "g")
                outs = [_up(torch.full((n,), SENTINEL, dtype=dt), dev, misaligned=mis == j) for j in range(nout)]
                refs = [torch.full((n,), SENTINEL, dtype=dt) for _ in range(nout)]
                be.scale_fanout(outs, gd, factors_all[:nout], dt_dev=dt_val.to(dev) if use_dt else None)
                dbl.scale_fanout(refs, g, factors_all[:nout], dt_dev=dt_val if use_dt else None)
                torch.cuda.synchronize()
                for j in range(nout):
                    assert torch.equal(outs[j].cpu(), refs[j]), (dtype, n, nout, use_dt, mis, j)
                assert torch.equal(gd.cpu(), g)


# ------------------------------------------------------------------------------------------------------------------------------
# xde_commit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_commit_is_predicated_on_accept(be, dbl, dev, dtype, n):
    """(y0, f0) <- (y1, f1) when `ctrl.accept`, nothing otherwise: destinations equal the sources (accept) or keep their sentinel
    (no accept); the sources are unchanged; aligned, and with each of the four operands misaligned in turn."""
    dt = DT[dtype]
    y1, f1 = _rand(n, dt, 2), _rand(n, dt, 3)
    for accept in (0, 1):
        ch = _hip.XdeCtrl()
        ch.accept = accept
        cd, cc = _ctrl_pair(ch, dev)
        for mis in ((None,) if n == 0 else (None, 0, 1, 2, 3)):
            y0d = _up(torch.full((n,), SENTINEL, dtype=dt), dev, misaligned=mis == 0)
            y1d = _up(y1, dev, misaligned=mis == 1)
            f0d = _up(torch.full((n,), SENTINEL, dtype=dt), dev, misaligned=mis == 2)
            f1d = _up(f1, dev, misaligned=mis == 3)
            be.commit(cd, y0d, y1d, f0d, f1d)
            y0r, f0r = torch.full((n,), SENTINEL, dtype=dt), torch.full((n,), SENTINEL, dtype=dt)
            dbl.commit(cc, y0r, y1, f0r, f1)
            torch.cuda.synchronize()
            assert torch.equal(y0d.cpu(), y0r) and torch.equal(f0d.cpu(), f0r), (dtype, n, accept, mis)
            want = (y1, f1) if accept else (torch.full((n,), SENTINEL, dtype=dt),) * 2
            assert torch.equal(y0d.cpu(), want[0]) and torch.equal(f0d.cpu(), want[1]), (dtype, n, accept, mis)
            assert torch.equal(y1d.cpu(), y1) and torch.equal(f1d.cpu(), f1)


# ------------------------------------------------------------------------------------------------------------------------------
# xde_dense_eval / xde_dense_commit
# ------------------------------------------------------------------------------------------------------------------------------
def _step(tdtype, direction, rows, seed):
    """One accepted step [t0, t1] in the time dtype with `rows` output times inside it, framed by one time before and one after."""
    TT = NPT[tdtype]
    rng = np.random.RandomState(seed)
    t0 = TT(rng.uniform(-1, 1))
    t1 = TT(t0 + direction * TT(rng.uniform(0.05, 0.5)))
    inner = np.sort(rng.uniform(0.0, 1.0, size=rows))
    if rows:
        inner[-1] = 1.0  # the last row at t1 itself
    t_out = [float(TT(t0 + (t1 - t0) * TT(x))) for x in inner]
    t_span = torch.tensor([float(t0) - direction] + t_out + [float(t1) + direction], dtype=torch.float64)
    ch = _hip.XdeCtrl()
    ch.t0, ch.t1, ch.dt_last = float(t0), float(t1), float(TT(t1 - t0))
    ch.accept, ch.out_begin, ch.out_end = 1, 1, 1 + rows
    ch.n_steps = 7
    return ch, t_span


def _dense_commit_case(be, dbl, dev, dtype, tdtype, n, nk, rows, direction, accept, f1_is_last_k, mis, seed):
    dt = DT[dtype]
    ch, t_span = _step(tdtype, direction, rows, seed)
    ch.accept = accept
    cd, cc = _ctrl_pair(ch, dev)
    y0, y1 = _rand(n, dt, seed + 1), _rand(n, dt, seed + 2)
    ks = [_rand(n, dt, seed + 10 + j) for j in range(nk)]
    f1 = ks[-1] if (f1_is_last_k and nk > 1) else _rand(n, dt, seed + 3)
    mid = list(np.linspace(-0.21, 0.37, nk))
    tag = (dtype, tdtype, n, nk, rows, direction, accept, f1_is_last_k, mis)
    # device operands (the launch writes y0 and ks[0] in place)
    y0d, y1d = _up(y0, dev, misaligned=mis == "y0"), _up(y1, dev, misaligned=mis == "y1")
    ksd = [_up(k, dev) for k in ks]
    f1d = ksd[-1] if f1 is ks[-1] else _up(f1, dev)
    out = torch.full((rows + 2, n), SENTINEL, dtype=dt, device=dev)
    be.dense_commit(out, ksd, mid, y0d, y1d, f1d, cd, t_span.to(dev), _hip.dtype_code(DT[tdtype]))
    # the double, on copies
    y0r, ksr = y0.clone(), [k.clone() for k in ks]
    f1r = ksr[-1] if f1 is ks[-1] else f1.clone()
    ref = torch.full((rows + 2, n), SENTINEL, dtype=dt)
    dbl.dense_commit(ref, ksr, mid, y0r, y1.clone(), f1r, cc, t_span, _hip.dtype_code(DT[tdtype]))
    torch.cuda.synchronize()
    got = out.cpu()
    # (1) covered rows equal dense_eval's, (2) every other row keeps its sentinel
    assert torch.equal(got, ref), tag
    lo, hi = (1, 1 + rows) if accept else (1, 1)
    untouched = torch.cat([got[:lo], got[hi:]])
    assert (untouched == SENTINEL).all(), tag
    if accept and rows and n:
        assert not (got[lo:hi] == SENTINEL).any(), tag
        plain = torch.full((rows + 2, n), SENTINEL, dtype=dt)
        dbl.dense_eval(plain, ks, mid, y0, y1, f1, cc, t_span, _hip.dtype_code(DT[tdtype]))
        assert torch.equal(got, plain), tag
    # (3) the hand-over: y0 <- y1, ks[0] <- f1 exactly (from the values BEFORE the launch); nothing else is touched
    assert torch.equal(y0d.cpu(), y1 if accept else y0), tag
    assert torch.equal(ksd[0].cpu(), f1 if accept else ks[0]), tag
    assert torch.equal(y0d.cpu(), y0r) and torch.equal(ksd[0].cpu(), ksr[0]), tag
    for j in range(1, nk):
        assert torch.equal(ksd[j].cpu(), ks[j]), tag + (j,)
    assert torch.equal(y1d.cpu(), y1) and torch.equal(f1d.cpu(), f1), tag


@pytest.mark.parametrize("tdtype", ["f32", "f64"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_dense_commit_rows_operands_and_hand_over(be, dbl, dev, dtype, tdtype):
    """`xde_dense_commit`: rows covered by the step 0 (the hand-over-only branch), 1, 4, 5, 9 (past the four precomputed fractions);
    nk = 1, 2, 6, 7 (compile-time counts), 8, 13 (the generic loop); forward and reverse time; n % width != 0 (scalar kernel) and == 0
    (vector kernel); no accept (nothing happens); `f1` the last stage (as the solvers pass it) and a tensor of its own."""
    seed = 100
    for nk in (1, 2, 6, 7, 8, 13):
        for rows in (0, 1, 4, 5, 9):
            for direction in (1, -1):
                for n in (1031, 1032):
                    seed += 1
                    _dense_commit_case(be, dbl, dev, dtype, tdtype, n, nk, rows, direction, 1, (seed % 2) == 0, None, seed)
        for rows in (0, 4):
            seed += 1
            _dense_commit_case(be, dbl, dev, dtype, tdtype, 1032, nk, rows, 1, 0, True, None, seed)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_dense_commit_sizes_and_misalignment(be, dbl, dev, dtype, n):
    """The size sweep (n = 4101 and 257 are no multiples of the vector width: the launcher takes the scalar kernel; 1 << 20 makes
    several passes of the 512-workgroup grid) with and without output rows, accept 0 / 1, then `y0` or `y1` misaligned."""
    for rows in (0, 2):
        for accept in (0, 1):
            _dense_commit_case(be, dbl, dev, dtype, dtype, n, 6, rows, 1, accept, True, None, 900 + rows + accept)
    if n:
        for mis in ("y0", "y1"):
            _dense_commit_case(be, dbl, dev, dtype, "f64", n, 6, 2, -1, 1, True, mis, 950)


@pytest.mark.parametrize("tdtype", ["f32", "f64"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_dense_eval_many_rows_and_operand_counts(be, dbl, dev, dtype, tdtype):
    """`xde_dense_eval` where the seeded sweep of test_gpu_kernels.py does not go: 5 and 9 rows inside one step (rows past the four
    precomputed fractions recompute `x` per row), nk = 1, and the generic loop at nk = 9, 13, 14; with and without the operand select
    (`sel_used` 0 and 1); vector and scalar kernels (n = 1031, and n = 1032 with `y1` misaligned); rows outside the step keep their
    sentinel; no operand is written."""
    dt = DT[dtype]
    seed = 300
    for nk in (1, 9, 13, 14):
        for rows in (0, 1, 4, 5, 9):
            for select in (None, 0, 1):
                for n in (1031, 1032):
                    seed += 1
                    direction = 1 if seed % 3 else -1
                    ch, t_span = _step(tdtype, direction, rows, seed)
                    ch.sel_used = int(bool(select))
                    cd, cc = _ctrl_pair(ch, dev)
                    y0, y1, f1 = _rand(n, dt, seed + 1), _rand(n, dt, seed + 2), _rand(n, dt, seed + 3)
                    ks = [_rand(n, dt, seed + 10 + j) for j in range(nk)]
                    y0b, k0b = (None, None) if select is None else (_rand(n, dt, seed + 4), _rand(n, dt, seed + 5))
                    mid = list(np.linspace(-0.21, 0.37, nk))
                    ops = [y0, y1, f1] + ks + ([] if select is None else [y0b, k0b])
                    opd = [_up(x, dev, misaligned=(i == 1 and rows == 5 and n == 1032 and select is None)) for i, x in enumerate(ops)]
                    y0d, y1d, f1d, ksd = opd[0], opd[1], opd[2], opd[3 : 3 + nk]
                    y0bd, k0bd = (None, None) if select is None else (opd[-2], opd[-1])
                    out = torch.full((rows + 2, n), SENTINEL, dtype=dt, device=dev)
                    ref = torch.full((rows + 2, n), SENTINEL, dtype=dt)
                    be.dense_eval(out, ksd, mid, y0d, y1d, f1d, cd, t_span.to(dev), _hip.dtype_code(DT[tdtype]), y0_alt=y0bd, k0_alt=k0bd)
                    dbl.dense_eval(ref, ks, mid, y0, y1, f1, cc, t_span, _hip.dtype_code(DT[tdtype]), y0_alt=y0b, k0_alt=k0b)
                    torch.cuda.synchronize()
                    tag = (dtype, tdtype, nk, rows, select, n, direction)
                    got = out.cpu()
                    assert torch.equal(got, ref), tag
                    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), tag
                    if rows:
                        assert not (got[1:-1] == SENTINEL).any(), tag
                    for a, b in zip(opd, ops):
                        assert torch.equal(a.cpu(), b), tag
                    if select is not None and rows:  # the select decides: the other operand pair gives other rows
                        other = torch.full((rows + 2, n), SENTINEL, dtype=dt)
                        ch.sel_used = 1 - ch.sel_used
                        dbl.dense_eval(other, ks, mid, y0, y1, f1, _ctrl_pair(ch, dev)[1], t_span, _hip.dtype_code(DT[tdtype]), y0_alt=y0b, k0_alt=k0b)
                        assert not torch.equal(other, ref), tag


# ------------------------------------------------------------------------------------------------------------------------------
# xde_ctrl_retarget
# ------------------------------------------------------------------------------------------------------------------------------
SET_BY_RETARGET = ("seq", "n_out", "out_begin", "out_end", "next_out", "done", "steps_in_interval", "status")
_MASK = (1 << 64) - 1


def _mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _MASK
    x ^= x >> 31
    return x


def _checksum(block):
    """The published block's `chk`: the position-salted sum over its other 8-byte words (csrc/xde_control_device.hpp)."""
    words = np.frombuffer(bytes(block), dtype=np.uint64)
    skip = _hip.XdeCtrl.chk.offset // 8
    return sum(_mix64((int(w) + 0x9E3779B97F4A7C15 * (i + 1)) & _MASK) for i, w in enumerate(words) if i != skip) & _MASK


def _busy_block():
    """A control block in the middle of a solve: every field holds a value of its own, so a field the launch should not touch shows."""
    ch = _hip.XdeCtrl()
    ch.t0, ch.t1, ch.dt, ch.dt_last, ch.t_plan = 0.125, 0.5, 0.0625, 0.375, 0.5625
    ch.ratio_prev, ch.ratio, ch.nonfinite = 0.3, 0.7, 0.0
    for i in range(_hip.XDE_MAX_SEG):
        ch.ratio_seg[i] = 0.01 * (i + 1)
    ch.n_steps, ch.n_accept, ch.n_reject, ch.steps_in_interval = 41, 29, 12, 17
    ch.accept, ch.sel_used, ch.status = 1, 1, _hip.STATUS_OK
    ch.out_begin, ch.out_end, ch.next_out, ch.n_out, ch.done = 3, 5, 5, 9, 0
    ch.next_step_index, ch.on_step_t = 2, 1
    ch.chk = 0x1234
    ch.reserved[0], ch.reserved[1] = 11, 22
    return ch


def _fields(c):
    out = {}
    for f, _t in _hip.XdeCtrl._fields_:
        v = getattr(c, f)
        out[f] = tuple(v) if isinstance(v, C.Array) else v
    return out


@pytest.mark.parametrize("mirrored", [False, True])
def test_ctrl_retarget_field_by_field(be, dbl, dev, mirrored):
    """`xde_ctrl_retarget` against the double: every field it sets (`seq`, `n_out`, `out_begin`, `out_end`, `next_out`, `done`,
    `steps_in_interval`, `status`) and every other field unchanged.  No accept; no accepted step yet; forward and reverse time; the new
    list covered not at all, partly, fully (`done == 1`); a time EXACTLY equal to t1 (covered: `<=`); status MAX_STEPS (reset to OK),
    NONFINITE and DT_UNDERFLOW (sticky).  With a host mirror, the block published for the new `seq` is the one in device memory."""
    checksummed = (int(os.environ.get("XDE_CTRL_FLAGS", "15")) & 8) != 0
    p = _hip.XdeCtrlParams()
    p.rtol, p.atol, p.safety, p.ifactor, p.dfactor, p.order = 1e-5, 1e-7, 0.9, 10.0, 0.2, 5.0
    p.max_step, p.max_num_steps, p.n_stage, p.n_seg = float("inf"), 1000, 6, 1
    p.seg_count[0] = 1.0
    # (name, direction, t1, list, edits of the busy block, expected out_end, expected done)
    cases = [
        ("not covered", 1, 0.5, [0.75, 1.0], {}, 0, 0),
        ("partly covered", 1, 0.5, [0.25, 0.4375, 0.75], {}, 2, 0),
        ("fully covered", 1, 0.5, [0.25, 0.375], {}, 2, 1),
        ("a time equal to t1", 1, 0.5, [0.25, 0.5, 0.75], {}, 2, 0),
        ("only t1 itself", 1, 0.5, [0.5], {}, 1, 1),
        ("one ulp past t1", 1, 0.5, [float(np.nextafter(0.5, 1.0))], {}, 0, 0),
        ("reverse, partly", -1, -0.5, [-0.25, -0.5, -0.75], {}, 2, 0),
        ("reverse, fully", -1, -0.5, [0.25, -0.5], {}, 2, 1),
        ("reverse, not covered", -1, -0.5, [float(np.nextafter(-0.5, -1.0)), -2.0], {}, 0, 0),
        ("rejected step", 1, 0.5, [0.25, 0.375], {"accept": 0}, 0, 0),
        ("no accepted step yet", 1, 0.5, [0.25, 0.375], {"n_accept": 0}, 0, 0),
        ("MAX_STEPS is reset", 1, 0.5, [0.75], {"status": _hip.STATUS_MAX_STEPS}, 0, 0),
        ("NONFINITE is sticky", 1, 0.5, [0.75], {"status": _hip.STATUS_NONFINITE}, 0, 0),
        ("DT_UNDERFLOW is sticky", 1, 0.5, [0.25], {"status": _hip.STATUS_DT_UNDERFLOW}, 1, 1),
    ]
    ctrl = be.new_ctrl(dev) if mirrored else None
    for name, direction, t1, times, edits, want_end, want_done in cases:
        p.direction = direction
        ch = _busy_block()
        ch.t1 = t1
        ch.t0 = t1 - direction * 0.375
        for k, v in edits.items():
            setattr(ch, k, v)
        if mirrored:
            m = be._mirrors[ctrl.data_ptr()]
            ch.seq = m.seq  # the sequence number the binding expects this block to carry
            ctrl.copy_(torch.frombuffer(bytearray(bytes(ch)), dtype=torch.uint8))
            cd, cc = ctrl, torch.frombuffer(bytearray(bytes(ch)), dtype=torch.uint8)
        else:
            ch.seq = 1000
            cd, cc = _ctrl_pair(ch, dev)
        t_span = torch.tensor(times, dtype=torch.float64)
        be.ctrl_retarget(cd, p, t_span.to(dev), len(times))
        dbl.ctrl_retarget(cc, p, t_span, len(times))
        read = be.ctrl_read(cd)  # (through the host mirror when there is one)
        torch.cuda.synchronize()
        in_memory = _hip.XdeCtrl.from_buffer_copy(cd.cpu().numpy().tobytes())
        before, got, want = _fields(ch), _fields(in_memory), _fields(dbl.ctrl_read(cc))
        for f in before:
            if f in SET_BY_RETARGET:
                assert got[f] == want[f], (name, f, got[f], want[f])
            elif f != "chk":
                assert got[f] == before[f], (name, f, "changed", before[f], got[f])
        # the double's answers, stated once more without it
        assert got["seq"] == before["seq"] + 1 and got["n_out"] == len(times) and got["out_begin"] == 0, name
        assert (got["out_end"], got["next_out"], got["done"]) == (want_end, want_end, want_done), (name, got)
        assert got["steps_in_interval"] == 0, name
        assert got["status"] == (_hip.STATUS_OK if before["status"] == _hip.STATUS_MAX_STEPS else before["status"]), name
        if checksummed:
            assert got["chk"] == _checksum(in_memory), name
        else:
            assert got["chk"] == before["chk"], name
        assert bytes(read) == bytes(in_memory), (name, "the block read back is not the block in device memory", _fields(read), got)


# ------------------------------------------------------------------------------------------------------------------------------
# xde_error_ratio
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_error_ratio_bit_exact_and_counts_nonfinite(be, dbl, dev, dtype, n):
    """out = (sum_j k_j (dt c_j)) / (atol + rtol max(|y0|, |y1|)), element-wise and therefore bit-exact; nk = 1, 5, 7; `dt` from the
    host and from the control block; with and without the operand select, each under both values of `ctrl.accept` (without `y0_alt`
    an accepted step selects nothing).  NaN / Inf planted in the SELECTED y0 at
    the first element, at a vector-tail element and in the middle (and, in other numbers, in the operand that is not selected):
    `nonfinite_out` is the count of the selected operand exactly, ADDED to what it held; then `y0` or `out` misaligned."""
    dt = DT[dtype]
    rtol, atol = 1e-3, 1e-6
    spots = sorted({0, n // 2, n - 1}) if n else []
    nan_inf = [float("nan"), float("inf"), float("-inf")]
    for nk in (1, 5, 7):
        ks = [_rand(n, dt, 20 + j) for j in range(nk)]
        c_err = list(np.linspace(1.2e-3, -7.5e-3, nk))
        y1 = _rand(n, dt, 2)
        for mode in ("host dt", "ctrl dt, accept 0", "ctrl dt, accept 1", "select, accept 0", "select, accept 1"):
            for mis in ((None,) if (n == 0 or nk != 5) else (None, "y0", "out")):
                y0, y0b, k0b = _rand(n, dt, 1), _rand(n, dt, 5), _rand(n, dt, 6)
                select = mode.startswith("select")
                accept = int(mode.endswith("1"))
                chosen, other = (y0b, y0) if (select and accept) else (y0, y0b)
                for i, s in enumerate(spots):
                    chosen[s] = nan_inf[i % 3]
                if n > 8:  # the operand NOT selected holds other non-finite elements: they must not be counted
                    other[1], other[3], other[n - 2], other[n // 3] = float("nan"), float("inf"), float("nan"), float("inf")
                ch = _hip.XdeCtrl()
                ch.dt, ch.accept = float(np.float32(0.0123)), accept
                cd, cc = _ctrl_pair(ch, dev)
                kw_g, kw_r = {}, {}
                if mode == "host dt":
                    kw_g = kw_r = {"dt_host": 0.0371}
                else:
                    kw_g, kw_r = {"ctrl": cd}, {"ctrl": cc}
                    if select:
                        kw_g = dict(kw_g, y0_alt=y0b.to(dev), k0_alt=k0b.to(dev))
                        kw_r = dict(kw_r, y0_alt=y0b, k0_alt=k0b)
                out = _up(torch.full((n,), SENTINEL, dtype=dt), dev, misaligned=mis == "out")
                ref = torch.full((n,), SENTINEL, dtype=dt)
                nf_g, nf_r = torch.tensor([3.0], dtype=torch.float64, device=dev), torch.tensor([3.0], dtype=torch.float64)
                be.error_ratio(out, [k.to(dev) for k in ks], c_err, _up(y0, dev, misaligned=mis == "y0"), y1.to(dev), rtol, atol,
                               nonfinite_out=nf_g, **kw_g)
                dbl.error_ratio(ref, ks, c_err, y0, y1, rtol, atol, nonfinite_out=nf_r, **kw_r)
                torch.cuda.synchronize()
                tag = (dtype, n, nk, mode, mis)
                assert _same(out, ref), tag
                assert nf_g.item() == nf_r.item() == 3.0 + len(spots), tag + (nf_g.item(), nf_r.item())
