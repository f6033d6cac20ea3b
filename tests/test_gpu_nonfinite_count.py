"""The error-norm pass's SECOND output: the count of non-finite elements of the attempt's y0 (the reference's
`assert isfinite(y0).all()`, base_adaptive_solver_rk.py:201), on every kernel that produces it and through every way it reaches the
controller.  For a NaN the count is redundant (the ratio is NaN too); for +-Inf it is the only guard — tol = atol + rtol * inf = inf,
e / inf = 0, the ratio stays finite — so a kernel that loses one count turns the reference's assertion into a silent wrong answer.

Reference of every count: plain numpy on the operands the test made, `count_nonzero(~isfinite(y0_selected[start : start + len]))`
per segment, EXACT.  The value of the same launch is held to tests/_cpu_double.py's `error_norm_partial`: the same NaN-ness per
segment and, where finite, the bars test_gpu_kernels.py::test_error_norm_and_control uses (2e-6 relative fp32, 1e-12 fp64).

Which kernel a case reaches is decided by the dispatch of xde_error_norm_partial (csrc/xde_norm.hip) and xde_error_norm_control
(csrc/xde_control.hip); `_kernel_for` restates those conditions and every case asserts the kernel it means to reach.  The sizes are
derived from the kernels' constants (vector width W, workgroup 256, default norm grid 512, the one-workgroup kernel's 1024 lanes);
only the default environment is tested (the library reads XDE_NORM_GRID / XDE_NT / XDE_CTRL_FLAGS once per process)."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from ._cpu_double import NumpyDoubleBackend

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
WIDTH = {"f32": 4, "f64": 2}  # elements of one 16-byte vector load
BLOCK = 256  # kBlock
NORM_GRID = 512  # norm_grid_cap(): workgroups of a norm launch
SINGLE_BLOCK = 1024  # kSingleBlock: lanes of xde_errnorm_control_single_kernel
SINGLE_MAX = 1 << 16  # largest state xde_error_norm_control serves with that kernel
WAVE = 64
NORMS = {"rms": _hip.NORM_RMS, "linf": _hip.NORM_LINF}
REL = {"f32": 2e-6, "f64": 1e-12}  # test_error_norm_and_control's / test_fused_error_norm_control_equals_two_launches' bars
RTOL, ATOL = 1e-3, 1e-5
DT0 = float(np.float32(0.01))  # a step the fp32 time arithmetic of the control block keeps exactly: the dt every launch and the reference read

# +inf, -inf, a quiet NaN, a signalling NaN (quiet bit clear, payload set): planted as BITS, so that no copy can quiet the last one
SPECIAL = {"f32": np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001], dtype=np.uint32).view(np.int32),
           "f64": np.array([0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF4000000000001], dtype=np.uint64).view(np.int64)}
# finite values that must never be counted: +-max finite, the smallest subnormal, -0.0
DECOY = {"f32": np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000000], dtype=np.uint32).view(np.int32),
         "f64": np.array([0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000000], dtype=np.uint64).view(np.int64)}


def _sizes(dtype):
    """The smallest sizes at which each structure of the kernels exists."""
    w = WIDTH[dtype]
    return {
        "one": 1,  # the scalar tail alone
        "vec_tail": w + 1,  # one vector and a tail
        "multi": w * (3 * BLOCK + 37) + (w - 1),  # several workgroups, one pass, a ragged last wave, a full tail
        # lanes 0..36 of workgroup 0 alone have a second iteration: one wave leaves the loop at two different trip counts
        "two_pass": w * (NORM_GRID * BLOCK + 37) + (w - 1),
        "single": w * (2 * SINGLE_BLOCK + 37) + (w - 1),  # the same for the 1024-lane workgroup
    }


def _kernel_for(entry, nk, e_pre, aligned, ctrl, total, dtype):
    """The dispatch conditions of xde_error_norm_partial / xde_error_norm_control in the default environment (k0_alt never comes
    with e_pre, and no operand here reaches the 64 MiB of `big_operand`)."""
    assert total * (4 if dtype == "f32" else 8) < (64 << 20)
    body = "errnorm_body<PRE>" if e_pre else ("errnorm_body<NK>" if nk <= 8 else ("errnorm_body<NK>" if aligned else "errnorm_generic"))
    how = "vec" if aligned else "scalar"
    if entry == "fused":
        return ("xde_errnorm_control_single_kernel" if total <= SINGLE_MAX else "xde_errnorm_control_kernel", how, body)
    if aligned and e_pre and nk == 1 and ctrl:
        return ("xde_errnorm_pre_kernel", "vec", "errnorm_pre_body")
    if aligned and nk > 8 and not e_pre:
        return ("xde_errnorm_wide_kernel", "vec", body)
    return ("xde_errnorm_kernel", how, body)


@pytest.fixture(scope="module")
def be():
    return _hip.get_backend()


@pytest.fixture(scope="module")
def dbl():
    return NumpyDoubleBackend()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class _Operands:
    """The operands of one error-norm launch on the device, each with a host twin that shares no memory with it; plants go into
    both, as bit patterns, and are taken back by `restore`.  `aligned=False`: every operand is a `[1:]` view (4 / 8 bytes off a
    16-byte boundary)."""

    def __init__(self, dev, dtype, total, nk, *, e_pre=False, alt=False, aligned=True):
        self.dtype, self.total, self.nk, self.alt, self.dev = dtype, total, nk, alt, dev
        self.itype = np.int32 if dtype == "f32" else np.int64
        self.tint = torch.int32 if dtype == "f32" else torch.int64
        self.host, self.d = {}, {}
        off = 0 if aligned else 1
        names = ["y0", "y1"] + ["k{}".format(j) for j in range(nk)] + (["e_pre"] if e_pre else []) + (
            ["y0_alt"] + ([] if e_pre else ["k0_alt"]) if alt else [])
        for i, name in enumerate(names):
            buf = torch.randn(total + off, generator=torch.Generator().manual_seed(100 + i), dtype=DT[dtype])
            if name == "y1":  # (computed once, on the host: both sides hold the same bits)
                buf[off:] = self.host["y0"] + 1e-3 * buf[off:]
            elif name == "e_pre":
                buf.mul_(1e-3)
            self.host[name] = buf[off:]
            self.d[name] = buf.to(dev)[off:]
        assert all((t.data_ptr() % 16 == 0) == aligned for t in self.d.values())
        # (tableau-sized coefficients: the estimate is ~1e-3 of the state, the ratio O(1))
        self.c_err = [float(c) for c in np.linspace(-7.5e-2, 9.1e-2, nk)]
        self._undo = []

    def ks(self, side):
        return [side["k{}".format(j)] for j in range(self.nk)]

    def plant(self, name, idx, bits):
        idx = np.unique(np.asarray(idx, dtype=np.int64))
        bits = np.resize(np.asarray(bits, dtype=self.itype), idx.shape)
        h = self.host[name].numpy().view(self.itype)
        self._undo.append((name, idx, h[idx].copy()))
        self._write(name, idx, bits)

    def _write(self, name, idx, bits):
        self.host[name].numpy().view(self.itype)[idx] = bits
        self.d[name].view(self.tint)[torch.from_numpy(idx).to(self.dev)] = torch.from_numpy(bits).to(self.dev)

    def restore(self):
        for name, idx, old in reversed(self._undo):
            self._write(name, idx, old)
        self._undo = []


def _params(dtype, norm, lens):
    p = _hip.XdeCtrlParams()
    p.rtol, p.atol, p.min_step, p.max_step = RTOL, ATOL, 0.0, float("inf")
    p.safety, p.ifactor, p.dfactor, p.order = 0.9, 10.0, 0.2, 5.0
    p.max_num_steps = 2**31 - 1
    p.time_dtype = _hip.XDE_F32
    p.state_dtype = _hip.dtype_code(DT[dtype])
    p.direction, p.norm_kind, p.n_stage, p.n_seg = 1, NORMS[norm], 6, len(lens)
    for i, a in enumerate([0.2, 0.3, 0.8, 8 / 9, 1.0, 1.0]):
        p.alpha[i] = a
    for i, l in enumerate(lens):
        p.seg_count[i] = float(l)
    return p


class _Rig:
    """One workspace, one control block and one sums buffer, the launches of a case and their reference."""

    def __init__(self, be, dbl, dev, dtype, norm, segl):
        self.be, self.dbl, self.dev, self.dtype, self.norm, self.segl = be, dbl, dev, dtype, norm, segl
        self.segs = _hip.make_segments(segl)
        self.p = _params(dtype, norm, [l for _, l in segl])
        self.ws, self.sums, self.ctrl = be.new_workspace(dev), be.new_sums(dev), be.new_ctrl(dev)
        self.ts = torch.zeros(_hip.XDE_MAX_STAGE, dtype=DT[dtype], device=dev)
        self.t_span = torch.tensor([0.0, 10.0], dtype=torch.float64, device=dev)

    def arm(self, accept=0):
        """A freshly constructed block (dt = DT0, status OK), with `accept` set the way the previous attempt's controller would."""
        self.be.ctrl_init(self.ctrl, self.p, 0.0, DT0, 2, self.t_span, None, self.ts)
        if accept:
            o = _hip.XdeCtrl.accept.offset
            self.ctrl[o : o + 4].view(torch.int32).fill_(1)

    def _alt(self, ops, e_pre):
        kw = {}
        if ops.alt:
            kw["y0_alt"] = ops.d["y0_alt"]
            if not e_pre:
                kw["k0_alt"] = ops.d["k0_alt"]
        return kw

    def partial(self, ops, ctrl):
        """xde_error_norm_partial -> xde_norm_finalize: (per-segment values, per-segment counts)."""
        e_pre = ops.d.get("e_pre")
        kw = dict(ctrl=self.ctrl, **self._alt(ops, e_pre is not None)) if ctrl else dict(dt_host=DT0)
        self.be.error_norm_partial(ops.ks(ops.d), ops.c_err, ops.d["y0"], ops.d["y1"], RTOL, ATOL, self.segs, NORMS[self.norm], self.ws,
                                   e_pre=e_pre, **kw)
        self.be.norm_finalize(self.ws, 0, self.sums)
        s = self.sums.cpu().numpy()
        n = len(self.segl)
        assert not s[n : _hip.XDE_MAX_SEG].any() and not s[_hip.XDE_MAX_SEG + n :].any()  # nothing beyond the launch's segments
        return s[:n].copy(), s[_hip.XDE_MAX_SEG : _hip.XDE_MAX_SEG + n].copy()

    def control(self):
        """xde_rk_control on the partial records the last `partial` left."""
        self.be.rk_control(self.ctrl, self.p, self.ws, None, self.t_span, None, self.ts)
        return self.be.ctrl_read(self.ctrl)

    def fused(self, ops):
        """xde_error_norm_control."""
        e_pre = ops.d.get("e_pre")
        self.be.error_norm_control(ops.ks(ops.d), ops.c_err, ops.d["y0"], ops.d["y1"], self.segs, self.ws, self.ctrl, self.p, self.t_span,
                                   None, self.ts, e_pre=e_pre, **self._alt(ops, e_pre is not None))
        return self.be.ctrl_read(self.ctrl)

    def reference(self, ops, accept=0):
        """(counts by numpy, values by the CPU double) for the y0 that `accept` selects."""
        sel = bool(ops.alt and accept)
        y0s = ops.host["y0_alt" if sel else "y0"].numpy()
        counts = np.array([np.count_nonzero(~np.isfinite(y0s[s : s + l])) for s, l in self.segl], dtype=np.float64)
        ch = _hip.XdeCtrl()
        ch.dt, ch.accept = DT0, int(accept)
        ctrl = torch.frombuffer(bytearray(bytes(ch)), dtype=torch.uint8)
        e_pre = ops.host.get("e_pre")
        kw = {}
        if ops.alt:
            kw["y0_alt"] = ops.host["y0_alt"]
            if e_pre is None:
                kw["k0_alt"] = ops.host["k0_alt"]
        with np.errstate(all="ignore"):
            self.dbl.error_norm_partial(ops.ks(ops.host), ops.c_err, ops.host["y0"], ops.host["y1"], RTOL, ATOL, self.segs, NORMS[self.norm],
                                        None, ctrl=ctrl, e_pre=e_pre, **kw)
        vals, nfs, _, _ = self.dbl._slots[0]
        assert list(nfs) == list(counts)  # (the double's count is the numpy statement)
        return counts, np.asarray(vals, dtype=np.float64)

    def seg_ratio(self, vals):
        """Per-segment norm from per-segment sums (RMS) / maxima (LINF): the quantity the value bars are stated for."""
        lens = np.array([l for _, l in self.segl], dtype=np.float64)
        with np.errstate(all="ignore"):
            return np.sqrt(vals / lens) if self.norm == "rms" else np.abs(vals)

    def check_values(self, got_ratio, want_vals, what):
        want = self.seg_ratio(want_vals)
        got = np.asarray(got_ratio, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
        fin, inf = np.isfinite(want), np.isinf(want)
        assert np.array_equal(got[inf], want[inf]), (what, got, want)
        if fin.any():
            assert got[fin] == pytest.approx(want[fin], rel=REL[self.dtype], abs=0.0), (what, got, want)

    def check(self, ops, entry, ctrl, what, accept=0):
        """One launch through `entry` against the reference: counts exact (per segment where the entry point shows them, their sum
        and the status in the block), values to the bars."""
        counts, vals = self.reference(ops, accept)
        status = _hip.STATUS_NONFINITE if counts.sum() > 0 else _hip.STATUS_OK
        if entry == "partial":
            if ctrl:
                self.arm(accept)
            gv, gn = self.partial(ops, ctrl)
            assert np.array_equal(gn, counts), (what, gn, counts)
            self.check_values(self.seg_ratio(gv), vals, what)
            if not ctrl:
                return
            c = self.control()
        else:
            self.arm(accept)
            c = self.fused(ops)
        assert c.nonfinite == counts.sum(), (what, c.nonfinite, counts)
        assert c.status == status, (what, c.status, status)
        assert c.sel_used == int(accept)
        self.check_values(list(c.ratio_seg)[: len(self.segl)], vals, what)


def _plant_sets(n, w, seed=0):
    """[(label, element indices)]: the places where a count can get lost, for a one-segment state of `n` elements."""
    nvec = n // w
    vec = lambda v: [w * v + j for j in range(w)]  # noqa: E731
    sets = [("element 0", [0])]
    if nvec:
        sets.append(("last vector-path element", [nvec * w - 1]))
        sets.append(("all W elements of one vector", vec(nvec // 2)))
    for j in range(n - nvec * w):
        sets.append(("scalar tail element {}".format(j), [nvec * w + j]))
    if n - nvec * w > 1:
        sets.append(("the whole scalar tail", list(range(nvec * w, n))))
    if nvec >= 2 * WAVE:
        sets.append(("everything one wave reads in one iteration", [e for v in range(WAVE, 2 * WAVE) for e in vec(v)]))
        sets.append(("one element in each of two waves of a workgroup", [w * 5 + 1, w * (WAVE + 5)]))
    if nvec >= 2 * BLOCK:
        sets.append(("one element in each of two workgroups", [w * 7, w * (BLOCK + 7) + w - 1]))
        sets.append(("the ragged last wave", [w * (nvec - 1)]))
    if nvec > NORM_GRID * BLOCK:  # second iterations of workgroup 0's first wave, its lanes without one, and the next wave
        for v in (NORM_GRID * BLOCK, NORM_GRID * BLOCK + 36, 37, 63, 64):
            sets.append(("vector {}".format(v), [w * v + v % w]))
        sets.append(("both trip counts of one wave", [w * v + v % w for v in (NORM_GRID * BLOCK, NORM_GRID * BLOCK + 36, 37, 63, 64)]))
    if nvec > SINGLE_BLOCK:
        sets.append(("second iteration of the 1024-lane workgroup", [w * SINGLE_BLOCK, w * (SINGLE_BLOCK + 36) + 1, w * 37]))
    if n >= 100:
        rng = np.random.default_rng(seed)
        sets.append(("a random 1 % mask", list(np.flatnonzero(rng.random(n) < 0.01))))
    sets.append(("several together", sorted({e for _, s in sets[: -1 if n >= 100 else None] for e in s})))
    return sets


# id -> (entry point, nk, e_pre, aligned, ctrl, alt, sizes, the kernel it reaches)
_P = ("one", "vec_tail", "multi", "two_pass")
PATHS = {
    "vec-nk1": ("partial", 1, False, True, False, False, _P, ("xde_errnorm_kernel", "vec", "errnorm_body<NK>")),
    "vec-nk3-ctrl": ("partial", 3, False, True, True, False, _P, ("xde_errnorm_kernel", "vec", "errnorm_body<NK>")),
    "vec-nk8-ctrl-alt": ("partial", 8, False, True, True, True, _P, ("xde_errnorm_kernel", "vec", "errnorm_body<NK>")),
    "scalar-nk3": ("partial", 3, False, False, False, False, _P, ("xde_errnorm_kernel", "scalar", "errnorm_body<NK>")),
    "scalar-nk1-ctrl-alt": ("partial", 1, False, False, True, True, _P, ("xde_errnorm_kernel", "scalar", "errnorm_body<NK>")),
    "pre-body": ("partial", 1, True, True, False, False, _P, ("xde_errnorm_kernel", "vec", "errnorm_body<PRE>")),
    "pre-body-scalar-ctrl": ("partial", 1, True, False, True, False, _P, ("xde_errnorm_kernel", "scalar", "errnorm_body<PRE>")),
    "pre-kernel": ("partial", 1, True, True, True, False, _P, ("xde_errnorm_pre_kernel", "vec", "errnorm_pre_body")),
    "pre-kernel-alt": ("partial", 1, True, True, True, True, _P, ("xde_errnorm_pre_kernel", "vec", "errnorm_pre_body")),
    "wide-nk9": ("partial", 9, False, True, False, False, _P, ("xde_errnorm_wide_kernel", "vec", "errnorm_body<NK>")),
    "wide-nk11-ctrl": ("partial", 11, False, True, True, False, _P, ("xde_errnorm_wide_kernel", "vec", "errnorm_body<NK>")),
    "wide-nk14": ("partial", 14, False, True, False, False, _P, ("xde_errnorm_wide_kernel", "vec", "errnorm_body<NK>")),
    "generic-nk11": ("partial", 11, False, False, False, False, _P, ("xde_errnorm_kernel", "scalar", "errnorm_generic")),
    "ticketed-vec": ("fused", 3, False, True, True, False, ("two_pass",), ("xde_errnorm_control_kernel", "vec", "errnorm_body<NK>")),
    "ticketed-scalar": ("fused", 3, False, False, True, False, ("two_pass",), ("xde_errnorm_control_kernel", "scalar", "errnorm_body<NK>")),
    "ticketed-vec-pre": ("fused", 1, True, True, True, True, ("two_pass",), ("xde_errnorm_control_kernel", "vec", "errnorm_body<PRE>")),
    "ticketed-scalar-pre": ("fused", 1, True, False, True, False, ("two_pass",), ("xde_errnorm_control_kernel", "scalar", "errnorm_body<PRE>")),
    "single-vec": ("fused", 3, False, True, True, False, ("one", "vec_tail", "multi", "single"),
                   ("xde_errnorm_control_single_kernel", "vec", "errnorm_body<NK>")),
    "single-scalar": ("fused", 3, False, False, True, False, ("one", "vec_tail", "multi", "single"),
                      ("xde_errnorm_control_single_kernel", "scalar", "errnorm_body<NK>")),
    "single-vec-pre-alt": ("fused", 1, True, True, True, True, ("one", "vec_tail", "multi", "single"),
                           ("xde_errnorm_control_single_kernel", "vec", "errnorm_body<PRE>")),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("norm", ["rms", "linf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_count_equals_numpy_on_every_path(be, dbl, dev, dtype, norm, path):
    """Every plant set alone, then several together, on every kernel and size: the per-segment count is numpy's, exactly (through
    xde_norm_finalize and, where the case has a control block, through xde_rk_control / xde_error_norm_control as `nonfinite` and
    `status`), and the launch's value keeps the double's NaN-ness and bars."""
    entry, nk, e_pre, aligned, ctrl, alt, sizes, kernel = PATHS[path]
    w = WIDTH[dtype]
    for size in sizes:
        n = _sizes(dtype)[size]
        assert _kernel_for(entry, nk, e_pre, aligned, ctrl, n, dtype) == kernel
        ops = _Operands(dev, dtype, n, nk, e_pre=e_pre, alt=alt, aligned=aligned)
        rig = _Rig(be, dbl, dev, dtype, norm, [(0, n)])
        rig.check(ops, entry, ctrl, (size, "clean"))
        for i, (label, idx) in enumerate(_plant_sets(n, w)):
            ops.plant("y0", idx, np.roll(SPECIAL[dtype], i))
            rig.check(ops, entry, ctrl, (size, label))
            ops.restore()
        rig.check(ops, entry, ctrl, (size, "clean again"))


@pytest.mark.parametrize("path", ["vec-nk3-ctrl", "scalar-nk3", "pre-kernel", "wide-nk11-ctrl", "generic-nk11", "ticketed-vec-pre", "single-vec"])
@pytest.mark.parametrize("norm", ["rms", "linf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_decoys_are_not_counted(be, dbl, dev, dtype, norm, path):
    """+-max finite, the smallest subnormal and -0.0 in y0 next to a plant count nothing; NaN / Inf in y1, in every k_j and in e_pre
    with a clean y0 change the VALUE (the double says how) and leave the count at 0."""
    entry, nk, e_pre, aligned, ctrl, alt, sizes, _ = PATHS[path]
    w = WIDTH[dtype]
    n = _sizes(dtype)[sizes[-2] if entry == "partial" else sizes[-1]]  # "multi" for the partial paths: vector path + ragged wave + tail
    ops = _Operands(dev, dtype, n, nk, e_pre=e_pre, alt=alt, aligned=aligned)
    rig = _Rig(be, dbl, dev, dtype, norm, [(0, n)])
    nvec = n // w
    spots = [0, w * (nvec // 2) + 1, w * (nvec - 1), n - 1]  # first vector, a middle one, the ragged last wave, the scalar tail
    for s in spots:
        neigh = [e for e in (s - 1, s + 1, s + 2, s - 2) if 0 <= e < n and e not in spots]
        ops.plant("y0", neigh, DECOY[dtype])
    rig.check(ops, entry, ctrl, "decoys alone")
    assert rig.reference(ops)[0].sum() == 0
    ops.plant("y0", spots, SPECIAL[dtype])
    rig.check(ops, entry, ctrl, "decoys next to plants")
    assert rig.reference(ops)[0].sum() == len(spots)
    ops.restore()
    others = ["y1"] + ["k{}".format(j) for j in range(nk)] + (["e_pre"] if e_pre else [])
    for i, name in enumerate(others):
        ops.plant(name, spots, np.roll(SPECIAL[dtype], i))
        rig.check(ops, entry, ctrl, "non-finite " + name)
        assert rig.reference(ops)[0].sum() == 0
        ops.restore()
    for name in others:
        ops.plant(name, spots, SPECIAL[dtype][2:3])
    counts, vals = rig.reference(ops)
    assert counts.sum() == 0 and np.isnan(vals).all()  # (a NaN in every other operand: the value IS NaN, the count is not touched)
    rig.check(ops, entry, ctrl, "NaN everywhere but y0")


@pytest.mark.parametrize("path", ["vec-nk8-ctrl-alt", "scalar-nk1-ctrl-alt", "pre-kernel-alt", "ticketed-vec-pre", "single-vec-pre-alt"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_count_follows_the_selected_y0(be, dbl, dev, dtype, path):
    """Speculative select: the launch counts the y0 it READS — `y0_alt` when the block says the previous attempt was accepted,
    `y0` otherwise (the pre kernel and every e_pre launch take y0_alt without a k0_alt)."""
    entry, nk, e_pre, aligned, ctrl, alt, sizes, kernel = PATHS[path]
    assert alt and ctrl
    w = WIDTH[dtype]
    n = _sizes(dtype)[sizes[-1]]
    assert _kernel_for(entry, nk, e_pre, aligned, ctrl, n, dtype) == kernel
    ops = _Operands(dev, dtype, n, nk, e_pre=e_pre, alt=alt, aligned=aligned)
    assert ("k0_alt" in ops.d) == (not e_pre)
    rig = _Rig(be, dbl, dev, dtype, "rms", [(0, n)])
    nvec = n // w
    where = {"y0": [3, w * (nvec - 1) + 1, n - 1], "y0_alt": [0, w * 37 % n, w * (nvec // 2), n - 2, n - 1]}
    for planted in (["y0"], ["y0_alt"], ["y0", "y0_alt"]):
        for name in planted:
            ops.plant(name, where[name], SPECIAL[dtype])
        for accept in (0, 1):
            counts, _ = rig.reference(ops, accept)
            read = "y0_alt" if accept else "y0"
            assert counts.sum() == (len(set(where[read])) if read in planted else 0)
            rig.check(ops, entry, ctrl, (planted, accept), accept=accept)
        ops.restore()


def _layout(lens, w):
    segl, off = [], 0
    for l in lens:
        segl.append((off, l))
        off += -(-l // w) * w
    return segl, off


# (74154 elements: above the one-workgroup kernel's reach; 11154: within it)
LENS_BIG, LENS_SMALL = [1, 4099, 3, 70001, 50], [1, 4099, 3, 7001, 50]


@pytest.mark.parametrize("path,lens", [("vec-nk3-ctrl", LENS_BIG), ("scalar-nk3", LENS_BIG), ("pre-kernel-alt", LENS_BIG), ("wide-nk11-ctrl", LENS_BIG),
                                       ("ticketed-vec", LENS_BIG), ("ticketed-scalar-pre", LENS_BIG), ("single-vec", LENS_SMALL),
                                       ("single-scalar", LENS_SMALL), ("single-vec-pre-alt", LENS_SMALL)])
@pytest.mark.parametrize("norm", ["rms", "linf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_per_segment_counts_of_a_padded_layout(be, dbl, dev, dtype, norm, path, lens):
    """A five-segment tuple layout with starts rounded up to W and the pads of EVERY operand filled with NaN: a pad is never read,
    so it is never counted and never reaches the value; each segment's count lands in that segment's word."""
    entry, nk, e_pre, aligned, ctrl, alt, _, kernel = PATHS[path]
    w = WIDTH[dtype]
    segl, total = _layout(lens, w)
    assert _kernel_for(entry, nk, e_pre, aligned, ctrl, sum(lens), dtype) == kernel
    ops = _Operands(dev, dtype, total, nk, e_pre=e_pre, alt=alt, aligned=aligned)
    pads = [e for s, l in segl for e in range(s + l, s + -(-l // w) * w)]
    assert pads
    for name in list(ops.d):
        ops.plant(name, pads, SPECIAL[dtype][2:4])
    ops._undo = []  # (the pads stay NaN)
    rig = _Rig(be, dbl, dev, dtype, norm, segl)
    rig.check(ops, entry, ctrl, "pads only")
    assert rig.reference(ops)[0].sum() == 0 and not np.isnan(rig.reference(ops)[1]).any()

    def spots(s, l):  # first element, last vector-path element, every tail element
        return sorted({s, s + max(l // w * w - 1, 0)} | set(range(s + l // w * w, s + l)))

    for i, (s, l) in enumerate(segl):
        ops.plant("y0", spots(s, l), np.roll(SPECIAL[dtype], i))
        counts, _ = rig.reference(ops)
        assert counts[i] == len(spots(s, l)) and counts.sum() == counts[i]
        rig.check(ops, entry, ctrl, ("segment", i))
        ops.restore()
    for i, (s, l) in enumerate(segl):
        ops.plant("y0", spots(s, l), np.roll(SPECIAL[dtype], i))
    rig.check(ops, entry, ctrl, "every segment")
    if alt:
        rig.check(ops, entry, ctrl, "every segment, the clean alternative selected", accept=1)


@pytest.mark.parametrize("entry", ["partial", "fused"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_stale_records_and_sticky_status_on_one_workspace(be, dbl, dev, dtype, entry):
    """tests/_controller_scripts.py's "sticky_nonfinite" with kernels producing the numbers, on ONE workspace and control block:
    (1) a two-pass launch whose plant a high-numbered workgroup owns; (2) clean launches with smaller grids — the records the first
    launch left beyond them are masked, the count is 0 (first a state still above the one-workgroup kernel's reach, so that the
    fused entry point's ticketed kernel meets the stale records too, then W (3 * 256 + 37) elements); (3) a planted launch;
    (4) a clean one — `nonfinite` reads 0.0 again while `status` stays STATUS_NONFINITE."""
    w = WIDTH[dtype]
    n_big, n_mid, n_small = _sizes(dtype)["two_pass"], w * (300 * BLOCK + 37), w * (3 * BLOCK + 37)
    assert n_mid > SINGLE_MAX and -(-n_mid // (w * BLOCK)) < NORM_GRID - 3
    rigs = {}
    for n in (n_big, n_mid, n_small):
        rigs[n] = r = _Rig(be, dbl, dev, dtype, "rms", [(0, n)])
        r.ws, r.ctrl, r.sums, r.ts = rigs[n_big].ws, rigs[n_big].ctrl, rigs[n_big].sums, rigs[n_big].ts
    big, mid, small = (_Operands(dev, dtype, n, 1, e_pre=True) for n in (n_big, n_mid, n_small))
    owner = NORM_GRID - 3  # the workgroup that reads vectors [owner * 256, owner * 256 + 256) in the first pass
    big.plant("y0", [w * (owner * BLOCK + 70) + 1], SPECIAL[dtype][0:1])

    def launch(ops):
        r = rigs[ops.total]
        if entry == "partial":
            _, gn = r.partial(ops, True)
            c = r.control()
            assert c.nonfinite == gn.sum()
        else:
            c = r.fused(ops)
        return c

    rigs[n_big].arm()
    c = launch(big)
    assert (c.nonfinite, c.status) == (1.0, _hip.STATUS_NONFINITE)
    # a freshly constructed block on the SAME workspace: a smaller grid's launch must not see workgroup `owner`'s record
    rigs[n_mid].arm()
    c = launch(mid)
    assert (c.nonfinite, c.status) == (0.0, _hip.STATUS_OK)
    c = launch(small)
    assert (c.nonfinite, c.status) == (0.0, _hip.STATUS_OK)
    small.plant("y0", [0, n_small - 1], SPECIAL[dtype][1:3])
    c = launch(small)
    assert (c.nonfinite, c.status) == (2.0, _hip.STATUS_NONFINITE)
    small.restore()
    c = launch(small)
    assert (c.nonfinite, c.status) == (0.0, _hip.STATUS_NONFINITE)  # the count is this attempt's, the status is the solve's
    assert c.n_steps == 4


@pytest.mark.parametrize("size", ["vec_tail", "single", "two_pass"])
@pytest.mark.parametrize("e_pre", [False, True])
@pytest.mark.parametrize("norm", ["rms", "linf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fused_launch_leaves_what_the_two_launches_leave(be, dbl, dev, dtype, norm, e_pre, size):
    """For the same operands xde_error_norm_control leaves the `nonfinite`, `status`, `accept` and ratio NaN-ness that
    xde_error_norm_partial + xde_rk_control leave — clean, with +-Inf in y0 (finite ratio: the count alone speaks) and with a NaN."""
    w = WIDTH[dtype]
    n = _sizes(dtype)[size]
    ops = _Operands(dev, dtype, n, 1 if e_pre else 3, e_pre=e_pre, alt=True)
    rig = _Rig(be, dbl, dev, dtype, norm, [(0, n)])
    nvec = n // w
    cases = [("clean", [], None), ("inf", [0, w * (nvec - 1), n - 1], SPECIAL[dtype][0:2]), ("nan", [n // 2], SPECIAL[dtype][2:3]),
             ("all four", [1, n // 3, n - 2, n - 1], SPECIAL[dtype])]
    for label, idx, bits in cases:
        for accept in (0, 1):
            if idx:
                ops.plant("y0_alt" if accept else "y0", idx, bits)
            rig.arm(accept)
            rig.partial(ops, True)
            a = rig.control()
            rig.arm(accept)
            b = rig.fused(ops)
            assert (a.nonfinite, a.status, a.accept, a.sel_used) == (b.nonfinite, b.status, b.accept, b.sel_used), (label, accept)
            assert a.nonfinite == len(set(idx)), (label, accept)
            assert np.isnan(a.ratio) == np.isnan(b.ratio), (label, accept, a.ratio, b.ratio)
            if label == "inf":
                assert np.isfinite(a.ratio) and a.status == _hip.STATUS_NONFINITE  # e / inf = 0: no other guard than the count
            if np.isfinite(a.ratio):
                assert a.ratio == pytest.approx(b.ratio, rel=REL[dtype])
            ops.restore()
