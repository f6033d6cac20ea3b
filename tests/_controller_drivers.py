"""Drivers shared by the step-controller tests: a script of tests/_controller_scripts.py through the numpy double (`run_double`) and
through the kernels (`gpu_run`), the field view of a control block, and the digest of a run."""
import ctypes as C
import hashlib

import numpy as np
import torch

from paddlexde_amd import _hip

from . import _controller_scripts as S
from ._cpu_double import NumpyDoubleBackend

SENTINEL = -777.0


def fields(c):
    out = {}
    for f, _t in _hip.XdeCtrl._fields_:
        v = getattr(c, f)
        out[f] = tuple(v) if isinstance(v, C.Array) else v
    return out


def same(a, b):
    """Equality with NaN equal to NaN, element-wise for tuples."""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def fill_sums(sums, s, i):
    vals, nfs = s.attempts[i]
    sums.zero_()
    sums[: s.n_seg] = torch.tensor(vals, dtype=torch.float64)
    sums[_hip.XDE_MAX_SEG : _hip.XDE_MAX_SEG + s.n_seg] = torch.tensor(nfs, dtype=torch.float64)


def run_double(s):
    """The double over script `s`: ([block after init, block after attempt 1, ...], [stage times after init, ...])."""
    d = NumpyDoubleBackend()
    table = (C.c_double * (2 * len(s.replay)))(*S.replay_flat(s)) if s.replay is not None else None
    p = S.build_params(_hip, s, C.addressof(table) if table is not None else None)
    ts = torch.tensor(s.t_span, dtype=torch.float64)
    st = None if s.step_t is None else torch.tensor(s.step_t, dtype=torch.float64)
    ctrl, sums = d.new_ctrl(None), d.new_sums(None)
    t_stage = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=torch.float32 if s.sdt == "f32" else torch.float64)
    d.ctrl_init(ctrl, p, s.t_span[0], s.first_step, len(s.t_span), ts, st, t_stage)
    blocks, stages = [d.ctrl_read(ctrl)], [t_stage.numpy().copy()]
    for i in range(len(s.attempts)):
        fill_sums(sums, s, i)
        d.rk_control(ctrl, p, None, sums, ts, st, t_stage)
        blocks.append(d.ctrl_read(ctrl))
        stages.append(t_stage.numpy().copy())
    assert torch.equal(ts, torch.tensor(s.t_span, dtype=torch.float64))
    return blocks, stages


def block_of(t):
    return _hip.XdeCtrl.from_buffer_copy(t.cpu().numpy().tobytes())


def gpu_run(be, dev, s, mirrored):
    """Script `s` through `be.ctrl_init` and one `be.rk_control(ctrl, p, None, sums, ...)` per attempt.  Returns the blocks in device
    memory and the whole stage-time buffers, after init and after every launch.  Checks on the way: with a host mirror the block handed
    out by `ctrl_read` is byte-equal to the one in device memory; `t_span`, `step_t` and the sums are unchanged at the end."""
    table = torch.tensor(S.replay_flat(s), dtype=torch.float64, device=dev) if s.replay is not None else None
    p = S.build_params(_hip, s, table.data_ptr() if table is not None else None)
    ts_h = torch.tensor(s.t_span, dtype=torch.float64)
    st_h = None if s.step_t is None else torch.tensor(s.step_t, dtype=torch.float64)
    ts, st = ts_h.to(dev), None if st_h is None else st_h.to(dev)
    sums_h = torch.zeros(max(len(s.attempts), 1), 2 * _hip.XDE_MAX_SEG, dtype=torch.float64)
    for i, (vals, nfs) in enumerate(s.attempts):
        sums_h[i, : s.n_seg] = torch.tensor(vals, dtype=torch.float64)
        sums_h[i, _hip.XDE_MAX_SEG : _hip.XDE_MAX_SEG + s.n_seg] = torch.tensor(nfs, dtype=torch.float64)
    sums = sums_h.to(dev)
    ctrl = be.new_ctrl(dev) if mirrored else torch.zeros(C.sizeof(_hip.XdeCtrl), dtype=torch.uint8, device=dev)
    t_stage = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=torch.float32 if s.sdt == "f32" else torch.float64, device=dev)
    be.ctrl_init(ctrl, p, s.t_span[0], s.first_step, len(s.t_span), ts, st, t_stage)
    blocks, stages = [block_of(ctrl)], [t_stage.cpu().numpy().copy()]
    for i in range(len(s.attempts)):
        be.rk_control(ctrl, p, None, sums[i], ts, st, t_stage)
        read = be.ctrl_read(ctrl)  # (with a mirror: the pinned ring, no HIP call)
        blocks.append(block_of(ctrl))
        stages.append(t_stage.cpu().numpy().copy())
        if mirrored:
            assert bytes(read) == bytes(blocks[-1]), (s.id, i, "the block read through the mirror is not the block in device memory")
    assert torch.equal(ts.cpu(), ts_h) and (st is None or torch.equal(st.cpu(), st_h)), (s.id, "a time table was written")
    assert np.array_equal(sums.cpu().numpy(), sums_h.numpy(), equal_nan=True), (s.id, "the sums were written")
    return blocks, stages


def digest(s, blocks, stages):
    """One digest of a run: every field but `chk` / `reserved` (`seq` counted from the init block's), and the stage times."""
    h = hashlib.sha256()
    for b, ts in zip(blocks, stages):
        c = _hip.XdeCtrl.from_buffer_copy(bytes(b))
        c.seq -= blocks[0].seq
        c.chk = 0
        c.reserved[0] = c.reserved[1] = 0
        h.update(bytes(c))
        h.update(ts.tobytes())
    return h.hexdigest()
