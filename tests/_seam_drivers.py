"""Drivers of the resident seam launch called DIRECTLY (`_seam_attempt` on crafted operands), shared by tests/test_gpu_seam_kernel.py and
its fresh-process child tests/_seam_nt_child.py: the shapes of the register carry, the operands, and the two runs both of them make —

`state_machine`: NORM_LINF (an exact max) against the numpy double of tests/_seam_double.py, attempt by attempt, bit for bit;
`carry_case`:    either norm against the three launches the seam replaces (`error_norm_partial(e_pre=)` -> `rk_control(ws)` ->
                 `stage_combine(ctrl=, y0_alt=y1, k0_alt=k_last)`), byte for byte, at a given number of vectors per lane.

Both return a digest of everything they compared, so a child under another load policy (XDE_NT=0) can be held to the parent's run.
Every function takes the backend and the device as arguments: nothing here needs a GPU by itself."""
import ctypes as C
import hashlib

import numpy as np
import torch

from paddlexde_amd import _hip

from ._controller_drivers import SENTINEL, block_of, fields
from .test_gpu_controller_kernels import FUSED_TARGETS, _mid_solve_params, assert_blocks_equal

DT = {"f32": torch.float32, "f64": torch.float64}
NPT = {"f32": np.float32, "f64": np.float64}
WIDTH = {"f32": 4, "f64": 2}  # elements per 16-byte vector
IVIEW = {"f32": torch.int32, "f64": torch.int64}
KIND = {"rms": _hip.NORM_RMS, "linf": _hip.NORM_LINF}
A21, C_LAST = 0.2, 0.025  # dopri5's a21 and (to two digits) its last error coefficient
GRID, BLOCK = 512, 256  # the error-norm pass's grid cap and its workgroup
LANES = GRID * BLOCK
DEPTHS = (16, 13, 9, 8, 5, 4, 1)  # vectors per lane: both sides of every edge of the kernel's batches of 4, the full carry, one


def carry_n(p, width):
    """The state of `p` vectors per lane: 512 workgroups, a last batch row that ends in the MIDDLE of workgroup 37 (the lanes after it
    take the clamped reload, workgroups 38.. skip the batch), and a scalar tail of width - 1 elements.  p = 1: 3077 (a few workgroups)."""
    return 3077 if p == 1 else ((p - 1) * LANES + 37 * BLOCK + 19) * width + (width - 1)


def geometry(n, width):
    blocks = max(1, min(-(-n // (BLOCK * width)), GRID))
    return blocks, -(-(n // width) // (blocks * BLOCK))


def check_plan(be, n, sdt, per_lane=None):
    """The device must hold the whole grid at once (512 resident) and the plan must be the geometry stated above: anything else is a
    failure, not a skip."""
    plan = be._seam_plan(n, DT[sdt])
    blocks, pl = geometry(n, WIDTH[sdt])
    assert plan == {"blocks": blocks, "per_lane": pl, "resident": 512, "fits": 1}, (n, sdt, plan)
    if per_lane is not None:
        assert plan["per_lane"] == per_lane and (per_lane <= 1 or plan["blocks"] == 512), (n, sdt, plan)
    return plan


def operands(n, sdt, seed):
    """(k_last, e_pre, y0, f0, y1, y0_alt, f0_alt) on the host; e_pre and k_last are of order 1 (the runs rescale them)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=g, dtype=DT[sdt])  # noqa: E731
    y0 = r()
    y1 = y0 + 1e-3 * r()
    return {"k": r(), "e": r(), "y0": y0, "f0": r(), "y1": y1, "y0a": y0 + 1e-2 * r(), "f0a": r()}


def same_bytes(a, b):
    """Two device (or host) tensors of one floating dtype, compared as bytes (NaN payloads and signed zeros included)."""
    iv = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(iv), b.view(iv)))


def block_bytes(c, seq0=0):
    """A control block without what no comparison reads: `seq` counted from `seq0`, `chk` / `reserved` blanked."""
    c = _hip.XdeCtrl.from_buffer_copy(bytes(c))
    c.seq -= seq0
    c.chk = 0
    c.reserved[0] = c.reserved[1] = 0
    return bytes(c)


def stated_out(o, ka, sdt, dt_new, accepted, selected):
    """`out` as the header states it, without the double's stage_combine: accepted `y1 + k_last * (T(a21) * T(dt'))`, rejected
    `y0 + f0 * (...)` on the candidates the attempt ran on."""
    T = NPT[sdt]
    c1 = T(A21) * T(dt_new)
    with np.errstate(all="ignore"):
        if accepted:
            return o["y1"].numpy() + ka.numpy() * c1
        yb, fb = (o["y0a"], o["f0a"]) if selected else (o["y0"], o["f0"])
        return yb.numpy() + fb.numpy() * c1


# ------------------------------------------------------------------------------------------------------------------------------
# NORM_LINF against the numpy double
# ------------------------------------------------------------------------------------------------------------------------------
STEP_T = [0.5, 0.0, -1 / 128, -1 / 16, -3.0]
T_SPAN = [0.0, -1 / 16, -1 / 16, -1e6]


def probe_ratio(dbl, cd, p, o, ts, st, sd, alt, k=None, e=None):
    """The ratio the double's seam attempt reports for these operands, measured on scratch copies of its block and stage times."""
    pc, ps = cd.clone(), sd.clone()
    k, e = o["k"] if k is None else k, o["e"] if e is None else e
    dbl._seam_attempt(k, C_LAST, e, o["y0"], o["f0"], o["y1"], torch.empty_like(e), A21, None, pc, p, ts, st, ps,
                      y0_alt=o["y0a"] if alt else None, f0_alt=o["f0a"] if alt else None)
    return dbl.ctrl_read(pc).ratio


def state_machine(be, dbl, dev, sdt, tdt, n):
    """14 attempts (FUSED_TARGETS) in reverse time with `step_t`; every attempt: all fields of the block but `chk` / `reserved`, the
    stage times, `ctrl_read`, and `out`, each equal to the double's, bit for bit.  Odd attempts pass (y0_alt, f0_alt) — the operand
    select then follows the previous attempt's verdict — and `out` as the very tensor given as `e_pre`.  Returns the run's digest."""
    dt = DT[sdt]
    check_plan(be, n, sdt, per_lane=0 if n < WIDTH[sdt] else 1)
    o = operands(n, sdt, 5)
    od = {name: t.to(dev) for name, t in o.items()}
    st = torch.tensor(STEP_T, dtype=torch.float64)
    ts = torch.tensor(T_SPAN, dtype=torch.float64)
    p = _mid_solve_params(sdt, _hip.NORM_LINF, [n], tdt=tdt, direction=-1, n_step_t=len(STEP_T))
    ts_d, st_d = ts.to(dev), st.to(dev)
    cg, cd = be.new_ctrl(dev), dbl.new_ctrl(None)
    sg = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
    sd = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt)
    ws = be.new_workspace(dev)
    be.ctrl_init(cg, p, 0.0, -1 / 64, 4, ts_d, st_d, sg)
    dbl.ctrl_init(cd, p, 0.0, -1 / 64, 4, ts, st, sd)
    seq0 = block_of(cg).seq
    assert_blocks_equal(block_of(cg), dbl.ctrl_read(cd), (sdt, tdt, n, "init"), seq0)
    h = hashlib.sha256()
    clipped = 0
    for i, target in enumerate(FUSED_TARGETS):
        alt = alias = i % 2 == 1
        tag = (sdt, tdt, n, i, target)
        before = dbl.ctrl_read(cd)
        scale = target / probe_ratio(dbl, cd, p, o, ts, st, sd, alt) if target else 0.0
        ka, ea = o["k"] * scale, o["e"] * scale
        ka_d, ea_d = ka.to(dev), ea.to(dev, copy=True)
        out_d = ea_d if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        out_h = ea if alias else torch.full((n,), SENTINEL, dtype=dt)
        be._seam_attempt(ka_d, C_LAST, ea_d, od["y0"], od["f0"], od["y1"], out_d, A21, ws, cg, p, ts_d, st_d, sg,
                         y0_alt=od["y0a"] if alt else None, f0_alt=od["f0a"] if alt else None)
        dbl._seam_attempt(ka, C_LAST, ea, o["y0"], o["f0"], o["y1"], out_h, A21, None, cd, p, ts, st, sd,
                          y0_alt=o["y0a"] if alt else None, f0_alt=o["f0a"] if alt else None)
        read = be.ctrl_read(cg)
        got, want = block_of(cg), dbl.ctrl_read(cd)
        # the double's own `out` is the header's statement of it (so the reference does not rest on the double's stage_combine)
        stated = stated_out(o, ka, sdt, want.dt, want.accept, alt and before.accept)
        assert stated.tobytes() == out_h.numpy().tobytes(), tag
        assert bytes(read) == bytes(got), tag
        assert_blocks_equal(got, want, tag, seq0)
        stage = sg.cpu().numpy()
        assert stage.tobytes() == sd.numpy().tobytes(), tag + (stage, sd.numpy())
        assert (stage[p.n_stage:] == SENTINEL).all(), tag
        out_g = out_d.cpu().numpy()
        assert out_g.tobytes() == out_h.numpy().tobytes(), tag + ("out", int(want.accept), np.flatnonzero(out_g != out_h.numpy())[:4])
        assert be._seam_expired(cg) == 0, tag
        clipped += got.on_step_t
        if target:
            assert abs(got.ratio / target - 1) < 1e-3, tag + (got.ratio,)
        for part in (block_bytes(got, seq0), stage.tobytes(), out_g.tobytes()):
            h.update(part)
    for name in ("y0", "f0", "y1", "y0a", "f0a"):
        assert same_bytes(od[name].cpu(), o[name]), (sdt, tdt, n, name, "an input was written")
    # (a rejected clipped step, an accepted one that lands on the two rows at -1/16, the index moved on to the last entry)
    assert clipped >= 2 and got.n_accept >= 5 and got.n_reject >= 4 and (got.next_out, got.next_step_index) == (3, 4), fields(got)
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------------------
# either norm against the three launches
# ------------------------------------------------------------------------------------------------------------------------------
def three_launches(be, k, e_pre, y0, f0, y1, out, ws, ctrl, p, ts, st, stage, segs, y0_alt=None, f0_alt=None):
    """What the seam launch replaces, as tests/_seam_double.py composes it.  The candidates are chosen on the host from the block as
    it stands BEFORE the controller runs (the solver knows them the same way); the combine's own select then follows the new verdict."""
    sel = y0_alt is not None and block_of(ctrl).accept != 0
    yb, fb = (y0_alt, f0_alt) if sel else (y0, f0)
    be.error_norm_partial([k], [C_LAST], y0, y1, p.rtol, p.atol, segs, p.norm_kind, ws, ctrl=ctrl, y0_alt=y0_alt, e_pre=e_pre)
    be.rk_control(ctrl, p, ws, None, ts, st, stage)
    be.stage_combine(out, yb, [fb], [A21], _hip.COMBINE_RK, ctrl=ctrl, y0_alt=y1, k0_alt=k)


CARRY_T_SPAN = [0.0, 0.004, 0.03, 10.0]
CARRY_SCALES = ((1e-7, 1), (1e2, 0))  # (scale of e_pre and k_last, the verdict it must give): ratio < 1, then ratio > 1


def carry_case(be, dev, sdt, norm, p_lane, ws_a, ws_b, gen=None):
    """Two consecutive attempts at `p_lane` vectors per lane from two byte-identical copies of one mid-solve block: blocks (`chk` too),
    stage times and `out` byte-identical between the seam launch and the three launches.  Attempt 0 is accepted and writes an `out` of
    its own; attempt 1 runs on (y0_alt, f0_alt), is rejected, and writes `out` over its `e_pre`.  Returns the digest of the seam side."""
    dt, w = DT[sdt], WIDTH[sdt]
    n = carry_n(p_lane, w)
    check_plan(be, n, sdt, per_lane=p_lane)
    gen = gen or torch.Generator(device=dev).manual_seed(11 + p_lane)
    r = lambda: torch.randn(n, generator=gen, dtype=dt, device=dev)  # noqa: E731
    y0, f0, k, e, y0a, f0a = r(), r(), r(), r(), r(), r()
    y1 = y0 + 1e-3 * r()
    pr = _mid_solve_params(sdt, KIND[norm], [n])
    segs = _hip.make_segments([(0, n)])
    ts = torch.tensor(CARRY_T_SPAN, dtype=torch.float64, device=dev)
    a = torch.zeros(C.sizeof(_hip.XdeCtrl), dtype=torch.uint8, device=dev)
    sa = torch.full((_hip.XDE_MAX_STAGE,), SENTINEL, dtype=dt, device=dev)
    be.ctrl_init(a, pr, 0.0, 0.01, 4, ts, None, sa)
    b, sb = a.clone(), sa.clone()
    h = hashlib.sha256()
    for attempt, (scale, verdict) in enumerate(CARRY_SCALES):
        tag = (sdt, norm, p_lane, n, attempt)
        alt = alias = attempt == 1
        ka = k * scale
        ea, eb = e * scale, e * scale
        oa = ea if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        ob = eb if alias else torch.full((n,), SENTINEL, dtype=dt, device=dev)
        be._seam_attempt(ka, C_LAST, ea, y0, f0, y1, oa, A21, ws_a, a, pr, ts, None, sa, y0_alt=y0a if alt else None,
                         f0_alt=f0a if alt else None)
        three_launches(be, ka, eb, y0, f0, y1, ob, ws_b, b, pr, ts, None, sb, segs, y0a if alt else None, f0a if alt else None)
        ga, gb = block_of(a), block_of(b)
        assert bytes(ga) == bytes(gb), tag + (fields(ga), fields(gb))
        assert same_bytes(sa, sb), tag + (sa.cpu(), sb.cpu())
        differ = torch.nonzero(oa.view(IVIEW[sdt]) != ob.view(IVIEW[sdt]))[:4].flatten().tolist()
        assert same_bytes(oa, ob), tag + ("out", int(ga.accept), differ)
        assert ga.n_steps == attempt + 1 and ga.accept == verdict and ga.ratio == ga.ratio and ga.ratio > 0, tag + (fields(ga),)
        assert ga.nonfinite == 0 and ga.status == 0, tag + (fields(ga),)
        assert be._seam_expired(a) == 0, tag
        for part in (bytes(ga), sa.cpu().numpy().tobytes(), oa.cpu().numpy().tobytes()):
            h.update(part)
    return h.hexdigest()


def carry_run(be, dev, sdt, norm, p_lane, ws_a, ws_b):
    """`carry_case` on workspaces that hold the records of a wider grid: at one vector per lane (a few workgroups) the 512-workgroup case
    of 4 vectors per lane runs first on the same workspaces, whatever ran before."""
    if p_lane == 1:
        carry_case(be, dev, sdt, norm, 4, ws_a, ws_b)
    return carry_case(be, dev, sdt, norm, p_lane, ws_a, ws_b)
