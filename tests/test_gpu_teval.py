"""Per-sample output times on the GPU: the two kernels of include/xde_hip_teval.h against tests/_teval_oracle.py bit for bit (aligned
and one element off, rising and falling time, rows with an empty range, a whole row inside the step, equal neighbours, a query equal
to t1 and one equal to t0, all-NaN rows and padded rows, sentinels around and inside every output), and the end-to-end cases of
tests/_teval_cases.py with the HIP backend: the forward bit for bit against the union solve, the gradients against the existing
``backprop="steps"`` union solve plus gather."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import Dopri5, _hip, odeint
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _teval_cases as TC
from . import _teval_oracle as TO
from .test_gpu_rows import SENTINEL, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
ROWS = (1, 3, 65)
QS = (1, 2, 7, 33)
NK_OF_Q = {1: 1, 2: 3, 7: 7, 33: 9}  # operands of the midpoint sum: one, a few, the last unrolled count, the loop (Dopri8's)
T0, T1 = 0.25, 0.75  # the step (exact in both time dtypes)


def step_times(rows, Q, seed, TT):
    """``tq [rows, Q]`` (float64 holding TT values) and ``cnt``: by row, an empty range (one time before the step, the rest after it), a
    whole row inside the step, a row with a query equal to t0 (excluded), equal neighbours and a query equal to t1, an all-NaN row, a
    row padded from its middle on, and a row spread over [0, 1]."""
    rng = np.random.RandomState(seed)
    tq = np.full((rows, Q), np.nan)
    for r in range(rows):
        kind = (r + rows) % 6
        if kind == 0:
            row = np.sort(rng.uniform(0.8, 1.0, Q))
            if Q > 1:
                row[0] = 0.1
        elif kind == 1:
            row = np.sort(rng.uniform(0.3, 0.7, Q))
        elif kind == 2:
            row = np.sort(rng.uniform(0.3, 0.7, Q))
            row[0] = T0
            if Q > 1:
                row[-1] = T1
            if Q > 3:
                row[2] = row[1]
        elif kind == 3:
            continue
        elif kind == 4:
            row = np.full(Q, np.nan)
            row[: Q // 2] = np.sort(rng.uniform(0.2, 0.9, Q // 2))
        else:
            row = np.sort(rng.uniform(0.0, 1.0, Q))
        tq[r] = row
    tq = tq.astype(TT).astype(np.float64)
    cnt = (~np.isnan(tq)).cumprod(axis=1).sum(axis=1).astype(np.int32)
    return tq, cnt


def _cases(dtype):
    other = torch.float64 if dtype == torch.float32 else torch.float32
    for rows in ROWS:
        for Q in QS:
            for direction in (1, -1):
                yield rows, Q, direction, dtype
    yield 65, 7, 1, other  # the time dtype that is not the state's
    yield 65, 7, -1, other


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 130, 1030])
def test_dense_equals_the_oracle_bit_for_bit(dtype, D, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    for rows, Q, d, tdtype in _cases(dtype):
        TT = _NPT[tdtype]
        tq, cnt = step_times(rows, Q, rows * 131 + Q + D, TT)
        tq = d * tq
        t0, t1, dt = d * T0, d * T1, d * float(TT(0.5000001))
        rng = np.random.RandomState(rows * 7 + Q * 3 + D)
        nk = NK_OF_Q[Q]
        mk = lambda: Guarded((rows, D), dtype, misalign, fill=torch.from_numpy(rng.randn(rows, D).astype(T)))  # noqa: E731
        y0, y1, f0, f1 = mk(), mk(), mk(), mk()
        # the midpoint operands as a solve hands them over: k[0] is f0, and (from three on) the last one is f1
        ks = [f0] + [mk() for _ in range(nk - 1)]
        if nk >= 3 and nk != 9:
            ks[-1] = f1
        mid = [0.5, -0.125, 0.3, 0.07, -0.9, 1.5, 0.25, 0.01, -0.6][:nk]
        out = Guarded((Q, rows, D), dtype, misalign)
        want = np.full((Q, rows, D), SENTINEL, dtype=T)
        TO.dense(want, tq, cnt, [k.numpy() for k in ks], mid, y0.numpy(), y1.numpy(), f0.numpy(), f1.numpy(), t0, t1, dt, d, TT)
        be._teval_dense(out.view, torch.from_numpy(tq).to(DEV), torch.from_numpy(cnt).to(DEV), [k.view for k in ks], mid, y0.view, y1.view,
                        f0.view, f1.view, t0, t1, dt, d, _hip.dtype_code(tdtype))
        got = out.numpy()
        assert np.array_equal(got, want) and out.guards_intact(), (rows, Q, d, tdtype)  # exactly the member entries were written
        written = int((want != SENTINEL).any(axis=2).sum())
        assert written == sum(len(TO.members(tq[r], cnt[r], t0, t1, d, TT)) for r in range(rows))
        if rows == 65 and Q >= 2:
            assert 0 < written < rows * Q


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 130, 1030])
def test_cotangent_equals_the_oracle_bit_for_bit(dtype, D, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    for rows, Q, d, tdtype in _cases(dtype):
        TT = _NPT[tdtype]
        tq, cnt = step_times(rows, Q, rows * 137 + Q + D, TT)
        tq = d * tq
        t0, t1, dt = d * T0, d * T1, d * float(TT(0.5000001))
        rng = np.random.RandomState(rows * 11 + Q * 5 + D)
        gv = rng.randn(Q, rows, D).astype(T)
        gv[np.arange(Q)[:, None] >= cnt[None, :]] = np.nan  # what the loss put on padded entries is never read
        g = Guarded((Q, rows, D), dtype, misalign, fill=torch.from_numpy(gv))
        pre = [rng.randn(rows, D).astype(T) for _ in range(5)]
        tq_d, cnt_d = torch.from_numpy(tq).to(DEV), torch.from_numpy(cnt).to(DEV)
        # no bit, each bit alone, and the sweep's own mask with one output NULL (every variant at Q = 7, two of them elsewhere)
        variants = [(0, None), (1, None), (2, None), (4, None), (8, None), (16, None), (0b10, 3), (0b11111, 0)]
        for acc, null in variants if Q == 7 else [variants[0], variants[6]]:
            outs = [Guarded((rows, D), dtype, misalign, fill=torch.from_numpy(p)) for p in pre]
            want = [p.copy() for p in pre]
            TO.cotangent([None if j == null else w for j, w in enumerate(want)], gv, tq, cnt, t0, t1, dt, d, TT, acc)
            be._teval_cotangent([None if j == null else o.view for j, o in enumerate(outs)], g.view, tq_d, cnt_d, t0, t1, dt, d,
                                _hip.dtype_code(tdtype), acc_mask=acc)
            for j, (o, w) in enumerate(zip(outs, want)):
                assert np.array_equal(o.numpy(), w) and o.guards_intact(), (rows, Q, d, tdtype, acc, null, j)
                assert np.isfinite(o.numpy()).all()
        assert g.guards_intact()


# ----------------------------------------------------------------------------------------------
# end to end with the HIP backend
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, tdtype, reverse", [(torch.float32, torch.float32, False), (torch.float64, torch.float64, False),
                                                    (torch.float32, torch.float64, False), (torch.float64, torch.float64, True)],
                         ids=["fp32", "fp64", "fp32-state-fp64-time", "fp64-falling"])
def test_forward_equals_the_union_solve_on_the_device_bit_for_bit(dtype, tdtype, reverse):
    func, y0, ends = TC.five_row_problem(dtype, reverse, DEV)
    tq = TC.five_row_times(tdtype, reverse).to(DEV)
    with torch.no_grad():
        sol, steps = TC.solve_teval(func, y0, ends, tq, Dopri5, tdtype)
        union, idx = TC.solve_union(func, y0, ends, tq, Dopri5, tdtype)
    assert sol.shape == (7, 5, 3) and sol.dtype == dtype and sol.is_cuda
    assert torch.equal(sol, TC.gather(union, idx))
    assert bool((sol[4:, 3] == 0).all()) and bool((sol[2:, 4] == 0).all()) and torch.equal(sol[0, 1], y0[1])
    held = TC.held_per_step(steps, tq, ends, tdtype)
    assert any(max(h) >= 2 for h in held), "some step holds two queries of one row"
    assert any(0 < sum(1 for x in h if x) < 5 for h in held), "some step holds queries of some rows only"
    assert any(sum(h) == 0 for h in held), "some step holds none"
    assert sum(sum(h) for h in held) == int((~torch.isnan(tq)).sum()) - 1


def _grads(f, y0, tq, **opt):
    y = y0.clone().requires_grad_()
    sol, steps = TC.solve_teval(f, y, TC.MLP_ENDS, tq, Dopri5, y0.dtype, **opt)
    w = TC.loss_weights(sol)
    return sol.detach(), torch.autograd.grad(TC.loss_of(sol, w), [y] + list(f.parameters())), steps, w


def _union_grads(f, y0, tq, w):
    """The existing ``backprop="steps"`` on the union of the times, gathered on the device."""
    times, idx = TC.union_of(tq, TC.MLP_ENDS)
    y = y0.clone().requires_grad_()
    t = torch.tensor(times, dtype=y0.dtype, device=DEV)
    union = odeint(f, y, t, Dopri5, rtol=1e-5, atol=1e-7, options={"backprop": "steps", "norm": _rms_norm, "dtype": y0.dtype})
    sol = TC.gather(union, idx)
    return sol.detach(), torch.autograd.grad(TC.loss_of(sol, w), [y] + list(f.parameters()))


@pytest.mark.parametrize("dtype, bar", [(torch.float64, 1e-10), (torch.float32, 1e-4)], ids=["fp64", "fp32"])
def test_gradients_match_the_steps_route_on_the_union(dtype, bar, record_property):
    """fp64 <= 1e-10, fp32 <= 1e-4 (the steps route's own fp32 bar).  The sums differ by added zeros and by association inside a step
    only.  Measured on an MI355X: 1.1e-16 (fp64) and 2.2e-08 (fp32) over 15 accepted steps."""
    f, y0 = TC.MLP(dtype).to(DEV), TC.mlp_y0(dtype, DEV)
    tq = torch.tensor(TC.MLP_TIMES, dtype=dtype, device=DEV)
    sol, grads, steps, w = _grads(f, y0, tq)
    usol, ugrads = _union_grads(f, y0, tq, w)
    assert torch.equal(sol, usol)
    errs = [TC.rel(a, b) for a, b in zip(grads, ugrads)]
    record_property("teval_grad_rel_" + str(dtype).split(".")[-1], max(errs))
    print("t_eval gradients vs the steps route on the union, {}: max normwise rel = {:.3e} over {} accepted steps".format(
        dtype, max(errs), len(steps)))
    assert max(errs) <= bar, errs
    # what the loss puts on padded entries and on the row without an observation reaches nothing: exactly
    pad = torch.isnan(tq).t()
    y = y0.clone().requires_grad_()
    out, _ = TC.solve_teval(f, y, TC.MLP_ENDS, tq, Dopri5, dtype)
    noise = torch.where(pad[:, :, None], torch.full_like(w, 1e6), torch.zeros_like(w))
    g2 = torch.autograd.grad(TC.loss_of(out, w) + (out * noise).sum(), [y] + list(f.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(grads, g2))
    assert bool((grads[0][2] == 0).all()) and bool((sol[pad] == 0).all())


def test_memory_returns_after_backward():
    f, y0 = TC.MLP(torch.float32).to(DEV), TC.mlp_y0(torch.float32, DEV)
    tq = torch.tensor(TC.MLP_TIMES, dtype=torch.float32, device=DEV)
    t = torch.tensor(TC.MLP_ENDS, device=DEV)

    def once():
        y = y0.clone().requires_grad_()
        sol = odeint(f, y, t, Dopri5, rtol=1e-5, atol=1e-7, options={"t_eval": tq, "norm": _rms_norm})
        sol.square().sum().backward()
        del sol, y

    once()  # the per-device work sets and time tables are pooled on first use
    for p in f.parameters():
        p.grad = None
    gc.collect()  # (garbage of earlier tests must neither count nor be freed during the measured call)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    gc.disable()  # reference counting alone has to release what the call allocated
    try:
        once()
        for p in f.parameters():
            p.grad = None
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        gc.enable()


def test_latent_ode_demo_loss_falls():
    """examples/latent_ode_demo.py: spirals observed at per-row random times with a share of padding, trained through ``t_eval``."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import latent_ode_demo

    losses = latent_ode_demo.train(max_steps=40, log_every=0)
    head, tail = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    assert tail < 0.9 * head, (head, tail)
