"""The Hermite tape of ``ddeint_steps`` on the GPU: xde_dde_tape_gather and xde_dde_tape_gather_backward against
tests/_dde_tape_oracle.py bit for bit (fp32 and fp64, aligned and one element off, strided history rows next to contiguous tape nodes,
two delays in one interval, sigma = 0 and sigma = 1, dtau null, a tile inside a wider array, guard elements around every output, a
refused call leaving its outputs standing), the end-to-end cases of tests/_dde_tape_cases.py with the HIP backend, and the demo."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.xde.steps_dde import hermite_weights

from . import _dde_tape_oracle as DO
from ._dde_tape_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
MAXL = _hip.XDE_DDE_MAX_LAGS
# (rows, D, L): the smallest case; nothing divides the vector width; whole vectors; the element path (D = 7); a row longer than a wave's
# vectors with a remainder; a full launch of delays; more rows than a workgroup has lanes; and, beyond the issue's list, a row of 34
# fp32 vectors (the 16-byte path in both dtypes with more than one vector per row)
SHAPES = [(1, 1, 1), (1, 3, 2), (2, 4, 3), (3, 7, 1), (5, 130, 2), (2, 5, MAXL), (257, 6, 2), (3, 136, 2)]
TH = 3


@pytest.fixture
def dev():
    return DEV


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
            self.view.copy_(fill)

    def guards_intact(self):
        g = torch.cat([self.full[: self.off], self.full[self.off + self.n :]])
        return bool((g == SENTINEL).all())

    def untouched(self):
        return bool((self.full == SENTINEL).all())


def _case(rows, D, L, dtype, misalign, swap=False):
    """Operands and weights of one launch.  Delay 0 reads the history's last interval — strided rows, its end state a contiguous tape
    node — at sigma = 0 (``swap``: 1); the last delay sits at sigma = 1, in the same interval when there are two delays and else in
    the tape interval delays 1 and 2 share; the others cycle over a history interval and tape intervals.  Returns
    (srcs, keys, w, wd): ``keys[i]`` names the tape tensor behind ``srcs[i]`` (None: a history row)."""
    gen = torch.Generator().manual_seed(rows * 1031 + D * 17 + L)
    mk = lambda *shape: Guarded(shape, dtype, misalign, fill=torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype)).view  # noqa: E731
    his, hf = mk(rows, TH, D), mk(rows, TH, D)
    n_nodes = 4
    ys, fs = [mk(rows, D) for _ in range(n_nodes)], [mk(rows, D) for _ in range(n_nodes)]
    srcs, keys, w, wd = [], [], [], []
    for j in range(L):
        sigma = (1.0 if swap else 0.0) if j == 0 else (1.0 if j == L - 1 else (0.3 + 0.4 * (j % 2)))
        last_of_two = L == 2 and j == 1
        if j == 0 or last_of_two or (j > 2 and j < L - 1 and j % 3 == 0):
            i = TH - 2 if (j == 0 or last_of_two) else 0
            end_y = (ys[0], ("y", 0)) if i + 1 == TH - 1 else (his[:, i + 1, :], None)
            ops = [(his[:, i, :], None), (hf[:, i, :], None), end_y, (hf[:, i + 1, :], None)]
            h = 0.25
        else:
            m = 1 if (j in (1, 2) or j == L - 1) else j % (n_nodes - 1)
            ops = [(ys[m], ("y", m)), (fs[m], ("f", m)), (ys[m + 1], ("y", m + 1)), (fs[m + 1], ("f", m + 1))]
            h = 0.125
        a, b = hermite_weights(sigma, h)
        srcs += [x for x, _ in ops]
        keys += [k for _, k in ops]
        w += a
        wd += b
    return srcs, keys, w, wd


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D, L", SHAPES)
def test_gather_equals_the_oracle_bit_for_bit(dtype, rows, D, L, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    if L == 1:  # (one delay: sigma = 1 in a launch of its own)
        srcs, _, w, wd = _case(rows, D, L, dtype, misalign, swap=True)
        assert w == [0.0, 0.0, 1.0, 0.0]
        out = Guarded((rows, L, D), dtype, misalign)
        be._dde_tape_gather(out.view, None, srcs, w)
        assert torch.equal(out.view[:, 0], srcs[2]) and out.guards_intact()
    srcs, _, w, wd = _case(rows, D, L, dtype, misalign)
    assert w[:4] == [1.0, 0.0, 0.0, 0.0] and (L == 1 or w[-4:] == [0.0, 0.0, 1.0, 0.0])
    before = [x.cpu().numpy().copy() for x in srcs]
    want, want_d = DO.gather(before, w, wd, T)
    out, dtau = Guarded((rows, L, D), dtype, misalign), Guarded((rows, L, D), dtype, misalign)
    be._dde_tape_gather(out.view, dtau.view, srcs, w, wd)
    assert np.array_equal(out.view.cpu().numpy(), want) and np.array_equal(dtau.view.cpu().numpy(), want_d)
    assert out.guards_intact() and dtau.guards_intact()
    assert np.array_equal(out.view.cpu().numpy()[:, 0], before[0])  # sigma = 0: the interval's left state
    assert L == 1 or np.array_equal(out.view.cpu().numpy()[:, L - 1], before[4 * L - 2])  # sigma = 1: its right state
    # dtau null: the same values, the other buffer untouched
    only, spare = Guarded((rows, L, D), dtype, misalign), Guarded((rows, L, D), dtype, misalign)
    be._dde_tape_gather(only.view, None, srcs, w)
    assert torch.equal(only.view, out.view) and only.guards_intact() and spare.untouched()
    # a tile at j0 = 2 of a wider array, straight through the C ABI: the other delays' places keep their fill
    Ltot = L + 3
    wide = Guarded((rows, Ltot, D), dtype, misalign)
    strides = [int(x.stride(0)) if rows > 1 else D for x in srcs]
    rc = be.lib.xde_dde_tape_gather(wide.view.data_ptr(), None, _hip._ptr_array(srcs), (_hip.C.c_int64 * len(strides))(*strides), _hip.dbl_array(w),
                                    None, rows, D, L, 2, Ltot, _hip.dtype_code(dtype), _hip.stream_of(torch.device(DEV)))
    assert rc == _hip.XDE_OK, be.lib.xde_last_error().decode()
    got = wide.view.cpu().numpy()
    assert np.array_equal(got[:, 2 : 2 + L], want) and np.all(got[:, :2] == SENTINEL) and np.all(got[:, 2 + L :] == SENTINEL) and wide.guards_intact()
    # a refused call (an output over an operand) leaves its outputs standing
    with pytest.raises(_hip.XdeError, match="xde_dde_tape_gather"):
        be._dde_tape_gather(spare.view, None, srcs[:-1] + [spare.view[:, 0, :]], w)
    assert spare.untouched()
    # the operands kept their bits
    assert all(np.array_equal(x.cpu().numpy(), b) for x, b in zip(srcs, before))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D, L", SHAPES)
def test_gather_backward_equals_the_oracle_bit_for_bit(dtype, rows, D, L, misalign):
    """The cotangents of the distinct tape tensors of the same launch plan: a tensor two delays read is one output with two terms."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    _, keys, w, _ = _case(rows, D, L, dtype, misalign)
    order = sorted({k for k in keys if k is not None})
    terms = [[(i // 4, w[i]) for i, k in enumerate(keys) if k == key] for key in order]
    assert L == 1 or max(len(ts) for ts in terms) >= 2
    gen = torch.Generator().manual_seed(L)
    g = Guarded((rows, L, D), dtype, misalign, fill=torch.randn(rows, L, D, generator=gen, dtype=torch.float64).to(dtype))
    wants = DO.gather_backward(g.view.cpu().numpy(), terms, 0, T)
    outs = [Guarded((rows, D), dtype, misalign) for _ in terms]
    be._dde_tape_gather_backward([o.view for o in outs], terms, g.view)
    for o, want in zip(outs, wants):
        assert np.array_equal(o.view.cpu().numpy(), want) and o.guards_intact()
    # the delays from j0 = 1 on, as a tile of their own
    if L > 1:
        sub = [[(j - 1, x) for j, x in ts if j >= 1] for ts in terms]
        sub = [ts for ts in sub if ts]
        wants = DO.gather_backward(g.view.cpu().numpy(), sub, 1, T)
        outs = [Guarded((rows, D), dtype, misalign) for _ in sub]
        be._dde_tape_gather_backward([o.view for o in outs], sub, g.view, 1)
        for o, want in zip(outs, wants):
            assert np.array_equal(o.view.cpu().numpy(), want) and o.guards_intact()
    # a refused call (an output over g) leaves its outputs standing
    spare = Guarded((rows, D), dtype, misalign)
    inside = g.full[g.off : g.off + rows * D].view(rows, D)  # (a contiguous [rows, D] array that lies in g)
    kept = g.full.clone()
    with pytest.raises(_hip.XdeError, match="xde_dde_tape_gather_backward"):
        be._dde_tape_gather_backward([spare.view, inside], [[(0, 1.0)], [(0, 1.0)]], g.view)
    assert spare.untouched() and torch.equal(g.full, kept)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_operand_off_the_vector_grid_sends_the_launch_down_the_element_path(dtype):
    """Every buffer 16-byte aligned and D whole vectors, but for ONE operand (forward) or ONE output (backward) a single element off:
    the launch must not move vectors through it.  The same bits as the oracle, guards intact."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    rows, D, L = 3, 136, 2
    srcs, keys, w, wd = _case(rows, D, L, dtype, False)
    for slot in (1, 6):  # a strided history row, a contiguous tape node
        mixed = list(srcs)
        if mixed[slot].stride(0) == D:
            mixed[slot] = Guarded((rows, D), dtype, True, fill=srcs[slot]).view
        else:  # a history row: the whole history one element off
            mixed[slot] = Guarded((rows, TH, D), dtype, True, fill=torch.randn(rows, TH, D, dtype=torch.float64).to(dtype)).view[:, 1, :]
        assert mixed[slot].data_ptr() % 16 != 0 and all(x.data_ptr() % 16 == 0 for i, x in enumerate(mixed) if i != slot and x is not srcs[slot])
        want, want_d = DO.gather([x.cpu().numpy() for x in mixed], w, wd, T)
        out, dtau = Guarded((rows, L, D), dtype, False), Guarded((rows, L, D), dtype, False)
        be._dde_tape_gather(out.view, dtau.view, mixed, w, wd)
        assert np.array_equal(out.view.cpu().numpy(), want) and np.array_equal(dtau.view.cpu().numpy(), want_d)
        assert out.guards_intact() and dtau.guards_intact()
    order = sorted({k for k in keys if k is not None})
    terms = [[(i // 4, w[i]) for i, k in enumerate(keys) if k == key] for key in order]
    g = Guarded((rows, L, D), dtype, False, fill=torch.randn(rows, L, D, dtype=torch.float64).to(dtype))
    outs = [Guarded((rows, D), dtype, q == len(terms) - 1) for q in range(len(terms))]  # (g and the other outputs aligned)
    be._dde_tape_gather_backward([o.view for o in outs], terms, g.view)
    for o, want in zip(outs, DO.gather_backward(g.view.cpu().numpy(), terms, 0, T)):
        assert np.array_equal(o.view.cpu().numpy(), want) and o.guards_intact()


def test_the_tile_loop_takes_a_second_trip():
    """fp32, 4100 x 512, L = 2: 524800 vector items against the launch's cap of 2048 workgroups of 256 lanes (524288): the last rows are
    a second trip of the tile loop, in both kernels.  (8 MiB an operand: the smallest size at which the loop can go wrong.)"""
    be = _hip.get_backend()
    dtype, T = torch.float32, np.float32
    rows, D, L = 4100, 512, 2
    assert rows * (D // 4) > 2048 * 256
    srcs, keys, w, wd = _case(rows, D, L, dtype, False)
    want, _ = DO.gather([x.cpu().numpy() for x in srcs], w, None, T)
    out = Guarded((rows, L, D), dtype, False)
    be._dde_tape_gather(out.view, None, srcs, w)
    assert np.array_equal(out.view.cpu().numpy(), want) and out.guards_intact()
    order = sorted({k for k in keys if k is not None})
    terms = [[(i // 4, w[i]) for i, k in enumerate(keys) if k == key] for key in order]
    outs = [Guarded((rows, D), dtype, False) for _ in terms]
    be._dde_tape_gather_backward([o.view for o in outs], terms, out.view)
    for o, ref in zip(outs, DO.gather_backward(want, terms, 0, T)):
        assert np.array_equal(o.view.cpu().numpy(), ref) and o.guards_intact()


def test_dde_steps_demo_trains_the_delay():
    """examples/dde_steps_demo.py, a few iterations in this process: finite losses that fall, and a gradient on the learned delay."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dde_steps_demo

    hist = dde_steps_demo.train(iters=6, log_every=0)
    assert len(hist) == 6
    assert all(np.isfinite(rec["loss"]) and np.isfinite(rec["delay_grad"]) for rec in hist)
    assert hist[-1]["loss"] < hist[0]["loss"] and all(rec["delay_grad"] != 0.0 for rec in hist)
