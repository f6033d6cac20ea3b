"""Logsignature windows on the GPU: xde_logsig_windows and xde_logsig_windows_backward against tests/_logsig_oracle.py bit for bit
(float32 and float64, aligned and one element off, guard elements around every output) on every launch plan, NaN staying in its own
windows, a refused call leaving its output standing, the cases of tests/_logsig_cases.py with the HIP backend, and the demo."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _logsig_oracle as LO
from ._logsig_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
# (B, T, C, L, depth): no pairs; n = 1, zero areas; the smallest with areas; a short last window; more pairs than lanes of a wave and an
# odd C (4 x 4 tiles); K = 2080, a team of 256 lanes; many items per workgroup; a window longer than any staged chunk (the LDS of a
# workgroup holds fewer than 1229 points of 5 channels forward, fewer than 1222 rows backward) beside a window of one step; tiles in
# two batches and the cotangents read from global memory (C > 88); depth 1; one window of all points (L beyond T - 1)
SHAPES = [(1, 2, 1, 1, 2), (1, 2, 2, 1, 2), (2, 5, 2, 2, 2), (3, 8, 3, 3, 2), (2, 9, 33, 4, 2), (1, 4, 64, 3, 2), (130, 3, 2, 2, 2),
          (1, 1302, 5, 1300, 2), (1, 4, 90, 3, 2), (3, 8, 3, 3, 1), (2, 6, 17, 40, 2)]


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


_CASES = {}


def _case(shape, dtype):
    """The operands of a shape and what the oracle makes of them, computed once: x, gout, out, gx (numpy)."""
    key = (shape, dtype)
    if key not in _CASES:
        B, Tn, C, L, depth = shape
        rs = np.random.RandomState(B * 7 + Tn * 3 + C)
        T = _NPT[dtype]
        x = np.cumsum(0.3 * rs.randn(B, Tn, C), axis=1).astype(T)
        gout = rs.randn(B, LO.n_windows(Tn, L), LO.channels(C, depth)).astype(T)
        _CASES[key] = (x, gout, LO.windows(x, L, depth), LO.backward(gout, x, L, depth))
    return _CASES[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_kernels_equal_the_oracle_bit_for_bit(dtype, shape, misalign):
    be = _hip.get_backend()
    B, Tn, C, L, depth = shape
    X, GOUT, want, gwant = _case(shape, dtype)
    x = Guarded(X.shape, dtype, misalign, fill=torch.from_numpy(X)).view
    gout = Guarded(GOUT.shape, dtype, misalign, fill=torch.from_numpy(GOUT)).view
    out = Guarded(want.shape, dtype, misalign)
    be._logsig_windows(out.view, x, L, depth)
    got = out.view.cpu().numpy()
    assert np.array_equal(got, want), float(np.abs(got.astype(np.float64) - want).max())
    assert out.guards_intact()
    gx = Guarded(X.shape, dtype, misalign)
    be._logsig_windows_backward(gx.view, gout, x, L, depth)
    got = gx.view.cpu().numpy()
    assert np.array_equal(got, gwant), float(np.abs(got.astype(np.float64) - gwant).max())
    assert gx.guards_intact()
    # the operands kept their bits, and two launches give the same bits
    assert np.array_equal(x.cpu().numpy(), X) and np.array_equal(gout.cpu().numpy(), GOUT)
    again = torch.empty_like(out.view)
    be._logsig_windows(again, x, L, depth)
    assert torch.equal(again, out.view)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_nan_entry_poisons_only_its_own_windows(dtype):
    """(2, 13, 3), L = 4: a NaN inside window 1 of row 0 and one on the knot between windows 1 and 2 of row 1.  Both kernels equal the
    oracle (NaN where it has NaN); every other window, and every point that lies in no poisoned window, has the clean run's bits."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    X = np.cumsum(0.3 * np.random.RandomState(3).randn(2, 13, 3), axis=1).astype(T)
    GOUT = np.random.RandomState(4).randn(2, 3, 6).astype(T)
    bad = X.copy()
    bad[0, 6, 1] = np.nan
    bad[1, 8, 2] = np.nan
    runs = []
    for series in (X, bad):
        x, gout = torch.from_numpy(series).to(DEV), torch.from_numpy(GOUT).to(DEV)
        out, gx = torch.empty(2, 3, 6, dtype=dtype, device=DEV), torch.empty(2, 13, 3, dtype=dtype, device=DEV)
        be._logsig_windows(out, x, 4, 2)
        be._logsig_windows_backward(gx, gout, x, 4, 2)
        runs.append((out.cpu().numpy(), gx.cpu().numpy()))
        assert np.array_equal(runs[-1][0], LO.windows(series, 4, 2), equal_nan=True)
        assert np.array_equal(runs[-1][1], LO.backward(GOUT, series, 4, 2), equal_nan=True)
    (out0, gx0), (out1, gx1) = runs
    assert not np.isnan(out0).any() and not np.isnan(gx0).any()
    poisoned = np.zeros((2, 3), dtype=bool)
    poisoned[0, 1] = poisoned[1, 1] = poisoned[1, 2] = True
    assert np.isnan(out1[poisoned]).any(axis=-1).all() and np.array_equal(out1[~poisoned], out0[~poisoned])
    clean_points = np.ones((2, 13), dtype=bool)
    clean_points[0, 4:9] = clean_points[1, 4:13] = False
    assert np.array_equal(gx1[clean_points], gx0[clean_points]) and np.isnan(gx1[0, 4:9]).any() and np.isnan(gx1[1, 4:13]).any()


def test_a_refused_call_leaves_its_output_standing():
    lib = _hip.load_library()
    x = torch.randn(2, 9, 3, device=DEV)
    gout = torch.randn(2, 2, 6, device=DEV)
    out, gx = Guarded((2, 2, 6), torch.float32, False), Guarded((2, 9, 3), torch.float32, False)
    st = _hip.stream_of(x.device)
    for kw in (dict(depth=3), dict(C=513), dict(L=0), dict(T=1), dict(dtype=7)):
        a = dict(dict(B=2, T=9, C=3, L=4, depth=2, dtype=_hip.XDE_F32), **kw)
        tail = (a["B"], a["T"], a["C"], a["L"], a["depth"], a["dtype"], st)
        assert lib.xde_logsig_windows(out.view.data_ptr(), x.data_ptr(), *tail) == _hip.XDE_EBADARG
        assert lib.xde_logsig_windows_backward(gx.view.data_ptr(), gout.data_ptr(), x.data_ptr(), *tail) == _hip.XDE_EBADARG
    tail = (2, 9, 3, 4, 2, _hip.XDE_F32, st)
    assert lib.xde_logsig_windows(x.data_ptr(), x.data_ptr(), *tail) == _hip.XDE_EBADARG  # (out over x)
    assert lib.xde_logsig_windows_backward(x.data_ptr(), gout.data_ptr(), x.data_ptr(), *tail) == _hip.XDE_EBADARG
    with pytest.raises(_hip.XdeError, match="shape"):
        _hip.get_backend()._logsig_windows(out.view, x, 2, 2)  # (W = 4 at L = 2: the output's shape is refused before the launch)
    torch.cuda.synchronize()
    assert out.untouched() and gx.untouched()


def test_gradcheck_on_the_device():
    from paddlexde_amd.interpolation import logsig_windows

    x = torch.randn(2, 7, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s: logsig_windows(s, 2, 3), (x,))


def test_cde_demo_with_logsignature_windows_runs_with_a_falling_loss():
    """examples/cde_demo.py --logsig 2 --window 8, a few iterations in this process: 257 points, 32 windows, a field of 6 columns."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=8, n=64, logsig=2, window=8, log_every=0)
    print("demo losses:", losses)
    assert len(losses) == 8 and all(np.isfinite(losses)) and losses[-1] < losses[0]
