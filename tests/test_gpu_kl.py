"""The KL term of a latent SDE on the GPU: xde_sde_kl_step against xde_sde_em_step (the path, bit for bit) and tests/_kl_oracle.py (the
row sums, within the double sum's bound), its modes and aliases, xde_sde_kl_backward against numpy on the read-back Z for every mask of
outputs, guard elements around every output, the end-to-end cases of tests/_kl_cases.py with the HIP backend, and the latent SDE demo."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _kl_oracle as KL
from . import _sde_oracle as SO
from ._kl_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
# (rows, D): a single element, rows that straddle Philox blocks (D % W != 0) with 1 to 64 lanes a row, whole blocks, a row of exactly one
# wave's vectors (256 fp32) and just past it, a row longer than a pass of 64 lanes, and more rows than one workgroup's waves hold
SHAPES = [(1, 1), (3, 3), (5, 4), (7, 5), (3, 64), (2, 255), (3, 256), (2, 260), (1, 1027), (257, 6)]


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


def _operands(rows, D, dtype, misalign):
    gen = torch.Generator().manual_seed(rows * 1031 + D)
    mk = lambda scale=1.0: Guarded((rows, D), dtype, misalign, fill=scale * torch.randn(rows, D, generator=gen, dtype=torch.float64).to(dtype)).view  # noqa: E731
    y0, f, h, gy = mk(), mk(), mk(), mk()
    g = Guarded((rows, D), dtype, misalign, fill=(0.5 + torch.rand(rows, D, generator=gen, dtype=torch.float64)).to(dtype)).view
    acc0 = torch.rand(rows, generator=gen, dtype=torch.float64).to(DEV) * 3.0
    gacc = torch.randn(rows, generator=gen, dtype=torch.float64).to(DEV)
    return y0, f, g, h, gy, acc0, gacc


def _noise(shape, seed, k, dtype):
    out = torch.empty(shape, dtype=dtype, device=DEV)
    _hip.get_backend()._sde_noise(out, seed, k)
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_kl_step_is_the_em_step_and_the_oracles_row_sums(dtype, rows, D, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    y0, f, g, h, _, acc0, _ = _operands(rows, D, dtype, misalign)
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s = SO.s_of(dt, T)
    em = Guarded((rows, D), dtype, misalign).view
    be._sde_em_step(em, y0, f, g, float(dt), float(s), seed, k)
    # the path: xde_sde_em_step's bits, out of place and in place
    y1, acc1 = Guarded((rows, D), dtype, misalign), Guarded((rows,), torch.float64, False)
    be._sde_kl_step(y1.view, acc1.view, y0, f, g, h, acc0, float(dt), float(s), seed, k)
    assert torch.equal(y1.view, em) and y1.guards_intact() and acc1.guards_intact()
    inplace = Guarded((rows, D), dtype, misalign, fill=y0)
    acc_in = Guarded((rows,), torch.float64, False, fill=acc0)
    be._sde_kl_step(inplace.view, acc_in.view, inplace.view, f, g, h, acc_in.view, float(dt), float(s), seed, k)  # (both aliases)
    assert torch.equal(inplace.view, em) and inplace.guards_intact() and acc_in.guards_intact()
    assert torch.equal(acc_in.view, acc1.view)
    # the row sums: every term is IEEE-exact, a double sum of D non-negative terms is within (D - 1) 2^-53 of the exact one in any
    # order, and the scale and the add round once each
    want, inc = KL.accumulate(acc0.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), h.cpu().numpy(), dt, T)
    err = np.abs(acc1.view.cpu().numpy() - want)
    bound = (D + 2) * 2.0**-53 * (np.abs(acc0.cpu().numpy()) + np.abs(inc))
    print("acc1: worst error / bound", float((err / bound).max()))
    assert np.all(err <= bound), (err.max(), bound.min())
    # modes and determinism
    again = torch.empty_like(acc0)
    be._sde_kl_step(torch.empty_like(y0), again, y0, f, g, h, acc0, float(dt), float(s), seed, k)
    assert torch.equal(again, acc1.view)  # (two launches, the same bits)
    only = Guarded((rows,), torch.float64, False)
    be._sde_kl_step(None, only.view, None, f, g, h, acc0, float(dt), 0.0, 0, 0)
    assert torch.equal(only.view, acc1.view) and only.guards_intact()  # (accumulate only: the fused mode's bits)
    z0, none = torch.empty_like(acc0), torch.empty_like(acc0)
    be._sde_kl_step(torch.empty_like(y0), z0, y0, f, g, h, torch.zeros_like(acc0), float(dt), float(s), seed, k)
    be._sde_kl_step(torch.empty_like(y0), none, y0, f, g, h, None, float(dt), float(s), seed, k)
    assert torch.equal(none, z0)  # (acc0 null: the bits of acc0 = 0)
    be._sde_kl_step(None, none, None, f, g, h, None, float(dt), 0.0, 0, 0)
    assert torch.equal(none, z0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D", SHAPES)
def test_kl_backward_equals_numpy_bit_for_bit_for_every_mask(dtype, rows, D, misalign):
    """With and without gy1, every mask of null outputs: the written outputs are the header's formulas on the read-back Z, a buffer
    standing for a skipped output keeps its fill, and so do the guard elements around every output."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    _, f, g, h, gy, _, gacc = _operands(rows, D, dtype, misalign)
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s = SO.s_of(dt, T)
    z = _noise((rows, D), seed, k, dtype)
    F, G, H, GY, GA = (x.cpu().numpy() for x in (f, g, h, gy, gacc))
    for with_gy in (True, False):
        wants = KL.kl_backward(GY if with_gy else None, GA, F, G, H, dt, s, z, T)
        for mask in itertools.product((1, 0), repeat=3):
            outs = [Guarded((rows, D), dtype, misalign) for _ in range(3)]
            be._sde_kl_backward(*[o.view if m else None for o, m in zip(outs, mask)], gy if with_gy else None, gacc, f, g, h, float(dt),
                                float(s), seed, k)
            for o, m, want in zip(outs, mask, wants):
                if m:
                    assert np.array_equal(o.view.cpu().numpy(), want), (with_gy, mask)
                    assert o.guards_intact(), (with_gy, mask)
                else:
                    assert o.untouched(), (with_gy, mask)


def test_latent_sde_demo_runs_and_its_loss_is_finite():
    """examples/latent_sde_demo.py --iters 3 (in this process, as the SDE demo's test runs its demo): the loss and both of its terms are
    finite at every step."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import latent_sde_demo

    hist = latent_sde_demo.train(iters=3, log_every=0)
    assert len(hist) == 3 and hist[-1]["iters"] == 3
    for rec in hist:
        assert all(np.isfinite(rec[key]) for key in ("loss", "recon", "kl")), rec
