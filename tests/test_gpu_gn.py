"""General and scalar noise on the GPU: xde_sde_gn_step against tests/_gn_oracle.py on the read-back Z bit for bit (out of place and in
place, aligned and one element off, dt negative and dt = s = 0), xde_sde_gn_backward against numpy for every mask of outputs, guard
elements around every output, determinism, the second moments of the increment, the end-to-end cases of tests/_gn_cases.py with the
HIP backend, and the SDE-GAN demo."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _gn_oracle as GN
from . import _sde_oracle as SO
from ._gn_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0
# (rows, D, M): the smallest case; scalar noise; nothing divides the vector width; whole vectors; an odd D with whole vectors of M; M
# past one chunk of 32 with a straddled Philox block; one row spanning workgroups; many rows per workgroup; rows that do not divide the
# tile
SHAPES = [(1, 1, 1), (3, 3, 1), (2, 5, 3), (5, 4, 4), (3, 7, 8), (1, 2, 67), (2, 300, 5), (300, 1, 3), (257, 6, 2)]


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


def _operands(rows, D, M, dtype, misalign):
    gen = torch.Generator().manual_seed(rows * 1031 + D * 17 + M)
    mk = lambda *shape: Guarded(shape, dtype, misalign, fill=torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype)).view  # noqa: E731
    return mk(rows, D), mk(rows, D), mk(rows, D, M), mk(rows, D)  # y0, f, g, gy


def _noise(rows, M, seed, k, dtype):
    out = torch.empty(rows, M, dtype=dtype, device=DEV)
    _hip.get_backend()._sde_noise(out, seed, k)
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D, M", SHAPES)
def test_gn_step_equals_the_oracle_bit_for_bit(dtype, rows, D, M, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    y0, f, g, _ = _operands(rows, D, M, dtype, misalign)
    seed, k = 0x5EED, 17
    z = _noise(rows, M, seed, k, dtype)
    Y0, F, G = (x.cpu().numpy() for x in (y0, f, g))
    for dt in (T(0.0123), T(-0.0123), T(0.0)):
        s = SO.s_of(dt, T)
        want = GN.gn_step(Y0, F, G, dt, s, z, T)
        y1 = Guarded((rows, D), dtype, misalign)
        be._sde_gn_step(y1.view, y0, f, g, float(dt), float(s), seed, k)
        assert np.array_equal(y1.view.cpu().numpy(), want), float(dt)
        assert y1.guards_intact()
        inplace = Guarded((rows, D), dtype, misalign, fill=y0)
        be._sde_gn_step(inplace.view, inplace.view, f, g, float(dt), float(s), seed, k)
        assert np.array_equal(inplace.view.cpu().numpy(), want) and inplace.guards_intact()
        again = torch.empty_like(y0)
        be._sde_gn_step(again, y0, f, g, float(dt), float(s), seed, k)
        assert torch.equal(again, y1.view)  # (two launches, the same bits)
    assert np.array_equal(GN.gn_step(Y0, F, G, T(0.0), T(0.0), z, T), Y0)  # (a zero-length step returns y0)
    # the operands kept their bits
    assert np.array_equal(y0.cpu().numpy(), Y0) and np.array_equal(f.cpu().numpy(), F) and np.array_equal(g.cpu().numpy(), G)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows, D, M", SHAPES)
def test_gn_backward_equals_numpy_bit_for_bit_for_every_mask(dtype, rows, D, M, misalign):
    """Every mask of null outputs: the written outputs are the header's formulas on the read-back Z, a buffer standing for a skipped
    output keeps its fill, and so do the guard elements around every output; two launches give the same bits."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    _, _, _, gy = _operands(rows, D, M, dtype, misalign)
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s = SO.s_of(dt, T)
    wants = GN.gn_backward(gy.cpu().numpy(), dt, s, _noise(rows, M, seed, k, dtype), T)
    for mask in itertools.product((1, 0), repeat=2):
        outs = [Guarded((rows, D), dtype, misalign), Guarded((rows, D, M), dtype, misalign)]
        be._sde_gn_backward(*[o.view if m else None for o, m in zip(outs, mask)], gy, M, float(dt), float(s), seed, k)
        for o, m, want in zip(outs, mask, wants):
            if m:
                assert np.array_equal(o.view.cpu().numpy(), want), mask
                assert o.guards_intact(), mask
            else:
                assert o.untouched(), mask
    again = torch.empty(rows, D, M, dtype=dtype, device=DEV)
    be._sde_gn_backward(None, again, gy, M, float(dt), float(s), seed, k)
    assert np.array_equal(again.cpu().numpy(), wants[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_second_moments_of_the_increment(dtype):
    """rows = 2^14, D = 3, M = 2, a constant G, f = 0, y0 = 0, dt = 0.25: y = G w with w ~ N(0, dt I), so E[y y^T] = dt G G^T = S.  Every
    entry of the sample mean of y y^T lies within 6 standard errors, sqrt((S_ii S_jj + S_ij^2)/n) — the variance of y_i y_j under the
    target covariance (Isserlis), not under the sample."""
    be = _hip.get_backend()
    n, D, M, dt = 1 << 14, 3, 2, 0.25
    G = np.array([[1.0, 0.5], [-0.25, 0.75], [0.5, -1.0]])
    g = torch.as_tensor(G, dtype=dtype).expand(n, D, M).contiguous().to(DEV)
    y0 = torch.zeros(n, D, dtype=dtype, device=DEV)
    y1 = torch.empty_like(y0)
    be._sde_gn_step(y1, y0, torch.zeros_like(y0), g, dt, float(SO.s_of(dt, _NPT[dtype])), 0xABCDEF, 5)
    y = y1.cpu().numpy().astype(np.float64)
    S = dt * G @ G.T
    got = y.T @ y / n
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / n)
    print("second moments: worst |error| / standard error", float((np.abs(got - S) / se).max()))
    assert np.all(np.abs(got - S) <= 6 * se), (got, S, se)


def test_sde_gan_demo_runs_and_the_generators_diffusion_takes_a_gradient():
    """examples/sde_gan_demo.py, two iterations in this process: finite losses, and the score's gradient reaches a parameter of the
    generator's diffusion through cdeint, the differentiable control and the general-noise steps."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sde_gan_demo

    hist = sde_gan_demo.train(iters=2, log_every=0)
    assert len(hist) == 2 and hist[-1]["iters"] == 2
    for rec in hist:
        assert np.isfinite(rec["d_loss"]) and np.isfinite(rec["g_loss"]), rec
        assert np.isfinite(rec["diffusion_grad"]) and rec["diffusion_grad"] > 0, rec
