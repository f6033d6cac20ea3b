"""sdeint's Milstein steps on the GPU: xde_sde_milstein_support / _support_backward / _step / _backward against numpy on the read-back Z
(bit for bit), the end-to-end cases of tests/_milstein_cases.py with the HIP backend (walk, Euler equality, strong order 1, gradients),
and the SDE demo trained through Milstein."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.solver import Milstein

from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from ._milstein_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0


@pytest.fixture
def dev():
    return DEV


def _noise(n, seed, k, dtype):
    out = torch.empty(n, dtype=dtype, device=DEV)
    _hip.get_backend()._sde_noise(out, seed, k)
    return out.cpu().numpy()


def _operands(n, misalign, dtype, count):
    g = torch.Generator().manual_seed(n)
    ops = []
    for _ in range(count):
        x = torch.randn(n + 1, generator=g, dtype=dtype).to(DEV)
        ops.append(x[1:] if misalign else x[:-1])  # (misaligned: the scalar path)
    return ops


def _like(x, misalign):
    """A sentinel-filled output with x's alignment."""
    o = torch.full((x.numel() + 1,), SENTINEL, dtype=x.dtype, device=DEV)
    return o[1:] if misalign else o[:-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n, misalign", [(1, False), (7, False), (4099, False), (65536 * 3 + 5, False), (1001, True)])
def test_milstein_kernels_equal_numpy_bit_for_bit(dtype, n, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    y0, f, g_in, gb, gy = _operands(n, misalign, dtype, 5)
    Y0, F, G, GB, GY = (x.cpu().numpy() for x in (y0, f, g_in, gb, gy))
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s, c = SO.s_of(dt, T), MO.c_of(dt, T)
    z = _noise(n, seed, k, dtype)
    w, q = MO.correction(dt, z, T)
    step = lambda out, src: be._sde_milstein_step(out, src, f, g_in, gb, float(dt), float(s), float(c), seed, k)  # noqa: E731
    # the support point, forward and backward (no generator)
    yb = _like(y0, misalign)
    be._sde_milstein_support(yb, y0, f, g_in, float(dt), float(s))
    assert np.array_equal(yb.cpu().numpy(), (Y0 + F * dt) + G * s)
    inplace = _like(y0, misalign)
    inplace.copy_(y0)
    be._sde_milstein_support(inplace, inplace, f, g_in, float(dt), float(s))  # (yb may be y0)
    assert np.array_equal(inplace.cpu().numpy(), (Y0 + F * dt) + G * s)
    for want_f, want_g in ((True, True), (True, False), (False, True)):
        gf, gg = _like(gy, misalign), _like(gy, misalign)
        be._sde_milstein_support_backward(gf if want_f else None, gg if want_g else None, gy, float(dt), float(s))
        assert np.array_equal(gf.cpu().numpy(), GY * dt if want_f else np.full(n, T(SENTINEL)))
        assert np.array_equal(gg.cpu().numpy(), GY * s if want_g else np.full(n, T(SENTINEL)))
    # the step, out of place and with y1 aliasing y0
    want = ((Y0 + F * dt) + G * w) + (GB - G) * q
    y1 = _like(y0, misalign)
    step(y1, y0)
    assert np.array_equal(y1.cpu().numpy(), want)
    inplace = _like(y0, misalign)
    inplace.copy_(y0)
    step(inplace, inplace)
    assert np.array_equal(inplace.cpu().numpy(), want)
    # with gb == g the step is the Euler-Maruyama kernel's, bit for bit
    em, mil = _like(y0, misalign), _like(y0, misalign)
    be._sde_em_step(em, y0, f, g_in, float(dt), float(s), seed, k)
    be._sde_milstein_step(mil, y0, f, g_in, g_in, float(dt), float(s), float(c), seed, k)
    assert np.array_equal(em.cpu().numpy(), mil.cpu().numpy())
    # the backward: all three outputs, then each alone and each pair (the others keep their fill)
    wants = (GY * dt, GY * (w - q), GY * q)
    for mask in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        outs = [_like(gy, misalign) for _ in range(3)]
        be._sde_milstein_backward(*[o if m else None for o, m in zip(outs, mask)], gy, float(dt), float(s), float(c), seed, k)
        for o, m, wnt in zip(outs, mask, wants):
            assert np.array_equal(o.cpu().numpy(), wnt if m else np.full(n, T(SENTINEL))), mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_milstein_kernels_past_the_grid_cap_equal_numpy_bit_for_bit(dtype):
    """The support point, the step and the full backward at _sde_oracle.wrap_n: the lanes wrap around the capped grid."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    n = SO.wrap_n(T)
    g = torch.Generator().manual_seed(6)
    y0, f, g_in, gb, gy = (torch.randn(n, generator=g, dtype=dtype).to(DEV) for _ in range(5))
    Y0, F, G, GB, GY = (x.cpu().numpy() for x in (y0, f, g_in, gb, gy))
    seed, k, dt = 0xC0FFEE, 3, T(0.0371)
    s, c = SO.s_of(dt, T), MO.c_of(dt, T)
    w, q = MO.correction(dt, _noise(n, seed, k, dtype), T)
    out = torch.empty_like(y0)
    be._sde_milstein_support(out, y0, f, g_in, float(dt), float(s))
    assert np.array_equal(out.cpu().numpy(), (Y0 + F * dt) + G * s)
    be._sde_milstein_step(out, y0, f, g_in, gb, float(dt), float(s), float(c), seed, k)
    assert np.array_equal(out.cpu().numpy(), ((Y0 + F * dt) + G * w) + (GB - G) * q)
    outs = [torch.empty_like(gy) for _ in range(3)]
    be._sde_milstein_backward(*outs, gy, float(dt), float(s), float(c), seed, k)
    for o, want in zip(outs, (GY * dt, GY * (w - q), GY * q)):
        assert np.array_equal(o.cpu().numpy(), want)


def test_a_zero_length_step_returns_y0_exactly():
    be = _hip.get_backend()
    n = 4099
    y0, f, g_in, gb, gy = _operands(n, False, torch.float64, 5)
    y1, yb = torch.empty_like(y0), torch.empty_like(y0)
    be._sde_milstein_support(yb, y0, f, g_in, 0.0, 0.0)
    be._sde_milstein_step(y1, y0, f, g_in, gb, 0.0, 0.0, 0.0, 3, 2)
    assert torch.equal(y1, y0) and torch.equal(yb, y0)
    gf, gg, ggb = (torch.full_like(gy, SENTINEL) for _ in range(3))
    be._sde_milstein_backward(gf, gg, ggb, gy, 0.0, 0.0, 0.0, 3, 2)
    for o in (gf, gg, ggb):
        assert float(o.abs().max()) == 0.0


def test_sde_demo_loss_decreases_with_milstein():
    """examples/sde_demo.py trained through sdeint(Milstein): the bar of the Euler demo test."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sde_demo

    losses = sde_demo.train(max_steps=120, solver=Milstein, log_every=0)
    head, tail = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    assert tail < 0.9 * head, (head, tail)
