"""sdeint's reversible Heun steps and sdeint_adjoint on the GPU: the four xde_sde_rheun_* kernels against numpy on the read-back draw
(bit for bit), the end-to-end cases of tests/_rheun_cases.py with the HIP backend (walk, strong order 1, gradients, the adjoint), the
adjoint's memory against the step count, and the SDE demo trained through the adjoint."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _rheun_oracle as RO
from . import _sde_oracle as SO
from ._rheun_cases import *  # noqa: F401,F403
from ._rheun_cases import ReversibleHeun, reverse_after_forward, sdeint, sdeint_adjoint

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SENTINEL = 7.0


@pytest.fixture
def dev():
    return DEV


def _draw(n, seed, k, dtype):
    x = torch.empty(n, dtype=dtype, device=DEV)
    _hip.get_backend()._sde_noise(x, seed, k)
    return x.cpu().numpy()


def _operands(n, misalign, dtype, count, seed=None):
    g = torch.Generator().manual_seed(n if seed is None else seed)
    ops = []
    for _ in range(count):
        x = torch.randn(n + 1, generator=g, dtype=dtype).to(DEV)
        ops.append(x[1:] if misalign else x[:-1])  # (misaligned: the scalar path)
    return ops


def _like(x, misalign, value=None):
    """An output with x's alignment, filled with the sentinel or holding a copy of ``value``."""
    o = torch.full((x.numel() + 1,), SENTINEL, dtype=x.dtype, device=DEV)
    o = o[1:] if misalign else o[:-1]
    if value is not None:
        o.copy_(value)
    return o


def _check_kernels(dtype, n, misalign, dt, seed, k):
    """The four kernels on n elements: both directions, every permitted aliasing, every null combination; a refused call leaves its
    outputs' fill standing."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    y0, yh0, f0, f1, g0, g1, ay, ayh, af, ag, v = ops = _operands(n, misalign, dtype, 11)
    Y, YH, F0, F1, G0, G1, AY, AYH, AF, AG, V = (x.cpu().numpy() for x in ops)
    dt = T(dt)
    s = float(SO.s_of(dt, T))
    z = _draw(n, seed, k, dtype)
    for d in (1, -1):
        want = RO.predict(Y, YH, F0, G0, dt, z, T, d)
        out = _like(y0, misalign)
        be._sde_rheun_predict(out, y0, yh0, f0, g0, float(dt), s, d, seed, k)
        assert np.array_equal(out.cpu().numpy(), want)
        inplace = _like(y0, misalign, yh0)  # (yh1 aliasing yh0)
        be._sde_rheun_predict(inplace, y0, inplace, f0, g0, float(dt), s, d, seed, k)
        assert np.array_equal(inplace.cpu().numpy(), want)
        want = RO.correct(Y, F0, F1, G0, G1, dt, z, T, d)
        out = _like(y0, misalign)
        be._sde_rheun_correct(out, y0, f0, f1, g0, g1, float(dt), s, d, seed, k)
        assert np.array_equal(out.cpu().numpy(), want)
        inplace = _like(y0, misalign, y0)  # (y1 aliasing y0)
        be._sde_rheun_correct(inplace, inplace, f0, f1, g0, g1, float(dt), s, d, seed, k)
        assert np.array_equal(inplace.cpu().numpy(), want)
    # the stage: with af1, ag1 and without (the first backward step), out of place and with bf = af1, bg = ag1
    for a, b, A, B in ((af, ag, AF, AG), (None, None, None, None)):
        want = RO.adjoint_stage(A, B, AY, dt, z, T)
        bf, bg = _like(y0, misalign), _like(y0, misalign)
        be._sde_rheun_adjoint_stage(bf, bg, a, b, ay, float(dt), s, seed, k)
        assert np.array_equal(bf.cpu().numpy(), want[0]) and np.array_equal(bg.cpu().numpy(), want[1])
    bf, bg = _like(y0, misalign, af), _like(y0, misalign, ag)
    be._sde_rheun_adjoint_stage(bf, bg, bf, bg, ay, float(dt), s, seed, k)
    want = RO.adjoint_stage(AF, AG, AY, dt, z, T)
    assert np.array_equal(bf.cpu().numpy(), want[0]) and np.array_equal(bg.cpu().numpy(), want[1])
    for a, b in ((af, None), (None, ag)):  # (one of the two null: refused, nothing written)
        bf, bg = _like(y0, misalign), _like(y0, misalign)
        with pytest.raises(_hip.XdeError, match="null pointer"):
            be._sde_rheun_adjoint_stage(bf, bg, a, b, ay, float(dt), s, seed, k)
        assert float((bf - SENTINEL).abs().max()) == 0.0 and float((bg - SENTINEL).abs().max()) == 0.0
    # the step: with ayh1 and without, out of place and with ay0 = ay1, ayh0 = ayh1
    for h, H in ((ayh, AYH), (None, None)):
        want = RO.adjoint_step(AY, H, V, dt, z, T)
        outs = [_like(y0, misalign) for _ in range(4)]
        be._sde_rheun_adjoint_step(*outs, ay, h, v, float(dt), s, seed, k)
        for o, w in zip(outs, want):
            assert np.array_equal(o.cpu().numpy(), w)
        a0 = _like(y0, misalign, ay)
        outs = [a0, _like(y0, misalign, h), _like(y0, misalign), _like(y0, misalign)]
        be._sde_rheun_adjoint_step(*outs, a0, outs[1] if h is not None else None, v, float(dt), s, seed, k)
        for o, w in zip(outs, want):
            assert np.array_equal(o.cpu().numpy(), w)


# ----------------------------------------------------------------------------------------------
# the kernels against numpy on the read-back draw
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n, misalign", [(1, False), (7, False), (4099, False), (65536 * 3 + 5, False), (1001, True)])
def test_rheun_kernels_equal_numpy_bit_for_bit(dtype, n, misalign):
    _check_kernels(dtype, n, misalign, -0.0123, 0x5EED, 17)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rheun_kernels_past_the_grid_cap_equal_numpy_bit_for_bit(dtype):
    """The four kernels at _sde_oracle.wrap_n: the lanes wrap around the capped grid."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    n = SO.wrap_n(T)
    g = torch.Generator().manual_seed(6)
    y0, yh0, f0, f1, g0, g1, v = ops = [torch.randn(n, generator=g, dtype=dtype).to(DEV) for _ in range(7)]
    Y, YH, F0, F1, G0, G1, V = (x.cpu().numpy() for x in ops)
    seed, k, dt = 0xC0FFEE, 3, T(0.0371)
    s = float(SO.s_of(dt, T))
    z = _draw(n, seed, k, dtype)
    outs = [torch.empty_like(y0) for _ in range(4)]
    be._sde_rheun_predict(outs[0], y0, yh0, f0, g0, float(dt), s, 1, seed, k)
    assert np.array_equal(outs[0].cpu().numpy(), RO.predict(Y, YH, F0, G0, dt, z, T))
    be._sde_rheun_correct(outs[0], y0, f0, f1, g0, g1, float(dt), s, -1, seed, k)
    assert np.array_equal(outs[0].cpu().numpy(), RO.correct(Y, F0, F1, G0, G1, dt, z, T, -1))
    # (the operands stand in for the cotangents)
    be._sde_rheun_adjoint_stage(outs[0], outs[1], f0, g0, y0, float(dt), s, seed, k)
    for o, want in zip(outs, RO.adjoint_stage(F0, G0, Y, dt, z, T)):
        assert np.array_equal(o.cpu().numpy(), want)
    be._sde_rheun_adjoint_step(*outs, y0, yh0, v, float(dt), s, seed, k)
    for o, want in zip(outs, RO.adjoint_step(Y, YH, V, dt, z, T)):
        assert np.array_equal(o.cpu().numpy(), want)


def test_a_zero_length_step_returns_y0_exactly():
    """dt = s = 0: correct returns y0, predict 2 y0 - yh0, and the cotangent launches their dt = s = 0 values (the generator skipped)."""
    be = _hip.get_backend()
    n = 4099
    y0, yh0, f0, f1, g0, g1, ay, ayh, af, ag, v = _operands(n, False, torch.float64, 11)
    for d in (1, -1):
        out = torch.full_like(y0, SENTINEL)
        be._sde_rheun_correct(out, y0, f0, f1, g0, g1, 0.0, 0.0, d, 3, 2)
        assert torch.equal(out, y0)
        be._sde_rheun_predict(out, y0, yh0, f0, g0, 0.0, 0.0, d, 3, 2)
        assert torch.equal(out, (y0 + y0) - yh0)
    bf, bg = torch.full_like(y0, SENTINEL), torch.full_like(y0, SENTINEL)
    be._sde_rheun_adjoint_stage(bf, bg, af, ag, ay, 0.0, 0.0, 3, 2)
    assert torch.equal(bf, af) and torch.equal(bg, ag)
    be._sde_rheun_adjoint_stage(bf, bg, None, None, ay, 0.0, 0.0, 3, 2)
    assert float(bf.abs().max()) == 0.0 and float(bg.abs().max()) == 0.0
    outs = [torch.full_like(y0, SENTINEL) for _ in range(4)]
    be._sde_rheun_adjoint_step(*outs, ay, ayh, v, 0.0, 0.0, 3, 2)
    A = ayh + v
    assert torch.equal(outs[0], ay + (A + A)) and torch.equal(outs[1], -A)
    assert float(outs[2].abs().max()) == 0.0 and float(outs[3].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reverse_after_forward_returns_the_state(dtype):
    reverse_after_forward(DEV, dtype)


# ----------------------------------------------------------------------------------------------
# memory
# ----------------------------------------------------------------------------------------------
def test_adjoint_memory_does_not_grow_with_the_step_count():
    """y0 (64, 1, 256) fp32, t = [0, 1], step_size 1/32 and 1/512: the peak of torch.cuda.max_memory_allocated over forward plus
    backward.  The adjoint's peak at 512 steps exceeds its peak at 32 by at most 4 states' bytes (the host tables are a few KB); the
    through-the-steps peak at 512 exceeds the adjoint's by at least 100 states' bytes (it keeps at least 3 operands per step)."""
    torch.manual_seed(0)
    dev = torch.device(DEV)

    class Coef(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.tensor(-0.5))
            self.b = torch.nn.Parameter(torch.tensor(0.1))

        def forward(self, t, y):
            return torch.tanh(y * self.a) + self.b

    f, g = Coef().to(dev), Coef().to(dev)
    y0 = (0.5 + torch.rand(64, 1, 256)).to(dev).requires_grad_(True)
    t = torch.tensor([0.0, 1.0])
    state = y0.numel() * y0.element_size()

    def peak(call, h, **kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        sol = call(f, g, y0, t, solver=ReversibleHeun, options={"norm": None, "seed": 2, "step_size": h}, **kw)
        torch.autograd.grad(sol.sum(), [y0] + list(f.parameters()) + list(g.parameters()))
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base

    peak(sdeint_adjoint, 1.0 / 32)  # (warm-up: the library's and the allocator's first-call blocks)
    a32, a512, s512 = peak(sdeint_adjoint, 1.0 / 32), peak(sdeint_adjoint, 1.0 / 512), peak(sdeint, 1.0 / 512)
    print("peak bytes / state bytes: adjoint at 32 steps", a32 / state, "at 512", a512 / state, "through the steps at 512", s512 / state)
    assert a512 - a32 <= 4 * state, (a32 / state, a512 / state)
    assert s512 - a512 >= 100 * state, (s512 / state, a512 / state)


# ----------------------------------------------------------------------------------------------
# the demo
# ----------------------------------------------------------------------------------------------
def test_sde_demo_loss_decreases_with_the_adjoint():
    """examples/sde_demo.py trained through sdeint_adjoint(ReversibleHeun): the bar of the other demo tests."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sde_demo

    losses = sde_demo.train(max_steps=120, solver=ReversibleHeun, adjoint=True, log_every=0)
    head, tail = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    assert tail < 0.9 * head, (head, tail)
