"""sdeint's SRK steps on the GPU: the second draw against tests/_srk_oracle.py, the six xde_sde_srk_* kernels against numpy on the
read-back draws (bit for bit), the end-to-end cases of tests/_srk_cases.py with the HIP backend (walk, strong order 1.5, gradients), and
the SDE demo trained through SRK."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.solver import SRK

from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from . import _srk_oracle as KO
from ._srk_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
_EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}
SENTINEL = 7.0


@pytest.fixture
def dev():
    return DEV


def _draws(n, seed, k, dtype):
    be = _hip.get_backend()
    out = []
    for draw in (0, 1):
        x = torch.empty(n, dtype=dtype, device=DEV)
        be._sde_noise(x, seed, k, draw=draw)
        out.append(x.cpu().numpy())
    return out


def _operands(n, misalign, dtype, count, seed=None):
    g = torch.Generator().manual_seed(n if seed is None else seed)
    ops = []
    for _ in range(count):
        x = torch.randn(n + 1, generator=g, dtype=dtype).to(DEV)
        ops.append(x[1:] if misalign else x[:-1])  # (misaligned: the scalar path)
    return ops


def _like(x, misalign):
    """A sentinel-filled output with x's alignment."""
    o = torch.full((x.numel() + 1,), SENTINEL, dtype=x.dtype, device=DEV)
    return o[1:] if misalign else o[:-1]


def _masked(launch, n_out, groups, wants, like, misalign, T):
    """``launch(*outs)`` with every combination of its output groups but the empty one: a written output equals its ``wants``, a skipped
    one (given as None) keeps the fill of the buffer standing for it."""
    for bits in range(1, 1 << len(groups)):
        mask = [0] * n_out
        for gi, (lo, hi) in enumerate(groups):
            if bits >> gi & 1:
                mask[lo:hi] = [1] * (hi - lo)
        outs = [_like(like, misalign) for _ in range(n_out)]
        launch(*[o if m else None for o, m in zip(outs, mask)])
        for o, m, want in zip(outs, mask, wants):
            assert np.array_equal(o.cpu().numpy(), want if m else np.full(like.numel(), T(SENTINEL))), mask


# ----------------------------------------------------------------------------------------------
# the second draw
# ----------------------------------------------------------------------------------------------
def test_the_second_draws_words_equal_the_oracle_bit_for_bit():
    be = _hip.get_backend()
    for seed, k, n in ((0, 0, 5), ((1 << 64) - 1, (1 << 32) - 1, 4097), (0xDEADBEEF12345678, 7, 65537)):
        out, out0, old = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
        be._sde_noise(out, seed, k, bits=True, draw=1)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), KO.words(-(-n // 4), seed, k, 1).reshape(-1)[:n]), (seed, k, n)
        rc = be.lib.xde_sde_noise_draw(out0.data_ptr(), n, seed, k, 0, _hip.XDE_NOISE_BITS, _hip.XDE_F32, None)
        assert rc == _hip.XDE_OK
        be._sde_noise(old, seed, k, bits=True)
        torch.cuda.synchronize()
        assert torch.equal(out0, old) and not torch.equal(out, old)  # (draw 0 through the new entry point is xde_sde_noise's)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_second_draw_is_the_oracles_within_the_math_library_bound(dtype):
    """DESIGN section 10's bound, |V_gpu - V_ref| <= eps * (13 |V_ref| + 4 r), on the counter with last word 1; V is not Z, and draw 0
    through xde_sde_noise_draw is Z bit for bit."""
    be = _hip.get_backend()
    eps = _EPS[dtype]
    for seed, k, n in ((3, 0, 1 << 18), ((1 << 64) - 1, 123456, 1001)):
        z, v = _draws(n, seed, k, dtype)
        ref, r = KO.normals(n, seed, k, _NPT[dtype], 1, with_r=True)
        err = np.abs(v.astype(np.float64) - ref)
        bound = eps * (13.0 * np.abs(ref) + 4.0 * r)
        worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (seed, k, worst, v[worst], ref[worst], err[worst] / eps)
        assert not np.array_equal(z, v)
        z0 = torch.empty(n, dtype=dtype, device=DEV)
        rc = be.lib.xde_sde_noise_draw(z0.data_ptr(), n, seed, k, 0, _hip.XDE_NOISE_NORMAL, _hip.dtype_code(dtype), None)
        torch.cuda.synchronize()
        assert rc == _hip.XDE_OK and np.array_equal(z0.cpu().numpy(), z)


# ----------------------------------------------------------------------------------------------
# the kernels against numpy on the read-back draws
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n, misalign", [(1, False), (7, False), (4099, False), (65536 * 3 + 5, False), (1001, True)])
def test_srk_kernels_equal_numpy_bit_for_bit(dtype, n, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    y0, a1, a2, b1, b2, b3, b4, g1, g2, g3 = ops = _operands(n, misalign, dtype, 10)
    Y, A1, A2, B1, B2, B3, B4, H1, H2, H3 = (x.cpu().numpy() for x in ops)
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s, c, c3 = float(SO.s_of(dt, T)), float(MO.c_of(dt, T)), float(KO.c3_of(dt, T))
    z, v = _draws(n, seed, k, dtype)
    # stage 1 (both draws), stage 2 (no generator)
    outs = [_like(y0, misalign) for _ in range(3)]
    be._sde_srk_stage1(*outs, y0, a1, b1, float(dt), s, seed, k)
    for o, want in zip(outs, KO.stage1(Y, A1, B1, dt, z, v, T)):
        assert np.array_equal(o.cpu().numpy(), want)
    G4 = _like(y0, misalign)
    be._sde_srk_stage2(G4, y0, a1, b1, b2, b3, float(dt), s)
    assert np.array_equal(G4.cpu().numpy(), KO.stage2(Y, A1, B1, B2, B3, dt, T))
    # the step, out of place and with y1 aliasing y0
    want = KO.srk_step(Y, A1, A2, B1, B2, B3, B4, dt, z, v, T)
    y1 = _like(y0, misalign)
    be._sde_srk_step(y1, y0, a1, a2, b1, b2, b3, b4, float(dt), s, c, c3, seed, k)
    assert np.array_equal(y1.cpu().numpy(), want)
    inplace = _like(y0, misalign)
    inplace.copy_(y0)
    be._sde_srk_step(inplace, inplace, a1, a2, b1, b2, b3, b4, float(dt), s, c, c3, seed, k)
    assert np.array_equal(inplace.cpu().numpy(), want)
    # the backwards: every group mask, the skipped outputs keep their fill
    _masked(lambda *o: be._sde_srk_stage1_backward(*o, g1, g2, g3, float(dt), s, seed, k), 3, ((0, 1), (1, 2), (2, 3)),
            KO.stage1_backward(H1, H2, H3, dt, z, v, T), g1, misalign, T)
    _masked(lambda *o: be._sde_srk_stage2_backward(*o, g1, float(dt), s), 4, ((0, 1), (1, 4)), KO.stage2_backward(H1, dt, T), g1, misalign, T)
    _masked(lambda *o: be._sde_srk_step_backward(*o, g1, float(dt), s, c, c3, seed, k), 6, ((0, 2), (2, 6)),
            KO.step_backward(H1, dt, z, v, T), g1, misalign, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_srk_kernels_past_the_grid_cap_equal_numpy_bit_for_bit(dtype):
    """The three forward kernels and the full backwards at _sde_oracle.wrap_n: the lanes wrap around the capped grid."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    n = SO.wrap_n(T)
    g = torch.Generator().manual_seed(6)
    y0, a1, a2, b1, b2, b3, b4 = ops = [torch.randn(n, generator=g, dtype=dtype).to(DEV) for _ in range(7)]
    Y, A1, A2, B1, B2, B3, B4 = (x.cpu().numpy() for x in ops)
    seed, k, dt = 0xC0FFEE, 3, T(0.0371)
    s, c, c3 = float(SO.s_of(dt, T)), float(MO.c_of(dt, T)), float(KO.c3_of(dt, T))
    z, v = _draws(n, seed, k, dtype)
    outs = [torch.empty_like(y0) for _ in range(6)]
    be._sde_srk_stage1(*outs[:3], y0, a1, b1, float(dt), s, seed, k)
    for o, want in zip(outs, KO.stage1(Y, A1, B1, dt, z, v, T)):
        assert np.array_equal(o.cpu().numpy(), want)
    be._sde_srk_stage2(outs[0], y0, a1, b1, b2, b3, float(dt), s)
    assert np.array_equal(outs[0].cpu().numpy(), KO.stage2(Y, A1, B1, B2, B3, dt, T))
    be._sde_srk_step(outs[0], y0, a1, a2, b1, b2, b3, b4, float(dt), s, c, c3, seed, k)
    assert np.array_equal(outs[0].cpu().numpy(), KO.srk_step(Y, A1, A2, B1, B2, B3, B4, dt, z, v, T))
    # (the operands stand in for the cotangents)
    be._sde_srk_stage1_backward(*outs[:3], a1, a2, b1, float(dt), s, seed, k)
    for o, want in zip(outs, KO.stage1_backward(A1, A2, B1, dt, z, v, T)):
        assert np.array_equal(o.cpu().numpy(), want)
    be._sde_srk_stage2_backward(*outs[:4], a1, float(dt), s)
    for o, want in zip(outs, KO.stage2_backward(A1, dt, T)):
        assert np.array_equal(o.cpu().numpy(), want)
    be._sde_srk_step_backward(*outs, a1, float(dt), s, c, c3, seed, k)
    for o, want in zip(outs, KO.step_backward(A1, dt, z, v, T)):
        assert np.array_equal(o.cpu().numpy(), want)


def test_a_zero_length_step_returns_y0_exactly():
    be = _hip.get_backend()
    n = 4099
    y0, a1, a2, b1, b2, b3, b4, gy = _operands(n, False, torch.float64, 8)
    outs = [torch.full_like(y0, SENTINEL) for _ in range(6)]
    be._sde_srk_stage1(*outs[:3], y0, a1, b1, 0.0, 0.0, 3, 2)
    be._sde_srk_stage2(outs[3], y0, a1, b1, b2, b3, 0.0, 0.0)
    be._sde_srk_step(outs[4], y0, a1, a2, b1, b2, b3, b4, 0.0, 0.0, 0.0, 0.0, 3, 2)
    for o in outs[:5]:
        assert torch.equal(o, y0)
    outs = [torch.full_like(y0, SENTINEL) for _ in range(6)]
    be._sde_srk_step_backward(*outs, gy, 0.0, 0.0, 0.0, 0.0, 3, 2)
    for o in outs:
        assert float(o.abs().max()) == 0.0
    outs = [torch.full_like(y0, SENTINEL) for _ in range(4)]
    be._sde_srk_stage2_backward(*outs, gy, 0.0, 0.0)
    for o in outs:
        assert float(o.abs().max()) == 0.0
    outs = [torch.full_like(y0, SENTINEL) for _ in range(3)]
    be._sde_srk_stage1_backward(*outs, gy, a1, a2, 0.0, 0.0, 3, 2)
    assert torch.equal(outs[0], (gy + a1) + a2) and float(outs[1].abs().max()) == 0.0 and float(outs[2].abs().max()) == 0.0


def test_sde_demo_loss_decreases_with_srk():
    """examples/sde_demo.py trained through sdeint(SRK): the bar of the Euler and Milstein demo tests."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sde_demo

    losses = sde_demo.train(max_steps=120, solver=SRK, log_every=0)
    head, tail = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    assert tail < 0.9 * head, (head, tail)
