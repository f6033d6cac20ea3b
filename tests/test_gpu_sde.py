"""sdeint on the GPU: the generator against tests/_sde_oracle.py (Philox words bit for bit, normals within the math library's error
bound of DESIGN section 10), the statistics of its normals, xde_sde_em_step / xde_sde_em_backward against numpy on the read-back Z, the
end-to-end cases of tests/_sde_cases.py with the HIP backend, the moments of an Ornstein-Uhlenbeck recursion, the strong order of
Euler-Maruyama, and the SDE demo."""
import os
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler

from . import _sde_oracle as SO
from ._sde_cases import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
_EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}
SENTINEL = 7.0


@pytest.fixture
def dev():
    return DEV


def _noise(n, seed, k, dtype):
    out = torch.empty(n, dtype=dtype, device=DEV)
    _hip.get_backend()._sde_noise(out, seed, k)
    return out


# ----------------------------------------------------------------------------------------------
# the generator
# ----------------------------------------------------------------------------------------------
def test_philox_words_equal_the_oracle_bit_for_bit():
    be = _hip.get_backend()
    rng = np.random.RandomState(0)
    seeds = [0, 1, (1 << 64) - 1, 0xFFFFFFFF, 1 << 32] + [int(rng.randint(0, 1 << 62)) * 4 + int(rng.randint(0, 4)) for _ in range(27)]
    for i, seed in enumerate(seeds):
        for k in (0, 1, 7, (1 << 32) - 1):
            n = (1, 3, 4, 5, 1023, 4097, 65537)[(i + k) % 7]
            out = torch.empty(n, dtype=torch.int32, device=DEV)
            be._sde_noise(out, seed, k, bits=True)
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, SO.words(-(-n // 4), seed, k).reshape(-1)[:n]), (seed, k, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_normals_are_the_oracles_within_the_math_library_bound(dtype):
    """|Z_gpu - Z_ref| <= eps * (13 |Z_ref| + 4 r), eps = 2^-24 (fp32) / 2^-53 (fp64), r = sqrt(-2 log u1)."""
    eps = _EPS[dtype]
    for seed, k, n in ((3, 0, 1 << 20), (0xDEADBEEF12345678, 5, (1 << 20) + 3), ((1 << 64) - 1, 123456, 1001)):
        got = _noise(n, seed, k, dtype).cpu().numpy().astype(np.float64)
        ref, r = SO.normals(n, seed, k, _NPT[dtype], with_r=True)
        err = np.abs(got - ref)
        bound = eps * (13.0 * np.abs(ref) + 4.0 * r)
        worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (seed, k, worst, got[worst], ref[worst], err[worst] / eps)
        assert np.abs(got).max() <= (5.77 if dtype == torch.float32 else 8.58)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_statistics_of_2_24_normals(dtype):
    N = 1 << 24
    z = _noise(N, 2024, 3, dtype).double()
    m = z.mean()
    c = z - m
    var = (c * c).mean()
    skew = (c**3).mean() / var**1.5
    kurt = (c**4).mean() / var**2 - 3.0
    se = lambda v: 5.0 * (v / N) ** 0.5  # noqa: E731  (5 standard errors of a moment of N independent normals)
    assert abs(float(m)) < se(1.0), float(m)
    assert abs(float(var) - 1.0) < se(2.0), float(var)
    assert abs(float(skew)) < se(6.0), float(skew)
    assert abs(float(kurt)) < se(24.0), float(kurt)

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return float((a * b).mean() / ((a * a).mean() * (b * b).mean()).sqrt())

    assert abs(corr(z[:-1], z[1:])) < se(1.0)  # neighbouring elements (the two normals of one Box-Muller pair among them)
    assert abs(corr(z[0::2], z[1::2])) < 5.0 * (2.0 / N) ** 0.5  # the pairs themselves
    assert abs(corr(z, _noise(N, 2024, 4, dtype).double())) < se(1.0)  # step k against step k + 1
    assert abs(corr(z, _noise(N, 2025, 3, dtype).double())) < se(1.0)  # two seeds


# ----------------------------------------------------------------------------------------------
# the step kernels against numpy on the read-back Z
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n, misalign", [(1, False), (7, False), (4099, False), (65536 * 3 + 5, False), (1001, True)])
def test_em_step_and_backward_equal_numpy_bit_for_bit(dtype, n, misalign):
    be = _hip.get_backend()
    T = _NPT[dtype]
    g = torch.Generator().manual_seed(n)
    ops = []
    for _ in range(5):
        x = torch.randn(n + 1, generator=g, dtype=dtype).to(DEV)
        ops.append(x[1:] if misalign else x[:-1])  # (misaligned: the scalar path)
    y0, f, gg_in, gy = ops[0], ops[1], ops[2], ops[3]
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s = SO.s_of(dt, T)
    z = _noise(n, seed, k, dtype).cpu().numpy()
    y1 = torch.empty_like(y0)
    be._sde_em_step(y1, y0, f, gg_in, float(dt), float(s), seed, k)
    Y0, F, G, GY = (x.cpu().numpy() for x in (y0, f, gg_in, gy))
    want = (Y0 + F * dt) + G * (s * z)
    assert np.array_equal(y1.cpu().numpy(), want)
    inplace = y0.clone()
    be._sde_em_step(inplace, inplace, f, gg_in, float(dt), float(s), seed, k)
    assert np.array_equal(inplace.cpu().numpy(), want)
    gf, gg = torch.empty_like(gy), torch.empty_like(gy)
    be._sde_em_backward(gf, gg, gy, float(dt), float(s), seed, k)
    assert np.array_equal(gf.cpu().numpy(), GY * dt) and np.array_equal(gg.cpu().numpy(), GY * (s * z))
    only = torch.full_like(gy, 7.0)
    be._sde_em_backward(None, only, gy, float(dt), float(s), seed, k)
    assert np.array_equal(only.cpu().numpy(), GY * (s * z))
    only = torch.full_like(gy, 7.0)
    be._sde_em_backward(only, None, gy, float(dt), float(s), seed, k)
    assert np.array_equal(only.cpu().numpy(), GY * dt)


def _like(x, misalign):
    """A sentinel-filled output with x's alignment."""
    o = torch.full((x.numel() + 1,), SENTINEL, dtype=x.dtype, device=DEV)
    return o[1:] if misalign else o[:-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n, misalign", [(7, False), (1001, True)])
def test_em_backward_writes_exactly_the_outputs_it_is_given(dtype, n, misalign):
    """Every output mask, with the outputs misaligned as well as the cotangent: a skipped output goes in as null, and a buffer standing
    for it keeps its fill."""
    be = _hip.get_backend()
    T = _NPT[dtype]
    x = torch.randn(n + 1, generator=torch.Generator().manual_seed(n), dtype=dtype).to(DEV)
    gy = x[1:] if misalign else x[:-1]
    seed, k, dt = 0x5EED, 17, T(-0.0123)
    s = SO.s_of(dt, T)
    GY = gy.cpu().numpy()
    wants = (GY * dt, GY * (s * _noise(n, seed, k, dtype).cpu().numpy()))
    for mask in ((1, 1), (1, 0), (0, 1)):
        outs = [_like(gy, misalign) for _ in range(2)]
        be._sde_em_backward(*[o if m else None for o, m in zip(outs, mask)], gy, float(dt), float(s), seed, k)
        for o, m, want in zip(outs, mask, wants):
            assert np.array_equal(o.cpu().numpy(), want if m else np.full(n, T(SENTINEL))), mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_em_kernels_past_the_grid_cap_equal_numpy_bit_for_bit(dtype):
    be = _hip.get_backend()
    T = _NPT[dtype]
    n = SO.wrap_n(_NPT[dtype])
    g = torch.Generator().manual_seed(5)
    y0, f, gd, gy = (torch.randn(n, generator=g, dtype=dtype).to(DEV) for _ in range(4))
    seed, k, dt = 0xC0FFEE, 3, T(0.0371)
    s = SO.s_of(dt, T)
    z = _noise(n, seed, k, dtype).cpu().numpy()
    Y0, F, G, GY = (x.cpu().numpy() for x in (y0, f, gd, gy))
    y1 = torch.empty_like(y0)
    be._sde_em_step(y1, y0, f, gd, float(dt), float(s), seed, k)
    assert np.array_equal(y1.cpu().numpy(), (Y0 + F * dt) + G * (s * z))
    gf, gg = torch.empty_like(gy), torch.empty_like(gy)
    be._sde_em_backward(gf, gg, gy, float(dt), float(s), seed, k)
    assert np.array_equal(gf.cpu().numpy(), GY * dt) and np.array_equal(gg.cpu().numpy(), GY * (s * z))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_noise_of_an_element_does_not_depend_on_the_launch_shape(dtype):
    """The Z that the EM step implies, ``y1 - (y0 + f*dt)`` with g = 1 and s = 1 (so s*Z is Z), is xde_sde_noise's at the same
    (seed, k), element for element, at the size where the step's lanes wrap around the grid: the step kernel's loop index is the
    generator's counter.  y0 and f are zero, so that ``(y0 + f*dt) + Z`` rounds nothing away and the difference is Z exactly."""
    be = _hip.get_backend()
    n = SO.wrap_n(_NPT[dtype])
    seed, k, dt = 0xC0FFEE, 9, 0.0371
    y0, f = torch.zeros(n, dtype=dtype, device=DEV), torch.zeros(n, dtype=dtype, device=DEV)
    y1 = torch.empty_like(y0)
    be._sde_em_step(y1, y0, f, torch.ones_like(y0), dt, 1.0, seed, k)
    implied = y1.cpu().numpy() - (y0.cpu().numpy() + f.cpu().numpy() * _NPT[dtype](dt))
    assert np.array_equal(implied, _noise(n, seed, k, dtype).cpu().numpy())


# ----------------------------------------------------------------------------------------------
# what the recursion should do
# ----------------------------------------------------------------------------------------------
def test_ornstein_uhlenbeck_moments_are_the_em_recursions():
    """dX = -theta X dt + sigma dW, 2^20 paths: EM gives X_N = a^N x0 + sigma sqrt(h) sum_j a^(N-1-j) Z_j with a = 1 - theta h,
    so mean x0 a^N and variance sigma^2 h sum_j a^(2j) exactly — no discretisation bias to allow for."""
    M, theta, sigma, x0, N = 1 << 20, 1.5, 0.8, 1.0, 40
    h = 1.0 / 32
    t = torch.arange(N + 1, dtype=torch.float64) * h
    y0 = torch.full((1, M), x0, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        sol = sdeint(lambda t_, y: -theta * y, lambda t_, y: torch.full_like(y, sigma), y0, t, solver=Euler,
                     options={"norm": None, "seed": 99})
    xT = sol[-1]
    a = 1.0 - theta * h
    mean, var = x0 * a**N, sigma**2 * h * sum(a ** (2 * j) for j in range(N))
    m, v = float(xT.mean()), float(xT.var())
    assert abs(m - mean) < 5.0 * (var / M) ** 0.5, (m, mean)
    assert abs(v - var) < 5.0 * var * (2.0 / (M - 1)) ** 0.5, (v, var)


def test_strong_order_one_half_on_geometric_brownian_motion():
    """dX = lam X dt + mu X dW on [0, 1], X0 = 1, 2^16 paths, h = 2^-3 .. 2^-8: W_T from sdeint(0, 1) with the same seed and grid, the
    exact solution exp((lam - mu^2/2) T + mu W_T); the slope of log E|X_EM - X| against log h lies in [0.4, 0.6]."""
    lam, mu, M, seed = 2.0, 1.0, 1 << 16, 11
    hs, errs = [], []
    ones = torch.ones(1, M, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        for p in range(3, 9):
            N = 2**p
            t = torch.arange(N + 1, dtype=torch.float64) / N
            o = {"norm": None, "seed": seed}
            W = sdeint(lambda t_, y: torch.zeros_like(y), lambda t_, y: torch.ones_like(y), torch.zeros_like(ones), t, solver=Euler,
                       options=o)[-1]
            X = sdeint(lambda t_, y: lam * y, lambda t_, y: mu * y, ones, t, solver=Euler, options=o)[-1]
            exact = torch.exp((lam - 0.5 * mu * mu) * 1.0 + mu * W)
            hs.append(1.0 / N)
            errs.append(float((X - exact).abs().mean()))
    slope = float(np.polyfit(np.log(hs), np.log(errs), 1)[0])
    assert 0.4 <= slope <= 0.6, (slope, errs)


def test_sde_demo_loss_decreases():
    """examples/sde_demo.py (counterpart of the reference's example/sde_demo.py): MLP drift and diffusion trained through sdeint(Euler)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sde_demo

    losses = sde_demo.train(max_steps=120, log_every=0)
    head, tail = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    assert tail < 0.9 * head, (head, tail)
