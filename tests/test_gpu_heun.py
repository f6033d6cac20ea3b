"""Heun on the GPU: xde_sde_gn_heun_predict / _correct / _backward against the header's formulas in numpy on the read-back Z, bit for bit;
the walk of sdeint(..., solver=Heun) under every noise type; its gradients against framework ops; and that it is Stratonovich."""
import itertools

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler, Heun
from paddlexde_amd.solver.base_fixed_solver import step_size_grid

from . import _gn_oracle as GN
from . import _sde_cases as SC
from . import _sde_oracle as SO
from ._gn_cases import Coeffs, gn_noise
from .test_gpu_gn import DEV, Guarded, _noise, _operands

pytestmark = pytest.mark.gpu
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SHAPES = [(1, 1, 1), (2, 5, 3), (3, 7, 8), (1, 2, 67), (2, 300, 5), (300, 1, 3), (257, 6, 2)]
SEED, K = 0x5EED, 17
on_shapes = pytest.mark.parametrize("dtype, misalign, rows, D, M", [(d, a) + shape for d in _NPT for a in (False, True) for shape in SHAPES])


@on_shapes
def test_predict_and_correct_equal_numpy_bit_for_bit(dtype, rows, D, M, misalign):
    be, T = _hip.get_backend(), _NPT[dtype]
    y0, f0, g0, f1 = _operands(rows, D, M, dtype, misalign)
    g1 = Guarded((rows, D, M), dtype, misalign, fill=torch.cos(g0)).view
    Y0, F0, G0, F1, G1 = before = [x.cpu().numpy() for x in (y0, f0, g0, f1, g1)]
    z, half = _noise(rows, M, SEED, K, dtype), T(0.5)
    for dt in (T(0.0123), T(-0.0123), T(0.0)):
        s = SO.s_of(dt, T)
        w = GN.increments(z, s, T)
        a, b = GN.matvec(G0, w, T), GN.matvec(G1, w, T)
        want_p, want_1 = (Y0 + F0 * dt) + a, (Y0 + (F0 + F1) * (half * dt)) + (a + b) * half
        yp, a0, y1, inplace = (Guarded((rows, D), dtype, misalign, fill=fill) for fill in (None, None, None, y0))
        be._sde_gn_heun_predict(yp.view, a0.view, y0, f0, g0, float(dt), float(s), SEED, K)
        assert np.array_equal(yp.view.cpu().numpy(), want_p) and np.array_equal(a0.view.cpu().numpy(), a), float(dt)
        again = [torch.empty_like(y0) for _ in range(3)]
        be._sde_gn_step(again[0], y0, f0, g0, float(dt), float(s), SEED, K)
        assert torch.equal(yp.view, again[0]) and want_p.dtype == want_1.dtype == T
        be._sde_gn_heun_correct(y1.view, y0, f0, f1, a0.view, g1, float(dt), float(s), SEED, K)
        be._sde_gn_heun_correct(inplace.view, inplace.view, f0, f1, a0.view, g1, float(dt), float(s), SEED, K)
        assert np.array_equal(y1.view.cpu().numpy(), want_1) and torch.equal(inplace.view, y1.view), float(dt)
        assert all(x.guards_intact() for x in (yp, a0, y1, inplace))
        again[0].zero_()  # (two launches, the same bits)
        be._sde_gn_heun_predict(again[0], again[1], y0, f0, g0, float(dt), float(s), SEED, K)
        be._sde_gn_heun_correct(again[2], y0, f0, f1, again[1], g1, float(dt), float(s), SEED, K)
        assert all(torch.equal(x, y.view) for x, y in zip(again, (yp, a0, y1)))
    assert all(np.array_equal(x.cpu().numpy(), want) for x, want in zip((y0, f0, g0, f1, g1), before))  # the operands kept their bits


@on_shapes
def test_backward_equals_numpy_bit_for_bit_for_every_mask(dtype, rows, D, M, misalign):
    """Both uses, (cf, ca) = (dt/2, 1/2) and (dt, 1), with gc absent and present and with gy absent, for every mask of null outputs, at
    every dt (dt = 0: s = 0, so gg is signed zeros, which compare equal to numpy's)."""
    be, T = _hip.get_backend(), _NPT[dtype]
    _, gc, _, gy = _operands(rows, D, M, dtype, misalign)
    GY, GC = gy.cpu().numpy(), gc.cpu().numpy()
    for dt in (T(0.0123), T(-0.0123), T(0.0)):
        s = SO.s_of(dt, T)
        w = GN.increments(_noise(rows, M, SEED, K, dtype), s, T)
        for (cf, ca), (has_gy, has_gc) in itertools.product(((T(0.5) * dt, T(0.5)), (dt, T(1.0))), ((1, 0), (1, 1), (0, 1))):
            h = GY * ca
            c = ((h + GC) if has_gc else h) if has_gy else GC
            wants = (GY * cf, h, c[..., :, None] * w[..., None, :])
            for mask in itertools.product((1, 0), repeat=3):
                if not has_gy and (mask[0] or mask[1]):
                    continue
                outs = [Guarded(shape, dtype, misalign) for shape in ((rows, D), (rows, D), (rows, D, M))]
                be._sde_gn_heun_backward(*[o.view if m else None for o, m in zip(outs, mask)], gy if has_gy else None, gc if has_gc else None, M,
                                         float(cf), float(ca), float(s), SEED, K)
                for o, m, want in zip(outs, mask, wants):  # (a written output is the formula inside intact guards, a skipped one keeps its fill)
                    assert (np.array_equal(o.view.cpu().numpy(), want) and o.guards_intact()) if m else o.untouched(), (mask, has_gy, has_gc, float(ca))


def _heun_states(noise_type, co, y0, grid, seed, dtype):
    """The walk's states on ``grid``: the header's formulas in numpy; diagonal noise: the two existing launches called directly."""
    be, T = _hip.get_backend(), _NPT[dtype]
    y = y0.clone() if noise_type == "diagonal" else y0.cpu().numpy()
    out = [y]
    for k in range(len(grid) - 1):
        t0, t1, dt = grid[k], grid[k + 1], grid[k + 1] - grid[k]
        s = SO.s_of(dt, T)
        if noise_type == "diagonal":
            f0, g0, yp, y1 = SC.drift(t0, y), SC.diffusion(t0, y), torch.empty_like(y), torch.empty_like(y)
            be._sde_em_step(yp, y, f0, g0, float(dt), float(s), seed, k)
            be._sde_rheun_correct(y1, y, f0, SC.drift(t1, yp), g0, SC.diffusion(t1, yp), float(dt), float(s), 1, seed, k)
            y = y1
        else:
            w = GN.increments(gn_noise(tuple(y0.shape), co.M, seed, k, dtype, DEV), s, T)
            f0, a = SC.drift(t0, y), GN.matvec(co.diffusion_np(t0, y), w, T)
            yp = (y + f0 * dt) + a
            y = (y + (f0 + SC.drift(t1, yp)) * (T(0.5) * dt)) + (a + GN.matvec(co.diffusion_np(t1, yp), w, T)) * T(0.5)
        out.append(y)
    return np.stack([x.cpu().numpy() if torch.is_tensor(x) else x for x in out])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("noise_type, M", [("general", 3), ("scalar", 1), ("diagonal", None)])
def test_walk_equals_its_statement_bit_for_bit(dtype, noise_type, M):
    t_np = np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0], dtype=_NPT[dtype])
    grid, y0, seed, co = step_size_grid(t_np, 0.1), SC._y0(dtype, DEV, shape=(4, 5)), 0x1234_5678_9ABC_DEF0, Coeffs(5, M or 1, dtype, DEV)
    with torch.no_grad():
        sol = sdeint(SC.drift, co.diffusion if M else SC.diffusion, y0, torch.as_tensor(t_np), solver=Heun,
                     options=SC._opts(seed=seed, noise_type=noise_type, step_size=0.1, interp="linear"))
    want = SO.layout(SO.rows_at(_heun_states(noise_type, co, y0, grid, seed, dtype), grid, t_np))
    assert sol.shape == (6 * 4, 5) and sol.dtype == dtype and np.array_equal(sol.cpu().numpy(), want)


def test_gradients_equal_the_walk_in_framework_ops():
    """d ys.sum() / d (y0, the diffusion's matrix, the drift's scalar) through the HIP nodes against autograd through the same walk in
    framework ops: they differ by the order of autograd's accumulation only, so the bar is 64 ulp on each gradient's largest magnitude."""
    dtype, M, seed = torch.float64, 2, 11
    t_np = np.array([0.0, 0.2, 0.35, 0.6, 1.0])
    y0, P, lam = leaves = [x.requires_grad_(True) for x in (SC._y0(dtype, DEV, shape=(2, 3)), Coeffs(3, M, dtype, DEV).p.clone(),
                                                            torch.tensor(-0.75, dtype=dtype, device=DEV))]
    drift, diffusion = (lambda t, y: y * lam + (y * y) * 0.125), (lambda t, y: y.unsqueeze(-1) * P + 0.25)
    sol = sdeint(drift, diffusion, y0, torch.as_tensor(t_np), solver=Heun, options=SC._opts(seed=seed, noise_type="general"))
    got = torch.autograd.grad(sol.sum(), leaves)
    y, rows = y0, [y0]
    for k in range(len(t_np) - 1):
        dt = t_np[k + 1] - t_np[k]
        w = torch.as_tensor(GN.increments(gn_noise((2, 3), M, seed, k, dtype, DEV), SO.s_of(dt, np.float64), np.float64)).to(DEV)
        mv = lambda g: g[..., 0] * w[..., 0:1] + g[..., 1] * w[..., 1:2]  # noqa: E731
        f0, a = drift(None, y), mv(diffusion(None, y))
        yp = (y + f0 * float(dt)) + a
        y = (y + (f0 + drift(None, yp)) * (0.5 * float(dt))) + (a + mv(diffusion(None, yp))) * 0.5
        rows.append(y)
    ref = torch.cat(rows, dim=-2)
    want = torch.autograd.grad(ref.sum(), leaves)
    gaps = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
    print("heun gradients against framework ops, relative to the largest magnitude (y0, P, lam):", gaps)
    assert torch.equal(sol.detach(), ref.detach()) and all(float(b.abs().max()) > 0 for b in want) and max(gaps) <= 64 * np.finfo(np.float64).eps, gaps


def test_heun_is_stratonovich_and_euler_is_ito():
    """dy = a y dt + y (b1 o dW1 + b2 o dW2), y0 = 1: the Stratonovich solution is exp(a T + b.W(T)), the Ito solution a factor e^0.5 below
    (|b| = 1).  Heun's mean relative error is the smaller to the first, Euler's on the same seed to the second."""
    dtype, n, steps, a, seed = torch.float64, 1024, 256, 0.5, 2024
    b, t = torch.tensor([0.6, 0.8], dtype=dtype, device=DEV), torch.linspace(0.0, 1.0, steps + 1, dtype=dtype)
    W = sum(GN.increments(gn_noise((n, 1), 2, seed, k, dtype, DEV), SO.s_of(1.0 / steps, np.float64), np.float64) for k in range(steps))
    strat, ito, err = np.exp(a + W @ b.cpu().numpy()), np.exp(a - 0.5 + W @ b.cpu().numpy()), {}
    for solver in (Heun, Euler):
        with torch.no_grad():
            sol = sdeint(lambda t_, y: y * a, lambda t_, y: y.unsqueeze(-1) * b, torch.ones(n, 1, dtype=dtype, device=DEV), t, solver=solver,
                         options=SC._opts(seed=seed, noise_type="general"))
        y = sol[-n:, 0].cpu().numpy()
        err[solver] = (float(np.mean(np.abs(y - strat) / strat)), float(np.mean(np.abs(y - ito) / ito)))
    print("mean relative error to (Stratonovich, Ito): Heun", err[Heun], "Euler", err[Euler])
    assert err[Heun][0] < err[Heun][1] and err[Euler][1] < err[Euler][0]
