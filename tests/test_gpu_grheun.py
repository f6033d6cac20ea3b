"""GeneralReversibleHeun on the GPU: the four xde_sde_gn_rheun_* entry points against the header's formulas in numpy on the read-back Z, bit
for bit; the walk on its two routes; sdeint_adjoint's matrix-noise sweep against autograd through the recursion; and its memory."""
import importlib

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint, sdeint_adjoint
from paddlexde_amd.solver import GeneralReversibleHeun, ReversibleHeun
from paddlexde_amd.solver.base_fixed_solver import _SubSteps, step_size_grid

from . import _gn_oracle as GN
from . import _sde_cases as SC
from . import _sde_oracle as SO
from ._gn_cases import Coeffs, gn_noise
from .test_gpu_gn import DEV, Guarded, _noise, _operands

ADJ = importlib.import_module("paddlexde_amd.functional.sdeint_adjoint")  # (the package attribute of that name is the function)
pytestmark = pytest.mark.gpu
_NPT = {torch.float32: np.float32, torch.float64: np.float64}
SHAPES = [(1, 1, 1), (3, 5, 2), (1, 2, 67), (2, 300, 5), (257, 6, 2)]
SEED, K = 0x5EED, 17
on_shapes = pytest.mark.parametrize("dtype, misalign, rows, D, M", [(d, a) + shape for d in _NPT for a in (False, True) for shape in SHAPES])
np_ = lambda x: x.cpu().numpy()  # noqa: E731


@on_shapes
def test_predict_and_seam_equal_their_statements_bit_for_bit(dtype, rows, D, M, misalign):
    """(dt, s) forward, reversed (both negated) and zero; the seam with k1 = k0 + 1 and k0 - 1 and dt1 != dt0, out of place and in place."""
    be, T = _hip.get_backend(), _NPT[dtype]
    y0, f0, g0, f1 = _operands(rows, D, M, dtype, misalign)
    yh0, g1 = Guarded((rows, D), dtype, misalign, fill=torch.sin(y0)).view, Guarded((rows, D, M), dtype, misalign, fill=torch.cos(g0)).view
    Y0, F0, G0, F1, YH0, G1 = before = [np_(x) for x in (y0, f0, g0, f1, yh0, g1)]
    for sign, k1 in ((1, K + 1), (-1, K - 1), (0, K + 1)):
        dt0, dt1 = T(sign * 0.0123), T(sign * 0.0371)
        s0, s1 = T(sign) * SO.s_of(dt0, T), T(sign) * SO.s_of(dt1, T)
        a = GN.matvec(G0, GN.increments(_noise(rows, M, SEED, K, dtype), s0, T), T)
        yh1, a0 = Guarded((rows, D), dtype, misalign), Guarded((rows, D), dtype, misalign)
        be._sde_gn_rheun_predict(yh1.view, a0.view, y0, yh0, f0, g0, float(dt0), float(s0), SEED, K)
        assert np.array_equal(np_(yh1.view), (((Y0 + Y0) - YH0) + F0 * dt0) + a) and np.array_equal(np_(a0.view), a), sign
        ref = [torch.empty_like(y0) for _ in range(3)]  # the two launches the seam stands for
        be._sde_gn_heun_correct(ref[0], y0, f0, f1, a0.view, g1, float(dt0), float(s0), SEED, K)
        be._sde_gn_rheun_predict(ref[1], ref[2], ref[0], yh1.view, f1, g1, float(dt1), float(s1), SEED, k1)
        a1 = GN.matvec(G1, GN.increments(_noise(rows, M, SEED, k1, dtype), s1, T), T)
        assert np.array_equal(np_(ref[2]), a1) and np.array_equal(np_(ref[1]), (((np_(ref[0]) + np_(ref[0])) - np_(yh1.view)) + F1 * dt1) + a1)
        for first in (None, y0):  # (y1 apart from y0, then y1 = y0)
            outs = [Guarded((rows, D), dtype, misalign, fill=fill) for fill in (first, None, None)]
            be._sde_gn_rheun_seam(*[o.view for o in outs], outs[0].view if first is not None else y0, f0, f1, a0.view, yh1.view, g1, float(dt0),
                                  float(s0), K, float(dt1), float(s1), k1, SEED)
            assert all(torch.equal(o.view, r) and o.guards_intact() for o, r in zip(outs, ref)), (sign, first is not None)
        assert yh1.guards_intact() and a0.guards_intact()
    assert all(np.array_equal(np_(x), want) for x, want in zip((y0, f0, g0, f1, yh0, g1), before))  # the operands kept their bits


@on_shapes
def test_adjoint_stage_and_step_equal_numpy_bit_for_bit(dtype, rows, D, M, misalign):
    be, T = _hip.get_backend(), _NPT[dtype]
    ay, af, _, c = _operands(rows, D, M, dtype, misalign)
    ayh, v = Guarded((rows, D), dtype, misalign, fill=torch.sin(ay)).view, Guarded((rows, D), dtype, misalign, fill=torch.cos(af)).view
    AY, AF, C, AYH, V = [np_(x) for x in (ay, af, c, ayh, v)]
    half = T(0.5)
    for dt in (T(0.0123), T(-0.0123), T(0.0)):
        s0, s1 = SO.s_of(dt, T), SO.s_of(T(3) * dt, T)
        w0, w1 = (GN.increments(_noise(rows, M, SEED, k, dtype), s, T) for k, s in ((K, s0), (K + 1, s1)))
        outer = lambda x, w: x[..., :, None] * w[..., None, :]  # noqa: E731
        # the full form out of place and with bf = af1; the first backward step (af1, c1 null); the tail (ay1 null: no bf)
        for (has_f, has_c, has_ay), inplace in (((1, 1, 1), False), ((1, 1, 1), True), ((0, 0, 1), False), ((0, 1, 0), False)):
            want_g = (outer(C, w1) + outer(AY * half, w0)) if has_c and has_ay else (outer(C, w1) if has_c else outer(AY * half, w0))
            want_f = (AF + AY * (half * dt)) if has_f else AY * (half * dt)
            bf, bg = Guarded((rows, D), dtype, misalign, fill=af if inplace else None), Guarded((rows, D, M), dtype, misalign)
            be._sde_gn_rheun_adjoint_stage(bf.view if has_ay else None, bg.view, (bf.view if inplace else af) if has_f else None, c if has_c else None,
                                           ay if has_ay else None, float(dt), float(s0), K, float(s1), K + 1, SEED)
            assert np.array_equal(np_(bg.view), want_g) and bg.guards_intact(), (float(dt), has_f, has_c, has_ay)
            assert (np.array_equal(np_(bf.view), want_f) and bf.guards_intact()) if has_ay else bf.untouched()
        for has_h, inplace in ((1, False), (1, True), (0, False), (0, True)):
            A = (AYH + V) if has_h else V
            wants = (AY + (A + A), -A, AY * (half * dt) + A * dt, AY * half + A)
            outs = [Guarded((rows, D), dtype, misalign, fill=fill if inplace else None) for fill in (ay, ayh, None, None)]
            be._sde_gn_rheun_adjoint_step(*[o.view for o in outs], outs[0].view if inplace else ay,
                                          (outs[1].view if inplace else ayh) if has_h else None, v, float(dt))
            assert all(np.array_equal(np_(o.view), want) and o.guards_intact() for o, want in zip(outs, wants)), (float(dt), has_h, inplace)
    assert all(np.array_equal(np_(x), want) for x, want in zip((ay, af, c, ayh, v), (AY, AF, C, AYH, V)))


def _states(co, y0, grid, seed, dtype):
    """The walk's states on ``grid``: the header's formulas in numpy."""
    T, half = _NPT[dtype], _NPT[dtype](0.5)
    y = yh = np_(y0)
    f, g, out = SC.drift(grid[0], y), co.diffusion_np(grid[0], y), [y]
    for k in range(len(grid) - 1):
        dt = grid[k + 1] - grid[k]
        w = GN.increments(gn_noise(tuple(y0.shape), co.M, seed, k, dtype, DEV), SO.s_of(dt, T), T)
        a = GN.matvec(g, w, T)
        yh1 = (((y + y) - yh) + f * dt) + a
        f1, g1 = SC.drift(grid[k + 1], yh1), co.diffusion_np(grid[k + 1], yh1)
        y = (y + (f + f1) * (half * dt)) + (a + GN.matvec(g1, w, T)) * half
        yh, f, g = yh1, f1, g1
        out.append(y)
    return np.stack(out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("step_size", [None, 0.1])
@pytest.mark.parametrize("noise_type, M", [("general", 3), ("scalar", 1), ("diagonal", None)])
def test_walk_on_both_routes_equals_its_statement_bit_for_bit(dtype, noise_type, M, step_size, monkeypatch):
    t_np = np.array([0.0, 0.13, 0.4, 0.4, 0.75, 1.0], dtype=_NPT[dtype])
    grid = t_np if step_size is None else step_size_grid(t_np, step_size)
    y0, seed, co = SC._y0(dtype, DEV, shape=(4, 5)), 0x1234_5678_9ABC_DEF0, Coeffs(5, M or 1, dtype, DEV)
    o = SC._opts(seed=seed, noise_type=noise_type, **({} if step_size is None else dict(step_size=step_size, interp="linear")))
    be, calls = _hip.get_backend(), []
    for name in ("_sde_gn_rheun_predict", "_sde_gn_rheun_seam", "_sde_gn_heun_correct"):
        monkeypatch.setattr(be, name, lambda *a, _f=getattr(be, name), _n=name: (calls.append(_n), _f(*a))[1])
    solve = lambda cls, y: sdeint(SC.drift, co.diffusion if M else SC.diffusion, y, torch.as_tensor(t_np), solver=cls, options=o)  # noqa: E731
    with torch.no_grad():
        sol = solve(GeneralReversibleHeun, y0)
    seam_calls, n = list(calls), len(grid) - 1
    through = solve(GeneralReversibleHeun, y0.clone().requires_grad_(True))
    assert sol.shape == (6 * 4, 5) and sol.dtype == dtype and torch.equal(sol, through.detach())
    if M is None:
        with torch.no_grad():
            assert torch.equal(sol, solve(ReversibleHeun, y0)) and not calls
        return
    assert np.array_equal(np_(sol), SO.layout(SO.rows_at(_states(co, y0, grid, seed, dtype), grid, t_np)))
    # one matrix launch per interior step on the seam route, two per step on the other
    assert seam_calls == ["_sde_gn_rheun_predict"] + ["_sde_gn_rheun_seam"] * (n - 1) + ["_sde_gn_heun_correct"]
    assert calls[len(seam_calls):] == ["_sde_gn_rheun_predict", "_sde_gn_heun_correct"] * n


def _sweep_np(Y0, lam, P, w, dts, rows, n_out, W):
    """The sweep restated in numpy float64 for drift y*lam and diffusion y[.., None]*P + 0.25: the forward, then reconstruction and
    cotangent recursion with the analytic vjp.  ``rows[k]``: (j, weight of the step's end) of the outputs step k produces; ``W``:
    [n_out, *Y0.shape] cotangents.  Returns (grad_y0, grad_lam, grad_P, y0 as reconstructed)."""
    mv = lambda g, wk: np.einsum("...dm,...m->...d", g, wk)  # noqa: E731
    drift, diff = (lambda y: y * lam), (lambda y: y[..., None] * P + 0.25)
    n, y, yh = len(dts), Y0, Y0
    for k in range(n):
        a = mv(diff(yh), w[k])
        yh1 = 2 * y - yh + drift(yh) * dts[k] + a
        y, yh = y + (drift(yh) + drift(yh1)) * (0.5 * dts[k]) + (a + mv(diff(yh1), w[k])) * 0.5, yh1
    a_y, a_yh, a_f, c, g_lam, g_P = np.zeros_like(Y0), np.zeros_like(Y0), np.zeros_like(Y0), np.zeros_like(Y0), 0.0, np.zeros_like(P)

    def vjp(yh, bf, bg):
        return bf * lam + (bg * P).sum(-1), (bf * yh).sum(), (bg * yh[..., None]).sum(axis=tuple(range(Y0.ndim - 1)))

    for k in range(n - 1, -1, -1):
        for j, wb in rows[k]:
            a_y = a_y + W[j] * wb
        bf = a_f + a_y * (0.5 * dts[k])
        bg = c[..., None] * (w[k + 1][..., None, :] if k + 1 < n else 0.0) + (0.5 * a_y)[..., None] * w[k][..., None, :]
        v, dl, dP = vjp(yh, bf, bg)
        g_lam, g_P, A = g_lam + dl, g_P + dP, a_yh + v
        a_y, a_yh, a_f, c = a_y + 2 * A, -A, a_y * (0.5 * dts[k]) + A * dts[k], a_y * 0.5 + A
        yh0 = 2 * y - yh - drift(yh) * dts[k] - mv(diff(yh), w[k])
        y, yh = y - (drift(yh) + drift(yh0)) * (0.5 * dts[k]) - (mv(diff(yh), w[k]) + mv(diff(yh0), w[k])) * 0.5, yh0
        for j, wb in rows[k]:
            a_y = a_y + W[j] * (1.0 - wb)
    v, dl, dP = vjp(yh, a_f, c[..., None] * w[0][..., None, :])
    return a_y + a_yh + v + W[0], g_lam + dl, g_P + dP, y


@pytest.mark.parametrize("step_size", [None, 0.05])
def test_adjoint_equals_the_gradient_through_the_steps(step_size):
    """Gradients of sum(sol * W) with respect to (y0, lam, P): through the HIP nodes within 64 ulp of autograd through the recursion in
    framework ops, relative to each gradient's largest magnitude; the adjoint, and the y0 it reconstructs, within 16 times what the
    numpy restatement of the sweep shows on the same inputs (measured on an MI355X: DESIGN section 22)."""
    dtype, M, seed, shape = torch.float64, 2, 11, (2, 3)
    t_np = np.linspace(0.0, 1.0, 9)
    grid = t_np if step_size is None else step_size_grid(t_np, step_size)
    plan = _SubSteps(t_np, None if step_size is None else grid, "linear")
    wb = lambda kind, w: 1.0 if kind == _hip.XDE_ROW_COPY_B else (0.0 if kind == _hip.XDE_ROW_COPY_A else float(w[0]))  # noqa: E731
    rows = [[(j, wb(kind, w)) for j, kind, w in r] for r in plan.rows]
    y0, P, lam = leaves = [x.requires_grad_(True) for x in (SC._y0(dtype, DEV, shape=shape), Coeffs(3, M, dtype, DEV).p.clone(),
                                                            torch.tensor(-0.75, dtype=dtype, device=DEV))]
    W = torch.randn(9 * 2, 3, generator=torch.Generator().manual_seed(3), dtype=dtype).to(DEV)
    drift, diffusion = (lambda t, y: y * lam), (lambda t, y: y.unsqueeze(-1) * P + 0.25)
    o = SC._opts(seed=seed, noise_type="general", **({} if step_size is None else dict(step_size=step_size, interp="linear")))
    dts = [float(grid[k + 1] - grid[k]) for k in range(len(grid) - 1)]
    w = [GN.increments(gn_noise(shape, M, seed, k, dtype, DEV), SO.s_of(dt, np.float64), np.float64) for k, dt in enumerate(dts)]
    # the reference: autograd through the recursion in float64 framework ops
    y, yh, out = y0, y0, [None] * 9
    out[0] = y0
    for k, dt in enumerate(dts):
        wk = torch.as_tensor(w[k]).to(DEV)
        mv = lambda g: g[..., 0] * wk[..., 0:1] + g[..., 1] * wk[..., 1:2]  # noqa: E731
        a = mv(diffusion(None, yh))
        yh1 = (((y + y) - yh) + drift(None, yh) * dt) + a
        y1 = (y + (drift(None, yh) + drift(None, yh1)) * (0.5 * dt)) + (a + mv(diffusion(None, yh1))) * 0.5
        for j, b in rows[k]:
            out[j] = y1 if b == 1.0 else (y if b == 0.0 else y + b * (y1 - y))
        y, yh = y1, yh1
    want = torch.autograd.grad((torch.cat(out, dim=-2) * W).sum(), leaves)
    gap = lambda got: [float((torch.as_tensor(a).to(b) - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]  # noqa: E731
    t = torch.as_tensor(t_np)
    through = gap(torch.autograd.grad((sdeint(drift, diffusion, y0, t, solver=GeneralReversibleHeun, options=o) * W).sum(), leaves))
    adjoint = gap(torch.autograd.grad((sdeint_adjoint(drift, diffusion, y0, t, solver=GeneralReversibleHeun, options=o, adjoint_params=(P, lam)) * W).sum(), leaves))
    gy, gl, gP, y_np = _sweep_np(np_(y0.detach()), float(lam.detach()), np_(P.detach()), w, dts, rows, 9, np_(W).reshape(9, 2, 3))
    restated = gap((gy, gP, gl))
    with torch.no_grad():
        xde, solution, yh_end, g_, gd_, plan_ = ADJ._solve(drift, diffusion, y0.detach(), t, 1e-7, 1e-9, o, GeneralReversibleHeun)
    rec = ADJ._sweep_gn(xde, (P, lam), solution, yh_end, g_, gd_, plan_, W, shape)[2]
    err, err_np = float((rec - y0).abs().max() / y0.abs().max()), float(np.abs(y_np - np_(y0.detach())).max() / np_(y0.detach()).max())
    print("gaps to the reference (y0, P, lam): through the steps", through, "adjoint", adjoint, "numpy restatement", restated,
          "| y0 reconstructed: sweep", err, "restatement", err_np)
    assert max(through) <= 64 * np.finfo(np.float64).eps, through
    assert all(a <= 16 * r for a, r in zip(adjoint, restated)) and err <= 16 * err_np, (adjoint, restated, err, err_np)


def test_adjoint_memory_does_not_grow_with_the_step_count():
    """y0 (64, 1, 256) fp32, M = 4, t = [0, 1]: the adjoint's peak over forward plus backward at 512 steps exceeds its peak at 32 by less
    than one [rows, D, M] matrix; back-propagating through 512 steps peaks at more than ten times the adjoint's."""
    dev, M = torch.device(DEV), 4

    class Drift(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.tensor(-0.5))

        def forward(self, t, y):
            return torch.tanh(y * self.a)

    class Diffusion(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.b = torch.nn.Parameter(torch.linspace(0.1, 0.4, M))

        def forward(self, t, y):
            return torch.tanh(y).unsqueeze(-1) * self.b + 0.1

    f, g = Drift().to(dev), Diffusion().to(dev)
    y0 = (0.5 + torch.rand(64, 1, 256, generator=torch.Generator().manual_seed(0))).to(dev).requires_grad_(True)
    t, matrix = torch.tensor([0.0, 1.0]), y0.numel() * M * y0.element_size()

    def peak(call, h):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        sol = call(f, g, y0, t, solver=GeneralReversibleHeun, options={"norm": None, "seed": 2, "step_size": h, "noise_type": "general"})
        torch.autograd.grad(sol.sum(), [y0] + list(f.parameters()) + list(g.parameters()))
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base

    peak(sdeint_adjoint, 1.0 / 32)  # (warm-up: the library's and the allocator's first-call blocks)
    a32, a512, s512 = peak(sdeint_adjoint, 1.0 / 32), peak(sdeint_adjoint, 1.0 / 512), peak(sdeint, 1.0 / 512)
    print("peak bytes / matrix bytes: adjoint at 32 steps", a32 / matrix, "at 512", a512 / matrix, "through the steps at 512", s512 / matrix)
    assert a512 - a32 < matrix and s512 > 10 * a512, (a32 / matrix, a512 / matrix, s512 / matrix)
