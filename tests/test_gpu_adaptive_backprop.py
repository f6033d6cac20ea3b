"""options["backprop"] = "steps" on the MI355X: gradients against the eager twin (tests/_backprop_twin.py) and against finite
differences of the product's own forward, the recompute's bit-equality with the forward, the two kernels against numpy, and the
memory the sweep leaves behind."""
import copy
import gc

import numpy as np
import pytest
import torch

from paddlexde_amd import Dopri5, _hip, odeint
from paddlexde_amd.utils.ode_utils import _rms_norm

from ._backprop_twin import twin_odeint
from .test_adaptive_backprop_host import SOLVERS, T_OUT, Linear, MLP, rel

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _loss(sol, w):
    return (sol * w).sum() + (sol**2).sum() * 0.1


def _steps_run(func, y0, t, solver, rtol=1e-5, atol=1e-7, **opts):
    steps, attempts = [], []

    def hook(i, y0_, y1, ks, c):
        attempts.append((float(c.dt_last), bool(c.accept)))
        if c.accept:
            steps.append((float(c.t0), float(c.t1), float(c.dt_last), int(c.out_begin), int(c.out_end)))

    y0 = y0.clone().requires_grad_()
    opts = dict(dict(backprop="steps", norm=_rms_norm, dtype=t.dtype, _step_hook=hook), **opts)
    sol = odeint(func, y0, t, solver, rtol=rtol, atol=atol, options=opts)
    w = torch.linspace(-1.0, 1.0, sol.numel(), dtype=sol.dtype, device=sol.device).reshape(sol.shape)
    grads = torch.autograd.grad(_loss(sol, w), [y0] + list(func.parameters()))
    return sol.detach(), grads, steps, attempts, w


def _twin(func, y0, t, name, steps, w):
    y0 = y0.clone().requires_grad_()
    sol = twin_odeint(func, y0, t, name, [s[:3] for s in steps])
    return sol.detach(), torch.autograd.grad(_loss(sol, w), [y0] + list(func.parameters()))


@pytest.mark.parametrize("solver,name", SOLVERS, ids=[n for _, n in SOLVERS])
@pytest.mark.parametrize("problem", ["mlp", "linear"])
def test_fp64_gradients_match_the_cpu_twin(solver, name, problem):
    f = (MLP() if problem == "mlp" else Linear()).to(DEV)
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4)
    t = torch.tensor(T_OUT, dtype=torch.float64)
    sol, grads, steps, _, w = _steps_run(f, y0.to(DEV), t.to(DEV), solver)
    assert any(oe - ob >= 2 for *_, ob, oe in steps) and any(oe == ob for *_, ob, oe in steps[:-1]), steps
    fc = copy.deepcopy(f).cpu()
    tsol, tgrads = _twin(fc, y0, t, name, steps, w.cpu())
    assert rel(sol.cpu(), tsol) <= 1e-10
    for a, b in zip(grads, tgrads):
        assert rel(a.cpu(), b) <= 1e-10, (name, rel(a.cpu(), b))


def test_fp64_reverse_time_matches_the_cpu_twin():
    f = MLP().to(DEV)
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4)
    t = torch.tensor([1.6, 1.5, 1.45, 0.7, 0.0], dtype=torch.float64)
    _, grads, steps, _, w = _steps_run(f, y0.to(DEV), t.to(DEV), Dopri5)
    _, tgrads = _twin(copy.deepcopy(f).cpu(), y0, t, "dopri5", steps, w.cpu())
    for a, b in zip(grads, tgrads):
        assert rel(a.cpu(), b) <= 1e-10


class Spiral(torch.nn.Module):  # config 3's func (example/ode_demo.py:17-33)
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(42)
        self.net = torch.nn.Sequential(torch.nn.Linear(2, 50), torch.nn.Tanh(), torch.nn.Linear(50, 2))
        for m in self.net:
            if isinstance(m, torch.nn.Linear):
                with torch.no_grad():
                    m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=g))
                    m.bias.zero_()

    def forward(self, t, y):
        return self.net(y**3)


def config3():
    f = Spiral().to(DEV)
    y0 = (torch.rand(8192, 2, generator=torch.Generator().manual_seed(0)) * 4 - 2).to(DEV)
    t = torch.linspace(0.0, 25.0, 1000)[:32].to(DEV)
    return f, y0, t


def test_fp32_config3_matches_the_fp32_twin(record_property):
    f, y0, t = config3()
    _, grads, steps, _, w = _steps_run(f, y0, t, Dopri5)
    _, tgrads = _twin(f, y0, t, "dopri5", steps, w)
    errs = [rel(a, b) for a, b in zip(grads, tgrads)]
    record_property("config3_fp32_rel", max(errs))
    print("config 3 fp32, steps vs fp32 twin: max normwise rel = {:.3e} over {} accepted steps".format(max(errs), len(steps)))
    assert max(errs) <= 1e-4, errs


def test_fp64_finite_differences_of_the_pinned_forward():
    f = MLP().to(DEV)
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64, device=DEV).reshape(3, 4)
    t = torch.tensor(T_OUT, dtype=torch.float64, device=DEV)
    _, grads, steps, attempts, w = _steps_run(f, y0, t, Dopri5)
    pin = dict(first_step=attempts[0][0], _replay=attempts)

    def L(y):
        with torch.no_grad():
            s = odeint(f, y, t, Dopri5, rtol=1e-5, atol=1e-7, options=dict(norm=_rms_norm, dtype=torch.float64, **pin))
        return float(_loss(s, w))

    _, g_pinned, _, _, _ = _steps_run(f, y0, t, Dopri5, **pin)
    assert rel(g_pinned[0], grads[0]) <= 1e-12  # pinning changes nothing but the controller's inputs
    gen = torch.Generator().manual_seed(3)
    eps = 1e-6
    for _ in range(3):
        v = torch.randn(y0.shape, generator=gen, dtype=torch.float64).to(DEV)
        fd = (L(y0 + eps * v) - L(y0 - eps * v)) / (2 * eps)
        ad = float((g_pinned[0] * v).sum())
        assert abs(fd - ad) <= 1e-6 * abs(ad), (fd, ad)


def test_recompute_is_bit_equal_to_the_forward():
    for solver, name in SOLVERS:
        fwd_t, per_attempt, probes = [], [], []
        f = MLP().to(DEV)

        def func(t_, y, f=f):
            if not torch.is_grad_enabled():
                fwd_t.append(t_.detach().clone())
            return f(t_, y)

        S = len(solver.tableau.alpha)

        def hook(i, y0_, y1, ks, c):
            if c.accept:
                per_attempt.append([x.item() for x in fwd_t[-S:]])

        y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64, device=DEV).reshape(3, 4).requires_grad_()
        t = torch.tensor(T_OUT, dtype=torch.float64, device=DEV)
        sol = odeint(_Wrap(func, f), y0, t, solver, rtol=1e-5, atol=1e-7,
                     options=dict(backprop="steps", norm=_rms_norm, dtype=torch.float64, _step_hook=hook,
                                  _backprop_probe=lambda n, y1, kept, ts: probes.append((n, torch.equal(y1, kept),
                                                                                         [x.item() for x in ts]))))
        sol.sum().backward()
        assert len(probes) == len(per_attempt) > 0
        for n, same, ts in probes:
            assert same, (name, n)
            assert ts == per_attempt[n], (name, n, ts, per_attempt[n])  # python floats of the same fp64 values: bit equality


class _Wrap(torch.nn.Module):
    def __init__(self, fn, mod):
        super().__init__()
        self.mod = mod
        self.fn = fn

    def forward(self, t, y):
        return self.fn(t, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_stage_cotangent_kernel_against_numpy(dtype):
    be = _hip.get_backend()
    n = 3 * 2048 * 256 * 4 + 3  # past one grid-stride sweep; not a multiple of the vector width
    gen = torch.Generator().manual_seed(5)
    npd = np.float32 if dtype == torch.float32 else np.float64
    xs = [torch.randn(n, generator=gen, dtype=dtype).to(DEV) for _ in range(_hip.XDE_BP_MAX_X)]
    xh = [x.cpu().numpy() for x in xs]
    for nx in range(1, _hip.XDE_BP_MAX_X + 1):
        c = np.random.default_rng(nx).standard_normal(nx)
        c2 = np.random.default_rng(100 + nx).standard_normal(nx)
        for two in (False, True):
            out = torch.empty(n, dtype=dtype, device=DEV)
            out2 = torch.empty(n, dtype=dtype, device=DEV) if two else None
            be.stage_cotangent(out, xs[:nx], list(c), out2=out2, coef2=list(c2) if two else None)
            for o, cs in ((out, c), (out2, c2)):
                if o is None:
                    continue
                ref = xh[0] * npd(cs[0])
                for j in range(1, nx):
                    ref = ref + xh[j] * npd(cs[j])
                assert np.array_equal(o.cpu().numpy(), ref), (nx, two)
    # a misaligned operand takes the scalar path: same results
    out = torch.empty(n - 1, dtype=dtype, device=DEV)
    be.stage_cotangent(out, [xs[0][1:], xs[1][1:]], [0.5, -2.0])
    assert np.array_equal(out.cpu().numpy(), xh[0][1:] * npd(0.5) + xh[1][1:] * npd(-2.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_dense_cotangent_kernel_against_numpy(dtype):
    be = _hip.get_backend()
    npd = np.float32 if dtype == torch.float32 else np.float64
    gen = torch.Generator().manual_seed(6)
    for n in (1 << 20 | 3, 4 * 2048 * 256 * 4):
        for G in (1, 2, 3, 4, 6):
            g = torch.randn(G, n, generator=gen, dtype=dtype).to(DEV)
            gh = g.cpu().numpy()
            wts = np.random.default_rng(G).standard_normal((G, 5))
            base = [torch.randn(n, generator=gen, dtype=dtype).to(DEV) for _ in range(5)]
            for mask in (0, 0b10, 0b11111):
                live = [None if (mask == 0 and k == 2) else b.clone() for k, b in enumerate(base)]  # (a null output is skipped)
                be.dense_cotangent(live, g, wts.tolist(), acc_mask=mask)
                for k in range(5):
                    if live[k] is None:
                        continue
                    s = gh[0] * npd(wts[0, k])
                    if (mask >> k) & 1:
                        s = base[k].cpu().numpy() + s
                    for r in range(1, min(G, 4)):
                        s = s + gh[r] * npd(wts[r, k])
                    for r in range(4, G):  # the second launch accumulates what the first wrote
                        s = s + gh[r] * npd(wts[r, k])
                    assert np.array_equal(live[k].cpu().numpy(), s), (n, G, mask, k)


def test_memory_returns_after_backward():
    f, y0, t = config3()

    def once():
        y = y0.clone().requires_grad_()
        sol = odeint(f, y, t, Dopri5, rtol=1e-5, atol=1e-7, options={"backprop": "steps", "norm": _rms_norm})
        sol.square().sum().backward()
        del sol, y

    once()  # the per-device work sets and time tables are pooled on first use
    for p in f.parameters():
        p.grad = None
    gc.collect()  # (garbage of earlier tests must neither count nor be freed during the measured call)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    gc.disable()  # reference counting alone has to release what the call allocated
    try:
        once()
        for p in f.parameters():
            p.grad = None
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        gc.enable()
