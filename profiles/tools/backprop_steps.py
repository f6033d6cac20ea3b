"""Measurements of odeint(..., options={"backprop": "steps"}) (DESIGN sections 2, 4 and 7).

    python profiles/tools/backprop_steps.py [--out FILE] [--part timing|compare|firststep|kernels]

timing     backward time per accepted step, config 3's shape (spiral MLP, batch 8192, fp32) and 65536 x 128 fp32 with a
           torch.nn.Linear func; against the eager twin (tests/_backprop_twin.py) run with torch ops on the same GPU
compare    normwise relative difference of config 3's gradients, continuous adjoint vs "steps", at rtol/atol 1e-7/1e-9 and 1e-5/1e-7
firststep  size of the one deviation from the reference: the first step size held constant (here) vs carrying its
           select_initial_step graph (the reference), one fp64 run of the twin
kernels    the two backprop kernels at 32 MiB operands (run under `rocprofv3 --kernel-trace --stats -- python ...`)
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import Dopri5, _hip, odeint, odeint_adjoint  # noqa: E402
from paddlexde_amd.utils.ode_utils import _rms_norm  # noqa: E402
from tests._backprop_twin import twin_odeint  # noqa: E402

DEV = "cuda"


class Spiral(torch.nn.Module):
    def __init__(self, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(42)
        self.net = torch.nn.Sequential(torch.nn.Linear(2, 50), torch.nn.Tanh(), torch.nn.Linear(50, 2)).to(dtype)
        for m in self.net:
            if isinstance(m, torch.nn.Linear):
                with torch.no_grad():
                    m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=g))
                    m.bias.zero_()

    def forward(self, t, y):
        return self.net(y**3)


class Lin(torch.nn.Module):
    def __init__(self, d=128):
        super().__init__()
        self.lin = torch.nn.Linear(d, d, bias=False)
        with torch.no_grad():
            u = 0.1 * torch.randn(d, d, generator=torch.Generator().manual_seed(1))
            self.lin.weight.copy_(u - u.T)

    def forward(self, t, y):
        return self.lin(y)


def config3(dtype=torch.float32):
    f = Spiral(dtype).to(DEV)
    y0 = (torch.rand(8192, 2, generator=torch.Generator().manual_seed(0)) * 4 - 2).to(DEV, dtype)
    t = torch.linspace(0.0, 25.0, 1000)[:32].to(DEV)
    return f, y0, t


def big_linear():
    f = Lin().to(DEV)
    y0 = torch.randn(65536, 128, generator=torch.Generator().manual_seed(0)).to(DEV)
    t = torch.linspace(0.0, 1.0, 5).to(DEV)
    return f, y0, t


def sync():
    torch.cuda.synchronize()


def steps_solve(f, y0, t, rtol=1e-5, atol=1e-7, **opts):
    steps = []

    def hook(i, y0_, y1, ks, c):
        if c.accept:
            steps.append((float(c.t0), float(c.t1), float(c.dt_last)))

    y = y0.clone().requires_grad_()
    sol = odeint(f, y, t, Dopri5, rtol=rtol, atol=atol, options=dict(backprop="steps", norm=_rms_norm, _step_hook=hook, **opts))
    return y, sol, steps


def grads_of(y, sol, f):
    return torch.autograd.grad(sol.square().sum(), [y] + list(f.parameters()))


def timing(reps=3):
    out = {}
    for name, mk in (("config3_spiral_8192x2_fp32", config3), ("linear_65536x128_fp32", big_linear)):
        f, y0, t = mk()
        best = {}
        for _ in range(reps):
            sync()
            a = time.perf_counter()
            y, sol, steps = steps_solve(f, y0, t)
            sync()
            b = time.perf_counter()
            grads_of(y, sol, f)
            sync()
            c = time.perf_counter()
            y2 = y0.clone().requires_grad_()
            tsol = twin_odeint(f, y2, t, "dopri5", steps)
            sync()
            d = time.perf_counter()
            grads_of(y2, tsol, f)
            sync()
            e = time.perf_counter()
            for k, v in (("forward_ms", b - a), ("backward_ms", c - b), ("twin_forward_ms", d - c), ("twin_backward_ms", e - d)):
                best[k] = min(best.get(k, 1e30), v * 1e3)
            del y, sol, y2, tsol
        n = len(steps)
        best["n_accept"] = n
        best["backward_ms_per_step"] = best["backward_ms"] / n
        best["twin_backward_ms_per_step"] = best["twin_backward_ms"] / n
        out[name] = best
    return out


def rel(a, b):
    return float((a - b).norm() / b.norm())


def compare():
    out = {}
    f, y0, t = config3()
    for rtol, atol in ((1e-7, 1e-9), (1e-5, 1e-7)):
        y, sol, _ = steps_solve(f, y0, t, rtol=rtol, atol=atol)
        gs = grads_of(y, sol, f)
        y2 = y0.clone().requires_grad_()
        sol2 = odeint_adjoint(f, y2, t, solver=Dopri5, rtol=rtol, atol=atol, options={"norm": _rms_norm})
        ga = grads_of(y2, sol2, f)
        out["rtol={:g},atol={:g}".format(rtol, atol)] = {"y0": rel(ga[0], gs[0]), "params_max": max(rel(a, b) for a, b in zip(ga[1:], gs[1:]))}
    return out


def select_initial_step(f, t0, y0, order, rtol, atol):
    """The reference's heuristic (solver/base_adaptive_solver.py:33-72) as differentiable torch ops."""
    def norm(x):
        return x.square().mean().sqrt()

    f0 = f(torch.tensor(t0, dtype=y0.dtype, device=y0.device), y0)
    scale = atol + y0.abs() * rtol
    d0, d1 = norm(y0 / scale), norm(f0 / scale)
    h0 = 0.01 * d0 / d1 if (d0 >= 1e-5 and d1 >= 1e-5) else torch.tensor(1e-6, dtype=y0.dtype, device=y0.device)
    y1 = y0 + f0 * h0
    f1 = f(t0 + h0, y1)
    d2 = norm((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = torch.clamp(h0 * 1e-3, min=1e-6)
    else:
        h1 = (0.01 / torch.maximum(d1, d2)) ** (1.0 / order)
    return torch.minimum(100 * h0, h1)


def firststep():
    f, y0, t = config3(torch.float64)
    t = t.double()
    y0 = y0[:256]
    rtol, atol = 1e-7, 1e-9
    _, _, steps = steps_solve(f, y0, t, rtol=rtol, atol=atol, dtype=torch.float64)
    y = y0.clone().requires_grad_()
    sol = twin_odeint(f, y, t, "dopri5", steps)
    g_det = grads_of(y, sol, f)
    y = y0.clone().requires_grad_()
    h = select_initial_step(f, float(t[0]), y, 5, rtol, atol)
    if abs(float(h) - steps[0][2]) > 1e-12 * abs(steps[0][2]):  # the first attempt was rejected: its graph dies with it
        return {"first_dt": float(h), "first_accepted_dt": steps[0][2], "note": "first attempt rejected: no deviation"}
    sol = twin_odeint(f, y, t, "dopri5", steps, first_dt=h)
    g_att = grads_of(y, sol, f)
    return {"y0": rel(g_det[0], g_att[0]), "params_max": max(rel(a, b) for a, b in zip(g_det[1:], g_att[1:])),
            "n_accept": len(steps), "problem": "config 3's func, 256 of its states, fp64, rtol/atol 1e-7/1e-9"}


def kernels(reps=20):
    be = _hip.get_backend()
    n = (32 << 20) // 4
    xs = [torch.randn(n, device=DEV) for _ in range(8)]
    out, out2 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    g = torch.randn(4, n, device=DEV)
    outs = [torch.empty(n, device=DEV) for _ in range(5)]
    w = [[0.1 * (r + 1) * (k + 1) for k in range(5)] for r in range(4)]
    copy_dst = torch.empty(n, device=DEV)
    res = {}
    for label, fn, nbytes in (
            ("copy_32MiB", lambda: copy_dst.copy_(xs[0]), 2 * 4 * n),
            ("stage_cotangent_nx3", lambda: be.stage_cotangent(out, xs[:3], [1.0, 2.0, 3.0]), 4 * 4 * n),
            ("stage_cotangent_nx8_two", lambda: be.stage_cotangent(out, xs, [1.0] * 8, out2=out2, coef2=[0.5] * 8), 10 * 4 * n),
            ("dense_cotangent_G2", lambda: be.dense_cotangent(outs, g[:2], w[:2], acc_mask=0b10), (2 + 1 + 5) * 4 * n)):
        fn()
        sync()
        a = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        dt = (time.perf_counter() - a) / reps
        res[label] = {"us": dt * 1e6, "GB_s": nbytes / dt / 1e9}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--part", action="append", choices=["timing", "compare", "firststep", "kernels"])
    args = ap.parse_args()
    parts = args.part or ["timing", "compare", "firststep"]
    res = {p: globals()[p]() for p in parts}
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(s + "\n")
