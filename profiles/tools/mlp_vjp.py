"""Measurements of the fused MLP field's vector-Jacobian product.

    python profiles/tools/mlp_vjp.py [--out FILE] [--reps N] [--rounds R]

fp32, tanh, with bias, at rows x widths = 1000 x (2, 50, 2) (the spiral demo's field) and 65536 x (128, 128, 128, 128) (config 2's
state shape):
  fused   one MLPField.vjp call: xde_mlp_field_vjp's two launches (the route's host cost is in the figure)
  plain   _vjp_of on the same module with fuse = False: a taped F.linear / tanh forward and torch.autograd.grad, what the adjoint's
          augmented dynamics run without the hook
Every figure is the median over --rounds rounds; a round times the candidates one after the other (--reps calls each between two
device events, warmed), so they see the same machine state.  Then one whole backward solve of examples/ode_demo.py's training step by
odeint_adjoint (RK4, a batch of 20 windows of 10 times; the forward solve is outside the timed region), with and without the hook.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from paddlexde_amd import RK4, _hip, odeint_adjoint  # noqa: E402
from paddlexde_amd.functional._adjoint_dynamics import _vjp_of  # noqa: E402
from paddlexde_amd.xde import MLPField  # noqa: E402

DEV = "cuda"
SHAPES = [("spiral", 1000, (2, 50, 2)), ("config2", 65536, (128, 128, 128, 128))]


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _rounds(runs, reps, rounds):
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ms[k].append(_time(fn, reps))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def measure(reps, rounds):
    res = []
    for name, rows, widths in SHAPES:
        torch.manual_seed(0)
        fused, plain = (MLPField(widths[0], widths[1:-1], widths[-1]).to(DEV) for _ in range(2))
        plain.load_state_dict(fused.state_dict())
        plain.fuse = False
        y, a, t = torch.randn(rows, widths[0], device=DEV), torch.randn(rows, widths[-1], device=DEV), torch.tensor(0.5, device=DEV)
        params = tuple(plain.parameters())
        got, want = fused.vjp(t, y, a), _vjp_of(plain, t, y, params, a, False, retain=False)
        for g, w in zip((got[0], got[2]) + tuple(got[3:]), (want[0], want[2]) + tuple(want[3])):
            assert torch.allclose(g, w, rtol=1e-3, atol=1e-4 * float(w.abs().max()))
        med = _rounds({"fused": lambda: fused.vjp(t, y, a), "plain": lambda: _vjp_of(plain, t, y, params, a, False, retain=False)}, reps, rounds)
        flops = 3 * 2.0 * rows * sum(k * n for k, n in zip(widths, widths[1:]))  # the forward, the transposed and the outer product
        res.append({"shape": name, "rows": rows, "widths": widths, "ms": med, "plan": _hip.mlp_vjp_plan(rows, widths, torch.float32, "tanh"),
                    "speedup": round(med["plain"] / med["fused"], 3), "fused_TFLOPs": round(flops / med["fused"] / 1e9, 3)})
    return res


def demo_backward(reps, rounds):
    """The backward solve of the demo's training step by odeint_adjoint: a batch of 20 windows of 10 times, RK4."""
    import ode_demo

    t, true_y = ode_demo.make_data(DEV)
    y0, bt, _ = ode_demo.get_batch(t, true_y, 20, 10, torch.Generator().manual_seed(42))
    torch.manual_seed(0)
    func = ode_demo.ODEFunc(True).to(DEV)
    ms = {"hook": [], "plain": []}
    for _ in range(rounds):
        for key, kw in (("hook", {"adjoint_options": {"vjp": func.vjp}}), ("plain", {})):
            total = 0.0
            for i in range(reps + 2):
                loss = odeint_adjoint(func, y0[:, None, :], bt, solver=RK4, **kw).abs().mean()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loss.backward()
                b.record()
                b.synchronize()
                total += a.elapsed_time(b) if i >= 2 else 0.0
            ms[key].append(total / reps)
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    return {"solver": "RK4", "batch": 20, "times": 10, "ms": med, "speedup": round(med["plain"] / med["hook"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    doc = {"calls": measure(args.reps, args.rounds), "demo_backward_solve": demo_backward(max(args.reps // 5, 5), args.rounds)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
