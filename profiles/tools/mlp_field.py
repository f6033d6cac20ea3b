"""Measurements of the fused MLP field.

    python profiles/tools/mlp_field.py [--out FILE] [--reps N] [--rounds R]

fp32, tanh, with bias, under torch.no_grad(), at rows x widths = 1000 x (2, 50, 2) (the spiral demo's field) and
65536 x (128, 128, 128, 128) (config 2's state shape):
  fused   one xde_mlp_field launch (through MLPField.forward: the route's host cost is in the figure)
  plain   the same module with fuse = False: F.linear and torch.tanh
Every figure is the median over --rounds rounds; a round times the candidates one after the other (--reps calls each between two
device events, warmed), so they see the same machine state.  The flop rate is 2 rows sum_l widths[l] widths[l + 1] over the fused
call's time.  Then one whole forward solve of examples/ode_demo.py's problem by odeint_adjoint under no_grad (RK4, a batch of 20
windows of 10 times), with the demo's network as an MLPField and as nn.Sequential.  Prints one JSON object (and writes it to --out)."""
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
from paddlexde_amd.xde import MLPField  # noqa: E402

DEV = "cuda"
SHAPES = [("spiral", 1000, (2, 50, 2)), ("config2", 65536, (128, 128, 128, 128))]
FP32_MATRIX_PEAK_TFLOPS = 157.3  # MI355X data sheet: fp32 matrix = fp32 vector


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
        y = torch.randn(rows, widths[0], device=DEV)
        with torch.no_grad():
            assert torch.allclose(fused(0.0, y), plain(0.0, y), rtol=1e-4, atol=1e-5)
            med = _rounds({"fused": lambda: fused(0.0, y), "plain": lambda: plain(0.0, y)}, reps, rounds)
        flops = 2.0 * rows * sum(k * n for k, n in zip(widths, widths[1:]))
        row = {"shape": name, "rows": rows, "widths": widths, "ms": med, "plan": _hip.mlp_field_plan(rows, widths, torch.float32, "tanh"),
               "speedup": round(med["plain"] / med["fused"], 3), "fused_TFLOPs": round(flops / med["fused"] / 1e9, 3)}
        row["fused_of_matrix_peak"] = round(row["fused_TFLOPs"] / FP32_MATRIX_PEAK_TFLOPS, 4)
        res.append(row)
    return res


def demo_forward(reps, rounds):
    """One forward solve of the demo's training step by odeint_adjoint, under no_grad: a batch of 20 windows of 10 times, RK4."""
    import ode_demo

    t, true_y = ode_demo.make_data(DEV)
    y0, bt, _ = ode_demo.get_batch(t, true_y, 20, 10, torch.Generator().manual_seed(42))
    funcs = {}
    for key, fused in (("fused", True), ("plain", False)):
        torch.manual_seed(0)
        funcs[key] = ode_demo.ODEFunc(fused).to(DEV)
    with torch.no_grad():
        sols = {k: odeint_adjoint(f, y0[:, None, :], bt, solver=RK4) for k, f in funcs.items()}
        assert torch.allclose(sols["fused"], sols["plain"], rtol=1e-4, atol=1e-5)
        med = _rounds({k: (lambda f=f: odeint_adjoint(f, y0[:, None, :], bt, solver=RK4)) for k, f in funcs.items()}, reps, rounds)
    return {"solver": "RK4", "batch": 20, "times": 10, "ms": med, "speedup": round(med["plain"] / med["fused"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    doc = {"calls": measure(args.reps, args.rounds), "demo_forward_solve": demo_forward(max(args.reps // 10, 5), args.rounds)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
