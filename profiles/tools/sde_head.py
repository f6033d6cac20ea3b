"""Measurements of the fused last layer of a matrix diffusion.

    python profiles/tools/sde_head.py [--out FILE] [--reps N] [--rounds R]

At rows x D x M = 16384 x 64 x 8 with K = 64 (g is 32 MiB) and 256 x 16 x 3 with K = 32; fp32, tanh, with bias:
  fwd_fused     one xde_sdehead_step launch
  fwd_unfused   the parent's sequence: F.linear, tanh, the general-noise step launch
  bwd_fused     one xde_sdehead_backward launch, then ga = s W, gW = s^T a, gbias = sum_r s by torch
  bwd_unfused   the general-noise cotangent launch, tanh's backward, then the same three reductions on gpre
Every figure is the median over --rounds rounds; a round times the candidates one after the other (--reps launches each between two
device events, warmed), so they see the same machine state.  The flop rate is 2 rows D M K over the fused launch's time.  Then the peak
memory of one through-the-steps training step of examples/sde_gan_demo.py's generator at 64 steps, fused and plain, at a batch where g
dominates.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from paddlexde_amd import _hip  # noqa: E402

DEV = "cuda"
SHAPES = [("flagship", 16384, 64, 8, 64), ("demo", 256, 16, 3, 32)]
DT, S, SEED, STEP = 0.0625, 0.25, 7, 5
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


def measure(reps, rounds):
    be = _hip.get_backend()
    res = []
    for name, rows, D, M, K in SHAPES:
        g = torch.Generator().manual_seed(0)
        a = torch.randn(rows, K, generator=g).to(DEV)
        W = (torch.randn(D * M, K, generator=g) / K ** 0.5).to(DEV)
        bias = torch.randn(D * M, generator=g).to(DEV)
        y0, f, gy = (torch.randn(rows, D, generator=g).to(DEV) for _ in range(3))
        y1, y1u, gf = torch.empty_like(y0), torch.empty_like(y0), torch.empty_like(y0)
        s = torch.empty(rows, D * M, device=DEV)
        gg = torch.empty(rows, D, M, device=DEV)
        y = torch.tanh(torch.nn.functional.linear(a, W, bias))

        def reductions(x):
            return torch.matmul(x, W), torch.matmul(x.t(), a), x.sum(0)

        def fwd_unfused():
            be._sde_gn_step(y1u, y0, f, torch.tanh(torch.nn.functional.linear(a, W, bias)).reshape(rows, D, M), DT, S, SEED, STEP)

        def bwd_fused():
            be._sde_head_backward(s, gf, gy, a, W, bias, "tanh", DT, S, SEED, STEP)
            return reductions(s)

        def bwd_unfused():
            be._sde_gn_backward(gf, gg, gy, M, DT, S, SEED, STEP)
            return reductions(gg.reshape(rows, D * M) * (1.0 - y * y))

        runs = {"fwd_fused": lambda: be._sde_head_step(y1, y0, f, a, W, bias, "tanh", DT, S, SEED, STEP), "fwd_unfused": fwd_unfused,
                "bwd_fused": bwd_fused, "bwd_unfused": bwd_unfused}
        runs["fwd_fused"]()
        fwd_unfused()
        assert torch.allclose(y1, y1u, rtol=1e-4, atol=1e-4 * M)
        assert all(torch.allclose(p, q, rtol=1e-3, atol=1e-3) for p, q in zip(bwd_fused(), bwd_unfused()))
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(_time(fn, reps))
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        small = (rows * K + 3 * rows * D + D * M * K + D * M) * 4
        g_bytes = rows * D * M * 4
        row = {"shape": name, "rows": rows, "D": D, "M": M, "K": K, "g_MiB": round(g_bytes / 2**20, 2), "ms": med,
               "plan": _hip.sde_head_plan(rows, D, M, K, torch.float32, "tanh"),
               "bytes": {"fwd_fused": small, "fwd_unfused": small + 4 * g_bytes,  # GEMM (bias in its epilogue) writes g; tanh reads and writes; the step reads
                         "bwd_fused": small + 3 * g_bytes,                          # s written, read by two GEMMs (and the sum)
                         "bwd_unfused": small + 6 * g_bytes},                       # gg written, read with y, gpre written, read twice
               "fwd_fused_TFLOPs": round(2.0 * rows * D * M * K / med["fwd_fused"] / 1e9, 2),
               "fwd_speedup": round(med["fwd_unfused"] / med["fwd_fused"], 3), "bwd_speedup": round(med["bwd_unfused"] / med["bwd_fused"], 3)}
        row["fwd_fused_of_matrix_peak"] = round(row["fwd_fused_TFLOPs"] / FP32_MATRIX_PEAK_TFLOPS, 4)
        res.append(row)
    return res


def peak_memory(fused, batch=4096, steps=64):
    """max_memory_allocated over one training step of the demo's generator through sdeint(Euler) (gradients through the steps)."""
    import sde_gan_demo

    torch.manual_seed(0)
    gen = sde_gan_demo.Generator(fused_head=fused).to(DEV)
    v = torch.randn(batch, gen.latent, device=DEV)
    t = torch.linspace(0.0, 2.0, steps + 1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = gen(v, t, 0.0, seed=3).square().mean()
    loss.backward()
    torch.cuda.synchronize()
    return {"fused": fused, "batch": batch, "steps": steps, "D": gen.hidden, "M": gen.noise, "loss": round(float(loss), 6),
            "peak_MiB_over_start": round((torch.cuda.max_memory_allocated() - base) / 2**20, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    doc = {"kernels": measure(args.reps, args.rounds), "training_step_peak": [peak_memory(False), peak_memory(True)]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
