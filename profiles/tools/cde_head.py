"""Measurements of the fused last layer of a CDE field.

    python profiles/tools/cde_head.py [--out FILE] [--reps N] [--rounds R]

At B x H x C = 8192 x 64 x 32 with K = 128 (F is 64 MiB) and 256 x 32 x 8 with K = 32; fp32, the cubic control over Tn = 32:
  fwd_fused     one xde_cdehead_forward launch
  fwd_unfused   the parent's sequence: F.linear, tanh, the contraction launch
  bwd_fused     one xde_cdehead_backward launch, then ga = s W, gW = s^T a, gbias = sum_b s by torch
  bwd_unfused   the contraction's cotangent launch, tanh's backward, then the same three reductions on gpre
Every figure is the median over --rounds rounds; a round times the candidates one after the other (--reps launches each between two
device events, warmed), so they see the same machine state.  Bytes are the HBM traffic each route needs at least (W from L2 is not
counted); the flop rate is 2 B H C K over the fused launch's time.  Then the peak memory of one cdeint(RK4) training step of
examples/cde_demo.py's model, fused and not, at a shape where F dominates.  Prints one JSON object (and writes it to --out)."""
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
from paddlexde_amd.interpolation import CubicHermiteSpline  # noqa: E402
from paddlexde_amd.xde.base_cde import CdeContractFn  # noqa: E402

DEV = "cuda"
SHAPES = [("flagship", 8192, 64, 32, 128), ("small", 256, 32, 8, 32)]
TN = 32
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
    for name, B, H, C, K in SHAPES:
        g = torch.Generator().manual_seed(0)
        a = torch.randn(B, K, generator=g).to(DEV)
        W = (torch.randn(H * C, K, generator=g) / K ** 0.5).to(DEV)
        bias = torch.randn(H * C, generator=g).to(DEV)
        gout = torch.randn(B, H, generator=g).to(DEV)
        X = CubicHermiteSpline(torch.randn(B, TN, C, generator=g).to(DEV))
        t = torch.tensor(11.3, dtype=torch.float64, device=DEV)
        out, s = torch.empty(B, H, device=DEV), torch.empty(B, H * C, device=DEV)
        gF = torch.empty(B, H, C, device=DEV)
        y = torch.tanh(torch.nn.functional.linear(a, W, bias))

        def reductions(x):
            return torch.matmul(x, W), torch.matmul(x.t(), a), x.sum(0)

        def bwd_fused():
            be._cde_head_backward(s, gout, a, W, bias, X._series, None, X._t, t, "cubic", "tanh")
            return reductions(s)

        def bwd_unfused():
            be._cde_contract_backward(gF, gout, X._series, X._t, t, "cubic")
            return reductions(gF.reshape(B, H * C) * (1.0 - y * y))

        runs = {
            "fwd_fused": lambda: be._cde_head(out, a, W, bias, X._series, None, X._t, t, "cubic", "tanh"),
            "fwd_unfused": lambda: CdeContractFn.apply(torch.tanh(torch.nn.functional.linear(a, W, bias)).reshape(B, H, C), X._series, X._t, t,
                                                       "cubic"),
            "bwd_fused": bwd_fused,
            "bwd_unfused": bwd_unfused,
        }
        runs["fwd_fused"]()
        assert torch.allclose(out, runs["fwd_unfused"](), rtol=1e-4, atol=1e-4 * C)
        assert all(torch.allclose(p, q, rtol=1e-3, atol=1e-3) for p, q in zip(bwd_fused(), bwd_unfused()))
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(_time(fn, reps))
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        small = (B * K + B * H + 3 * B * C + H * C * K + H * C) * 4
        F_bytes = B * H * C * 4
        row = {"shape": name, "B": B, "H": H, "C": C, "K": K, "Tn": TN, "F_MiB": round(F_bytes / 2**20, 2), "ms": med,
               "bytes": {"fwd_fused": small, "fwd_unfused": small + 4 * F_bytes,  # GEMM (bias in its epilogue) writes F; tanh reads and writes; contraction reads
                         "bwd_fused": small + 3 * F_bytes,                          # s written, read by two GEMMs (and the sum)
                         "bwd_unfused": small + 6 * F_bytes},                       # gF written, read with y, gpre written, read twice
               "fwd_fused_TFLOPs": round(2.0 * B * H * C * K / med["fwd_fused"] / 1e9, 2),
               "fwd_speedup": round(med["fwd_unfused"] / med["fwd_fused"], 3), "bwd_speedup": round(med["bwd_unfused"] / med["bwd_fused"], 3)}
        row["fwd_fused_of_matrix_peak"] = round(row["fwd_fused_TFLOPs"] / FP32_MATRIX_PEAK_TFLOPS, 4)
        res.append(row)
    return res


def peak_memory(fused, n=4096, length=16, hidden=64):
    """max_memory_allocated over one training step of the demo's model through cdeint(RK4) (gradients through the steps)."""
    import cde_demo

    torch.manual_seed(0)
    series, labels = cde_demo.make_data(n, length, 0, DEV)
    X = CubicHermiteSpline(series)
    model = cde_demo.NeuralCDE(hidden, fused_head=fused).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(model(X), labels)
    loss.backward()
    torch.cuda.synchronize()
    return {"fused": fused, "n": n, "length": length, "hidden": hidden, "loss": round(float(loss), 6),
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
