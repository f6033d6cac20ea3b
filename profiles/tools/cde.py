"""Measurements of cdeint's contraction kernels.

    python profiles/tools/cde.py [--out FILE] [--reps N] [--rounds R]

At B x H x C = 8192 x 64 x 32 (F is 64 MiB in fp32) and, reported only, 256 x 32 x 8; fp32 and fp64; the cubic control over Tn = 32:
  fwd        xde_cde_contract: F read, out written, three series rows read per batch row — (B H C + B H + 3 B C) elt bytes over the
             launch time, as a fraction of a same-size device copy (F copied: 2 B H C elt bytes) timed in the same process
  bwd        xde_cde_contract_backward: gF written, gout and the series rows read, the same byte count and fraction
  framework  the same as framework ops: dX = X.derivative(t) (the spline launch: value and derivative written), then
             einsum("bhc,bc->bh", F, dX); backward gout[:, :, None] * dX[:, None, :] on the materialised dX
Every figure is the median over --rounds rounds; a round times the copy, the kernel and the framework sequence one after the other
(--reps launches each between two device events, warmed), so the three see the same machine state.
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps (the cde, spline and
copy rows of that run's kernel_stats.csv are kept as profiles/cde_kernel_stats.csv); counters, if wanted, in a run of their own.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402
from paddlexde_amd.interpolation import CubicHermiteSpline  # noqa: E402

DEV = "cuda"
SHAPES = [("flagship", 8192, 64, 32), ("small", 256, 32, 8)]
TN = 32


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
    for name, B, H, C in SHAPES:
        for dtype in (torch.float32, torch.float64):
            elt = torch.empty((), dtype=dtype).element_size()
            g = torch.Generator().manual_seed(0)
            F = torch.randn(B, H, C, generator=g).to(DEV, dtype)
            gout = torch.randn(B, H, generator=g).to(DEV, dtype)
            X = CubicHermiteSpline(torch.randn(B, TN, C, generator=g).to(DEV, dtype))
            t = torch.tensor(11.3, dtype=torch.float64, device=DEV)
            out, gF, F2 = torch.empty(B, H, dtype=dtype, device=DEV), torch.empty_like(F), torch.empty_like(F)
            runs = {
                "copy": lambda: F2.copy_(F),
                "fwd": lambda: be._cde_contract(out, F, X._series, X._t, t, "cubic"),
                "fwd_framework": lambda: torch.einsum("bhc,bc->bh", F, X.derivative(t)[:, 0, :]),
                "bwd": lambda: be._cde_contract_backward(gF, gout, X._series, X._t, t, "cubic"),
                "bwd_framework": lambda: gout[:, :, None] * X.derivative(t)[:, 0, :][:, None, :],
            }
            # same results first (the framework sum runs in another order: a tolerance of the dtype's size)
            tol = 1e-4 if dtype == torch.float32 else 1e-12
            runs["fwd"](), runs["bwd"]()
            assert torch.allclose(out, runs["fwd_framework"](), rtol=tol, atol=tol * C)
            assert torch.equal(gF, runs["bwd_framework"]())
            ms = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():
                    ms[k].append(_time(fn, reps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            moved = (B * H * C + B * H + 3 * B * C) * elt
            copy_gbs = 2 * B * H * C * elt / med["copy"] / 1e6
            row = {"shape": name, "B": B, "H": H, "C": C, "Tn": TN, "dtype": str(dtype).split(".")[-1], "F_MiB": round(B * H * C * elt / 2**20, 2),
                   "copy_ms": round(med["copy"], 4), "copy_GBps": round(copy_gbs, 1)}
            for k in ("fwd", "bwd"):
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_ms_spread"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
                row[k + "_GBps"] = round(moved / med[k] / 1e6, 1)
                row[k + "_of_copy"] = round(moved / med[k] / 1e6 / copy_gbs, 3)
                row[k + "_framework_ms"] = round(med[k + "_framework"], 4)
                row[k + "_speedup_over_framework"] = round(med[k + "_framework"] / med[k], 2)
            res.append(row)
            print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("profiles/tools/cde.py measures on the GPU: no device found")
    res = {"device": torch.cuda.get_device_name(0), "target_of_copy": 0.70, "kernels": measure(args.reps, args.rounds)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
