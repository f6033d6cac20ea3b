"""Measurements of sdeint's Milstein kernels.

    python profiles/tools/milstein.py [--out FILE] [--reps N]
    python profiles/tools/milstein.py --out FILE --kernel-stats CSV     (merge a rocprofv3 kernel_stats.csv into FILE)

At n = 65536 x 128, fp32 and fp64, each next to a same-size device copy (2 n elt bytes) timed in the same process:
  step      xde_sde_milstein_step: 5 n elt bytes (y0, f, g, gb read, y1 written)
  bwd       xde_sde_milstein_backward with all three outputs: 4 n elt bytes (gy1 read, gf, gg, ggb written)
  support   xde_sde_milstein_support: 4 n elt bytes, no generator
  noise     xde_sde_noise: the generator alone, writing n normals (n elt bytes)
  framework one Milstein step as framework ops on given f, g, gb: z = randn; w = s*z; q = c*(w*w - a);
            y1 = ((y0 + f*dt) + g*w) + (gb - g)*q
The times here are device events around back-to-back launches (launch gaps included).  Kernel durations come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/milstein.py --reps 20`, whose kernel_stats.csv the second
form merges: per kernel the average and minimum duration, and for the step and the backward the fraction of the copy rate (by events).
Prints one JSON object (and writes it to --out)."""
import argparse
import csv
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DEV = "cuda"
N_ROWS, N_COLS = 65536, 128
STATS_COMMAND = "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/milstein.py --reps 20"


def _time(fn, reps):
    import torch

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


def measure(reps):
    import torch

    from paddlexde_amd import _hip

    be = _hip.get_backend()
    res = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        n = N_ROWS * N_COLS
        g = torch.Generator().manual_seed(0)
        y0, f, gd, gb, gy = (torch.randn(N_ROWS, N_COLS, generator=g).to(DEV, dtype) for _ in range(5))
        y1, yb, gf, gg, ggb, z = (torch.empty_like(y0) for _ in range(6))
        dt = 1e-3
        s, c = math.sqrt(dt), 0.5 / math.sqrt(dt)
        copy_ms = _time(lambda: y1.copy_(y0), reps)
        copy_gbs = 2 * n * elt / copy_ms / 1e6
        step_ms = _time(lambda: be._sde_milstein_step(y1, y0, f, gd, gb, dt, s, c, 12345, 7), reps)
        bwd_ms = _time(lambda: be._sde_milstein_backward(gf, gg, ggb, gy, dt, s, c, 12345, 7), reps)
        sup_ms = _time(lambda: be._sde_milstein_support(yb, y0, f, gd, dt, s), reps)
        noise_ms = _time(lambda: be._sde_noise(z, 12345, 7), reps)

        def framework():
            w = s * torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)
            q = c * (w * w - dt)
            return ((y0 + f * dt) + gd * w) + (gb - gd) * q

        fw_ms = _time(framework, reps)

        def of_copy(elems, ms):
            return round(elems * n * elt / ms / 1e6 / copy_gbs, 3)

        row = {"dtype": str(dtype).split(".")[-1], "n": n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1),
               "step_ms": round(step_ms, 4), "step_bytes": 5 * n * elt, "step_of_copy": of_copy(5, step_ms),
               "bwd_ms": round(bwd_ms, 4), "bwd_bytes": 4 * n * elt, "bwd_of_copy": of_copy(4, bwd_ms),
               "support_ms": round(sup_ms, 4), "support_bytes": 4 * n * elt, "support_of_copy": of_copy(4, sup_ms),
               "noise_ms": round(noise_ms, 4), "step_memory_floor_ms": round(5 * n * elt / copy_gbs / 1e6, 4),
               "framework_ms": round(fw_ms, 4), "speedup_over_framework": round(fw_ms / step_ms, 2)}
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def merge_kernel_stats(out, path):
    """Per kernel of ours (and the copy) the call count, average and minimum duration from rocprofv3's kernel_stats.csv, and for the
    step / backward / support kernels the fraction of the copy rate that the events run in ``out`` measured."""
    with open(out) as fh:
        res = json.load(fh)
    kernels = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Name"]
            if name.startswith("xde_sde_") or "xde_sde_" in name or "copyBuffer" in name or name.startswith("at::native"):
                kernels[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(r["MinNs"]) / 1e3, 2)}
    of_copy = {}
    for row in res["kernels"]:
        t = "float" if row["dtype"] == "float32" else "double"
        # xde_sde_step_kernel<T, VEC, NOISE, formula, output mask> (csrc/xde_sde.hip)
        pick = {"step": ("xde_sde_step_kernel<{}, true, true, (anonymous namespace)::MilsteinStep, 1>".format(t), "step_bytes"),
                "bwd": ("xde_sde_step_kernel<{}, true, true, (anonymous namespace)::MilsteinBackward, 7>".format(t), "bwd_bytes"),
                "support": ("xde_sde_step_kernel<{}, true, false, (anonymous namespace)::EmStep, 1>".format(t), "support_bytes"),
                "noise": ("xde_sde_noise_kernel<{}, false>".format(t), None)}
        d = {}
        for key, (kname, nbytes) in pick.items():
            hit = [v for k, v in kernels.items() if kname in k]
            if not hit:
                continue
            d[key + "_us"] = hit[0]["avg_us"]
            if nbytes:
                d[key + "_of_copy"] = round(row[nbytes] / (hit[0]["avg_us"] * 1e-6) / 1e9 / row["copy_GBps"], 3)
        of_copy[row["dtype"]] = d
    res["rocprofv3_kernel_stats"] = {"command": STATS_COMMAND, "kernels": kernels, "of_copy (kernel time, copy rate by events)": of_copy}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["rocprofv3_kernel_stats"]["of_copy (kernel time, copy rate by events)"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats.csv to merge into --out")
    args = ap.parse_args()
    if args.kernel_stats:
        merge_kernel_stats(args.out, args.kernel_stats)
        sys.exit(0)
    import torch

    res = {"device": torch.cuda.get_device_name(0), "shape": [N_ROWS, N_COLS], "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
