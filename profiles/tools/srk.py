"""Measurements of sdeint's SRK kernels.

    python profiles/tools/srk.py [--out FILE] [--reps N]
    python profiles/tools/srk.py --out FILE --kernel-stats CSV     (merge a rocprofv3 kernel_stats.csv into FILE)

At n = 65536 x 128, fp32 and fp64, each next to a same-size device copy (2 n elt bytes) timed in the same process:
  stage1      xde_sde_srk_stage1: 6 n elt bytes (y0, a1, b1 read; Y2, G2, G3 written), both draws
  stage2      xde_sde_srk_stage2: 6 n (y0, a1, b1, b2, b3 read; G4 written), no generator
  step        xde_sde_srk_step: 8 n (y0, a1, a2, b1 .. b4 read; y1 written), both draws
  stage1_bwd  xde_sde_srk_stage1_backward with all three outputs: 6 n, both draws
  stage2_bwd  xde_sde_srk_stage2_backward with all four outputs: 5 n, no generator
  step_bwd    xde_sde_srk_step_backward with all six outputs: 7 n, both draws
  noise0 / 1  the generator alone per draw, writing n normals (n elt bytes).  Both draws run one kernel instantiation (the draw is a
              kernel argument), so only these event timings tell them apart: the merged kernel-trace row `noise_us` averages the two
  framework   the three launches of one SRK step as framework ops on given a1, a2, b1 .. b4: two randn, the random quantities, the
              four stage inputs and y1
The times here are device events around back-to-back launches (launch gaps included).  Kernel durations come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/srk.py --reps 20`, whose kernel_stats.csv the second
form merges: per kernel the average and minimum duration and the fraction of the copy rate (by events).
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
STATS_COMMAND = "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/srk.py --reps 20"
# name -> (elements moved per state element, the formula's instantiation in csrc/xde_sde.hip: NOISE, functor, output mask)
KERNELS = {"stage1": (6, "true, (anonymous namespace)::SrkStage1, 7"), "stage2": (6, "false, (anonymous namespace)::SrkStage2, 1"),
           "step": (8, "true, (anonymous namespace)::SrkStep, 1"), "stage1_bwd": (6, "true, (anonymous namespace)::SrkStage1Backward, 7"),
           "stage2_bwd": (5, "false, (anonymous namespace)::SrkStage2Backward, 15"),
           "step_bwd": (7, "true, (anonymous namespace)::SrkStepBackward, 63")}


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
        y0, a1, a2, b1, b2, b3, b4, gy, gz = (torch.randn(N_ROWS, N_COLS, generator=g).to(DEV, dtype) for _ in range(9))
        o = [torch.empty_like(y0) for _ in range(6)]
        dt = 1e-3
        s, c, c3 = math.sqrt(dt), 0.5 / math.sqrt(dt), 1.0 / (6.0 * dt)
        seed, k = 12345, 7
        copy_ms = _time(lambda: o[0].copy_(y0), reps)
        copy_gbs = 2 * n * elt / copy_ms / 1e6
        ms = {"stage1": _time(lambda: be._sde_srk_stage1(o[0], o[1], o[2], y0, a1, b1, dt, s, seed, k), reps),
              "stage2": _time(lambda: be._sde_srk_stage2(o[0], y0, a1, b1, b2, b3, dt, s), reps),
              "step": _time(lambda: be._sde_srk_step(o[0], y0, a1, a2, b1, b2, b3, b4, dt, s, c, c3, seed, k), reps),
              "stage1_bwd": _time(lambda: be._sde_srk_stage1_backward(o[0], o[1], o[2], gy, gz, a1, dt, s, seed, k), reps),
              "stage2_bwd": _time(lambda: be._sde_srk_stage2_backward(o[0], o[1], o[2], o[3], gy, dt, s), reps),
              "step_bwd": _time(lambda: be._sde_srk_step_backward(*o, gy, dt, s, c, c3, seed, k), reps)}
        noise_ms = [_time(lambda d=d: be._sde_noise(o[0], seed, k, draw=d), reps) for d in (0, 1)]
        r3 = 3.0**-0.5

        def framework():
            w = s * torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)
            p = 0.5 * (w + (s * torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)) * r3)
            q = c * (w * w - dt)
            u = c3 * ((w * w - 3.0 * dt) * w)
            Y2 = (y0 + a1 * (0.75 * dt)) + b1 * (1.5 * p)
            G2 = (y0 + a1 * (0.25 * dt)) + b1 * (0.5 * s)
            G3 = (y0 + a1 * dt) - b1 * s
            G4 = (y0 + a1 * (0.25 * dt)) + ((b1 * -5.0 + b2 * 3.0) + b3 * 0.5) * s
            e1, e2 = ((-w - q) + 2.0 * p) - 2.0 * u, (4.0 / 3.0) * ((w + q) - p) + (5.0 / 3.0) * u
            e3 = (2.0 / 3.0) * ((w - p) - u) - q / 3.0
            y1 = ((((y0 + (a1 / 3.0 + a2 * (2.0 / 3.0)) * dt) + b1 * e1) + b2 * e2) + b3 * e3) + b4 * u
            return Y2, G2, G3, G4, y1

        fw_ms = _time(framework, reps)
        step_ms = ms["stage1"] + ms["stage2"] + ms["step"]
        row = {"dtype": str(dtype).split(".")[-1], "n": n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1)}
        for name, (elems, _) in KERNELS.items():
            row[name + "_ms"] = round(ms[name], 4)
            row[name + "_bytes"] = elems * n * elt
            row[name + "_of_copy"] = round(elems * n * elt / ms[name] / 1e6 / copy_gbs, 3)
            row[name + "_memory_floor_ms"] = round(elems * n * elt / copy_gbs / 1e6, 4)
        row.update({"noise0_ms": round(noise_ms[0], 4), "noise1_ms": round(noise_ms[1], 4), "three_launches_ms": round(step_ms, 4),
                    "framework_ms": round(fw_ms, 4), "speedup_over_framework": round(fw_ms / step_ms, 2)})
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def merge_kernel_stats(out, path):
    """Per kernel of ours (and the copy) the call count, average and minimum duration from rocprofv3's kernel_stats.csv, and for the six
    SRK kernels the fraction of the copy rate that the events run in ``out`` measured."""
    with open(out) as fh:
        res = json.load(fh)
    kernels = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Name"]
            if "xde_sde_" in name or "copyBuffer" in name or name.startswith("at::native"):
                kernels[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(r["MinNs"]) / 1e3, 2)}
    of_copy = {}
    for row in res["kernels"]:
        t = "float" if row["dtype"] == "float32" else "double"
        d = {}
        for key, (_, inst) in KERNELS.items():  # xde_sde_step_kernel<T, VEC, NOISE, formula, output mask>
            hit = [v for k, v in kernels.items() if "xde_sde_step_kernel<{}, true, {}>".format(t, inst) in k]
            if hit:
                d[key + "_us"] = hit[0]["avg_us"]
                d[key + "_of_copy"] = round(row[key + "_bytes"] / (hit[0]["avg_us"] * 1e-6) / 1e9 / row["copy_GBps"], 3)
        hit = [v for k, v in kernels.items() if "xde_sde_noise_kernel<{}, false>".format(t) in k]
        if hit:
            d["noise_us"] = hit[0]["avg_us"]
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
