"""Measurements of sdeint's reversible Heun kernels.

    python profiles/tools/rheun.py [--out FILE] [--reps N]
    python profiles/tools/rheun.py --out FILE --kernel-stats CSV     (merge a rocprofv3 kernel_stats.csv into FILE)

At n = 65536 x 128, fp32 and fp64, each next to a same-size device copy (2 n elt bytes) timed in the same process:
  predict        xde_sde_rheun_predict: 5 n elt bytes (y0, yh0, f0, g0 read; yh1 written)
  correct        xde_sde_rheun_correct: 6 n (y0, f0, f1, g0, g1 read; y1 written)
  adjoint_stage  xde_sde_rheun_adjoint_stage with af1, ag1 given, in place (bf = af1, bg = ag1): 5 n
  adjoint_step   xde_sde_rheun_adjoint_step with ayh1 given, in place (ay0 = ay1, ayh0 = ayh1): 7 n
  forward        one forward step's two launches against the framework-op statement of the same formulas on given f1, g1 (one randn,
                 the prediction and the correction)
  backward       one backward-sweep step's four launches (stage, step, predict and correct at direction -1) against the framework-op
                 statement on a given v (one randn, the two cotangent formulas, the two reverse formulas)
The times here are device events around back-to-back launches (launch gaps included).  Kernel durations come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/rheun.py --reps 20`, whose kernel_stats.csv the second
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
STATS_COMMAND = "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/rheun.py --reps 20"
# name -> (elements moved per state element, the formula's instantiation in csrc/xde_sde.hip: NOISE, functor, output mask)
KERNELS = {"predict": (5, "true, (anonymous namespace)::RheunPredict, 1"), "correct": (6, "true, (anonymous namespace)::RheunCorrect, 1"),
           "adjoint_stage": (5, "true, (anonymous namespace)::RheunAdjointStage<false>, 3"),
           "adjoint_step": (7, "true, (anonymous namespace)::RheunAdjointStep<false>, 15")}


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
        y0, yh0, f0, f1, g0, g1, ay, ayh, af, ag, v = (torch.randn(N_ROWS, N_COLS, generator=g).to(DEV, dtype) for _ in range(11))
        o = [torch.empty_like(y0) for _ in range(4)]
        dt = 1e-3
        s = math.sqrt(dt)
        seed, k = 12345, 7
        copy_ms = _time(lambda: o[0].copy_(y0), reps)
        copy_gbs = 2 * n * elt / copy_ms / 1e6
        ms = {"predict": _time(lambda: be._sde_rheun_predict(o[0], y0, yh0, f0, g0, dt, s, 1, seed, k), reps),
              "correct": _time(lambda: be._sde_rheun_correct(o[0], y0, f0, f1, g0, g1, dt, s, 1, seed, k), reps),
              "adjoint_stage": _time(lambda: be._sde_rheun_adjoint_stage(af, ag, af, ag, ay, dt, s, seed, k), reps),
              "adjoint_step": _time(lambda: be._sde_rheun_adjoint_step(ay, ayh, o[2], o[3], ay, ayh, v, dt, s, seed, k), reps)}

        def forward_launches():
            be._sde_rheun_predict(o[0], y0, yh0, f0, g0, dt, s, 1, seed, k)
            be._sde_rheun_correct(o[1], y0, f0, f1, g0, g1, dt, s, 1, seed, k)

        def forward_framework():
            w = s * torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)
            yh1 = (((y0 + y0) - yh0) + f0 * dt) + g0 * w
            y1 = (y0 + (f0 + f1) * (0.5 * dt)) + (g0 + g1) * (0.5 * w)
            return yh1, y1

        def backward_launches():
            be._sde_rheun_adjoint_stage(af, ag, af, ag, ay, dt, s, seed, k)
            be._sde_rheun_adjoint_step(ay, ayh, af, ag, ay, ayh, v, dt, s, seed, k)
            be._sde_rheun_predict(o[0], y0, yh0, f0, g0, dt, s, -1, seed, k)
            be._sde_rheun_correct(o[1], y0, f0, f1, g0, g1, dt, s, -1, seed, k)

        def backward_framework():
            w = s * torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)
            bf, bg = af + ay * (0.5 * dt), ag + ay * (0.5 * w)
            A = ayh + v
            ay0, ayh0, af0, ag0 = ay + (A + A), -A, ay * (0.5 * dt) + A * dt, ay * (0.5 * w) + A * w
            yhb = (((y0 + y0) - yh0) - f0 * dt) - g0 * w
            yb = (y0 - (f0 + f1) * (0.5 * dt)) - (g0 + g1) * (0.5 * w)
            return bf, bg, ay0, ayh0, af0, ag0, yhb, yb

        fwd_ms, fwd_fw_ms = _time(forward_launches, reps), _time(forward_framework, reps)
        ay.normal_(), ayh.normal_(), af.normal_(), ag.normal_()  # (the in-place timings above grew them)
        bwd_ms, bwd_fw_ms = _time(backward_launches, reps), _time(backward_framework, reps)
        row = {"dtype": str(dtype).split(".")[-1], "n": n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1)}
        for name, (elems, _) in KERNELS.items():
            row[name + "_ms"] = round(ms[name], 4)
            row[name + "_bytes"] = elems * n * elt
            row[name + "_of_copy"] = round(elems * n * elt / ms[name] / 1e6 / copy_gbs, 3)
            row[name + "_memory_floor_ms"] = round(elems * n * elt / copy_gbs / 1e6, 4)
        row.update({"forward_step_ms": round(fwd_ms, 4), "forward_framework_ms": round(fwd_fw_ms, 4),
                    "forward_speedup_over_framework": round(fwd_fw_ms / fwd_ms, 2), "backward_step_ms": round(bwd_ms, 4),
                    "backward_framework_ms": round(bwd_fw_ms, 4), "backward_speedup_over_framework": round(bwd_fw_ms / bwd_ms, 2)})
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def merge_kernel_stats(out, path):
    """Per kernel of ours (and the copy) the call count, average and minimum duration from rocprofv3's kernel_stats.csv, and for the four
    reversible Heun kernels the fraction of the copy rate that the events run in ``out`` measured."""
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
