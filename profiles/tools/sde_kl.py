"""Measurements of the latent-SDE KL kernels, by the method of profiles/tools/sde.py.

    python profiles/tools/sde_kl.py [--out profiles/sde_kl.json] [--reps N]

At 65536 x 128 (the SDE profile's shape: 32 fp32 / 64 fp64 lanes a row) and 262144 x 8 (the sub-wave path: 2 / 4 lanes a row), fp32 and
fp64, every time an event time over ``reps`` launches and every rate a fraction of a same-size device copy (2 N elt bytes) timed in
the same process:
  fwd        xde_sde_kl_step: 5 N elt + 16 rows bytes (y0, f, g, h read, y1 written; acc0 read, acc1 written)
  acc        the accumulate-only mode: 3 N elt + 16 rows bytes
  bwd        xde_sde_kl_backward with gy1 and all three outputs: 4 N elt + 8 rows bytes read, 3 N elt written
  em         xde_sde_em_step alone (4 N elt), the launch fwd replaces
  framework  what fwd replaces: xde_sde_em_step plus ``((f - h)/g).square().sum(-1) * (0.5*dt) + acc`` in framework ops (float64 sum);
             framework_acc is those ops alone (what acc replaces), framework_bwd their autograd backward plus xde_sde_em_backward
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps, and reduce that
run's `*_kernel_trace.csv` to per-shape medians with

    python profiles/tools/sde_kl.py --reduce-trace profiles/sde_kl_kernel_trace.csv [--out profiles/sde_kl_kernel_medians.json]

(no GPU needed).  Counters, if any, come from a run of their own.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402

DEV = "cuda"
SHAPES = ((65536, 128), (262144, 8))


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


def measure(reps):
    be = _hip.get_backend()
    res = []
    for rows, D in SHAPES:
        for dtype in (torch.float32, torch.float64):
            elt = torch.empty((), dtype=dtype).element_size()
            n = rows * D
            gen = torch.Generator().manual_seed(0)
            y0, f, h, gy = (torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(4))
            gd = (0.5 + torch.rand(rows, D, generator=gen)).to(DEV, dtype)
            y1, gf, gg, gh = (torch.empty_like(y0) for _ in range(4))
            acc0 = torch.rand(rows, generator=gen, dtype=torch.float64).to(DEV)
            acc1, gacc = torch.empty_like(acc0), torch.ones_like(acc0)
            dt = 1e-3
            s = math.sqrt(dt)
            copy_ms = _time(lambda: y1.copy_(y0), reps)
            copy_gbs = 2 * n * elt / copy_ms / 1e6
            frac = lambda nbytes, ms: round(nbytes / ms / 1e6 / copy_gbs, 3)  # noqa: E731
            fwd_ms = _time(lambda: be._sde_kl_step(y1, acc1, y0, f, gd, h, acc0, dt, s, 12345, 7), reps)
            acc_ms = _time(lambda: be._sde_kl_step(None, acc1, None, f, gd, h, acc0, dt, 0.0, 0, 0), reps)
            bwd_ms = _time(lambda: be._sde_kl_backward(gf, gg, gh, gy, gacc, f, gd, h, dt, s, 12345, 7), reps)
            em_ms = _time(lambda: be._sde_em_step(y1, y0, f, gd, dt, s, 12345, 7), reps)

            def framework_acc():
                return ((f - h) / gd).square().sum(-1, dtype=torch.float64) * (0.5 * dt) + acc0

            def framework():
                be._sde_em_step(y1, y0, f, gd, dt, s, 12345, 7)
                return framework_acc()

            fr, gr, hr = (x.clone().requires_grad_(True) for x in (f, gd, h))

            def framework_bwd():
                be._sde_em_backward(gf, gg, gy, dt, s, 12345, 7)
                out = ((fr - hr) / gr).square().sum(-1, dtype=torch.float64) * (0.5 * dt) + acc0
                return torch.autograd.grad(out, (fr, gr, hr), gacc)

            fw_ms, fwa_ms, fwb_ms = _time(framework, reps), _time(framework_acc, reps), _time(framework_bwd, reps)
            row = {"dtype": str(dtype).split(".")[-1], "rows": rows, "D": D, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1),
                   "fwd_ms": round(fwd_ms, 4), "fwd_of_copy": frac(5 * n * elt + 16 * rows, fwd_ms),
                   "acc_ms": round(acc_ms, 4), "acc_of_copy": frac(3 * n * elt + 16 * rows, acc_ms),
                   "bwd_ms": round(bwd_ms, 4), "bwd_of_copy": frac(7 * n * elt + 8 * rows, bwd_ms),
                   "em_ms": round(em_ms, 4), "em_of_copy": frac(4 * n * elt, em_ms),
                   "framework_ms": round(fw_ms, 4), "fwd_speedup": round(fw_ms / fwd_ms, 2),
                   "framework_acc_ms": round(fwa_ms, 4), "acc_speedup": round(fwa_ms / acc_ms, 2),
                   "framework_bwd_ms": round(fwb_ms, 4), "bwd_speedup": round(fwb_ms / bwd_ms, 2)}
            res.append(row)
            print(json.dumps(row), flush=True)
    return res


def reduce_trace(path):
    """Per-shape kernel durations from the ``*_kernel_trace.csv`` of a `rocprofv3 --kernel-trace` run of this tool (no GPU needed).  The
    run measures the shapes of SHAPES one after the other with the same number of dispatches each, and both shapes launch the same
    grid, so the dispatches of a kernel are split by dispatch order: the i-th of len(SHAPES) equal parts belongs to SHAPES[i].  Returns
    one row per (kernel, dtype, variant) with the median and the minimum in microseconds per shape."""
    import collections
    import csv
    import re

    rows = sorted((r for r in csv.DictReader(open(path)) if "xde_sde" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    per = collections.defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"]
        m = re.search(r"(xde_sde_\w+)<(\w+), (\w+), (\w+)", name)
        if "_kl_" in name:  # <T, VEC, STEP | GY>
            variant = {"xde_sde_kl_step_kernel": {"true": "step", "false": "accumulate_only"},
                       "xde_sde_kl_backward_kernel": {"true": "with_gy1", "false": "without_gy1"}}[m.group(1)][m.group(4)]
        else:
            variant = "em_backward" if "EmBackward" in name else "em_step"
        per[(m.group(1), m.group(2), variant)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = []
    for (kernel, dtype, variant), us in sorted(per.items()):
        part = len(us) // len(SHAPES)
        row = {"kernel": kernel, "dtype": dtype, "variant": variant, "dispatches_per_shape": part}
        for i, (n_rows, D) in enumerate(SHAPES):
            v = sorted(us[i * part : (i + 1) * part])
            row["{}x{}".format(n_rows, D)] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
        out.append(row)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reduce-trace", metavar="CSV", help="reduce a rocprofv3 kernel trace of this tool to per-shape medians and exit")
    args = ap.parse_args()
    if args.reduce_trace:
        res = {"trace": os.path.basename(args.reduce_trace), "shapes": [list(x) for x in SHAPES], "kernels": reduce_trace(args.reduce_trace)}
        print(json.dumps(res, indent=1))
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        sys.exit(0)
    res = {"device": torch.cuda.get_device_name(0), "shapes": [list(x) for x in SHAPES], "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
