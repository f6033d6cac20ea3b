"""Measurements of sdeint's Euler-Maruyama kernels.

    python profiles/tools/sde.py [--out FILE] [--reps N]

At n = 65536 x 128, fp32 and fp64:
  fwd       xde_sde_em_step: 4 n elt bytes (y0, f, g read, y1 written) over the launch time, as a fraction of a same-size device copy
            (2 n elt bytes) timed in the same process
  bwd       xde_sde_em_backward with both outputs: 3 n elt bytes (gy1 read, gf and gg written), same fraction
  noise     xde_sde_noise: the generator alone, writing n normals (n elt bytes) — its time against fwd's tells whether the step is bound
            by the Philox rounds and Box-Muller (compute) or by memory
  framework the same step as framework ops: z = randn; y1 = (y0 + f*dt) + g*(s*z) (the speed-up of fwd over it)
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps, and, where fp64 looks
compute-bound, once under `rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES GRBM_GUI_ACTIVE` on its own.
Prints one JSON object (and writes it to --out)."""
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
N_ROWS, N_COLS = 65536, 128


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
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        n = N_ROWS * N_COLS
        g = torch.Generator().manual_seed(0)
        y0, f, gd, gy = (torch.randn(N_ROWS, N_COLS, generator=g).to(DEV, dtype) for _ in range(4))
        y1, gf, gg, z = (torch.empty_like(y0) for _ in range(4))
        dt = 1e-3
        s = math.sqrt(dt)
        copy_ms = _time(lambda: y1.copy_(y0), reps)
        copy_gbs = 2 * n * elt / copy_ms / 1e6
        fwd_ms = _time(lambda: be._sde_em_step(y1, y0, f, gd, dt, s, 12345, 7), reps)
        bwd_ms = _time(lambda: be._sde_em_backward(gf, gg, gy, dt, s, 12345, 7), reps)
        noise_ms = _time(lambda: be._sde_noise(z, 12345, 7), reps)

        def framework():
            zz = torch.randn(N_ROWS, N_COLS, dtype=dtype, device=DEV)
            return (y0 + f * dt) + gd * (s * zz)

        fw_ms = _time(framework, reps)
        row = {"dtype": str(dtype).split(".")[-1], "n": n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1),
               "fwd_ms": round(fwd_ms, 4), "fwd_GBps": round(4 * n * elt / fwd_ms / 1e6, 1),
               "fwd_of_copy": round(4 * n * elt / fwd_ms / 1e6 / copy_gbs, 3),
               "bwd_ms": round(bwd_ms, 4), "bwd_GBps": round(3 * n * elt / bwd_ms / 1e6, 1),
               "bwd_of_copy": round(3 * n * elt / bwd_ms / 1e6 / copy_gbs, 3),
               "noise_ms": round(noise_ms, 4), "fwd_memory_floor_ms": round(4 * n * elt / copy_gbs / 1e6, 4),
               "framework_ms": round(fw_ms, 4), "speedup_over_framework": round(fw_ms / fwd_ms, 2)}
        # bound: the generator alone against the memory time of the step at the copy rate
        row["bound"] = "compute" if noise_ms > row["fwd_memory_floor_ms"] else "memory"
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shape": [N_ROWS, N_COLS], "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
