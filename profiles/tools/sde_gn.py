"""Measurements of the general-noise Euler-Maruyama kernels, by the method of profiles/tools/sde_kl.py.

    python profiles/tools/sde_gn.py [--out profiles/sde_gn.json] [--reps N]

At (rows, D, M) = 65536 x 32 x 8 (a hidden state of 32 under an 8-dimensional Brownian motion) and 65536 x 128 x 1 (scalar noise), fp32
and fp64, every time an event time over ``reps`` launches and every rate a fraction of a device copy that moves the SAME bytes (a
buffer of half the launch's bytes, read and written) timed in the same process; N = rows * D:
  fwd        xde_sde_gn_step: (3 + M) N elt read (y0, f, g), N written
  bwd        xde_sde_gn_backward with both outputs: N elt read (gy1), (1 + M) N written (gf, gg)
  framework  the same step in framework ops: xde_sde_noise on a [rows, M] buffer, ``w = s*Z``, ``einsum("rdm,rm->rd", g, w)`` and
             ``(y0 + f*dt) + a``; framework_bwd: the noise launch, ``gy1*dt`` and ``gy1[..., None] * w[:, None, :]``
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps.  Counters, if any,
come from a run of their own.  Prints one JSON object (and writes it to --out)."""
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
SHAPES = ((65536, 32, 8), (65536, 128, 1))


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
    for rows, D, M in SHAPES:
        for dtype in (torch.float32, torch.float64):
            elt = torch.empty((), dtype=dtype).element_size()
            n = rows * D
            gen = torch.Generator().manual_seed(0)
            y0, f, gy = (torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(3))
            g = torch.randn(rows, D, M, generator=gen).to(DEV, dtype)
            y1, gf, gg = torch.empty_like(y0), torch.empty_like(y0), torch.empty_like(g)
            z = torch.empty(rows, M, dtype=dtype, device=DEV)
            dt = 1e-3
            s = math.sqrt(dt)
            fwd_bytes, bwd_bytes = (4 + M) * n * elt, (2 + M) * n * elt

            def copy_of(nbytes):
                src = torch.empty(nbytes // 2 // elt, dtype=dtype, device=DEV).normal_()
                dst = torch.empty_like(src)
                ms = _time(lambda: dst.copy_(src), reps)
                return ms, 2 * src.numel() * elt / ms / 1e6

            fwd_copy_ms, fwd_copy_gbs = copy_of(fwd_bytes)
            bwd_copy_ms, bwd_copy_gbs = copy_of(bwd_bytes)
            fwd_ms = _time(lambda: be._sde_gn_step(y1, y0, f, g, dt, s, 12345, 7), reps)
            bwd_ms = _time(lambda: be._sde_gn_backward(gf, gg, gy, M, dt, s, 12345, 7), reps)
            gf_ms = _time(lambda: be._sde_gn_backward(gf, None, gy, M, dt, s, 12345, 7), reps)

            def framework():
                be._sde_noise(z, 12345, 7)
                return (y0 + f * dt) + torch.einsum("rdm,rm->rd", g, s * z)

            def framework_bwd():
                be._sde_noise(z, 12345, 7)
                return gy * dt, gy.unsqueeze(-1) * (s * z).unsqueeze(1)

            fw_ms, fwb_ms = _time(framework, reps), _time(framework_bwd, reps)
            row = {"dtype": str(dtype).split(".")[-1], "rows": rows, "D": D, "M": M,
                   "fwd_copy_ms": round(fwd_copy_ms, 4), "fwd_copy_GBps": round(fwd_copy_gbs, 1),
                   "bwd_copy_ms": round(bwd_copy_ms, 4), "bwd_copy_GBps": round(bwd_copy_gbs, 1),
                   "fwd_ms": round(fwd_ms, 4), "fwd_of_copy": round(fwd_copy_ms / fwd_ms, 3),
                   "bwd_ms": round(bwd_ms, 4), "bwd_of_copy": round(bwd_copy_ms / bwd_ms, 3),
                   "bwd_gf_only_ms": round(gf_ms, 4),
                   "framework_ms": round(fw_ms, 4), "fwd_speedup": round(fw_ms / fwd_ms, 2),
                   "framework_bwd_ms": round(fwb_ms, 4), "bwd_speedup": round(fwb_ms / bwd_ms, 2)}
            res.append(row)
            print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shapes": [list(x) for x in SHAPES], "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
