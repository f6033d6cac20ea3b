"""Measurements of the Hermite-tape kernels of ddeint_steps, by the method of profiles/tools/sde_gn.py.

    python profiles/tools/dde_tape.py [--out profiles/dde_tape.json] [--reps N]

At (rows, D, L) = 65536 x 128 x 4, fp32 and fp64, every time an event time over ``reps`` launches and every rate a fraction of a
device copy that moves the SAME bytes (a buffer of half the launch's bytes, read and written) timed in the same process; N = rows * D.
The operands are what a stage of a walk reads: delay 0 in the history's last interval (strided rows, its end state a tape node),
delays 1 and 2 in one tape interval, delay 3 in the next:
  fwd        xde_dde_tape_gather without dtau: 4 L N elt read, L N written
  fwd_dtau   ... with dtau: 4 L N read, 2 L N written
  bwd        xde_dde_tape_gather_backward into the stage's distinct tape tensors (7 here): L N elt read, 7 N written
  framework  the same values in framework ops, per delay four operand reads and the weighted sum
             ``(ya*a0 + fa*a1) + (yb*a2 + fb*a3)``, stacked on the delay axis; framework_bwd: per tensor the sum of ``g[:, j] * w``
             over its terms
The yardstick is the project's 0.70 of the copy for fp32 streaming kernels; it is reported, not asserted.
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps.  Counters, if any,
come from a run of their own.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402
from paddlexde_amd.xde.steps_dde import hermite_weights  # noqa: E402

DEV = "cuda"
SHAPE = (65536, 128, 4)
YARDSTICK = 0.70


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
    rows, D, L = SHAPE
    res = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        n = rows * D
        gen = torch.Generator().manual_seed(0)
        his, hf = (torch.randn(rows, 2, D, generator=gen).to(DEV, dtype) for _ in range(2))
        ys, fs = ([torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(4)] for _ in range(2))
        srcs = [his[:, 0], hf[:, 0], ys[0], hf[:, 1]]
        keys = [None, None, 0, None]
        for m in (1, 1, 2):
            srcs += [ys[m], fs[m], ys[m + 1], fs[m + 1]]
            keys += [m, 4 + m, m + 1, 4 + m + 1]
        w, wd = [], []
        for sigma, h in ((0.4, 0.25), (0.3, 0.125), (0.7, 0.125), (0.5, 0.125)):
            a, b = hermite_weights(sigma, h)
            w += a
            wd += b
        order = sorted({k for k in keys if k is not None})
        terms = [[(i // 4, w[i]) for i, k in enumerate(keys) if k == key] for key in order]
        out, dtau = (torch.empty(rows, L, D, dtype=dtype, device=DEV) for _ in range(2))
        g = torch.randn(rows, L, D, generator=gen).to(DEV, dtype)
        gouts = [torch.empty(rows, D, dtype=dtype, device=DEV) for _ in order]
        nbytes = {"fwd": 5 * L * n * elt, "fwd_dtau": 6 * L * n * elt, "bwd": (L + len(order)) * n * elt}

        def copy_of(nb):
            src = torch.empty(nb // 2 // elt, dtype=dtype, device=DEV).normal_()
            dst = torch.empty_like(src)
            return _time(lambda: dst.copy_(src), reps)

        def framework():
            return torch.stack([(srcs[4 * j] * w[4 * j] + srcs[4 * j + 1] * w[4 * j + 1]) + (srcs[4 * j + 2] * w[4 * j + 2] + srcs[4 * j + 3] * w[4 * j + 3])
                                for j in range(L)], dim=1)

        def framework_bwd():
            outs = []
            for ts in terms:
                acc = g[:, ts[0][0]] * ts[0][1]
                for j, x in ts[1:]:
                    acc = acc + g[:, j] * x
                outs.append(acc)
            return outs

        ms = {"fwd": _time(lambda: be._dde_tape_gather(out, None, srcs, w), reps),
              "fwd_dtau": _time(lambda: be._dde_tape_gather(out, dtau, srcs, w, wd), reps),
              "bwd": _time(lambda: be._dde_tape_gather_backward(gouts, terms, g), reps)}
        row = {"dtype": str(dtype).split(".")[-1], "rows": rows, "D": D, "L": L, "bwd_outputs": len(order)}
        for name in ("fwd", "fwd_dtau", "bwd"):
            copy_ms = copy_of(nbytes[name])
            row.update({name + "_bytes": nbytes[name], name + "_ms": round(ms[name], 4), name + "_copy_ms": round(copy_ms, 4),
                        name + "_GBps": round(nbytes[name] / ms[name] / 1e6, 1), name + "_of_copy": round(copy_ms / ms[name], 3)})
        fw_ms, fwb_ms = _time(framework, reps), _time(framework_bwd, reps)
        row.update({"framework_ms": round(fw_ms, 4), "fwd_speedup": round(fw_ms / ms["fwd"], 2),
                    "framework_bwd_ms": round(fwb_ms, 4), "bwd_speedup": round(fwb_ms / ms["bwd"], 2), "yardstick_of_copy": YARDSTICK})
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
