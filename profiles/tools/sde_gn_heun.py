"""Measurement of the general-noise Heun launches, by the method of profiles/tools/sde_gn.py.

    python profiles/tools/sde_gn_heun.py [--out profiles/sde_gn_heun.json] [--reps N]

At (rows, D, M) = 65536 x 32 x 8, fp32, every time an event time over ``reps`` back-to-back launches after warm-up; N = rows * D:
  euler     xde_sde_gn_step: (3 + M) N elt read, N written
  heun      xde_sde_gn_heun_predict then xde_sde_gn_heun_correct: (3 + M) N + (4 + M) N read, 3 N written — (2 M + 10) N in all
  composed  the three-stream composition, timed as three xde_sde_gn_step launches (yp from g0, a second pass over g0, a pass over
            g1): (3 M + 12) N, three N more than the per-formula count (3 M + 9) N
  copy      a device copy that moves the bytes of the heun pair (a buffer of half of them, read and written): the bandwidth ceiling
The default 20000 launches make every timed window 0.5 to 1.6 s.  The operands of one pair (about 184 MB) and the copy's buffers fit in
the device's last-level cache, as they do for profiles/tools/sde_gn.py: the figures compare launches under the same conditions and are
not rates out of HBM.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402
from profiles.tools.sde_gn import DEV, _time  # noqa: E402


def measure(reps, rows=65536, D=32, M=8, dtype=torch.float32):
    be = _hip.get_backend()
    elt, n = torch.empty((), dtype=dtype).element_size(), rows * D
    gen = torch.Generator().manual_seed(0)
    y0, f0, f1 = (torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(3))
    g0, g1 = (torch.randn(rows, D, M, generator=gen).to(DEV, dtype) for _ in range(2))
    yp, a0, y1 = (torch.empty_like(y0) for _ in range(3))
    dt = 1e-3
    s = math.sqrt(dt)
    heun_bytes = (2 * M + 10) * n * elt

    def heun():
        be._sde_gn_heun_predict(yp, a0, y0, f0, g0, dt, s, 12345, 7)
        be._sde_gn_heun_correct(y1, y0, f0, f1, a0, g1, dt, s, 12345, 7)

    def composed():
        be._sde_gn_step(yp, y0, f0, g0, dt, s, 12345, 7)
        be._sde_gn_step(a0, y0, f0, g0, dt, s, 12345, 7)
        be._sde_gn_step(y1, y0, f1, g1, dt, s, 12345, 7)

    src = torch.empty(heun_bytes // 2 // elt, dtype=dtype, device=DEV).normal_()
    dst = torch.empty_like(src)
    res = {"rows": rows, "D": D, "M": M, "dtype": str(dtype).split(".")[-1], "heun_bytes": heun_bytes}
    # (each figure twice, alternating, so a drift of the machine shows as a spread)
    for rnd in (0, 1):
        res["copy_ms_%d" % rnd] = round(_time(lambda: dst.copy_(src), reps), 4)
        res["euler_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_step(y1, y0, f0, g0, dt, s, 12345, 7), reps), 4)
        res["heun_ms_%d" % rnd] = round(_time(heun, reps), 4)
        res["predict_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_heun_predict(yp, a0, y0, f0, g0, dt, s, 12345, 7), reps), 4)
        res["correct_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_heun_correct(y1, y0, f0, f1, a0, g1, dt, s, 12345, 7), reps), 4)
        res["composed_ms_%d" % rnd] = round(_time(composed, reps), 4)
    best = lambda key: min(res[key + "_0"], res[key + "_1"])  # noqa: E731
    res["heun_over_euler"] = round(best("heun_ms") / best("euler_ms"), 3)
    res["composed_over_euler"] = round(best("composed_ms") / best("euler_ms"), 3)
    res["heun_of_copy"] = round(best("copy_ms") / best("heun_ms"), 3)
    res["heun_GBps"] = round(heun_bytes / best("heun_ms") / 1e6, 1)
    res["copy_GBps"] = round(heun_bytes / best("copy_ms") / 1e6, 1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20000)
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), **measure(args.reps))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
