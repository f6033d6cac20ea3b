"""Measurement of the general-noise reversible Heun launches, by the method of profiles/tools/sde_gn_heun.py.

    python profiles/tools/sde_gn_rheun.py [--out profiles/sde_gn_rheun.json] [--reps N]

At (rows, D, M) = 65536 x 32 x 8, fp32, every time an event time over ``reps`` back-to-back launches after warm-up; N = rows * D:
  seam      xde_sde_gn_rheun_seam: (6 + M) N elt read, 3 N written — (M + 9) N
  pair      xde_sde_gn_heun_correct then xde_sde_gn_rheun_predict, what the seam stands for: (2 M + 12) N with the re-read of y1
  euler     xde_sde_gn_step, section 21's unit: the unfused pair is "two Euler steps"
  stage     xde_sde_gn_rheun_adjoint_stage, full form: 3 N read, (1 + M) N written
  copy      a device copy of the stage's bytes (a buffer of half of them, read and written)
  backward  one backward step of the sweep without its vjp — stage then xde_sde_gn_rheun_adjoint_step — against its statement in
            framework ops on the read-back increments
No time is a pass condition; the yardstick is the byte ratio (M + 8) / (2 M + 11).  The operands fit in the device's last-level cache,
as in sections 16 and 21: the figures compare launches under the same conditions and are not rates out of HBM.  Prints one JSON object
(and writes it to --out)."""
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
    y0, f0, f1, a0, yh1, ay, af, c, ayh, v = (torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(10))
    g1 = torch.randn(rows, D, M, generator=gen).to(DEV, dtype)
    y1, yh2, a1, bf, o1, o2, o3, o4 = (torch.empty_like(y0) for _ in range(8))
    bg = torch.empty_like(g1)
    dt, dt1, seed, k = 1e-3, 2e-3, 12345, 7
    s, s1 = math.sqrt(dt), math.sqrt(dt1)
    w0, w1 = torch.empty(rows, M, dtype=dtype, device=DEV), torch.empty(rows, M, dtype=dtype, device=DEV)
    be._sde_noise(w0, seed, k)
    be._sde_noise(w1, seed, k + 1)
    w0, w1 = (w0 * s).unsqueeze(-2), (w1 * s1).unsqueeze(-2)
    stage_bytes = (4 + M) * n * elt

    def pair():
        be._sde_gn_heun_correct(y1, y0, f0, f1, a0, g1, dt, s, seed, k)
        be._sde_gn_rheun_predict(yh2, a1, y1, yh1, f1, g1, dt1, s1, seed, k + 1)

    def backward():
        be._sde_gn_rheun_adjoint_stage(bf, bg, af, c, ay, dt, s, k, s1, k + 1, seed)
        be._sde_gn_rheun_adjoint_step(o1, o2, o3, o4, ay, ayh, v, dt)

    def backward_ops():
        af + ay * (0.5 * dt)
        c.unsqueeze(-1) * w1 + (ay * 0.5).unsqueeze(-1) * w0
        A = ayh + v
        return ay + (A + A), -A, ay * (0.5 * dt) + A * dt, ay * 0.5 + A

    src = torch.empty(stage_bytes // 2 // elt, dtype=dtype, device=DEV).normal_()
    dst = torch.empty_like(src)
    res = {"rows": rows, "D": D, "M": M, "dtype": str(dtype).split(".")[-1], "byte_ratio": round((M + 8) / (2 * M + 11), 3), "stage_bytes": stage_bytes}
    for rnd in (0, 1):  # (each figure twice, alternating, so a drift of the machine shows as a spread)
        res["euler_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_step(y1, y0, f0, g1, dt, s, seed, k), reps), 4)
        res["seam_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_rheun_seam(y1, yh2, a1, y0, f0, f1, a0, yh1, g1, dt, s, k, dt1, s1, k + 1, seed), reps), 4)
        res["pair_ms_%d" % rnd] = round(_time(pair, reps), 4)
        res["stage_ms_%d" % rnd] = round(_time(lambda: be._sde_gn_rheun_adjoint_stage(bf, bg, af, c, ay, dt, s, k, s1, k + 1, seed), reps), 4)
        res["copy_ms_%d" % rnd] = round(_time(lambda: dst.copy_(src), reps), 4)
        res["backward_ms_%d" % rnd] = round(_time(backward, reps), 4)
        res["backward_ops_ms_%d" % rnd] = round(_time(backward_ops, max(reps // 10, 10)), 4)
    best = lambda key: min(res[key + "_0"], res[key + "_1"])  # noqa: E731
    res["seam_over_pair"] = round(best("seam_ms") / best("pair_ms"), 3)
    res["pair_over_euler"] = round(best("pair_ms") / best("euler_ms"), 3)
    res["seam_over_euler"] = round(best("seam_ms") / best("euler_ms"), 3)
    res["stage_of_copy"] = round(best("copy_ms") / best("stage_ms"), 3)
    res["backward_over_ops"] = round(best("backward_ms") / best("backward_ops_ms"), 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5000)
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, **measure(args.reps))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
