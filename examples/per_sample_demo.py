#!/usr/bin/env python3
"""Per-sample adaptive stepping: every batch row its own step size (``options={"per_sample": True}``).

Five independent samples of ``y' = -lam (y - cos t)`` on ``[0, 2]`` with lam = 0.5, 2, 10, 50, 200 (D = 3), Dopri5 at rtol 1e-5,
atol 1e-7.  The default (joint) solve takes ONE step size for the whole batch from one RMS norm over all rows: the easy rows are
dragged through the stiffest row's attempts, and that row's error is diluted by the easy ones, so it misses its own tolerance.  Under
``per_sample`` every row is stepped as if it were solved alone.  Prints, per row, the attempts of both solves and the error against a
tight reference solve (rtol 1e-10, atol 1e-12, float64).

    python examples/per_sample_demo.py [--dtype float32]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paddlexde_amd import Dopri5, odeint  # noqa: E402
from paddlexde_amd.utils import _rms_norm  # noqa: E402

LAM = (0.5, 2.0, 10.0, 50.0, 200.0)
RTOL, ATOL = 1e-5, 1e-7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float64", choices=["float32", "float64"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this demo needs a ROCm device"
    dev, dtype = torch.device("cuda:0"), getattr(torch, args.dtype)

    def problem(dt_):
        lam = torch.tensor(LAM, dtype=dt_, device=dev)[:, None]
        y0 = (torch.ones(len(LAM), 3, dtype=dt_) * torch.tensor([1.0, 0.5, -0.25], dtype=dt_)).to(dev)
        t = torch.linspace(0.0, 2.0, 5, dtype=dt_, device=dev)
        return (lambda t_, y: -lam * (y - torch.cos(t_))), y0, t

    with torch.no_grad():
        f, y0, t = problem(torch.float64)
        exact = odeint(f, y0, t, Dopri5, rtol=1e-10, atol=1e-12, options={"per_sample": True, "dtype": torch.float64})
        f, y0, t = problem(dtype)
        joint_stats, rows_stats = {}, {}
        joint = odeint(f, y0, t, Dopri5, rtol=RTOL, atol=ATOL, options={"norm": _rms_norm, "dtype": dtype, "stats_out": joint_stats})
        rows = odeint(f, y0, t, Dopri5, rtol=RTOL, atol=ATOL, options={"per_sample": True, "dtype": dtype, "stats_out": rows_stats})

    def err(sol):
        # the largest error over the outputs, in units of the row's own tolerance atol + rtol |y|
        e = (sol.double() - exact).abs() / (ATOL + RTOL * exact.abs())
        return e.amax(dim=(0, 2)).tolist()

    ja, jr = joint_stats["n_accept"], joint_stats["n_reject"]
    ra, rr = rows_stats["n_accept"].tolist(), rows_stats["n_reject"].tolist()
    print("Dopri5, rtol {:g}, atol {:g}, {} on {}".format(RTOL, ATOL, args.dtype, torch.cuda.get_device_name(0)))
    print("joint solve: {} + {} = {} attempts for every row".format(ja, jr, ja + jr))
    print("{:>6} {:>22} {:>22} {:>16} {:>16}".format("lam", "per_sample attempts", "joint attempts", "per_sample err", "joint err"))
    for r, (ej, er) in enumerate(zip(err(joint), err(rows))):
        print("{:>6g} {:>22} {:>22} {:>16.3g} {:>16.3g}".format(LAM[r], "{} + {} = {}".format(ra[r], rr[r], ra[r] + rr[r]),
                                                              "{} + {} = {}".format(ja, jr, ja + jr), er, ej))
    print("(err: largest |y - y_exact| / (atol + rtol |y_exact|) over the outputs; the local tolerance is held per step, so a "
          "global error of a few units is what a solve of this length gives)")
    # a row under per_sample IS the row solved alone (bit for bit); how far the joint solve drags each row from its own solve:
    apart = ((joint.double() - rows.double()).abs() / (ATOL + RTOL * rows.double().abs())).amax(dim=(0, 2)).tolist()
    print("joint solve, distance of each row from its own solve in tolerance units: " + ", ".join("{:.3g}".format(x) for x in apart))
    print("lam = 200: {:.3g} tolerance units from the exact solution under per_sample, {:.3g} in the joint solve, which ends {:.3g} "
          "units away from the row's own solve".format(err(rows)[-1], err(joint)[-1], apart[-1]))


if __name__ == "__main__":
    main()
