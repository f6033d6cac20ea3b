"""Measurements of cdeint's contraction kernels on the natural cubic spline control.

    python profiles/tools/cde_natural.py [--out FILE] [--reps N] [--rounds R]

At B x H x C = 8192 x 64 x 32 (F is 64 MiB in fp32), Tn = 32, fp32 and fp64, alternating in ONE process, round by round:
  copy            a same-size device copy (F copied: 2 B H C elt bytes)
  cubic fwd/bwd   xde_cde_contract / _backward on the CubicHermiteSpline through the same series: (B H C + B H + 3 B C) elt bytes
  natural fwd/bwd xde_cde_contract_natural / _backward on the NaturalCubicSpline through it (a fifth of the interior entries missing,
                  the knots irregular): four control rows per batch row, (B H C + B H + 4 B C) elt bytes
  framework       the natural control as framework ops: dX = X.derivative(t) (the gather launch), then einsum("bhc,bc->bh", F, dX);
                  backward gout[:, :, None] * dX[:, None, :]
  coeffs          the coefficient launch of the control (once per control, not per step: its time only)
Every figure is the median over --rounds rounds of --reps launches between two device events, warmed.  THE CONDITION, per dtype and
direction: natural_ms <= cubic_ms * (natural bytes / cubic bytes) + 3 * max(spread of natural, spread of cubic), a spread being
max - min over the rounds.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402
from paddlexde_amd.interpolation import CubicHermiteSpline, NaturalCubicSpline  # noqa: E402

DEV = "cuda"
B, H, C, TN = 8192, 64, 32, 32


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


def measure(reps, rounds):
    be = _hip.get_backend()
    res = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        g = torch.Generator().manual_seed(0)
        F = torch.randn(B, H, C, generator=g).to(DEV, dtype)
        gout = torch.randn(B, H, generator=g).to(DEV, dtype)
        series = torch.randn(B, TN, C, generator=g).to(DEV, dtype)
        knots = torch.cumsum(0.25 + 1.5 * torch.rand(TN, generator=g), 0).to(DEV, dtype)
        holes = series.clone()
        holes[:, 1:-1][torch.rand(B, TN - 2, C, generator=g).to(DEV) < 0.2] = float("nan")
        Xc = CubicHermiteSpline(series)
        Xn = NaturalCubicSpline(holes, knots)
        tc = torch.tensor(11.3, dtype=torch.float64, device=DEV)
        tn = (0.37 * knots[0] + 0.63 * knots[-1]).to(torch.float64)
        out, gF, F2 = torch.empty(B, H, dtype=dtype, device=DEV), torch.empty_like(F), torch.empty_like(F)
        Y, M = torch.empty_like(holes), torch.empty_like(holes)
        runs = {
            "copy": lambda: F2.copy_(F),
            "cubic_fwd": lambda: be._cde_contract(out, F, Xc._series, Xc._t, tc, "cubic"),
            "natural_fwd": lambda: be._cde_contract_natural(out, F, Xn._series, Xn._coef, Xn._t, tn),
            "natural_fwd_framework": lambda: torch.einsum("bhc,bc->bh", F, Xn.derivative(tn)[:, 0, :]),
            "cubic_bwd": lambda: be._cde_contract_backward(gF, gout, Xc._series, Xc._t, tc, "cubic"),
            "natural_bwd": lambda: be._cde_contract_natural_backward(gF, gout, Xn._series, Xn._coef, Xn._t, tn),
            "natural_bwd_framework": lambda: gout[:, :, None] * Xn.derivative(tn)[:, 0, :][:, None, :],
            "coeffs": lambda: be._spline_natural_coeffs(Y, M, holes, knots),
        }
        # same results first (the framework sum runs in another order: a tolerance of the dtype's size)
        tol = 1e-4 if dtype == torch.float32 else 1e-12
        runs["natural_fwd"]()
        assert torch.allclose(out, runs["natural_fwd_framework"](), rtol=tol, atol=tol * C)
        runs["natural_bwd"]()
        assert torch.equal(gF, runs["natural_bwd_framework"]())
        runs["coeffs"]()
        assert torch.equal(Y, Xn._series) and torch.equal(M, Xn._coef)
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(_time(fn, reps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        moved = {"cubic": (B * H * C + B * H + 3 * B * C) * elt, "natural": (B * H * C + B * H + 4 * B * C) * elt}
        copy_gbs = 2 * B * H * C * elt / med["copy"] / 1e6
        row = {"B": B, "H": H, "C": C, "Tn": TN, "dtype": str(dtype).split(".")[-1], "F_MiB": round(B * H * C * elt / 2**20, 2),
               "copy_ms": round(med["copy"], 4), "copy_GBps": round(copy_gbs, 1), "byte_ratio": round(moved["natural"] / moved["cubic"], 5),
               "coeffs_ms": round(med["coeffs"], 4), "coeffs_ms_spread": [round(min(ms["coeffs"]), 4), round(max(ms["coeffs"]), 4)]}
        for d in ("fwd", "bwd"):
            for ctl in ("cubic", "natural"):
                k = ctl + "_" + d
                row[k + "_ms"] = round(med[k], 4)
                row[k + "_ms_spread"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
                row[k + "_of_copy"] = round(moved[ctl] / med[k] / 1e6 / copy_gbs, 3)
            allowed = med["cubic_" + d] * moved["natural"] / moved["cubic"] + 3 * max(spread["natural_" + d], spread["cubic_" + d])
            row[d + "_allowed_ms"] = round(allowed, 4)
            row[d + "_condition_met"] = bool(med["natural_" + d] <= allowed)
            row["natural_" + d + "_framework_ms"] = round(med["natural_" + d + "_framework"], 4)
            row["natural_" + d + "_speedup_over_framework"] = round(med["natural_" + d + "_framework"] / med["natural_" + d], 2)
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("profiles/tools/cde_natural.py measures on the GPU: no device found")
    res = {"device": torch.cuda.get_device_name(0), "kernels": measure(args.reps, args.rounds)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
