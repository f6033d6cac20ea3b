"""Measurements of the control-gradient kernels (include/xde_hip_cdegrad.h).

    python profiles/tools/cde_control_grad.py [--out FILE] [--reps N] [--rounds R]

At B x H x C = 8192 x 64 x 32 with Tn = 32 and, reported only, 256 x 32 x 8; fp32 and fp64; the natural and the cubic control:
  a            xde_cde_control_grad / _natural: F and gout read, the dense gradient written — (B H C + B H + n B Tn C) elt bytes (n = 1
               series, 2 for Y and M) over the launch time, as a fraction of a device copy that moves the same bytes (half of them
               read, half written) timed in the same process
  a_tn2        the same launch at Tn = 2, where no row is idle: what is left of `a` is the dense zero-fill of the Tn - 2 .. Tn - 4 rows
               X'(t) did not read
  fill         a memset of the gradient's bytes alone, for scale
  framework    the composition as framework ops: einsum("bh,bhc->bc", gout, F), the interval index read on the host (the composition
               needs it to index; t lives in device memory), the weights, and the rows assigned into torch.zeros
and once each at B C = 262144 columns, Tn = 32: coeffs_backward (b), gather_backward (c, one query time, both cotangents).
Every figure is the median over --rounds rounds that time the candidates one after the other (--reps launches each between two device
events, warmed), so they see the same machine state.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402

DEV = "cuda"
SHAPES = [("flagship", 8192, 64, 32), ("small", 256, 32, 8)]
TN = 32


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


def _framework(control, gout, F, knots, t_dev):
    """The gradient as framework ops (the middle of an interior interval, where every control reads its full set of rows)."""
    g = torch.einsum("bh,bhc->bc", gout, F)
    tau = t_dev.to(knots.dtype)
    B, C = g.shape
    if control == "natural":
        i = int(torch.searchsorted(knots, tau, right=True)) - 1  # the host read
        h, s = knots[i + 1] - knots[i], tau - knots[i]
        q = s * s / (2 * h)
        gY, gM = torch.zeros(B, len(knots), C, dtype=g.dtype, device=g.device), torch.zeros(B, len(knots), C, dtype=g.dtype, device=g.device)
        gY[:, i], gY[:, i + 1] = -g / h, g / h
        gM[:, i], gM[:, i + 1] = ((s - h / 3) - q) * g, (q - h / 6) * g
        return gY, gM
    i = int(torch.searchsorted(knots, tau, right=False)) - 1
    sx = tau - knots[i]  # (the unit grid)
    g0, g1, g2, g3 = 6 * sx * sx - 6 * sx, -6 * sx * sx + 6 * sx, 3 * sx * sx - 4 * sx + 1, 3 * sx * sx - 2 * sx
    gS = torch.zeros(B, len(knots), C, dtype=g.dtype, device=g.device)
    gS[:, i], gS[:, i + 1], gS[:, i + 2] = (g0 - g2) * g, ((g1 + g2) - g3) * g, g3 * g
    return (gS,)


def measure(reps, rounds):
    be = _hip.get_backend()
    res = []
    for name, B, H, C in SHAPES:
        for dtype in (torch.float32, torch.float64):
            elt = torch.empty((), dtype=dtype).element_size()
            gen = torch.Generator().manual_seed(0)
            F = torch.randn(B, H, C, generator=gen).to(DEV, dtype)
            gout = torch.randn(B, H, generator=gen).to(DEV, dtype)
            for control in ("natural", "cubic"):
                n_out = 2 if control == "natural" else 1
                knots = (torch.cumsum(0.5 + torch.rand(TN, generator=gen), 0) if control == "natural" else torch.arange(float(TN))).to(DEV, dtype)
                t = (0.5 * (knots[11] + knots[12])).to(torch.float64) if control == "natural" else torch.tensor(11.3, dtype=torch.float64, device=DEV)
                outs = [torch.empty(B, TN, C, dtype=dtype, device=DEV) for _ in range(n_out)]
                outs2 = [torch.empty(B, 2, C, dtype=dtype, device=DEV) for _ in range(n_out)]
                t2 = (0.5 * (knots[0] + knots[1])).to(torch.float64)
                moved = (B * H * C + B * H + n_out * B * TN * C) * elt
                src = torch.empty(moved // (2 * elt), dtype=dtype, device=DEV).normal_()
                dst = torch.empty_like(src)
                if control == "natural":
                    run_a = lambda: be._cde_control_grad_natural(outs[0], outs[1], gout, F, knots, t)  # noqa: E731
                    run_2 = lambda: be._cde_control_grad_natural(outs2[0], outs2[1], gout, F, knots[:2].contiguous(), t2)  # noqa: E731
                else:
                    run_a = lambda: be._cde_control_grad(outs[0], gout, F, knots, t, "cubic")  # noqa: E731
                    run_2 = lambda: be._cde_control_grad(outs2[0], gout, F, knots[:2].contiguous(), t2, "cubic")  # noqa: E731
                runs = {"copy": lambda: dst.copy_(src), "a": run_a, "a_tn2": run_2, "fill": lambda: [o.zero_() for o in outs],
                        "framework": lambda: _framework(control, gout, F, knots, t)}
                # same results first (the framework sum runs in another order: a tolerance of the dtype's size)
                tol = 1e-4 if dtype == torch.float32 else 1e-12
                run_a()
                for got, want in zip(outs, runs["framework"]()):
                    assert torch.allclose(got, want, rtol=tol, atol=tol * H), (name, dtype, control)
                ms = {k: [] for k in runs}
                for _ in range(rounds):
                    for k, fn in runs.items():
                        ms[k].append(_time(fn, reps))
                med = {k: statistics.median(v) for k, v in ms.items()}
                copy_gbs = moved / med["copy"] / 1e6
                row = {"shape": name, "B": B, "H": H, "C": C, "Tn": TN, "dtype": str(dtype).split(".")[-1], "control": control,
                       "moved_MiB": round(moved / 2**20, 2), "gradient_MiB": round(n_out * B * TN * C * elt / 2**20, 2),
                       "copy_ms": round(med["copy"], 4), "copy_GBps": round(copy_gbs, 1), "a_ms": round(med["a"], 4),
                       "a_ms_spread": [round(min(ms["a"]), 4), round(max(ms["a"]), 4)], "a_GBps": round(moved / med["a"] / 1e6, 1),
                       "a_of_copy": round(med["copy"] / med["a"], 3), "a_tn2_ms": round(med["a_tn2"], 4),
                       "a_share_beyond_tn2": round(1.0 - med["a_tn2"] / med["a"], 3), "fill_ms": round(med["fill"], 4),
                       "framework_ms": round(med["framework"], 4), "a_speedup_over_framework": round(med["framework"] / med["a"], 2)}
                res.append(row)
                print(json.dumps(row), flush=True)
    return res


def measure_spline(reps, rounds):
    """(b) and (c) at B C = 262144 columns, Tn = 32."""
    be = _hip.get_backend()
    B, C = 8192, 32
    res = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        gen = torch.Generator().manual_seed(1)
        knots = torch.cumsum(0.5 + torch.rand(TN, generator=gen), 0).to(DEV, dtype)
        series = torch.randn(B, TN, C, generator=gen)
        series[:, 1:-1][torch.rand(B, TN - 2, C, generator=gen) < 0.2] = float("nan")
        series = series.to(DEV, dtype)
        gY, gM = torch.randn(B, TN, C, generator=gen).to(DEV, dtype), torch.randn(B, TN, C, generator=gen).to(DEV, dtype)
        gS, oY, oM = torch.empty_like(gY), torch.empty_like(gY), torch.empty_like(gY)
        gv, gd = torch.randn(B, 1, C, generator=gen).to(DEV, dtype), torch.randn(B, 1, C, generator=gen).to(DEV, dtype)
        tq = knots[:1].contiguous()
        runs = {"coeffs_backward": lambda: be._spline_natural_coeffs_backward(gS, gY, gM, series, knots),
                "gather_backward": lambda: be._spline_natural_gather_backward(oY, oM, gv, gd, knots, tq)}
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(_time(fn, reps))
        row = {"columns": B * C, "Tn": TN, "dtype": str(dtype).split(".")[-1], "array_MiB": round(B * TN * C * elt / 2**20, 2)}
        for k in runs:
            row[k + "_ms"] = round(statistics.median(ms[k]), 4)
            row[k + "_ms_spread"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
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
        sys.exit("profiles/tools/cde_control_grad.py measures on the GPU: no device found")
    res = {"device": torch.cuda.get_device_name(0), "control_grad": measure(args.reps, args.rounds),
           "spline": measure_spline(args.reps, args.rounds)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
