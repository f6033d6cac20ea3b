"""Measurements of the logsignature-window kernels, by the method of profiles/tools/sde_gn.py.

    python profiles/tools/logsig.py [--out profiles/logsig.json] [--reps N]

At (B, T, C, L) = 4096 x 1025 x 8 x 16 (a long series of few channels: 64 windows of K = 36) and 4096 x 257 x 32 x 4 (64 windows of
K = 528: write-dominated), depth 2, fp32 and fp64, every time an event time over ``reps`` back-to-back launches and every rate a
fraction of a device copy that moves the SAME bytes (a buffer of half the launch's bytes, read and written) timed in the same process:
  fwd        xde_logsig_windows: B T C elt read, B W K written
  bwd        xde_logsig_windows_backward: B T C + B W K elt read, B T C written (x is read about twice: the polygon differences)
  framework  the same formulas in framework ops on the same inputs: a diff, the offsets from each window's first point, an einsum per
             window with its [B, W, C, C] intermediate, the antisymmetrisation, the triangular gather and the concatenation;
             framework_bwd: autograd's backward of that graph (the graph kept; the forward is not in the time)
The kernels are not plain streams — O(n C^2) float64 products per window — so the copy is a floor, not a target.  Run it once more
under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps.  Prints one JSON object (and writes it
to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402

DEV = "cuda"
SHAPES = ((4096, 1025, 8, 16), (4096, 257, 32, 4))


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


def framework_windows(x, L):
    """Depth 2 where L divides T - 1."""
    B, T, C = x.shape
    W = (T - 1) // L
    cur, nxt = x[:, :-1].reshape(B, W, L, C), x[:, 1:].reshape(B, W, L, C)
    u, d = (cur - cur[:, :, :1])[:, :, 1:], (nxt - cur)[:, :, 1:]
    M = torch.einsum("bwki,bwkj->bwij", u, d)
    iu, ju = torch.triu_indices(C, C, 1, device=x.device)
    return torch.cat([x[:, L::L] - x[:, :-1:L], (0.5 * (M - M.transpose(-1, -2)))[..., iu, ju]], dim=-1)


def measure(reps):
    be = _hip.get_backend()
    res = []
    for B, T, C, L in SHAPES:
        for dtype in (torch.float32, torch.float64):
            elt = torch.empty((), dtype=dtype).element_size()
            W, K = (T - 1) // L, _hip.logsig_channels(C, 2)
            gen = torch.Generator().manual_seed(0)
            x = torch.cumsum(0.1 * torch.randn(B, T, C, generator=gen), dim=1).to(DEV, dtype)
            out = torch.empty(B, W, K, dtype=dtype, device=DEV)
            gout = torch.empty_like(out).normal_()
            gx = torch.empty_like(x)
            fwd_bytes, bwd_bytes = (x.numel() + out.numel()) * elt, (2 * x.numel() + out.numel()) * elt

            def copy_of(nbytes):
                src = torch.empty(nbytes // 2 // elt, dtype=dtype, device=DEV).normal_()
                dst = torch.empty_like(src)
                ms = _time(lambda: dst.copy_(src), reps)
                return ms, 2 * src.numel() * elt / ms / 1e6

            fwd_copy_ms, fwd_copy_gbs = copy_of(fwd_bytes)
            bwd_copy_ms, bwd_copy_gbs = copy_of(bwd_bytes)
            fwd_ms = _time(lambda: be._logsig_windows(out, x, L, 2), reps)
            bwd_ms = _time(lambda: be._logsig_windows_backward(gx, gout, x, L, 2), reps)
            with torch.no_grad():
                fw_ms = _time(lambda: framework_windows(x, L), reps)
                close = float((framework_windows(x, L) - out).abs().max())
            xr = x.clone().requires_grad_(True)
            ref = framework_windows(xr, L)
            fwb_ms = _time(lambda: torch.autograd.grad(ref, xr, gout, retain_graph=True), reps)
            gclose = float((torch.autograd.grad(ref, xr, gout)[0] - gx).abs().max())
            del ref, xr
            row = {"dtype": str(dtype).split(".")[-1], "B": B, "T": T, "C": C, "L": L, "W": W, "K": K,
                   "fwd_copy_ms": round(fwd_copy_ms, 4), "fwd_copy_GBps": round(fwd_copy_gbs, 1),
                   "bwd_copy_ms": round(bwd_copy_ms, 4), "bwd_copy_GBps": round(bwd_copy_gbs, 1),
                   "fwd_ms": round(fwd_ms, 4), "fwd_of_copy": round(fwd_copy_ms / fwd_ms, 3),
                   "bwd_ms": round(bwd_ms, 4), "bwd_of_copy": round(bwd_copy_ms / bwd_ms, 3),
                   "framework_ms": round(fw_ms, 4), "fwd_speedup": round(fw_ms / fwd_ms, 2),
                   "framework_bwd_ms": round(fwb_ms, 4), "bwd_speedup": round(fwb_ms / bwd_ms, 2),
                   "fwd_max_abs_diff_to_framework": close, "bwd_max_abs_diff_to_framework": gclose}
            res.append(row)
            print(json.dumps(row), flush=True)
            del x, out, gout, gx
            torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shapes": [list(x) for x in SHAPES], "depth": 2, "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
