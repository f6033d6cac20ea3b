"""Measurements of the per-sample kernels, by the method of profiles/tools/sde_gn.py.

    python profiles/tools/rows.py [--out profiles/rows.json] [--reps N]

At (rows, D) = 65536 x 128 and 1024 x 1024, fp32 and fp64, every time an event time over ``reps`` launches and every rate a fraction of a device copy
that moves the SAME bytes (a buffer of half the launch's bytes, read and written) timed in the same process; N = rows * D:
  combine    xde_rows_stage_combine with Dopri5's last stage: 6 N elt read (y0, five k), 2 N written (y1, the error pre-sum)
  control    xde_rows_norm_control in the e_pre form: 4 N elt read (e_pre, k, y0, y1)
  commit     xde_rows_dense_commit on a step that holds no output: 2 N elt read (y1, f1), 2 N written (y0, f0)
  dense      xde_rows_dense_commit on a step that holds one output: 9 N elt read (six k, y0, y1, f1), 3 N written
  scaled     xde_rows_scaled_norm of a difference: 3 N elt read
Run it once more under `rocprofv3 --kernel-trace --stats -- python ...` for kernel durations without launch gaps.  Prints one JSON
object (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import _hip  # noqa: E402

DEV = "cuda"
SHAPES = ((65536, 128), (1024, 1024))  # many short rows (32 lanes a row); a batch of samples with a row per workgroup


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
    for (ROWS, D), dtype in ((sh, dt) for sh in SHAPES for dt in (torch.float32, torch.float64)):
        elt = torch.empty((), dtype=dtype).element_size()
        n = ROWS * D
        gen = torch.Generator().manual_seed(0)
        mk = lambda s=1.0: (torch.randn(ROWS, D, generator=gen) * s).to(DEV, dtype)  # noqa: E731
        y0, y1, f1 = mk(), mk(), mk()
        ks = [mk(1e-3) for _ in range(6)]
        out, out2 = torch.empty_like(y0), torch.empty_like(y0)
        t_span = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=DEV)
        sol = torch.empty(3, ROWS, D, dtype=dtype, device=DEV)
        norms = torch.empty(ROWS, dtype=torch.float64, device=DEV)
        p = _hip.XdeCtrlParams()
        p.rtol, p.atol, p.min_step, p.max_step, p.safety, p.ifactor, p.dfactor, p.order = 1e-5, 1e-7, 1e-3, 1e-3, 0.9, 10.0, 0.2, 5.0
        p.max_num_steps, p.direction, p.n_stage, p.n_seg, p.norm_kind = 2**31 - 1, 1, 6, 1, _hip.NORM_RMS
        p.time_dtype = p.state_dtype = _hip.dtype_code(dtype)
        for i, a in enumerate((0.2, 0.3, 0.8, 8.0 / 9.0, 1.0, 1.0)):
            p.alpha[i] = a
        ctl = _hip.RowsCtl(ROWS, 6, dtype, torch.device(DEV))
        coef = [0.1, 0.2, 0.3, 0.2, 0.1, 0.1]

        def arm(h, t, accept):
            """every row live at time ``t`` with step ``h``"""
            ctl.i32.zero_()
            ctl.f64.zero_()
            ctl.t.fill_(t)
            ctl.t_prev.fill_(t - h)
            ctl.h.fill_(h)
            ctl.h_used.fill_(h)
            ctl.next_out.fill_(1)
            ctl.accept.fill_(accept)

        def copy_of(nbytes):
            src = torch.empty(nbytes // 2 // elt, dtype=dtype, device=DEV).normal_()
            dst = torch.empty_like(src)
            return _time(lambda: dst.copy_(src), reps)

        def dense():
            ctl.next_out.fill_(1)  # (the one launch that moves what it reads: the cursor is put back, the fill's time subtracted)
            be._rows_dense_commit(sol, ks, coef, y0, y1, f1, ctl, p, t_span)

        fill_ms = _time(lambda: ctl.next_out.fill_(1), reps)
        # min_step = max_step = h: every launch of the controller accepts and proposes h again, so the launches repeat themselves
        cases = [
            ("combine", 8, (1e-3, 0.5, 0), lambda: be._rows_stage_combine(out, y0, ks[:5], coef[:5], ctl, out2=out2, coef2=coef[:5]), 0.0),
            ("control", 4, (1e-3, 0.25, 0), lambda: be._rows_norm_control([ks[5]], [0.1], y0, y1, ctl, p, t_span, e_pre=out2), 0.0),
            ("commit", 4, (1e-3, 0.5, 1), lambda: be._rows_dense_commit(sol, ks, coef, y0, y1, f1, ctl, p, t_span), 0.0),
            ("dense", 12, (1e-3, 1.0005, 1), dense, fill_ms),
            ("scaled", 3, (1e-3, 0.5, 0), lambda: be._rows_scaled_norm(norms, f1, ks[0], y0, 1e-5, 1e-7), 0.0),
        ]
        for name, arrays, state, fn, overhead in cases:
            arm(*state)
            copy_ms = copy_of(arrays * n * elt)
            ms = _time(fn, reps) - overhead
            row = {"kernel": name, "dtype": str(dtype).split(".")[-1], "rows": ROWS, "D": D, "bytes": arrays * n * elt,
                   "copy_ms": round(copy_ms, 4), "ms": round(ms, 4), "of_copy": round(copy_ms / ms, 3),
                   "GBps": round(arrays * n * elt / ms / 1e6, 1)}
            res.append(row)
            print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shapes": [list(x) for x in SHAPES], "yardstick_fp32_of_copy": 0.70, "kernels": measure(args.reps)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
