"""Measurements of per-sample output times, ``odeint(..., options={"t_eval": tq})``.

    python profiles/tools/teval.py [--out profiles/teval.json] [--reps N]

  train      256 x 64 fp32, Q = 16 times per row on [0, 1], Dopri5 (rtol 1e-5, atol 1e-7), a small MLP func: time and peak memory of
             forward + backward through ``t_eval``, and of the union route — ``backprop="steps"`` on the sorted union of all rows' times
             (4096 output rows of 256 x 64) plus a gather — in the same process, alternating; both on the sync pipeline.  Also the
             forward alone under ``no_grad`` against the union solve on its default pipeline.
  kernels    4096 x 64, Q = 32, fp32 and fp64: ``xde_teval_dense`` and ``xde_teval_cotangent`` on a step no row has a query in (the
             per-step overhead) and on a step every row has one query in, the latter as a fraction of a device copy that moves the
             SAME bytes (a buffer of half the launch's bytes, read and written), timed in the same process.
  large      4096 x 64 fp32, Q = 32, whose union solution (137 GB) cannot be allocated: that it runs, its time and its peak memory.

Every time is a host clock around work that ends in a device synchronise (train, large) or an event time over ``reps`` launches
(kernels).  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import Dopri5, _hip, odeint  # noqa: E402
from paddlexde_amd.utils import _rms_norm  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-5, 1e-7


class Func(torch.nn.Module):
    def __init__(self, D, hidden=64):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(D, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, D))

    def forward(self, t, y):
        return self.net(y)


def _problem(rows, D, Q, seed=0):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    f = Func(D).to(DEV)
    y0 = torch.randn(rows, D, generator=gen).to(DEV)
    tq = torch.sort(0.02 + 0.98 * torch.rand(rows, Q, generator=gen), dim=1).values
    return f, y0, tq.to(DEV), torch.tensor([0.0, 1.0], device=DEV)


def _wall(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
            "peak_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)}


def train(reps, rows=256, D=64, Q=16):
    f, y0, tq, t_span = _problem(rows, D, Q)
    u, inv = torch.unique(torch.cat([t_span, tq.reshape(-1)]), return_inverse=True)
    idx = inv[2:].reshape(rows, Q).t().contiguous()  # [Q, rows]
    col = torch.arange(rows, device=DEV)[None, :]
    st = {}

    def teval(grad=True):
        y = y0.clone().requires_grad_(grad)
        sol = odeint(f, y, t_span, Dopri5, rtol=RTOL, atol=ATOL, options={"t_eval": tq, "norm": _rms_norm, "stats_out": st})
        if grad:
            sol.square().sum().backward()

    def union(grad=True):
        y = y0.clone().requires_grad_(grad)
        opt = {"norm": _rms_norm, "backprop": "steps"} if grad else {"norm": _rms_norm}
        sol = odeint(f, y, u, Dopri5, rtol=RTOL, atol=ATOL, options=opt)[idx, col]
        if grad:
            sol.square().sum().backward()

    res = {"rows": rows, "D": D, "Q": Q, "union_rows": int(u.numel()), "union_solution_MB": round(u.numel() * rows * D * 4 / 1e6, 1)}
    a, b = [], []
    for _ in range(2):  # alternate the two routes
        a.append(_wall(teval, reps))
        b.append(_wall(union, reps))
    res["n_accept"] = st.get("n_accept")
    res["t_eval"], res["union"] = min(a, key=lambda r: r["ms_median"]), min(b, key=lambda r: r["ms_median"])
    res["t_eval_over_union"] = round(res["t_eval"]["ms_median"] / res["union"]["ms_median"], 3)
    with torch.no_grad():
        res["forward_t_eval"] = _wall(lambda: teval(False), reps)
        res["forward_union_default_pipeline"] = _wall(lambda: union(False), reps)
    return res


def _events(fn, reps):
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


def kernels(reps):
    be = _hip.get_backend()
    rows, D, Q = 4096, 64, 32
    out = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        code = _hip.dtype_code(dtype)
        gen = torch.Generator().manual_seed(0)
        y0, y1, f1 = (torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(3))
        ks = [torch.randn(rows, D, generator=gen).to(DEV, dtype) for _ in range(5)]  # Dopri5's midpoint operands, k[0] = f0
        mid = [0.1, 0.2, -0.3, 0.4, 0.05]
        # every row: one query in (0.25, 0.5], the others after it; the empty step is (0, 0.125]
        tq = torch.sort(0.55 + 0.4 * torch.rand(rows, Q, generator=gen, dtype=torch.float64), dim=1).values
        tq[:, 0] = 0.26 + 0.2 * torch.rand(rows, generator=gen, dtype=torch.float64)
        tq = tq.to(dtype).double().to(DEV)
        cnt = torch.full((rows,), Q, dtype=torch.int32, device=DEV)
        sol = torch.empty(Q, rows, D, dtype=dtype, device=DEV)
        g = torch.randn(Q, rows, D, generator=gen).to(DEV, dtype)
        outs = [torch.empty(rows, D, dtype=dtype, device=DEV) for _ in range(5)]
        n = rows * D * elt

        def dense(t0, t1):
            be._teval_dense(sol, tq, cnt, ks, mid, y0, y1, ks[0], f1, t0, t1, t1 - t0, 1, code)

        def cot(t0, t1):
            be._teval_cotangent(outs, g, tq, cnt, t0, t1, t1 - t0, 1, code, acc_mask=0b10)

        def copy_of(nb):
            src = torch.empty(nb // 2 // elt, dtype=dtype, device=DEV).normal_()
            dst = torch.empty_like(src)
            return _events(lambda: dst.copy_(src), reps)

        row = {"dtype": str(dtype).split(".")[-1], "rows": rows, "D": D, "Q": Q}
        # dense, one query per row: y0, y1, f1 and five k read, one row written; cotangent: one row of g and lambda read, five written
        for name, fn, nb in (("dense", dense, 9 * n), ("cotangent", cot, 7 * n)):
            empty_ms, full_ms = _events(lambda: fn(0.0, 0.125), reps), _events(lambda: fn(0.25, 0.5), reps)
            copy_ms = copy_of(nb)
            row.update({name + "_empty_step_us": round(empty_ms * 1e3, 2), name + "_one_query_us": round(full_ms * 1e3, 2),
                        name + "_bytes": nb, name + "_copy_us": round(copy_ms * 1e3, 2), name + "_of_copy": round(copy_ms / full_ms, 3)})
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def large(reps):
    rows, D, Q = 4096, 64, 32
    f, y0, tq, t_span = _problem(rows, D, Q)

    def teval():
        y = y0.clone().requires_grad_()
        sol = odeint(f, y, t_span, Dopri5, rtol=RTOL, atol=ATOL, options={"t_eval": tq, "norm": _rms_norm})
        sol.square().sum().backward()

    res = {"rows": rows, "D": D, "Q": Q, "result_MB": round(Q * rows * D * 4 / 1e6, 1),
           "union_solution_GB": round(rows * Q * rows * D * 4 / 1e9, 1)}
    res.update(_wall(teval, reps))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = kernels(50)
    res["train"] = train(args.reps)
    print(json.dumps(res["train"]), flush=True)
    res["large"] = large(args.reps)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
