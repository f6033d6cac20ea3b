"""Measurements of the fixed-step solvers' sub-stepping, options step_size / grid_constructor (DESIGN sections 4 and 7).

    python profiles/tools/substep.py [--out FILE] [--part kernels|e2e|spiral]

kernels  xde_interp_rows at n = 65536 x 128, fp32 and fp64, G in {1, 4, 8}, linear and cubic: bytes (R + G) n elt over the launch time,
         as a fraction of a same-size device copy (2 n elt bytes) timed in the same process.  Run it once more under
         `rocprofv3 --kernel-trace --stats -- python ...` for the kernel durations without launch gaps.
e2e      RK4 on the bench's linear func at 65536 x 128 fp32: 200 grid steps and 11 outputs with step_size, against today's workaround
         (the 201-point grid as t_span); ms per grid step and the output memory of each
spiral   the spiral (config 1's shape, [1, 2]) with step_size: pipeline "auto" (the captured step) against "sync"
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddlexde_amd import RK4, _hip, odeint  # noqa: E402
from paddlexde_amd.utils.ode_utils import _rms_norm  # noqa: E402

DEV = "cuda"
N_ROWS, N_COLS = 65536, 128


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernels(reps=50):
    be = _hip.get_backend()
    res = []
    for dtype in (torch.float32, torch.float64):
        elt = torch.empty((), dtype=dtype).element_size()
        n = N_ROWS * N_COLS
        g = torch.Generator().manual_seed(0)
        ops = [torch.randn(N_ROWS, 1, N_COLS, generator=g).to(DEV, dtype) for _ in range(4)]
        src, dst = ops[0].clone(), torch.empty_like(ops[0])
        copy_ms = _time(lambda: dst.copy_(src), reps)
        copy_gbs = 2 * n * elt / copy_ms / 1e6
        for cubic in (False, True):
            R = 4 if cubic else 2
            for G in (1, 4, 8):
                out = torch.empty(N_ROWS, G, N_COLS, dtype=dtype, device=DEV)  # rows strided into a [B, T*L, D] solution
                dsts = [out.narrow(1, r, 1) for r in range(G)]
                kinds = [_hip.XDE_ROW_INTERP] * G
                w = [(0.25, 0.5, 0.75, -0.125)] * G
                use = ops if cubic else ops[:2] + [None, None]
                ms = _time(lambda: be._interp_rows(dsts, kinds, w, *use), reps)
                gbs = (R + G) * n * elt / ms / 1e6
                res.append({"dtype": str(dtype).split(".")[-1], "mode": "cubic" if cubic else "linear", "G": G, "ms": round(ms, 4),
                            "GBps": round(gbs, 1), "copy_GBps": round(copy_gbs, 1), "of_copy": round(gbs / copy_gbs, 3)})
                print(json.dumps(res[-1]), flush=True)
    return res


class Lin(torch.nn.Module):
    def __init__(self, d=N_COLS):
        super().__init__()
        self.lin = torch.nn.Linear(d, d, bias=False)
        with torch.no_grad():
            u = 0.1 * torch.randn(d, d, generator=torch.Generator().manual_seed(1))
            self.lin.weight.copy_(u - u.T)

    def forward(self, t, y):
        return self.lin(y)


def e2e(reps=3):
    f = Lin().to(DEV)
    y0 = torch.randn(N_ROWS, 1, N_COLS, generator=torch.Generator().manual_seed(0)).to(DEV)
    h = 1.0 / 200
    t_out = torch.linspace(0.0, 1.0, 11, dtype=torch.float64)  # (0.1 apart: each output inside or at the end of a grid step)
    t_fine = torch.arange(201, dtype=torch.float64) * h
    out = {}
    with torch.no_grad():
        for name, t, opts in (("step_size", t_out, {"step_size": h}), ("fine_t_span", t_fine, {})):
            o = dict({"norm": _rms_norm, "pipeline": "sync"}, **opts)
            ms = _time(lambda: odeint(f, y0, t.to(DEV), solver=RK4, options=o), reps)
            sol = odeint(f, y0, t.to(DEV), solver=RK4, options=o)
            out[name] = {"ms": round(ms, 2), "ms_per_grid_step": round(ms / 200, 4), "outputs": len(t),
                         "output_MiB": round(sol.numel() * sol.element_size() / 2**20, 1)}
        a = odeint(f, y0, t_out.to(DEV), solver=RK4, options={"norm": _rms_norm, "step_size": h})
        b = odeint(f, y0, t_fine.to(DEV), solver=RK4, options={"norm": _rms_norm})[:, ::20]
        out["max_abs_diff_at_outputs"] = float((a - b).abs().max())
    out["step_size_over_fine"] = round(out["step_size"]["ms"] / out["fine_t_span"]["ms"], 4)
    print(json.dumps(out), flush=True)
    return out


def spiral(reps=5):
    y0 = torch.tensor([[2.0, 0.0]], device=DEV)
    t = torch.linspace(0.0, 25.0, 101).to(DEV)
    A = torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], device=DEV)
    out = {}
    with torch.no_grad():
        for p in ("sync", "auto"):
            o = {"norm": _rms_norm, "step_size": 0.025, "pipeline": p}
            ms = _time(lambda: odeint(lambda t_, y: (y * y * y) @ A, y0, t, solver=RK4, options=o), reps)
            out[p] = {"ms": round(ms, 2), "ms_per_grid_step": round(ms / 1000, 4)}
    out["grid_steps"], out["outputs"] = 1000, 101
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--part", action="append", choices=["kernels", "e2e", "spiral"])
    args = ap.parse_args()
    parts = args.part or ["kernels", "e2e", "spiral"]
    res = {"device": torch.cuda.get_device_name(0)}
    for p in parts:
        res[p] = globals()[p]()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
