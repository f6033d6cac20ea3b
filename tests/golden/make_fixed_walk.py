"""Generates tests/golden/fixed_walk_parent.json: what the fixed-step solvers' walk (solver/base_fixed_solver.py) computes on the
numpy double (tests/_sde_double.py) at the commit this is run at — per case the sha256 of the solution bytes, ``nfe``, the double's
launch list, the sha256 of every gradient and what an ``on_integrate_step_end`` hook saw.  tests/test_fixed_walk_host.py re-runs the
table and requires equality field by field, so a later change of the walk is held to this commit's results bit for bit.

    python -m tests.golden.make_fixed_walk        # at the commit whose walk is the yardstick
"""
import hashlib
import json
import os
import subprocess

import numpy as np
import torch

from paddlexde_amd import RK4, AdamsBashforthMoulton, Euler, Midpoint, _hip, ddeint
from paddlexde_amd.utils import _rms_norm
from paddlexde_amd.xde import BaseODE, BaseSDE

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fixed_walk_parent.json")

SOLVERS = {"euler": (Euler, {}), "midpoint": (Midpoint, {}), "rk4": (RK4, {}), "rk4_classic": (RK4, {"variant": "classic"}),
           "adams": (AdamsBashforthMoulton, {}), "adams_implicit": (AdamsBashforthMoulton, {"implicit": True})}
MODES = ("plain", "step_size", "grid")
SHAPES = {"1x2": (1, 2), "1x3": (1, 3), "3x2x2": (3, 2, 2)}  # rows contiguous and aligned (fp64) / 12-byte fp32 rows / a lead batch

# output times (all <= 15) and the non-uniform grids they are walked over (all <= 40 steps); "desc" mirrors "asc"
_ASC = [0.0, 0.05, 0.3, 0.5, 0.501, 0.75, 1.0]
_GRID = [0.0, 0.07, 0.2, 0.3, 0.45, 0.5, 0.62, 0.75, 0.9, 1.0]
SPANS = {
    "asc": (_ASC, _GRID),
    "desc": ([1.0 - x for x in _ASC], [1.0 - x for x in _GRID]),
    "repeated": ([0.0, 0.05, 0.3, 0.3, 0.5, 0.5, 1.0], _GRID),
    "on_grid": ([0.0, 0.25, 0.5, 1.0], [0.0, 0.125, 0.25, 0.3, 0.5, 0.8, 1.0]),  # (interp="": outputs on grid points only)
    "all_equal": ([0.25, 0.25, 0.25], [0.25]),
    "non_monotone": ([0.0, 0.3, 0.2, 0.2, 0.6], None),  # (plain walk only: a step per interval, whatever its sign)
    "identity": (_ASC, _ASC),  # a grid that IS t_span
}
STEP_SIZE = {"on_grid": 0.125}  # (default 0.1)

# (solver, interp, time dtype, state dtype, shape, span, grad, hook): every line runs in each of the three modes
_BASE = [
    ("euler", "linear", "f32", "f32", "1x3", "asc", "none", False),
    ("euler", "", "f64", "f64", "1x2", "on_grid", "none", False),
    ("euler", "linear", "f64", "f64", "1x2", "repeated", "y0", False),
    ("midpoint", "cubic", "f64", "f64", "1x2", "desc", "none", False),
    ("midpoint", "linear", "f64", "f64", "1x2", "asc", "none", True),
    ("midpoint", "linear", "f32", "f32", "3x2x2", "repeated", "param", False),
    ("rk4", "", "f64", "f64", "3x2x2", "on_grid", "none", False),
    ("rk4", "cubic", "f64", "f64", "3x2x2", "asc", "y0", False),
    ("rk4", "cubic", "f32", "f32", "1x3", "desc", "none", True),
    ("rk4", "linear", "f64", "f32", "1x3", "asc", "no_grad", False),
    ("rk4", "linear", "f64", "f64", "1x2", "all_equal", "none", False),
    ("rk4", "linear", "f64", "f64", "1x2", "identity", "none", False),
    ("rk4_classic", "linear", "f32", "f64", "1x2", "repeated", "none", False),
    ("rk4_classic", "cubic", "f64", "f64", "3x2x2", "desc", "y0", True),
    ("adams", "cubic", "f32", "f32", "3x2x2", "asc", "none", False),
    ("adams", "linear", "f64", "f64", "1x2", "desc", "y0", False),
    ("adams_implicit", "linear", "f32", "f32", "1x3", "asc", "none", False),
    ("adams_implicit", "", "f64", "f64", "1x2", "on_grid", "none", True),
]


def _cases():
    out = []
    for mode in MODES:
        for solver, interp, tt, st, shape, span, grad, hook in _BASE:
            out.append(dict(kind="ode", solver=solver, interp=interp, tt=tt, st=st, shape=shape, span=span, grad=grad, hook=hook, mode=mode))
        for st, span, grad in (("f32", "asc", "none"), ("f64", "repeated", "y0"), ("f64", "desc", "none")):
            out.append(dict(kind="sde", solver="euler", interp="linear", tt=st, st=st, shape="3x2x2", span=span, grad=grad, hook=False, mode=mode))
        for interp, grad in (("linear", "none"), ("cubic", "lags")):
            out.append(dict(kind="dde", solver="rk4", interp=interp, tt="f64", st="f64", shape="3x2x2", span="asc", grad=grad, hook=False, mode=mode))
        # func raises in the middle of a step (its 6th call): the per-step state must be idle again afterwards
        out.append(dict(kind="ode", solver="rk4", interp="cubic", tt="f64", st="f64", shape="1x2", span="asc", grad="none", hook=False, mode=mode,
                        raises=6))
    out.append(dict(kind="ode", solver="rk4", interp="linear", tt="f64", st="f64", shape="1x2", span="non_monotone", grad="none", hook=False,
                    mode="plain"))
    out.append(dict(kind="ode", solver="euler", interp="cubic", tt="f32", st="f32", shape="1x3", span="non_monotone", grad="y0", hook=True,
                    mode="plain"))
    for c in out:
        c["id"] = "-".join([c["mode"], c["kind"], c["solver"], c["interp"] or "raw", "t" + c["tt"], "y" + c["st"], c["shape"], c["span"],
                            "grad_" + c["grad"]] + (["hook"] if c["hook"] else []) + (["raises"] if c.get("raises") else []))
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
_DT = {"f32": torch.float32, "f64": torch.float64}
IDLE_FIELDS = ("_dt", "_t0_host", "_row", "_y1_out", "_k", "_g_ctrls", "_rec")


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x.detach().numpy()).tobytes()).hexdigest()


class _Func(torch.nn.Module):
    """Depends on t, so every column of the stage-time table reaches the bits; ``raises``: the call that fails."""

    def __init__(self, dtype, trainable, raises=None):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(-0.75, dtype=dtype), requires_grad=trainable)
        self.b = torch.nn.Parameter(torch.tensor([0.125, -0.25], dtype=dtype), requires_grad=trainable)
        self.calls, self.raises = 0, raises

    def forward(self, t, y):
        self.calls += 1
        if self.calls == self.raises:
            raise RuntimeError("func failed at call {}".format(self.calls))
        return y * self.a + (y * y) * self.b[0] + t * self.b[1]


class _OdeWithDt(BaseODE):
    """BaseODE whose ``move`` also uses the ``dt`` it is handed (BaseODE ignores it): the dt-like columns of the table count too."""

    def move(self, t0, dt, y0):
        return self.func(t0, y0) + dt * 0.0625


class _Hooked(_OdeWithDt):
    """Keeps the tensors the hook is handed (a hook may) and what they held when it was called."""

    def on_integrate_step_end(self, y0=None, y1=None, t0=None, t1=None):
        self.__dict__.setdefault("seen", []).append(((y0, y1, t0, t1), [sha(x) for x in (y0, y1, t0, t1)]))


def _recording(cls, made):
    class Recording(cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    Recording.__name__ = cls.__name__
    return Recording


def run_case(c):
    """-> (record, solver): the record is what the golden file holds for the case."""
    be = _hip.get_backend()
    tt, st = _DT[c["tt"]], _DT[c["st"]]
    times, grid = SPANS[c["span"]]
    t = torch.tensor(times, dtype=torch.float64).to(tt)
    shape = SHAPES[c["shape"]]
    y0 = (0.25 + 0.5 * torch.rand(shape, generator=torch.Generator().manual_seed(len(shape)), dtype=torch.float64)).to(st)
    y0.requires_grad_(c["grad"] == "y0")
    options = {}
    if c["mode"] == "step_size":
        options["step_size"] = STEP_SIZE.get(c["span"], 0.1)
    elif c["mode"] == "grid":
        g = torch.tensor(grid, dtype=torch.float64).to(tt)
        options["grid_constructor"] = lambda y, ts: g
    cls, extra = SOLVERS[c["solver"]]
    made, leaves = [], [y0] if c["grad"] == "y0" else []
    cls = _recording(cls, made)
    func = _Func(st, c["grad"] == "param", c.get("raises"))
    leaves += [p for p in func.parameters() if p.requires_grad]
    n0 = len(be.launches)
    rec, sol, xde = {}, None, None
    try:
        with torch.set_grad_enabled(c["grad"] != "no_grad"):
            if c["kind"] == "dde":
                rng = np.random.RandomState(2)
                ht = torch.arange(12, dtype=st)
                his = torch.from_numpy(np.sin(0.4 * np.arange(12.0))[None, :, None] * np.array([0.5, 1.0]) + 0.05 * rng.randn(3, 12, 2)).to(st)
                lags = torch.tensor([1.5, 4.25, 7.0], dtype=st, requires_grad=c["grad"] == "lags")
                leaves += [lags] if c["grad"] == "lags" else []
                sol, _ = ddeint(lambda yl, y: y * y * y * (-0.5) + yl[..., 0:1, :] * 0.25 - yl[..., 2:3, :] * 0.125, y0[:, :1], t, lags, his, ht,
                                solver=cls, options=dict({"norm": _rms_norm}, **options), fixed_solver_interp=c["interp"])
            else:
                if c["kind"] == "sde":
                    xde = BaseSDE(f=func, g=lambda t_, y: y * 0.5 + 0.25, y0=y0, t_span=t, seed=77)
                else:
                    xde = (_Hooked if c["hook"] else _OdeWithDt)(func, y0=y0, t_span=t)
                s = cls(xde=xde, y0=y0, rtol=1e-7, atol=1e-9, norm=_rms_norm, interp=c["interp"], **extra, **options)
                sol = s.integrate(t)
    except RuntimeError as e:
        if not c.get("raises"):
            raise
        rec["error"] = str(e)
    (s,) = made
    rec.update(nfe=s.nfe, launches=list(be.launches[n0:]))
    if sol is not None:
        rec.update(shape=list(sol.shape), sol=sha(sol))
        if leaves:
            w = torch.randn(sol.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(st)
            rec["grads"] = [sha(g) for g in torch.autograd.grad((sol * w).sum(), leaves)]
            rec["launches_backward"] = list(be.launches[n0 + len(rec["launches"]):])
    if c["hook"]:
        seen = xde.__dict__.get("seen", [])
        rec["hook_at_call"] = [h for _, h in seen]
        rec["hook_kept"] = [[sha(x) for x in kept] for kept, _ in seen]  # (the tensors it kept, read after the solve)
    return rec, s


def record():
    from .._sde_double import SdeDoubleBackend

    _hip._set_backend_for_testing(SdeDoubleBackend())
    try:
        return {c["id"]: run_case(c)[0] for c in CASES}
    finally:
        _hip._set_backend_for_testing(None)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(HERE))
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, check=True, capture_output=True, text=True).stdout.strip()
    with open(PATH, "w") as fh:
        json.dump({"parent": commit, "cases": record()}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", PATH, "at", commit, "-", len(CASES), "cases")
