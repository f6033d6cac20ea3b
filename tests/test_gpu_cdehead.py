"""The fused last layer of a CDE field (include/xde_hip_cdehead.h) against float64 on the CPU: an error bound, determinism and row
independence per shape — this kernel's sums run on the matrix cores, whose in-instruction order no host program can restate — and
one solve through the public interface against the unfused route.  On small integer operands the sums over k are exact under any
rounding, and there the launches are held to the header's float32 statement (tests/_head_exact.py, dX from the numpy doubles of the
contraction and of the natural spline) bit for bit: the order of the runs of c, the carries, the element mapping.
tests/_head_plans.py names the branches the shapes reach together; a sliced launch beyond the grid needs a small grid in a fresh
process (tests/_head_grid_child.py)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import cdeint
from paddlexde_amd.interpolation import CubicHermiteSpline, LinearInterpolation, NaturalCubicSpline
from paddlexde_amd.solver import RK4
from paddlexde_amd.xde import CDELinearHead

from . import _head_exact as E
from . import _head_plans as P
from ._spline_double import SplineDoubleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
# The device tanhf's error in ulps.  The ROCm release this was written against documents none, so it is measured:
# test_the_activation_s_error runs the kernel's own activation (K = 1, W = 1, C = 1, dX = 1) over 2^16 pre-activations in [-4, 4] against float64 — worst error 1.232 ulp on
# gfx950 — and the constant is twice that, rounded up.
TANH_ULP = 2.5
CAP = _hip.XDE_CDEHEAD_MAX_K
SPLINES = {"linear": LinearInterpolation, "cubic": CubicHermiteSpline, "natural": NaturalCubicSpline}

# B, H, C, K, Tn, control, bias, act, t on the device
TABLE = [
    (1, 1, 1, 1, 2, "linear", False, None, False),
    (31, 2, 3, 3, 8, "cubic", True, "tanh", True),
    (33, 7, 4, 8, 8, "natural", True, "tanh", True),       # two batch tiles; vector loads of a and W, vector stores of s
    (65, 7, 33, 33, 8, "cubic", True, "tanh", False),      # runs of c cut by chunks and by passes (H C = 231)
    (65, 33, 5, CAP, 2, "linear", False, "tanh", True),    # K at the cap
    (33, 2, 150, 8, 8, "cubic", True, "tanh", True),       # a run longer than a pass, dX tile in LDS
    (31, 1, 193, 3, 8, "natural", False, None, False),     # C beyond the dX tile: evaluated per use
    (65, 2051, 33, 3, 8, "cubic", True, "tanh", True),     # slices of several h (two passes each)
    (70001, 1, 3, 1, 2, "cubic", True, "tanh", True),      # more work items than workgroups
    (33, 33, 1, 12, 8, "natural", True, None, True),
    (1, 7, 5, 33, 8, "linear", True, "tanh", False),
    (33, 4, 5, 20, 8, "natural", True, "tanh", True),      # kq 3 of 4 registers; H C = 20 but the slices start at 5, 10, 15: s by element
    (31, 2, 3, 24, 8, "cubic", True, "tanh", False),       # the instantiation of 4 again, H C % 4 != 0
    (33, 2, 200, 72, 3, "linear", True, "tanh", False),    # kq 9 of 16: the k-loop leaves a group early; dX evaluated per use
    (65, 3, 5, 128, 8, "cubic", False, "tanh", True),      # kq 16 of 16
    (33, 3, 5, 136, 2, "linear", True, None, True),        # kq 17 of 32
    (32 * 4096 + 33, 2, 3, 5, 2, "cubic", True, "tanh", True),  # 4098 work items on 2048 workgroups: second and third items
]
MISALIGNED = (33, 7, 4, 8, 8, "natural", True, "tanh", True)  # K % 4 == 0 and H C % 4 == 0: only the pointers decide


def gamma(n):
    return n * U / (1.0 - n * U)


def make(B, H, C, K, Tn, control, bias, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, K, generator=g)
    W = torch.randn(H * C, K, generator=g) * (1.5 / K ** 0.5)  # |pre| <~ 3: tanh is not saturated everywhere
    b = torch.randn(H * C, generator=g) * 0.5 if bias else None
    series = torch.randn(B, Tn, C, generator=g).cumsum(1)
    X = SPLINES[control](series.to(DEV))
    coef = X._coef.reshape(B, Tn, C) if control == "natural" else None
    return a, W, b, X, X._series.reshape(B, Tn, C), coef, X._t, torch.randn(B, H, generator=g)


def reference(a, W, b, dX, gout, act):
    """float64 from the fp32 inputs: out, s and their elementwise bounds (module docstring of the header; the bounds below)."""
    a, W, dX, gout = a.double(), W.double(), dX.double(), gout.double()
    B, K = a.shape
    C = dX.shape[1]
    H = W.shape[0] // C
    pre = a @ W.t() + (0 if b is None else b.double())
    mag = a.abs() @ W.abs().t() + (0 if b is None else b.double().abs())
    y = torch.tanh(pre) if act == "tanh" else pre
    T = TANH_ULP if act == "tanh" else 0.0
    dy = gamma(K + 2) * mag + T * U * y.abs()  # |act'| <= 1
    y3, dy3, dx3 = y.reshape(B, H, C), dy.reshape(B, H, C), dX[:, None, :]
    out = (y3 * dx3).sum(-1)
    out_bound = (dx3.abs() * dy3).sum(-1) + gamma(C + 2) * (y3 * dx3).abs().sum(-1)
    gd = gout[:, :, None] * dx3
    if act == "tanh":
        d = 1.0 - y3 * y3
        dd = 2.0 * y3.abs() * dy3 + dy3 * dy3 + gamma(3) * (1.0 + y3 * y3)  # 1 - y y: the first-order term, then its two roundings
    else:
        d, dd = torch.ones_like(y3), torch.zeros_like(y3)
    s = gd * d
    s_bound = gd.abs() * dd + gamma(3) * s.abs()  # the products gout * dX and (.) * d
    return out, out_bound, s.reshape(B, H * C), s_bound.reshape(B, H * C)


def off16(x):
    """``x``'s elements in a contiguous tensor that starts one element past a 16-byte boundary."""
    view = torch.empty(x.numel() + 4, dtype=x.dtype, device=x.device)[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def launch(be, a, W, b, series, coef, knots, t, method, act, gout, misalign=False):
    """Both directions.  ``misalign``: a, W and s one element off 16 bytes."""
    B, H = a.shape[0], W.shape[0] // series.shape[-1]
    out = torch.empty(B, H, device=DEV)
    s = torch.empty(B, W.shape[0], device=DEV)
    if misalign:
        a, W, s = off16(a), off16(W), off16(s)
    be._cde_head(out, a, W, b, series, coef, knots, t, method, act)
    be._cde_head_backward(s, gout, a, W, b, series, coef, knots, t, method, act)
    return out, s


def features(B, H, C, K, backward, misalign=False):
    return P.cde_features(_hip.get_backend()._cde_head_plan(B, H, C, K, torch.float32, None), B, H, C, K, backward, misalign)


def control(row):
    """The operands of ``make`` for a table row, the launch's time and method, and dX[B, C] from the numpy double, whose bits the
    contraction's device functions are held to (tests/test_gpu_cde.py, tests/test_gpu_spline.py)."""
    B, H, C, K, Tn, kind, bias, act, t_dev = row
    a, W, b, X, series, coef, knots, gout = make(*row[:7])
    t = 0.5 * (Tn - 1) + 0.125
    tk = torch.tensor(t, dtype=torch.float64, device=DEV) if t_dev else t
    double, th = SplineDoubleBackend(), torch.tensor(t, dtype=torch.float64) if t_dev else t
    if kind == "natural":
        dX = double._natural_dx(series.cpu(), coef.cpu(), knots.cpu(), th)
    else:
        dX = double._cde_dx(series.cpu(), knots.cpu(), th, kind)
    return (a, W, b, gout), (series, coef, knots, tk, None if kind == "natural" else kind), np.ascontiguousarray(dX), X


def check_integer_operands(be, row, misalign=False):
    """a, W and bias small integers, identity: the sums over k are exact whatever the matrix instruction does inside (the condition is
    asserted, not measured), so out and s must be the float32 statement of the header bit for bit.  gout and the control stay random
    reals."""
    B, H, C, K = row[:4]
    (_, _, _, gout), ctl, dX, _ = control(row)
    a, W, b = E.integer_operands(B, H * C, K, row[6])
    assert E.integer_condition(a, W, b) < 2.0 ** 24
    dev = [None if x is None else torch.from_numpy(x).to(DEV) for x in (a, W, b)]
    out, s = launch(be, *dev, *ctl, None, gout.to(DEV), misalign=misalign)
    assert np.array_equal(out.cpu().numpy(), E.cde_forward(a, W, b, dX)), ("out", row, misalign)
    assert np.array_equal(s.cpu().numpy(), E.cde_backward(dX, gout.numpy())), ("s", row, misalign)


def check_bounds(be, row, misalign=False):
    """Random operands against float64 within the bounds of test_the_launches_are_within_their_bounds_of_float64_and_deterministic; dX
    from the control's own derivative on the device, which must be the double's bits."""
    B, H, C, K, Tn, kind, bias, act, t_dev = row
    (a, W, b, gout), ctl, dX_double, X = control(row)
    dX = X.derivative(torch.tensor([0.5 * (Tn - 1) + 0.125], device=DEV)).reshape(B, C).cpu()
    assert np.array_equal(dX.numpy(), dX_double), ("dX", row)
    dev = [None if x is None else x.to(DEV) for x in (a, W, b)]
    out, s = launch(be, *dev, *ctl, act, gout.to(DEV), misalign=misalign)
    ref, ref_bound, sref, sref_bound = reference(a, W, b, dX, gout, act)
    for name, got, want, bound in (("out", out, ref, ref_bound), ("s", s, sref, sref_bound)):
        err = (got.cpu().double() - want).abs()
        print("{} {}: worst err / bound = {:.3f}".format(row, name, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (name, row, misalign)
    return out, s


def test_the_suites_shapes_reach_every_reachable_branch():
    """Over every launch of this module's table and its misaligned shape at the default settings, per direction: all six instantiations,
    every place the k-loop can leave early, every load and store decision, both dX sources, the tile and run edges, the slices, and
    second and third work items (tests/_head_plans.py).  A condition, not a measurement: after a retune that moves a shape off its
    branch this names the branch."""
    for backward in (False, True):
        seen = set().union(*(features(*row[:4], backward) for row in TABLE)) | features(*MISALIGNED[:4], backward, misalign=True)
        assert P.gaps(P.cde_required(backward), seen) == [], backward


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r))
def test_integer_operands_give_the_header_s_float32_statement_bit_for_bit(row):
    check_integer_operands(_hip.get_backend(), row)


def test_operands_one_element_off_16_bytes_give_the_aligned_launch_s_bits():
    """a, W and s contiguous views that start 4 bytes past a 16-byte boundary, with K % 4 == 0 and H C % 4 == 0: the launch decides
    for element access from the pointers alone, and nothing else may change."""
    be = _hip.get_backend()
    assert {"a:scalar-by-pointer", "W:scalar-by-pointer", "s-scalar-by-pointer"} <= features(*MISALIGNED[:4], True, misalign=True)
    assert {"a:vec", "W:vec", "s-vec"} <= features(*MISALIGNED[:4], True)
    assert all(torch.equal(x, y) for x, y in zip(check_bounds(be, MISALIGNED, misalign=True), check_bounds(be, MISALIGNED)))
    check_integer_operands(be, MISALIGNED, misalign=True)


def test_a_sliced_launch_beyond_the_grid_in_a_child_process():
    """The plans the default settings cannot reach (the slicing keeps the items within the grid): a grid of 2 workgroups, read once
    per process, so in a fresh child (tests/_head_grid_child.py) — sliced shapes take second and third work items with dX in LDS and
    per use; the child asserts that from the plans and holds every launch to the integer statement bit for bit and to the float64
    bounds."""
    env = dict(os.environ, XDE_GRID_BLOCKS="2")
    r = subprocess.run([sys.executable, "-m", "tests._head_grid_child", "cde"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "CHILD DONE" in r.stdout, r.stdout[-2000:]
    assert [line for line in r.stdout.splitlines() if line.startswith("FAIL ")] == []


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r))
def test_the_launches_are_within_their_bounds_of_float64_and_deterministic(row):
    """Forward:  |out - ref| <= sum_c |dX| (gamma_{K+2} (sum_k |a||W| + |bias|) + T u |y|) + gamma_{C+2} sum_c |y dX|.
    Backward, with dy = gamma_{K+2} (sum_k |a||W| + |bias|) + T u |y| the same error of y, g = gout dX and d = 1 - y y:
    |s - ref| <= |g| (2 |y| dy + dy^2 + gamma_3 (1 + y^2)) + gamma_3 |g d|   (identity: gamma_3 |g|).
    Two launches give the same bits."""
    B, H, C, K, Tn, control, bias, act, t_dev = row
    be = _hip.get_backend()
    a, W, b, X, series, coef, knots, gout = make(*row[:7])
    t = 0.5 * (Tn - 1) + 0.125
    dX = X.derivative(torch.tensor([t], device=DEV)).reshape(B, C).cpu()
    dev = [None if x is None else x.to(DEV) for x in (a, W, b)]
    tk = torch.tensor(t, dtype=torch.float64, device=DEV) if t_dev else t
    method = None if control == "natural" else control
    args = (be, *dev, series, coef, knots, tk, method, act, gout.to(DEV))
    out, s = launch(*args)
    out2, s2 = launch(*args)
    assert torch.equal(out, out2) and torch.equal(s, s2)
    ref, ref_bound, sref, sref_bound = reference(a, W, b, dX, gout, act)
    for name, got, want, bound in (("out", out, ref, ref_bound), ("s", s, sref, sref_bound)):
        err = (got.cpu().double() - want).abs()
        print("{} {}: worst err / bound = {:.3f}".format(row, name, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), name


def test_a_row_does_not_depend_on_its_batch():
    be = _hip.get_backend()
    row = (65, 7, 33, 33, 8, "cubic", True)
    a, W, b, X, series, coef, knots, gout = make(*row)
    a, W, b, gout = a.to(DEV), W.to(DEV), b.to(DEV), gout.to(DEV)
    t = torch.tensor(2.625, dtype=torch.float64, device=DEV)
    out, s = launch(be, a, W, b, series, coef, knots, t, "cubic", "tanh", gout)
    for r in (0, 40, 64):
        one, s_one = launch(be, a[r:r + 1].clone(), W, b, series[r:r + 1].clone(), None, knots, t, "cubic", "tanh", gout[r:r + 1].clone())
        assert torch.equal(one[0], out[r]) and torch.equal(s_one[0], s[r]), r


def test_a_refused_call_leaves_the_output_standing():
    be = _hip.get_backend()
    a, W, b, X, series, coef, knots, gout = make(2, 3, 4, 5, 5, "cubic", True)
    a, W, b, gout = a.to(DEV), W.to(DEV), b.to(DEV), gout.to(DEV)
    out, s = torch.full((2, 3), 7.0, device=DEV), torch.full((2, 12), 7.0, device=DEV)
    with pytest.raises(_hip.XdeError, match="XDE_HISTORY_BEZIER is not a control path"):
        be._cde_head(out, a, W, b, series, None, knots, 1.5, "bez", "tanh")
    with pytest.raises(_hip.XdeError, match="XDE_HISTORY_BEZIER is not a control path"):
        be._cde_head_backward(s, gout, a, W, b, series, None, knots, 1.5, "bez", "tanh")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((s == 7.0).all())


def test_the_activation_s_error():
    """The kernel's own tanh against float64 (K = 1, W = 1, C = 1, dX = 1 isolates it): within TANH_ULP ulps, which is what the bounds
    rely on (the constant is twice the 1.232 ulp this measured on gfx950)."""
    be = _hip.get_backend()
    n = 1 << 16
    a = torch.linspace(-4.0, 4.0, n).reshape(n, 1)
    X = LinearInterpolation(torch.arange(2.0).reshape(1, 2, 1).expand(n, 2, 1).contiguous().to(DEV))
    assert bool((X.derivative(torch.tensor([0.5], device=DEV)) == 1.0).all())
    out = torch.empty(n, 1, device=DEV)
    be._cde_head(out, a.to(DEV), torch.ones(1, 1, device=DEV), None, X._series, None, X._t, 0.5, "linear", "tanh")
    want = torch.tanh(a.double())
    ulp = 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 23)
    worst = float(((out.cpu().double() - want).abs() / ulp).max())
    print("tanhf worst error: {:.3f} ulp".format(worst))
    assert worst <= TANH_ULP


def _rk4_alt(f, z, ts):
    for t0, t1 in zip(ts[:-1], ts[1:]):
        dt = t1 - t0
        k1 = f(t0, z)
        k2 = f(t0 + dt / 3, z + dt * k1 / 3)
        k3 = f(t0 + 2 * dt / 3, z + dt * (k1 - k2 / 3))  # (the solver's default variant, as the reference writes it)
        k4 = f(t1, z + dt * (k1 - k2 + k3))
        z = z + dt * (k1 + 3 * (k2 + k3) + k4) / 8
    return z


def _solve_difference_bound(evals_f, evals_p, lin, head, dX, B, H, C, dt=1.0):
    """A bound on max |z_fused - z_unfused| over the knots, from each route's own evaluations ``(t, z, a)``.

    Per evaluation a route is within ``delta`` of the exact field at its z: the head's bound (``reference``) plus the trunk's rounding
    ``da = gamma_{H+2} (|z||Wt|^T + |bt|) + T u |a|`` carried through the head, ``sum_c |dX| (|Wh| da)`` (``|act'| <= 1``).  A stage
    combine rounds to within ``eta = gamma_8 (|z| + 3 dt sum_c |dX|)`` (at most five terms, ``|k| <= sum_c |dX|``).  With ``L`` the
    field's Lipschitz constant in the max norm, ``max_h sum_c |dX| sum_j (|Wh||Wt|)[hC+c, j]``, and ``A = 3`` the largest row sum of the
    solver's stage coefficients: a state difference ``e`` gives stage differences ``dk <= (L (e + eta) + delta) / (1 - A dt L)`` and
    ``e' <= (e + eta)(1 + g) + dt c delta`` with ``c = 1 / (1 - A dt L)``, ``g = dt L c`` — both routes' delta and eta added."""
    Wt, bt, Wh, bh = (x.detach().cpu().double() for x in (lin.weight, lin.bias, head.weight, head.bias))
    rows = (Wh.abs() @ Wt.abs()).sum(1).reshape(H, C)
    per, L = [], 0.0
    for evals in (evals_f, evals_p):
        out = []
        for t, z, a in evals:
            dXt = dX(t)
            da = gamma(H + 2) * (z.abs() @ Wt.abs().t() + bt.abs()) + TANH_ULP * U * a.abs()
            trunk = ((da @ Wh.abs().t()).reshape(B, H, C) * dXt.abs()[:, None, :]).sum(-1)
            delta = float((reference(a.float(), Wh.float(), bh.float(), dXt, torch.zeros(B, H), "tanh")[1] + trunk).max())
            eta = gamma(8) * float(z.abs().max() + 3 * dt * dXt.abs().sum(-1).max())
            L = max(L, float((rows[None] * dXt.abs()[:, None, :]).sum(-1).max()))
            out.append((delta, eta))
        per.append(out)
    assert 3 * dt * L < 1, L
    c = 1.0 / (1.0 - 3 * dt * L)
    g, e = dt * L * c, 0.0
    for n in range(0, len(per[0]), 4):
        both = [(df + dp, ef + ep) for (df, ef), (dp, ep) in zip(per[0][n:n + 4], per[1][n:n + 4])]
        e = (e + max(x[1] for x in both)) * (1 + g) + dt * c * max(x[0] for x in both)
    return e


def test_cdeint_through_the_fused_head_against_the_unfused_route_and_float64():
    """cdeint(RK4) with a loss and backward(): the fused launches run and the contraction's do not; the forward agrees with the unfused
    GPU solve within the per-evaluation bounds of both routes summed along the solve (``_solve_difference_bound``); every gradient's
    max-normalised error against a float64 CPU composition is at most 4 times the unfused route's (both are fp32 sums of equal length
    in different orders)."""
    B, H, C, K, Tn = 5, 4, 3, 6, 6
    torch.manual_seed(3)
    X = CubicHermiteSpline(torch.randn(B, Tn, C).cumsum(1).mul(0.01).to(DEV))  # (small increments: 3 dt L < 1 in the bound)
    z0 = torch.randn(B, H)

    class Trunk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(H, K)

        def forward(self, t, z):
            return torch.tanh(self.lin(z))

    fused = CDELinearHead(Trunk(), K, H, C).to(DEV)
    plain = copy.deepcopy(fused)
    plain.fuse = False
    be = _hip.get_backend()
    calls = []
    spied = {name: getattr(be, name) for name in ("_cde_head", "_cde_head_backward", "_cde_contract", "_cde_contract_backward")}

    def solve(model):
        evals = []
        hook = model.trunk.register_forward_hook(lambda m, args, a: evals.append((float(args[0]), args[1].detach().cpu().double(),
                                                                                  a.detach().cpu().double())))
        z = z0.to(DEV).requires_grad_()
        out = cdeint(model, X, z, X.grid_points, RK4)
        hook.remove()
        out.square().sum().backward()
        return out.detach().cpu(), [z.grad.cpu()] + [p.grad.cpu() for p in model.parameters()], evals

    try:
        for name, fn in spied.items():
            setattr(be, name, lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1])
        out_f, grads_f, evals_f = solve(fused)
        n_fused = len(calls)
        assert set(calls) == {"_cde_head", "_cde_head_backward"} and calls.count("_cde_head") == 4 * (Tn - 1) == len(evals_f)
        out_p, grads_p, evals_p = solve(plain)
        assert set(calls[n_fused:]) == {"_cde_contract", "_cde_contract_backward"} and len(evals_p) == len(evals_f)
    finally:
        for name in spied:
            delattr(be, name)

    dX = lambda t: X.derivative(torch.tensor([float(t)], device=DEV)).reshape(B, C).cpu().double()  # noqa: E731
    bound = _solve_difference_bound(evals_f, evals_p, fused.trunk.lin, fused.head, dX, B, H, C)
    diff = float((out_f - out_p).abs().max())
    print("forward fused - unfused: {:.3e}, bound {:.3e}, err / bound = {:.3f}".format(diff, bound, diff / bound))
    assert diff <= bound
    # the float64 CPU composition of the same solve and loss (X'(t): the control's own fp32 bits)
    ref = copy.deepcopy(fused).cpu().double()
    zr = z0.double().requires_grad_()
    ts = [float(t) for t in X.grid_points.cpu()]
    states = [zr]
    for i in range(Tn - 1):
        states.append(_rk4_alt(lambda t, z: (ref(t, z) * dX(t)[:, None, :]).sum(-1), states[-1], ts[i:i + 2]))
    torch.stack(states).square().sum().backward()
    grads_r = [zr.grad] + [p.grad for p in ref.parameters()]
    for gf, gp, gr in zip(grads_f, grads_p, grads_r):
        scale = float(gr.abs().max())
        ef, ep = float((gf.double() - gr).abs().max()) / scale, float((gp.double() - gr).abs().max()) / scale
        print("gradient {}: fused {:.3e}, unfused {:.3e}, ratio {:.2f}".format(tuple(gr.shape), ef, ep, ef / max(ep, 1e-300)))
        assert ef <= 4 * max(ep, U)


def test_cde_demo_with_the_fused_head():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import cde_demo

    losses = cde_demo.train(max_steps=5, n=32, length=16, log_every=0, fused_head=True)
    assert all(np.isfinite(losses)), losses
