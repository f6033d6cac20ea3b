"""The fused last layer of a matrix diffusion (include/xde_hip_sdehead.h) against float64 on the CPU: the increments bit for bit, an
error bound per shape (this kernel's sums over k run on the matrix cores, whose in-instruction order no host program can restate),
determinism and row independence, and one solve through sdeint(Euler) against the plain route.  On small integer operands the sums
over k are exact under any rounding, and there the launches are held to the header's float32 statement (tests/_head_exact.py) bit for
bit: the order of the runs of m, the carries, the element mapping.  tests/_head_plans.py names the branches the shapes reach together;
a sliced launch beyond the grid needs a small grid in a fresh process (tests/_head_grid_child.py).

Measured on gfx950 (worst err / bound over the table): see DESIGN section 24."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler
from paddlexde_amd.xde import SDELinearHead

from . import _head_exact as E
from . import _head_plans as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TANH_ULP = 2.5  # the device tanhf's error in ulps: twice the 1.232 ulp measured through the CDE head's kernel
DT, S, SEED, STEP = 0.0625, 0.25, 0x1234567887654321, 3  # (s = sqrt(dt), exact in float32)

# rows, D, M, K, act, bias
TABLE = [
    (1, 1, 1, 1, None, False),      # the minimum
    (65, 3, 3, 5, "tanh", True),    # a 65th row; M % 4 != 0 and a partial last Philox block; odd K < 8; D M < 32
    (33, 5, 8, 33, "tanh", True),   # uneven k halves; D M = 40 crosses a 32-chunk
    (64, 4, 40, 8, None, True),     # a run of m longer than a chunk; 160 crosses a pass
    (7, 2, 130, 12, "tanh", True),  # a run longer than a whole pass: the carry survives a pass; increments generated per use
    (2, 130, 1, 4, "tanh", False),  # scalar noise, runs of length 1, slices
    (40, 16, 4, 128, "tanh", True),  # the two-tile cap
    (40, 16, 4, 256, "tanh", True),  # the one-tile cap
    (33, 3, 3, 20, "tanh", True),    # kq 3 of 8 registers: the k-loop leaves after its first group of four; vector loads
    (33, 3, 3, 27, None, True),      # kq 4 of 8, loads by element
    (33, 5, 8, 72, "tanh", True),    # kq 9 of 16
    (70, 3, 4, 136, "tanh", True),   # kq 17 of 32: the one-tile plan, three row tiles
    (130, 66, 1, 4, "tanh", True),   # slices with three row tiles of two tiles each
    (70, 2, 50, 12, "tanh", True),   # increments per use with a populated second tile; slice 1 starts at n = 50: s by element
    (64 * 4096 + 65, 2, 3, 5, "tanh", True),  # 4098 work items on 2048 workgroups: second and third items, the barrier, the parity
]
MISALIGNED = (33, 5, 8, 72)  # K % 4 == 0 and D M % 4 == 0: only the pointers send a, W and s to the element path
GF_NULL = (70, 2, 50, 12)


def gamma(n):
    return n * U / (1.0 - n * U)


def make(rows, D, M, K, bias, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, K, generator=g)
    W = torch.randn(D * M, K, generator=g) * (1.5 / K ** 0.5)  # |pre| <~ 3: tanh is not saturated everywhere
    b = torch.randn(D * M, generator=g) * 0.5 if bias else None
    y0, f, gy = (torch.randn(rows, D, generator=g) for _ in range(3))
    return [None if x is None else x.to(DEV) for x in (a, W, b, y0, f, gy)]


def increments(be, rows, M, seed=SEED, k=STEP, s=S):
    """w[r, m] = s * Z[r M + m] from the library's own noise query on a [rows, M] buffer: the bits the kernels must use."""
    z = torch.empty(rows, M, device=DEV)
    be._sde_noise(z, seed, k)
    return z * torch.tensor(s, dtype=torch.float32, device=DEV)


def off16(x):
    """``x``'s elements in a contiguous tensor that starts one element past a 16-byte boundary."""
    view = torch.empty(x.numel() + 4, dtype=x.dtype, device=x.device)[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def launch(be, ops, act, in_place=False, misalign=False, gf_null=False):
    """Both directions.  ``misalign``: a, W and s one element off 16 bytes; ``gf_null``: the backward without gf (None is returned)."""
    a, W, b, y0, f, gy = ops
    if misalign:
        a, W = off16(a), off16(W)
    y1 = y0.clone() if in_place else torch.empty_like(y0)
    be._sde_head_step(y1, y1 if in_place else y0, f, a, W, b, act, DT, S, SEED, STEP)
    s_out, gf = torch.empty(a.shape[0], W.shape[0], device=DEV), None if gf_null else torch.empty_like(gy)
    if misalign:
        s_out = off16(s_out)
    be._sde_head_backward(s_out, gf, gy, a, W, b, act, DT, S, SEED, STEP)
    return y1, s_out, gf


def features(rows, D, M, K, backward, misalign=False, gf_null=False):
    return P.sde_features(_hip.sde_head_plan(rows, D, M, K, torch.float32, None), rows, D, M, K, backward, misalign, gf_null)


def check_integer_operands(be, rows, D, M, K, bias, misalign=False, gf_null=False):
    """a, W and bias small integers, identity: the sums over k are exact whatever the matrix instruction does inside (the condition is
    asserted, not measured), so y1, s and gf must be the float32 statement of the header bit for bit.  y0, f, gy1 stay random reals."""
    a, W, b = E.integer_operands(rows, D * M, K, bias)
    assert E.integer_condition(a, W, b) < 2.0 ** 24
    rest = make(rows, D, M, 1, False, seed=1)[3:]
    ops = [None if x is None else torch.from_numpy(x).to(DEV) for x in (a, W, b)] + rest
    y1, s_out, gf = launch(be, ops, None, misalign=misalign, gf_null=gf_null)
    w = increments(be, rows, M).cpu().numpy()
    y0, f, gy = (x.cpu().numpy() for x in rest)
    want_s, want_gf = E.sde_backward(w, gy, DT)
    where = (rows, D, M, K, bias, misalign, gf_null)
    assert np.array_equal(y1.cpu().numpy(), E.sde_forward(a, W, b, w, y0, f, DT)), ("y1", where)
    assert np.array_equal(s_out.cpu().numpy(), want_s), ("s", where)
    assert gf_null or np.array_equal(gf.cpu().numpy(), want_gf), ("gf", where)


def check_bounds(be, row, misalign=False):
    """Random operands against float64 within the bounds of test_the_launches_are_within_their_bounds_of_float64_and_deterministic."""
    rows, D, M, K, act, bias = row
    ops = make(rows, D, M, K, bias)
    got = launch(be, ops, act, misalign=misalign)
    for name, x, (want, bound) in zip(("y1", "s", "gf"), got, reference(ops, increments(be, rows, M), act, M)):
        err = (x.cpu().double() - want).abs()
        print("{} {}: worst err / bound = {:.3f}".format(row, name, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (name, row, misalign)
    return got


def reference(ops, w, act, M):
    """float64 from the fp32 operand bits: y1, s, gf and their elementwise bounds (the test's docstring below)."""
    a, W, b, y0, f, gy = (None if x is None else x.cpu().double() for x in ops)
    w = w.cpu().double()
    rows, K = a.shape
    D = y0.shape[1]
    mag = a.abs() @ W.abs().t()
    pre = a @ W.t() + (0 if b is None else b)
    dpre = gamma(K + 2) * mag + (0 if b is None else U * (mag + b.abs()))
    y = torch.tanh(pre) if act == "tanh" else pre
    dy = dpre + (TANH_ULP * U * y.abs() if act == "tanh" else 0)  # |act'| <= 1
    y3, dy3, w3 = y.reshape(rows, D, M), dy.reshape(rows, D, M), w[:, None, :]
    p = y3 * w3
    acc = p.sum(-1)
    acc_bound = (w3.abs() * dy3).sum(-1) + U * p.abs().sum(-1) + gamma(M + 2) * p.abs().sum(-1)
    y1 = (y0 + f * DT) + acc
    y1_bound = acc_bound + 3 * U * (y0.abs() + (f * DT).abs() + acc.abs())
    gw = gy[:, :, None] * w3
    if act == "tanh":
        d = 1.0 - y3 * y3
        dd = 2.0 * y3.abs() * dy3 + dy3 * dy3 + gamma(3) * (1.0 + y3 * y3)  # 1 - y y: the first-order term, then its two roundings
    else:
        d, dd = torch.ones_like(y3), torch.zeros_like(y3)
    s = gw * d
    s_bound = gw.abs() * dd + gamma(3) * s.abs()  # the products gy1 * w and (.) * d
    return (y1, y1_bound), (s.reshape(rows, D * M), s_bound.reshape(rows, D * M)), (gy * DT, U * (gy * DT).abs())


HIGH_SEED, LAST_STEP = 0xfedcba9800000001, 2 ** 32 - 1  # the edge of 0 <= k < 2^32, under a seed whose high word is set


@pytest.mark.parametrize("M, m0, seed, k", [(1, 0, SEED, STEP), (3, 0, SEED, STEP), (3, 2, SEED, STEP), (8, 0, SEED, STEP), (8, 5, SEED, STEP),
                                            (8, 7, SEED, STEP), (3, 1, HIGH_SEED, LAST_STEP)],
                         ids=["1-0", "3-0", "3-2", "8-0", "8-5", "8-7", "3-1-last-step-high-seed"])
def test_the_increments_are_the_library_s_bit_for_bit(M, m0, seed, k):
    """a = 0, K = 1, identity, bias = 1 where m == m0: y1[r, d] is s * Z[r M + m0] (+-0 from every other m), for every d.  The last
    case is the last step the header admits; its increments are neither step 0's nor those of the seed's low word alone."""
    be = _hip.get_backend()
    rows, D = 65, 3
    bias = torch.zeros(D, M, device=DEV)
    bias[:, m0] = 1.0
    zero = torch.zeros(rows, D, device=DEV)
    y1 = torch.full((rows, D), 7.0, device=DEV)
    be._sde_head_step(y1, zero, zero.clone(), torch.zeros(rows, 1, device=DEV), torch.ones(D * M, 1, device=DEV), bias.reshape(-1), None, DT, S,
                      seed, k)
    w = increments(be, rows, M, seed, k)
    assert torch.equal(y1, w[:, m0:m0 + 1].expand(rows, D))
    if k == LAST_STEP:
        assert not torch.equal(w, increments(be, rows, M, seed, 0)) and not torch.equal(w, increments(be, rows, M, seed & 0xffffffff, k))


def test_the_table_meets_every_plan():
    plans = [_hip.sde_head_plan(*row[:4], torch.float32, row[4]) for row in TABLE]
    assert all(p["served"] for p in plans) and {p["tiles"] for p in plans} == {1, 2}
    assert any(p["S"] > 1 for p in plans) and any(p["S"] == 1 for p in plans) and {p["lds_w"] for p in plans} == {0, 1}


def test_the_suites_shapes_reach_every_reachable_branch():
    """Over every launch of this module at the default settings (the table, the misaligned shape, the backward without gf), per
    direction: every instantiation, every place the k-loop can leave early, every load and store decision, both increment sources,
    the tile and run edges, the slices, and second and third work items (tests/_head_plans.py).  A condition, not a measurement:
    after a retune that moves a shape off its branch this names the branch."""
    for backward in (False, True):
        seen = set().union(*(features(*row[:4], backward) for row in TABLE))
        seen |= features(*MISALIGNED, backward, misalign=True) | features(*GF_NULL, backward, gf_null=True)
        assert P.gaps(P.sde_required(backward), seen) == [], backward


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r))
def test_the_launches_are_within_their_bounds_of_float64_and_deterministic(row):
    """With dpre = gamma_{K+2} sum_k |a||W| + u (sum_k |a||W| + |bias|) (the bias's rounding; none without it) and
    dy = dpre + T u |y| (identity: dpre), p = y w:
    forward:  |y1 - ref| <= sum_m |w| dy + u sum_m |p| + gamma_{M+2} sum_m |p| + 3 u (|y0| + |f dt| + |sum_m p|);
    backward: |s - ref| <= |gy1 w| (2 |y| dy + dy^2 + gamma_3 (1 + y^2)) + gamma_3 |s|   (identity: gamma_3 |s|),  |gf - ref| <= u |gy1 dt|.
    Two launches give the same bits; the (65, 3, 3, 5) case also steps in place (y1 is y0) to the same bits."""
    rows, D, M, K, act, bias = row
    be = _hip.get_backend()
    got = check_bounds(be, row)
    ops = make(rows, D, M, K, bias)
    assert all(torch.equal(x, y) for x, y in zip(got, launch(be, ops, act)))
    if rows == 65:
        assert torch.equal(got[0], launch(be, ops, act, in_place=True)[0])


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r))
def test_integer_operands_give_the_header_s_float32_statement_bit_for_bit(row):
    check_integer_operands(_hip.get_backend(), *row[:4], row[5])


def test_operands_one_element_off_16_bytes_give_the_aligned_launch_s_bits():
    """a, W and s contiguous views that start 4 bytes past a 16-byte boundary, with K % 4 == 0 and D M % 4 == 0: the launch decides
    for element access from the pointers alone, and nothing else may change."""
    be = _hip.get_backend()
    row = MISALIGNED + ("tanh", True)
    assert {"a:scalar-by-pointer", "W:scalar-by-pointer", "s-scalar-by-pointer"} <= features(*MISALIGNED, True, misalign=True)
    assert {"a:vec", "W:vec", "s-vec"} <= features(*MISALIGNED, True)
    assert all(torch.equal(x, y) for x, y in zip(check_bounds(be, row, misalign=True), launch(be, make(*MISALIGNED, True), "tanh")))
    check_integer_operands(be, *MISALIGNED, True, misalign=True)


def test_the_backward_without_gf_writes_the_same_s():
    be = _hip.get_backend()
    ops = make(*GF_NULL, True)
    with_gf, without = launch(be, ops, "tanh"), launch(be, ops, "tanh", gf_null=True)
    assert without[2] is None and torch.equal(with_gf[1], without[1])
    check_integer_operands(be, *GF_NULL, True, gf_null=True)


def test_a_sliced_launch_beyond_the_grid_in_a_child_process():
    """The plans the default settings cannot reach (the slicing keeps the items within the grid): a grid of 2 workgroups, read once
    per process, so in a fresh child (tests/_head_grid_child.py) — sliced shapes take second and third work items in both increment
    sources and on the one-tile plan; the child asserts that from the plans and holds every launch to the integer statement bit for
    bit and to the float64 bounds."""
    env = dict(os.environ, XDE_GRID_BLOCKS="2")
    r = subprocess.run([sys.executable, "-m", "tests._head_grid_child", "sde"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "CHILD DONE" in r.stdout, r.stdout[-2000:]
    assert [line for line in r.stdout.splitlines() if line.startswith("FAIL ")] == []


def test_a_row_does_not_depend_on_its_batch():
    """The increment of flat element e depends on e only, so the first 65 rows of a 130-row launch are the 65-row launch, and row 0 is
    the one-row launch."""
    be = _hip.get_backend()
    big = make(130, 5, 8, 33, True)
    lead = lambda n: [x if i in (1, 2) else x[:n].clone() for i, x in enumerate(big)]  # noqa: E731  (W and bias are shared)
    out130, out65, out1 = launch(be, big, "tanh"), launch(be, lead(65), "tanh"), launch(be, lead(1), "tanh")
    assert all(torch.equal(x[:65], y) for x, y in zip(out130, out65))
    assert all(torch.equal(x[:1], y) for x, y in zip(out65, out1))


def test_sdeint_through_the_fused_head_against_the_plain_route_and_float64():
    """sdeint(Euler), 4 steps, a loss and backward(): the path and every gradient (y0, drift, trunk, head.weight, head.bias) of the
    fused route and of the plain route against a float64 CPU composition on the library's own increments.  The fused route's
    max-normalised error is at most 4 times the plain route's (or 2^-24): both are fp32 sums of equal length in different orders.
    The fused forward saves no tensor of rows D M elements; the plain one does."""
    B, D, M, K, steps, seed = 5, 4, 3, 6, 4, 11
    torch.manual_seed(5)

    class Net(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.lin = torch.nn.Linear(D, n)

        def forward(self, t, y):
            return torch.tanh(self.lin(y))

    drift, head = Net(D).to(DEV), SDELinearHead(Net(K), K, D, M).to(DEV)
    y0 = torch.randn(B, 1, D)
    t = torch.linspace(0.0, 1.0, steps + 1)  # dt = 0.25, s = 0.5
    be = _hip.get_backend()
    calls = []
    spied = {name: getattr(be, name) for name in ("_sde_head_step", "_sde_head_backward", "_sde_gn_step", "_sde_gn_backward")}

    def solve(f, g, fuse):
        g.fuse = fuse
        sizes = []
        y = y0.to(DEV).requires_grad_()
        with torch.autograd.graph.saved_tensors_hooks(lambda x: (sizes.append(x.numel()), x)[1], lambda x: x):
            xs = sdeint(f, g, y, t.to(DEV), Euler, options={"noise_type": "general", "seed": seed, "norm": None})
        xs.square().sum().backward()
        return [xs.detach().cpu(), y.grad.cpu()] + [p.grad.cpu() for p in list(f.parameters()) + list(g.parameters())], sizes

    try:
        for name, fn in spied.items():
            setattr(be, name, lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1])
        fused, sizes_f = solve(drift, head, True)
        assert calls == ["_sde_head_step"] * steps + ["_sde_head_backward"] * steps and B * D * M not in sizes_f
        del calls[:]
        plain, sizes_p = solve(copy.deepcopy(drift), copy.deepcopy(head), False)
        assert calls == ["_sde_gn_step"] * steps + ["_sde_gn_backward"] * steps and B * D * M in sizes_p
    finally:
        for name in spied:
            delattr(be, name)

    fr, gr = copy.deepcopy(drift).cpu().double(), copy.deepcopy(head).cpu().double()
    yr = y0.double().requires_grad_()
    path = [yr]
    for k in range(steps):
        w = increments(be, B, M, seed, k, 0.5).cpu().double().reshape(B, 1, 1, M)
        path.append(path[-1] + fr(t[k], path[-1]) * 0.25 + (gr(t[k], path[-1]) * w).sum(-1))
    xs = torch.cat(path, dim=-2)
    xs.square().sum().backward()
    ref = [xs.detach(), yr.grad] + [p.grad for p in list(fr.parameters()) + list(gr.parameters())]
    assert len(ref) == 2 + 2 + 4 and fused[0].shape == ref[0].shape
    for name, xf, xp, xr in zip(("path", "y0", "drift.w", "drift.b", "trunk.w", "trunk.b", "head.w", "head.b"), fused, plain, ref):
        scale = float(xr.abs().max())
        ef, ep = float((xf.double() - xr).abs().max()) / scale, float((xp.double() - xr).abs().max()) / scale
        print("{}: fused {:.3e}, plain {:.3e}, ratio {:.2f}".format(name, ef, ep, ef / max(ep, 1e-300)))
        assert ef <= 4 * max(ep, U), name
