"""The fused last layer of a matrix diffusion (include/xde_hip_sdehead.h) against float64 on the CPU: the increments bit for bit, an
error bound per shape (this kernel's sums over k run on the matrix cores, whose in-instruction order no host program can restate),
determinism and row independence, and one solve through sdeint(Euler) against the plain route.

Measured on gfx950 (worst err / bound over the table): see DESIGN section 24."""
import copy

import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler
from paddlexde_amd.xde import SDELinearHead

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
]


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


def launch(be, ops, act, in_place=False):
    a, W, b, y0, f, gy = ops
    y1 = y0.clone() if in_place else torch.empty_like(y0)
    be._sde_head_step(y1, y1 if in_place else y0, f, a, W, b, act, DT, S, SEED, STEP)
    s_out, gf = torch.empty(a.shape[0], W.shape[0], device=DEV), torch.empty_like(gy)
    be._sde_head_backward(s_out, gf, gy, a, W, b, act, DT, S, SEED, STEP)
    return y1, s_out, gf


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


@pytest.mark.parametrize("M, m0", [(1, 0), (3, 0), (3, 2), (8, 0), (8, 5), (8, 7)])
def test_the_increments_are_the_library_s_bit_for_bit(M, m0):
    """a = 0, K = 1, identity, bias = 1 where m == m0: y1[r, d] is s * Z[r M + m0] (+-0 from every other m), for every d."""
    be = _hip.get_backend()
    rows, D = 65, 3
    bias = torch.zeros(D, M, device=DEV)
    bias[:, m0] = 1.0
    zero = torch.zeros(rows, D, device=DEV)
    y1 = torch.full((rows, D), 7.0, device=DEV)
    be._sde_head_step(y1, zero, zero.clone(), torch.zeros(rows, 1, device=DEV), torch.ones(D * M, 1, device=DEV), bias.reshape(-1), None, DT, S,
                      SEED, STEP)
    assert torch.equal(y1, increments(be, rows, M)[:, m0:m0 + 1].expand(rows, D))


def test_the_table_meets_every_plan():
    plans = [_hip.sde_head_plan(*row[:4], torch.float32, row[4]) for row in TABLE]
    assert all(p["served"] for p in plans) and {p["tiles"] for p in plans} == {1, 2}
    assert any(p["S"] > 1 for p in plans) and any(p["S"] == 1 for p in plans) and {p["lds_w"] for p in plans} == {0, 1}


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r))
def test_the_launches_are_within_their_bounds_of_float64_and_deterministic(row):
    """With dpre = gamma_{K+2} sum_k |a||W| + u (sum_k |a||W| + |bias|) (the bias's rounding; none without it) and
    dy = dpre + T u |y| (identity: dpre), p = y w:
    forward:  |y1 - ref| <= sum_m |w| dy + u sum_m |p| + gamma_{M+2} sum_m |p| + 3 u (|y0| + |f dt| + |sum_m p|);
    backward: |s - ref| <= |gy1 w| (2 |y| dy + dy^2 + gamma_3 (1 + y^2)) + gamma_3 |s|   (identity: gamma_3 |s|),  |gf - ref| <= u |gy1 dt|.
    Two launches give the same bits; the (65, 3, 3, 5) case also steps in place (y1 is y0) to the same bits."""
    rows, D, M, K, act, bias = row
    be = _hip.get_backend()
    ops = make(rows, D, M, K, bias)
    got = launch(be, ops, act)
    assert all(torch.equal(x, y) for x, y in zip(got, launch(be, ops, act)))
    if rows == 65:
        assert torch.equal(got[0], launch(be, ops, act, in_place=True)[0])
    for name, x, (want, bound) in zip(("y1", "s", "gf"), got, reference(ops, increments(be, rows, M), act, M)):
        err = (x.cpu().double() - want).abs()
        print("{} {}: worst err / bound = {:.3f}".format(row, name, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), name


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
