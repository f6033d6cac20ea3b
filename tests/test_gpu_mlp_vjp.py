"""The fused MLP field's vector-Jacobian product (xde_mlp_field_vjp, include/xde_hip_mlp.h) on the device, one table of shapes: every
output against a float64 numpy statement of the header's formulas on the same float32 operands, within 4 times the plain float32
autograd route's own error (both are fp32 sums of equal length in different orders; the fused ones run on the matrix cores, whose
in-instruction order no host program can restate) with a floor of 4 ulps of the output's magnitude; ``f`` the forward launch's bits;
determinism; row independence of ``f`` and ``gx``; small-integer operands exactly; and the adjoint's backward solve through the hook."""
import copy

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import odeint_adjoint
from paddlexde_amd.solver import RK4
from paddlexde_amd.xde import MLPField

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# widths, act, bias, time
TABLE = [
    ((2, 50, 2), "tanh", True, True),         # the spiral demo's field with a time column: gt and the time column of gW_0
    ((3, 7, 5, 2), "tanh", True, False),      # nothing aligned
    ((4, 32, 64, 4), "tanh", True, False),    # aligned, exact chunks: x, a, f and gx by vector, two chunks of gW_1 per wave
    ((5, 33, 4), "tanh", False, False),       # one past a chunk; no bias
    ((2, 8, 8, 8, 2), "tanh", True, False),   # four layers
    ((3, 7, 5, 2), None, True, False),        # the identity between layers
    ((5, 33, 4), None, True, True),
]
IDS = ["-".join(str(x) for x in r[0] + r[1:]) for r in TABLE]
ROWS, MAX_BLOCKS = (1, 33, 100), (0, 1, 3)  # 100 rows: 4 items; max_blocks 1 puts all four through one slab, 3 makes the loop uneven


def make(row, rows, integers=False, seed=0):
    """The module (on the host), y, the cotangent and the time; ``integers``: the identity and small-integer, sparse operands."""
    widths, act, bias, time = row
    g = torch.Generator().manual_seed(len(widths) * 1000 + rows + 7919 * seed)
    torch.manual_seed(len(widths) * 1000 + rows + 7919 * seed)  # (the layers' initial weights come from the global generator)
    m = MLPField(widths[0], widths[1:-1], widths[-1], activation=None if integers else act, time=time, bias=bias)
    y, a, t = torch.randn(rows, widths[0], generator=g), torch.randn(rows, widths[-1], generator=g), 0.75
    if integers:
        y, a, t = [torch.randint(-1, 2, x.shape, generator=g).float() for x in (y, a)] + [3.0]
        for p in m.parameters():  # (about 4 weights of a row are not zero: see the bound in the test)
            p.data = torch.randint(-1, 2, p.shape, generator=g).float() * (torch.rand(p.shape, generator=g) < 4.0 / max(p.shape[-1], 8))
    return m, y, a, t


def reference(m, t, y, a, magnitude=False):
    """The header's formulas in float64 numpy from the float32 operand bits, in ``vjp``'s order: f, gt, gx, then gW_l, gb_l per layer.
    ``magnitude`` (identity only): the same sums over the operands' absolute values, a bound on every partial sum in any order.
    Second, the sum of the magnitudes of gt's terms, sum |dpre_0[r, n] W_0[n, K]|: gt is ONE number that its terms nearly cancel in
    (by a factor of 335 at 33 rows of the first shape), so an fp32 sum in any order is good to ulps of that, not of gt itself."""
    f64 = lambda x: np.abs(x.detach().double().numpy()) if magnitude else x.detach().double().numpy()  # noqa: E731
    tanh = m.activation == "tanh"
    assert not (magnitude and tanh)
    d, h, tcol, hs, gt, gt_terms = f64(a), f64(y), np.full((y.shape[0], 1), float(t)), [], None, 0.0  # (t >= 0 in this module)
    for i, layer in enumerate(m.layers):
        W, K = f64(layer.weight), h.shape[1]
        h = np.tanh(h) if tanh and i else h
        hs.append(h)
        h = h @ W[:, :K].T + (0.0 if layer.bias is None else f64(layer.bias)) + (tcol * W[:, K] if W.shape[1] > K else 0.0)
    f, grads = h, []
    for l in reversed(range(len(m.layers))):
        W, K = f64(m.layers[l].weight), hs[l].shape[1]
        gW = d.T @ hs[l]
        if W.shape[1] > K:
            gW, gt, gt_terms = np.hstack([gW, d.T @ tcol]), (d.sum(0) * W[:, K]).sum(), float((np.abs(d) @ np.abs(W[:, K])).sum())
        grads = [gW] + ([] if m.layers[l].bias is None else [d.sum(0)]) + grads
        d = d @ W[:, :K]
        d = d * (1.0 - hs[l] * hs[l]) if tanh and l else d
    return [f, gt, d] + grads, gt_terms


def both(m, t, y, a, max_blocks=0):
    m.vjp_max_blocks, m.fuse = max_blocks, True
    fused = m.vjp(t, y, a)
    m.fuse = False
    plain = m.vjp(t, y, a)
    m.vjp_max_blocks, m.fuse = 0, True
    return fused, plain


def err(got, want, scale=None):
    return float(np.abs(got.detach().cpu().double().numpy() - want).max() / max(scale or np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("row", TABLE, ids=IDS)
def test_every_output_is_within_the_plain_route_s_error_of_float64_on_every_grid(row, rows):
    m, y, a, t = make(row, rows)
    want, gt_terms = reference(m, t, y, a)
    m, y, a = m.to(DEV), y.to(DEV), a.to(DEV)
    with torch.no_grad():
        forward = m(t, y)
    first = None
    for max_blocks in MAX_BLOCKS:
        fused, plain = both(m, t, y, a, max_blocks)
        assert len(fused) == len(plain) == len(want) and (fused[1] is None) == (want[1] is None) == (not row[3])
        for i, (gf, gp, w) in enumerate(zip(fused, plain, want)):
            if w is None:
                continue
            assert gf.shape == gp.shape == w.shape and gf.dtype == torch.float32
            scale = gt_terms if i == 1 else None  # (gt against the magnitude of its terms, every array against its largest entry)
            ef, ep = err(gf, w, scale), err(gp, w, scale)
            print("{} rows {} max_blocks {} output {}: fused {:.3e}, plain {:.3e}, ratio {:.2f}".format(row, rows, max_blocks, i, ef, ep, ef / max(ep, U)))
            assert ef <= 4 * max(ep, U), (i, ef, ep)
        assert torch.equal(fused[0], forward)  # f: the forward launch's bits
        again = both(m, t, y, a, max_blocks)[0]
        assert all(x is None or torch.equal(x, z) for x, z in zip(fused, again))  # two calls, the same bits
        first = first or fused
        assert torch.equal(fused[0], first[0]) and torch.equal(fused[2], first[2])  # f and gx do not depend on the grid


def test_a_row_of_f_and_gx_does_not_depend_on_its_batch():
    m, y, a, t = make(TABLE[0], 100)
    m, y, a = m.to(DEV), y.to(DEV), a.to(DEV)
    batch = both(m, t, y, a)[0]
    for lo, hi in ((0, 33), (40, 41), (96, 100)):
        part = both(m, t, y[lo:hi], a[lo:hi], 1)[0]
        assert torch.equal(batch[0][lo:hi], part[0]) and torch.equal(batch[2][lo:hi], part[2]), (lo, hi)


@pytest.mark.parametrize("row", TABLE[:5], ids=IDS[:5])
def test_integer_operands_give_the_header_s_statement_exactly(row):
    m, y, a, t = make(row, 100, integers=True)
    want, bound = reference(m, t, y, a)[0], reference(m, t, y, a, magnitude=True)[0]
    assert max(float(b.max()) for b in bound if b is not None) < 2.0 ** 24  # every partial sum is an integer float32 holds, in any order
    assert all(np.abs(w).max() > 0 for w in want if np.ndim(w))  # (gt, a scalar, may cancel to zero)
    m, y, a = m.to(DEV), y.to(DEV), a.to(DEV)
    for max_blocks in MAX_BLOCKS:
        fused = both(m, t, y, a, max_blocks)[0]
        for i, (gf, w) in enumerate(zip(fused, want)):
            assert w is None or np.array_equal(gf.cpu().numpy(), w.astype(np.float32)), (max_blocks, i)


def test_the_backward_solve_through_the_hook_is_one_vjp_call_per_evaluation():
    """``odeint_adjoint`` with ``adjoint_options={"vjp": field.vjp}``: the backward solve calls ``_mlp_field_vjp`` once per evaluation of
    the augmented dynamics and ``_mlp_field`` never, and its gradients are as near a float64 run as those of the same call without the
    hook (the table's margin)."""
    torch.manual_seed(3)
    m = MLPField(2, 50).to(DEV)
    y0, t = torch.randn(64, 1, 2, device=DEV), torch.linspace(0.0, 1.0, 5, device=DEV)
    be, counts, evals = _hip.get_backend(), {"_mlp_field": 0, "_mlp_field_vjp": 0}, []

    def counted(name):
        launch = getattr(be, name)
        return lambda *args: (counts.__setitem__(name, counts[name] + 1), launch(*args))[1]

    def grads(field, y_start, tt, **kw):
        y_start = y_start.clone().requires_grad_(True)
        field.zero_grad()
        odeint_adjoint(field, y_start, tt, solver=RK4, **kw).square().sum().backward()
        return [y_start.grad] + [p.grad.clone() for p in field.parameters()]

    want = [g.cpu().numpy() for g in grads(copy.deepcopy(m).double(), y0.double(), t.double())]
    plain = grads(m, y0, t)
    vjp = m.vjp
    try:
        be._mlp_field, be._mlp_field_vjp = counted("_mlp_field"), counted("_mlp_field_vjp")
        y_start = y0.clone().requires_grad_(True)
        m.zero_grad()
        loss = odeint_adjoint(m, y_start, t, solver=RK4, adjoint_options={"vjp": lambda *args: (evals.append(1), vjp(*args))[1]}).square().sum()
        counts.update(_mlp_field=0, _mlp_field_vjp=0)  # (the forward solve is over: one _mlp_field call per stage)
        loss.backward()
        hooked = [y_start.grad] + [p.grad.clone() for p in m.parameters()]
    finally:
        del be._mlp_field, be._mlp_field_vjp
    assert counts["_mlp_field"] == 0 and counts["_mlp_field_vjp"] == len(evals) > 0
    for i, (gh, gp, w) in enumerate(zip(hooked, plain, want)):
        eh, ep = err(gh, w), err(gp, w)
        print("gradient {}: hook {:.3e}, plain {:.3e}, ratio {:.2f}".format(i, eh, ep, eh / max(ep, U)))
        assert eh <= 4 * max(ep, U), (i, eh, ep)
