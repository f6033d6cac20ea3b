"""The fused MLP field (include/xde_hip_mlp.h) on the device, one table of shapes: against float64 numpy on the same float32 operands
within 4 times the plain torch composition's own error (both are fp32 sums of equal length in different orders; the sums over k run
on the matrix cores, whose in-instruction order no host program can restate), determinism, and — on small integer operands with the
identity, where every sum is exact in any order — the header's statement bit for bit.  Then row independence, misaligned operands,
and the launch count and results of solves through ``odeint``."""
import copy

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import odeint
from paddlexde_amd.solver import RK4, Dopri5
from paddlexde_amd.xde import MLPField

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# rows, widths, act, bias, time (None, "scalar" or "rows")
TABLE = [
    (1, (2, 50, 2), "tanh", True, None),                  # the spiral demo's field on one row: two of the four waves have a chunk
    (31, (3, 20, 20, 3), "tanh", True, "scalar"),         # the latent ODE's depth; odd input: x and W_0 by element, W_1 by vector
    (33, (4, 33, 1), "tanh", False, None),                # a 33rd row; x by vector; a 33rd neuron; no bias; one output
    (65, (5, 1, 256, 4), None, True, "rows"),             # three tiles; a hidden layer of one; every wave two chunks; out by vector
    (65, (4, 256, 256, 50, 8), "tanh", True, "rows"),     # three hidden layers, k at the cap, the time column beside vector x
    (33, (4, 20, 5), None, True, "scalar"),               # the identity between layers
    (64 * 2048 + 1, (2, 5, 2), "tanh", True, None),       # paired tiles, 2049 items on 2048 workgroups: a second item of one row
    (32 * 2048 + 1, (2, 129, 1), "tanh", True, "scalar"),  # the same with single tiles (a hidden width beyond the pair width)
]
IDS = ["-".join(str(x) for x in (r[0],) + r[1] + r[2:]) for r in TABLE]
ALIGNED = (33, (4, 20, 8), "tanh", True, None)  # every width % 4 == 0: only the pointers send x, W and out to the element path


def make(row, integers=False, seed=0):
    """The module on the device and (y, t) of the row; ``integers``: small-integer inputs, times and sparse weights in {-1, 0, 1}."""
    rows, widths, act, bias, time = row
    g = torch.Generator().manual_seed(seed)
    m = MLPField(widths[0], widths[1:-1], widths[-1], activation=None if integers else act, time=time is not None, bias=bias)
    y = torch.randn(rows, widths[0], generator=g)
    t = torch.rand(rows, 1, generator=g) if time == "rows" else 0.75
    if integers:
        y, t = torch.randint(-2, 3, y.shape, generator=g).float(), (torch.randint(-2, 3, t.shape, generator=g).float() if time == "rows" else 3.0)
        for layer in m.layers:
            for p in layer.parameters():  # (about 8 weights of a row are not zero: the condition below holds through four layers)
                keep = torch.rand(p.shape, generator=g) < 8.0 / max(p.shape[-1], 8)
                p.data = torch.randint(-1, 2, p.shape, generator=g).float() * keep
    return m.to(DEV), y.to(DEV), (t.to(DEV) if torch.is_tensor(t) else t)


def reference(m, t, y):
    """float64 numpy from the float32 operand bits, and the largest magnitude any exact partial sum can reach."""
    h, mag = y.cpu().double().numpy(), y.cpu().abs().double().numpy()
    tcol = t.cpu().double().numpy().reshape(-1, 1) if torch.is_tensor(t) else np.full((h.shape[0], 1), float(t))
    worst = 0.0
    for i, layer in enumerate(m.layers):
        W = layer.weight.detach().cpu().double().numpy()
        b = 0.0 if layer.bias is None else layer.bias.detach().cpu().double().numpy()
        if i:
            h = np.tanh(h) if m.activation == "tanh" else h
        K = h.shape[1]
        pre, mag = h @ W[:, :K].T + b, mag @ np.abs(W[:, :K]).T + np.abs(b)
        if W.shape[1] > K:
            pre, mag = pre + tcol * W[:, K], mag + np.abs(tcol) * np.abs(W[:, K])
        h, worst = pre, max(worst, float(mag.max()))
    return h, worst


def fused_and_plain(m, t, y):
    with torch.no_grad():
        m.fuse = True
        fused = m(t, y)
        m.fuse = False
        plain = m(t, y)
        m.fuse = True
    return fused, plain


def off16(x):
    """``x``'s elements in a contiguous tensor that starts one element past a 16-byte boundary."""
    view = torch.empty(x.numel() + 4, dtype=x.dtype, device=x.device)[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def test_the_table_meets_every_plan():
    plans = [_hip.mlp_field_plan(r[0], r[1], torch.float32, r[2], r[4] is not None) for r in TABLE]
    assert all(p["served"] for p in plans) and {p["tiles"] for p in plans} == {1, 2}
    assert {p["x_vec"] for p in plans} == {0, 1} and {p["out_vec"] for p in plans} == {0, 1}
    assert {p["tiles"] for p in plans if p["items"] > p["blocks"]} == {1, 2} and any(p["items"] == 1 for p in plans)
    assert any(p["max_width"] == p["width_cap"] for p in plans) and any(1 < p["items"] <= p["blocks"] for p in plans)
    assert {len(r[1]) - 1 for r in TABLE} == {2, 3, 4} and {r[4] for r in TABLE} == {None, "scalar", "rows"}


@pytest.mark.parametrize("row", TABLE, ids=IDS)
def test_the_launch_is_within_the_plain_composition_s_error_of_float64_and_deterministic(row):
    m, y, t = make(row)
    (fused, plain), (want, _) = fused_and_plain(m, t, y), reference(m, t, y)
    assert fused.shape == plain.shape == want.shape and fused.dtype == torch.float32
    scale = np.abs(want).max()
    ef, ep = (float(np.abs(x.cpu().double().numpy() - want).max() / scale) for x in (fused, plain))
    print("{}: fused {:.3e}, plain {:.3e}, ratio {:.2f}".format(row, ef, ep, ef / max(ep, 1e-300)))
    assert ef <= 4 * max(ep, U)
    assert torch.equal(fused, fused_and_plain(m, t, y)[0])


@pytest.mark.parametrize("row", TABLE, ids=IDS)
def test_integer_operands_give_the_header_s_statement_bit_for_bit(row):
    m, y, t = make(row, integers=True)
    want, worst = reference(m, t, y)
    assert worst < 2.0 ** 24  # every product and partial sum is an integer float32 holds: exact in any order
    fused, plain = fused_and_plain(m, t, y)
    assert np.array_equal(fused.cpu().numpy(), want.astype(np.float32)) and np.abs(want).max() > 0


def test_a_row_does_not_depend_on_its_batch():
    m, y, t = make(TABLE[4])
    batch = fused_and_plain(m, t, y)[0]
    for r in (0, 31, 32, 64):
        assert torch.equal(batch[r:r + 1], fused_and_plain(m, t[r:r + 1], y[r:r + 1])[0]), r


def test_operands_one_element_off_16_bytes_give_the_aligned_launch_s_bits():
    plan = _hip.mlp_field_plan(ALIGNED[0], ALIGNED[1], torch.float32, "tanh")
    assert plan["x_vec"] == 1 and plan["out_vec"] == 1
    m, y, _ = make(ALIGNED)
    want = fused_and_plain(m, 0.0, y)[0]
    out = off16(torch.zeros_like(want))
    weights, biases = [off16(layer.weight.detach()) for layer in m.layers], [off16(layer.bias.detach()) for layer in m.layers]
    _hip.get_backend()._mlp_field(out, off16(y), None, 0.0, weights, biases, "tanh", False)
    assert torch.equal(out, want)


@pytest.mark.parametrize("solver", [RK4, Dopri5], ids=["rk4", "dopri5"])
def test_odeint_evaluates_the_field_in_one_launch_each(solver):
    """Under no_grad every evaluation of the field is one ``_mlp_field`` call, and the solve is as near a float64 solve of the same
    scheme as the plain route's is (the margin of the table's test); with grad on and a parameter that requires grad there is no such
    call and the gradients are the plain route's bits."""
    torch.manual_seed(3)
    m = MLPField(2, 50).to(DEV)
    fixed = solver is RK4
    y0 = torch.randn((20, 1, 2) if fixed else (20, 2), device=DEV)
    t = torch.linspace(0.0, 1.0, 6, device=DEV)
    kw = {} if fixed else dict(rtol=1e-5, atol=1e-7)
    be = _hip.get_backend()
    calls, evals, launch = [], [], be._mlp_field
    hook = m.register_forward_hook(lambda *a: evals.append(1))
    try:
        be._mlp_field = lambda *a: (calls.append(1), launch(*a))[1]
        with torch.no_grad():
            fused = odeint(m, y0, t, solver=solver, **kw)
            assert len(calls) == len(evals) > 0 and bool(torch.isfinite(fused).all())
            m.fuse = False
            plain = odeint(m, y0, t, solver=solver, **kw)
            assert len(calls) * 2 == len(evals)
            m.fuse = True
            ref = odeint(copy.deepcopy(m).double(), y0.double(), t.double(), solver=solver, **kw)
        scale = float(ref.abs().max())
        ef, ep = (float((x.double() - ref).abs().max()) / scale for x in (fused, plain))
        print("{}: fused {:.3e}, plain {:.3e}, ratio {:.2f}".format(solver.__name__, ef, ep, ef / max(ep, 1e-300)))
        assert ef <= 4 * max(ep, U)
        if fixed:
            del calls[:]
            grads = []
            for fuse in (True, False):
                m.fuse = fuse
                m.zero_grad()
                odeint(m, y0, t, solver=solver).square().sum().backward()
                grads.append([p.grad.clone() for p in m.parameters()])
            assert calls == [] and all(torch.equal(a, b) for a, b in zip(*grads)) and all(bool(g.abs().sum() > 0) for g in grads[0])
    finally:
        hook.remove()
        del be._mlp_field
