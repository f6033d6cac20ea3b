"""The fused MLP field's vector-Jacobian product without a GPU: its plan (include/xde_hip_mlp.h), every refusal of its launch by message
(nothing is enqueued: the pointers are never dereferenced), and ``MLPField.vjp`` on CPU tensors as torch's own gradients."""
import ctypes as C

import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.xde import MLPField

P = [0x100000 * (i + 1) for i in range(12)]  # (never dereferenced: every call is refused first)


def test_the_plan_says_what_is_served_and_what_it_takes():
    be = _hip.get_backend()
    spiral = be._mlp_vjp_plan(1000, (2, 50, 2), torch.float32, "tanh")
    assert (spiral["served"], spiral["tile_r"], spiral["pitch"], spiral["items"], spiral["blocks"]) == (1, 32, 32, 32, 32)
    assert (spiral["sum_widths"], spiral["lds_bytes"], spiral["lds_cap"], spiral["gx_vec"]) == (54, 54 * 128, _hip.XDE_MLP_VJP_LDS_BYTES, 0)
    assert spiral["params"] == 50 * (2 + 1) + 2 * (50 + 1) and be._mlp_vjp_plan(9, (2, 50, 2), torch.float32, "tanh", True)["params"] == 50 * 4 + 2 * 51
    big = be._mlp_vjp_plan(65536, (128, 128, 128, 128), torch.float32, "tanh")  # fills the LDS exactly; more items than the grid cap
    assert (big["served"], big["lds_bytes"], big["items"], big["blocks"], big["gx_vec"]) == (1, 65536, 2048, _hip.XDE_MLP_VJP_MAX_BLOCKS, 1)
    for rows, max_blocks, blocks in ((100, 0, 4), (100, 1, 1), (100, 3, 3), (100, 9, 4), (65536, 300, 256)):
        p = be._mlp_vjp_plan(rows, (3, 7, 5, 2), torch.float32, None, False, max_blocks)
        assert p["blocks"] == blocks and p["workspace_bytes"] == blocks * p["params"] * 4 and p["params"] == 7 * 4 + 5 * 8 + 2 * 6
    unserved = [((2, 8, 2), torch.float64, "tanh"), ((2, 8, 8, 8, 8, 2), torch.float32, "tanh"), ((2, 257, 2), torch.float32, "tanh"),
                ((128, 129, 128, 128), torch.float32, "tanh"), ((2, 8, 2), torch.float32, "relu")]
    assert [_hip.mlp_vjp_plan(4, w, dt, act)["served"] for w, dt, act in unserved] == [0] * 5
    assert _hip.mlp_vjp_plan(4, (128, 129, 128, 128), torch.float32, "tanh")["lds_bytes"] == 513 * 128
    for args, message in (((0, (2, 8, 2), torch.float32, None), "bad sizes"), ((4, (2, 0, 2), torch.float32, None), "bad sizes"),
                          ((4, (2, 8, 2), torch.float32, None, False, -1), "bad max_blocks")):
        with pytest.raises(_hip.XdeError, match="xde_mlp_vjp_plan failed.*" + message):
            be._mlp_vjp_plan(*args)
    assert be.lib.xde_mlp_vjp_plan(4, (C.c_int32 * 3)(2, 8, 2), 2, 0, 1, 0, 0, None) == _hip.XDE_EBADARG
    assert be.lib.xde_last_error().decode() == "xde_mlp_vjp_plan: null pointer"


REFUSALS = [
    (dict(f=None), "null pointer"), (dict(gx=None), "null pointer"), (dict(gW=None), "null pointer"), (dict(x=None), "null pointer"),
    (dict(a=None), "null pointer"), (dict(W=None), "null pointer"), (dict(widths=None), "null pointer"), (dict(workspace=None), "null pointer"),
    (dict(gt=None), "null pointer"), (dict(W=(P[2], None)), "null pointer"), (dict(gW=(None, P[7])), "null pointer"),
    (dict(rows=0), "bad sizes"), (dict(n_layers=0), "bad sizes"), (dict(widths=(2, 0, 2)), "bad sizes"), (dict(dtype=2), "bad dtype"),
    (dict(max_blocks=-1), "bad max_blocks"), (dict(act=2), "unknown act"), (dict(dtype=1), "fp32 only"),
    (dict(widths=(2, 8, 8, 8, 8, 2), n_layers=5, W=(P[2],) * 5, gW=(P[6],) * 5), "beyond XDE_MLP_MAX_LAYERS"),
    (dict(widths=(2, 257, 2)), "beyond XDE_MLP_MAX_WIDTH"), (dict(widths=(256, 256, 2)), "beyond the LDS bound of 512"),
    (dict(workspace_bytes=4 * (8 * 4 + 2 * 9) - 1), "workspace too small"), (dict(f=P[0] + 2), "operand not aligned"),
    (dict(gt=P[10] + 1), "operand not aligned"), (dict(a=P[11] + 2), "operand not aligned"), (dict(workspace=P[9] + 2), "operand not aligned"),
    (dict(gW=(P[6], P[7] + 1)), "operand not aligned"), (dict(gb=(P[8] + 2, None)), "operand not aligned"),
]


@pytest.mark.parametrize("change, message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_of_the_launch_by_message(change, message):
    lib = _hip.load_library()
    v = dict(f=P[0], gx=P[1], gW=(P[6], P[7]), gb=(P[8], None), gt=P[10], x=P[5], a=P[11], W=(P[2], P[3]), bias=(P[4], None), widths=(2, 8, 2),
             n_layers=2, rows=3, act=1, dtype=0, workspace=P[9], workspace_bytes=4 * (8 * 4 + 2 * 9), max_blocks=0)
    v.update(change)
    arr = lambda xs, ty: None if xs is None else (ty * len(xs))(*xs)  # noqa: E731
    rc = lib.xde_mlp_field_vjp(v["f"], v["gx"], arr(v["gW"], C.c_void_p), arr(v["gb"], C.c_void_p), v["gt"], v["x"], v["a"], None, 0.5,
                               arr(v["W"], C.c_void_p), arr(v["bias"], C.c_void_p), arr(v["widths"], C.c_int32), v["n_layers"], v["rows"],
                               v["act"], 1, v["dtype"], v["workspace"], v["workspace_bytes"], v["max_blocks"], None)
    err = lib.xde_last_error().decode()
    assert rc == _hip.XDE_EBADARG and err.startswith("xde_mlp_field_vjp:") and message in err, err


@pytest.mark.parametrize("time", [False, True], ids=["autonomous", "time"])
@pytest.mark.parametrize("act", ["tanh", None])
def test_on_cpu_tensors_the_vjp_is_autograd_of_the_plain_composition_bit_for_bit(act, time):
    torch.manual_seed(0)
    m = MLPField(3, (7, 5), 3, activation=act, time=time, bias=act is None)
    y, a, t = torch.randn(4, 2, 3), torch.randn(4, 2, 3), torch.tensor(0.5, requires_grad=True)
    f = m(t, y.requires_grad_(True))
    want = torch.autograd.grad(f, ([t] if time else []) + [y] + list(m.parameters()), a)
    got = m.vjp(0.5, y.detach(), a)
    assert len(got) == 3 + len(list(m.parameters())) and torch.equal(got[0], f) and not got[0].requires_grad
    assert (got[1] is None) if not time else (got[1].shape == () and torch.equal(got[1], want[0]))
    assert all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got[2:], want[int(time):]))
