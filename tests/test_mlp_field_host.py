"""The fused MLP field without a GPU: ``MLPField`` as the plain composition on CPU tensors, its constructor's refusals, the plan query
of include/xde_hip_mlp.h and every refusal of its launch by message (nothing is enqueued: the pointers are never dereferenced)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from paddlexde_amd import _hip
from paddlexde_amd.xde import MLPField

P = [0x100000 * (i + 1) for i in range(6)]  # (never dereferenced: every call is refused first)


@pytest.mark.parametrize("time", [False, True], ids=["autonomous", "time"])
@pytest.mark.parametrize("act", ["tanh", None])
def test_the_module_is_the_plain_composition_bit_for_bit(act, time):
    torch.manual_seed(0)
    m = MLPField(3, (7, 5), 2, activation=act, time=time, bias=act is None)
    assert [tuple(l.weight.shape) for l in m.layers] == [(7, 3 + time), (5, 7), (2, 5)] and m.fuse is True
    assert set(m.state_dict()) == {"layers.%d.%s" % (i, n) for i in range(3) for n in (("weight", "bias") if act is None else ("weight",))}
    y = torch.randn(4, 2, 3)
    for t in (0.5, torch.tensor(0.5), torch.full((4, 1, 1), 0.5)):
        h = torch.cat([y, torch.full((4, 2, 1), 0.5)], -1) if time else y
        for i, layer in enumerate(m.layers):
            h = F.linear(torch.tanh(h) if act and i else h, layer.weight, layer.bias)
        assert torch.equal(m(t, y), h) and h.shape == (4, 2, 2)
    assert MLPField(3, 8).widths == (3, 8, 3)


@pytest.mark.parametrize("kwargs, message", [
    (dict(activation="relu"), "'tanh' or None"), (dict(hidden=()), "1 to 3 ints"), (dict(hidden=(4, 4, 4, 4)), "1 to 3 ints"),
    (dict(hidden=0), "must be >= 1"), (dict(in_features=0), "must be >= 1"), (dict(out_features=-1), "must be >= 1")],
    ids=["relu", "no-hidden", "four-hidden", "hidden-0", "in-0", "out-negative"])
def test_the_constructor_refuses(kwargs, message):
    with pytest.raises(ValueError, match=message):
        MLPField(**{**dict(in_features=2, hidden=5), **kwargs})


def test_the_plan_says_what_is_served_and_how():
    be = _hip.get_backend()
    spiral, wide = be._mlp_plan(1000, (2, 50, 2), torch.float32, "tanh"), be._mlp_plan(1000, (4, 256, 256, 4), torch.float32, "tanh", True)
    for p in (spiral, wide):
        assert (p["served"], p["tiles"], p["tile_r"], p["tile_n"], p["pass_n"], p["items"], p["blocks"]) == (1, 1, 32, 32, 128, 32, 32)
        assert p["lds_bytes"] == 64 * 1024 and p["width_cap"] == _hip.XDE_MLP_MAX_WIDTH == 256
    assert (spiral["max_width"], spiral["x_vec"], spiral["out_vec"]) == (50, 0, 0) and (wide["max_width"], wide["x_vec"], wide["out_vec"]) == (256, 1, 1)
    big = be._mlp_plan(65536, (128, 128, 128, 128), torch.float32, "tanh")  # paired: the hidden widths fit twice and the rows fill the chip
    assert (big["tiles"], big["tile_r"], big["items"]) == (2, 64, 1024) and big["lds_bytes"] == 64 * 1024
    assert be._mlp_plan(65536, (128, 129, 128), torch.float32, "tanh")["tiles"] == 1
    assert be._mlp_plan(65536, (2, 50, 256), torch.float32, "tanh")["tiles"] == 2  # (the output's width is never in LDS)
    assert be._mlp_plan(4, (2, 257, 2), torch.float32, "tanh")["served"] == 0
    assert be._mlp_plan(4, (257, 8, 2), torch.float32, None)["served"] == 0 and be._mlp_plan(4, (2, 8, 257), torch.float32, None)["served"] == 0
    assert be._mlp_plan(4, (2, 8, 8, 8, 8, 2), torch.float32, "tanh")["served"] == 0  # 5 layers
    assert be._mlp_plan(4, (2, 8, 2), torch.float64, "tanh")["served"] == 0
    assert be._mlp_plan(4, (2, 8, 2), torch.float32, "relu")["served"] == 0
    assert _hip.mlp_field_plan(4, (2, 8, 2), torch.float32, None)["served"] == 1 and _hip.XDE_MLP_MAX_LAYERS == 4
    with pytest.raises(_hip.XdeError, match="xde_mlp_plan failed.*bad sizes"):
        be._mlp_plan(0, (2, 8, 2), torch.float32, None)
    with pytest.raises(_hip.XdeError, match="xde_mlp_plan failed.*bad sizes"):
        be._mlp_plan(4, (2, 0, 2), torch.float32, None)
    plan, w = _hip.XdeMlpPlan(), (C.c_int32 * 3)(2, 8, 2)
    for args, message in (((4, w, 2, 0, 1, 0, None), "null pointer"), ((4, None, 2, 0, 1, 0, plan), "null pointer"),
                          ((4, w, 2, 2, 1, 0, plan), "bad dtype"), ((4, w, 0, 0, 1, 0, plan), "bad sizes")):
        assert be.lib.xde_mlp_plan(*args) == _hip.XDE_EBADARG
        assert be.lib.xde_last_error().decode().startswith("xde_mlp_plan:") and message in be.lib.xde_last_error().decode()


REFUSALS = [
    (dict(out=None), "null pointer"), (dict(x=None), "null pointer"), (dict(W=None), "null pointer"), (dict(widths=None), "null pointer"),
    (dict(W=(P[2], None)), "null pointer"), (dict(rows=0), "bad sizes"), (dict(n_layers=0), "bad sizes"), (dict(widths=(2, 0, 2)), "bad sizes"),
    (dict(dtype=2), "bad dtype"), (dict(act=2), "unknown act"), (dict(dtype=1), "fp32 only"),
    (dict(widths=(2, 257, 2)), "beyond XDE_MLP_MAX_WIDTH"), (dict(widths=(2, 8, 257)), "beyond XDE_MLP_MAX_WIDTH"),
    (dict(widths=(2, 8, 8, 8, 8, 2), n_layers=5, W=(P[2],) * 5, bias=(None,) * 5), "beyond XDE_MLP_MAX_LAYERS"),
    (dict(out=P[0] + 2), "operand not aligned"), (dict(x=P[1] + 1), "operand not aligned"), (dict(t_rows=P[5] + 2), "operand not aligned"),
    (dict(W=(P[2], P[3] + 1)), "operand not aligned"), (dict(bias=(P[4] + 2, None)), "operand not aligned"),
]


@pytest.mark.parametrize("change, message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_of_the_launch_by_message(change, message):
    lib = _hip.load_library()
    v = dict(out=P[0], x=P[1], t_rows=None, W=(P[2], P[3]), bias=(P[4], None), widths=(2, 8, 2), n_layers=2, rows=3, act=1, dtype=0)
    v.update(change)
    arr = lambda xs, ty: None if xs is None else (ty * len(xs))(*xs)  # noqa: E731
    rc = lib.xde_mlp_field(v["out"], v["x"], v["t_rows"], 0.5, arr(v["W"], C.c_void_p), arr(v["bias"], C.c_void_p), arr(v["widths"], C.c_int32),
                           v["n_layers"], v["rows"], v["act"], 1, v["dtype"], None)
    err = lib.xde_last_error().decode()
    assert rc == _hip.XDE_EBADARG and err.startswith("xde_mlp_field:") and message in err, err
