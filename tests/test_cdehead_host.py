"""The fused last layer of a CDE field without a GPU: every refusal of include/xde_hip_cdehead.h's entry points by message, the plan's
``served`` flag, ``CDELinearHead`` as a plain ``func``, and the route ``CDEField`` chooses.  No launch happens here."""
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.xde import CDEField, CDELinearHead
from paddlexde_amd.xde.base_cde import CdeContractFn, CdeControlContractFn

CAP = _hip.XDE_CDEHEAD_MAX_K
P = [0x100000 * (i + 1) for i in range(9)]  # (never dereferenced: every call is refused first)

REFUSALS = [
    (dict(a=None), "null pointer"), (dict(W=None), "null pointer"), (dict(series=None), "null pointer"), (dict(knots=None), "null pointer"),
    (dict(big=None), "null pointer"),
    (dict(B=0), "need B, H, C, K >= 1"), (dict(H=0), "need B, H, C, K >= 1"), (dict(C=-1), "need B, H, C, K >= 1"), (dict(K=0), "need B, H, C, K >= 1"),
    (dict(H=(1 << 31) - 255, C=1), "need H * C <= 2^31 - 256"), (dict(Tn=1), "need Tn >= 2"), (dict(dtype=2), "bad dtype"),
    (dict(time_dtype=2), "bad time_dtype"), (dict(method=2), "XDE_HISTORY_BEZIER is not a control path"), (dict(method=3), "unknown method"),
    (dict(method=9), "unknown method"), (dict(act=2), "unknown act"), (dict(dtype=1), "fp32 only"), (dict(K=CAP + 1), "beyond XDE_CDEHEAD_MAX_K"),
    (dict(a=P[1] + 2), "operand not aligned"), (dict(bias=P[3] + 1), "operand not aligned"), (dict(coef=P[5] + 2), "operand not aligned"),
    (dict(t_dev=P[7] + 4, time_dtype=1), "t_dev not aligned"),
]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("change, message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_by_message(backward, change, message):
    lib = _hip.load_library()
    v = dict(big=P[0], a=P[1], W=P[2], bias=P[3], series=P[4], coef=None, knots=P[6], t_dev=None, t_host=0.5, time_dtype=1, B=2, H=3, C=4, K=5,
             Tn=6, method=1, act=1, dtype=0)
    v.update(change)
    tail = [v[k] for k in ("a", "W", "bias", "series", "coef", "knots", "t_dev", "t_host", "time_dtype", "B", "H", "C", "K", "Tn", "method",
                           "act", "dtype")] + [None]
    if backward:
        if change == dict(big=None):  # (and gout, the operand the forward has not)
            assert lib.xde_cdehead_backward(P[0], None, *tail) == _hip.XDE_EBADARG
            assert lib.xde_last_error().decode() == "xde_cdehead_backward: null pointer"
        rc, who = lib.xde_cdehead_backward(v["big"], P[8], *tail), "xde_cdehead_backward"
    else:
        rc, who = lib.xde_cdehead_forward(v["big"], *tail), "xde_cdehead_forward"
    err = lib.xde_last_error().decode()
    assert rc == _hip.XDE_EBADARG and err.startswith(who + ":") and message in err, err


def test_the_plan_says_what_is_served():
    be = _hip.get_backend()
    plan = be._cde_head_plan(8192, 64, 32, 128, torch.float32, "tanh")
    assert plan["served"] == 1 and plan["k_cap"] == CAP and (plan["tile_b"], plan["tile_n"], plan["kh"], plan["kq"]) == (32, 32, 64, 16)
    assert plan["items"] == 256 * plan["S"] and plan["S"] * plan["Hc"] >= 64 and plan["lds_bytes"] <= 64 * 1024
    assert be._cde_head_plan(4, 2, 3, CAP, torch.float32, None)["served"] == 1
    assert be._cde_head_plan(4, 2, 3, CAP + 1, torch.float32, None)["served"] == 0
    assert be._cde_head_plan(4, 2, 3, 8, torch.float64, "tanh")["served"] == 0
    assert be._cde_head_plan(4, 2, 3, 8, torch.float32, "relu")["served"] == 0
    with pytest.raises(_hip.XdeError, match="xde_cdehead_plan: bad sizes"):
        be._cde_head_plan(0, 2, 3, 8, torch.float32, None)
    plan = _hip.XdeCdeHeadPlan()
    for args, message in (((4, 2, 3, 8, 0, 1, None), "null pointer"), ((4, 2, 3, 8, 2, 1, plan), "bad dtype"), ((4, 2, 3, 0, 0, 1, plan), "bad sizes"),
                          ((4, 0, 3, 8, 0, 1, plan), "bad sizes"), ((4, 2, -1, 8, 0, 1, plan), "bad sizes")):
        assert be.lib.xde_cdehead_plan(*args) == _hip.XDE_EBADARG
        assert be.lib.xde_last_error().decode().startswith("xde_cdehead_plan:") and message in be.lib.xde_last_error().decode()


def test_the_module_is_the_plain_composition_and_refuses_other_activations():
    with pytest.raises(ValueError, match="'tanh' or None"):
        CDELinearHead(torch.nn.Identity(), 4, 3, 2, activation="relu")
    with pytest.raises(TypeError, match="trunk must be a module or a callable"):
        CDELinearHead(None, 4, 3, 2)
    with pytest.raises(ValueError, match="must be >= 1"):
        CDELinearHead(lambda t, z: z, 4, 0, 2)
    torch.manual_seed(0)
    lin = torch.nn.Linear(3, 4)
    z = torch.randn(5, 2, 3)
    for act in ("tanh", None):
        m = CDELinearHead(lambda t, z: torch.relu(lin(z)), 4, 3, 2, activation=act, bias=act is None)
        pre = torch.nn.functional.linear(torch.relu(lin(z)), m.head.weight, m.head.bias)
        want = (torch.tanh(pre) if act else pre).reshape(5, 2, 3, 2)
        assert m.head.weight.shape == (6, 4) and torch.equal(m(0.0, z), want)


class _Control:
    """What CDEField reads of a control, without the launches that build one."""

    def __new__(cls, kind, series, differentiable=False):
        X = object.__new__(kind)
        X._series, X._t, X.differentiable = series, torch.arange(float(series.shape[-2])), differentiable
        return X


def test_the_field_fuses_only_what_the_kernel_serves():
    from paddlexde_amd.interpolation import CubicHermiteSpline

    head = CDELinearHead(lambda t, z: z, 3, 3, 2)
    series = torch.zeros(4, 5, 2)
    field = CDEField(head, _Control(CubicHermiteSpline, series))
    assert field._contract is CdeContractFn and field._fused_head(torch.zeros(4, 3)) is True
    assert field._fused_head(torch.zeros(4, 3, dtype=torch.float64)) is False
    assert CDEField(head, _Control(CubicHermiteSpline, series, differentiable=True))._contract is CdeControlContractFn
    assert CDEField(head, _Control(CubicHermiteSpline, series, differentiable=True))._fused_head(torch.zeros(4, 3)) is False
    assert CDEField(CDELinearHead(lambda t, z: z, CAP + 1, 3, 2), _Control(CubicHermiteSpline, series))._fused_head(torch.zeros(4, 3)) is False
    assert CDEField(lambda t, z: z, _Control(CubicHermiteSpline, series))._fused_head(torch.zeros(4, 3)) is False
    head.fuse = False
    assert field._fused_head(torch.zeros(4, 3)) is False
