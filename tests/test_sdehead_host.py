"""The fused last layer of a matrix diffusion without a GPU: the plan query of include/xde_hip_sdehead.h, every refusal of its two
launches by message (nothing is enqueued: the pointers are never dereferenced), ``SDELinearHead`` as a plain diffusion, and the route
``sdeint`` chooses on the numpy double of the general-noise launches."""
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.solver import Euler, Heun
from paddlexde_amd.xde import SDELinearHead

CAP = _hip.XDE_SDEHEAD_MAX_K
P = [0x100000 * (i + 1) for i in range(7)]  # (never dereferenced: every call is refused first)

REFUSALS = [
    (dict(big=None), "null pointer"), (dict(src=None), "null pointer"), (dict(a=None), "null pointer"), (dict(W=None), "null pointer"),
    (dict(rows=0), "need rows, D, M, K >= 1"), (dict(D=0), "need rows, D, M, K >= 1"), (dict(M=-1), "need rows, D, M, K >= 1"),
    (dict(K=0), "need rows, D, M, K >= 1"), (dict(D=(1 << 31) - 255, M=1), "need D * M <= 2^31 - 256"), (dict(k=-1), "k out of range"),
    (dict(k=1 << 32), "k out of range"), (dict(dtype=2), "bad dtype"), (dict(act=2), "unknown act"), (dict(dtype=1), "fp32 only"),
    (dict(K=CAP + 1), "beyond XDE_SDEHEAD_MAX_K"), (dict(big=P[0] + 2), "operand not aligned"), (dict(a=P[3] + 1), "operand not aligned"),
    (dict(bias=P[5] + 2), "operand not aligned"), (dict(other=P[2] + 1), "operand not aligned"),
]


@pytest.mark.parametrize("backward", [False, True], ids=["step", "backward"])
@pytest.mark.parametrize("change, message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_by_message(backward, change, message):
    """``big`` = y1 | s_out, ``src`` = y0 | gy1, ``other`` = f (required) | gf (may be null)."""
    lib = _hip.load_library()
    v = dict(big=P[0], src=P[1], other=P[2], a=P[3], W=P[4], bias=P[5], rows=2, D=3, M=4, K=5, act=1, k=7, dtype=0)
    v.update(change)
    tail = [v[n] for n in ("a", "W", "bias", "rows", "D", "M", "K", "act")] + [0.25, -0.5, 9, v["k"], v["dtype"], None]  # (a negative s is legal)
    if backward:
        rc, who = lib.xde_sdehead_backward(v["big"], v["other"], v["src"], *tail), "xde_sdehead_backward"
    else:
        rc, who = lib.xde_sdehead_step(v["big"], v["src"], v["other"], *tail), "xde_sdehead_step"
        if change == dict(big=None):  # (and f, the operand the backward may leave out)
            assert lib.xde_sdehead_step(P[0], P[1], None, *tail) == _hip.XDE_EBADARG
    err = lib.xde_last_error().decode()
    assert rc == _hip.XDE_EBADARG and err.startswith(who + ":") and message in err, err


def test_the_plan_says_what_is_served_and_how():
    be = _hip.get_backend()
    plan = be._sde_head_plan(16384, 64, 8, 64, torch.float32, "tanh")
    assert plan["served"] == 1 and plan["k_cap"] == CAP and (plan["tiles"], plan["tile_r"], plan["tile_n"], plan["kh"], plan["kq"]) == (2, 64, 32, 32, 8)
    assert plan["items"] == 256 * plan["S"] and plan["S"] * plan["Dc"] >= 64 and plan["lds_w"] == 1 and plan["lds_bytes"] <= 80 * 1024
    for K in (1, 127, 128, 129, CAP):
        assert be._sde_head_plan(40, 16, 4, K, torch.float32, None)["tiles"] == (2 if K <= _hip.XDE_SDEHEAD_PAIR_K else 1)
    few = be._sde_head_plan(1024, 64, 8, 64, torch.float32, "tanh")  # an SDE-GAN batch: 16 row tiles against the chip
    assert few["S"] > 1 and few["Dc"] * few["S"] >= 64 and (few["Dc"] * 8) % 8 == 0 and few["items"] == 16 * few["S"]
    assert be._sde_head_plan(1 << 20, 64, 8, 64, torch.float32, "tanh")["S"] == 1
    assert be._sde_head_plan(4, 2, 200, 8, torch.float32, None)["lds_w"] == 0
    assert be._sde_head_plan(4, 2, 3, CAP + 1, torch.float32, None)["served"] == 0
    assert be._sde_head_plan(4, 2, 3, 8, torch.float64, "tanh")["served"] == 0
    assert be._sde_head_plan(4, 2, 3, 8, torch.float32, "relu")["served"] == 0
    with pytest.raises(_hip.XdeError, match="xde_sdehead_plan failed.*bad sizes"):
        be._sde_head_plan(0, 2, 3, 8, torch.float32, None)
    plan = _hip.XdeSdeHeadPlan()
    for args, message in (((4, 2, 3, 8, 0, 1, None), "null pointer"), ((4, 2, 3, 8, 2, 1, plan), "bad dtype"), ((4, 2, 3, 0, 0, 1, plan), "bad sizes")):
        assert be.lib.xde_sdehead_plan(*args) == _hip.XDE_EBADARG
        assert be.lib.xde_last_error().decode().startswith("xde_sdehead_plan:") and message in be.lib.xde_last_error().decode()


def test_the_module_is_the_plain_composition_and_refuses_other_activations():
    with pytest.raises(ValueError, match="'tanh' or None"):
        SDELinearHead(torch.nn.Identity(), 4, 3, 2, activation="relu")
    with pytest.raises(TypeError, match="trunk must be a module or a callable"):
        SDELinearHead(None, 4, 3, 2)
    with pytest.raises(ValueError, match="must be >= 1"):
        SDELinearHead(lambda t, y: y, 4, 3, 0)
    torch.manual_seed(0)
    lin = torch.nn.Linear(3, 4)
    y = torch.randn(5, 2, 3)
    for act in ("tanh", None):
        m = SDELinearHead(lambda t, y: torch.relu(lin(y)), 4, 3, 2, activation=act, bias=act is None)
        pre = torch.nn.functional.linear(torch.relu(lin(y)), m.head.weight, m.head.bias)
        want = (torch.tanh(pre) if act else pre).reshape(5, 2, 3, 2)
        assert m.head.weight.shape == (6, 4) and torch.equal(m(0.0, y), want)


@pytest.mark.parametrize("case", ["hidden beyond the cap", "float64", "fuse = False", "Heun"])
def test_what_the_kernel_does_not_serve_takes_the_general_noise_launches(case):
    """On the numpy double, which has no fused launch: the solve goes through sde_gn_* launches only, one step each."""
    from ._gn_double import GnDoubleBackend

    K = CAP + 1 if case == "hidden beyond the cap" else 4
    dtype = torch.float64 if case == "float64" else torch.float32
    lin = torch.nn.Linear(3, K).to(dtype)
    head = SDELinearHead(lambda t, y: torch.tanh(lin(y)), K, 3, 2).to(dtype)
    if case == "fuse = False":
        head.fuse = False
    _hip._set_backend_for_testing(GnDoubleBackend())
    try:
        be = _hip.get_backend()
        args = (lambda t, y: -y, head, torch.ones(2, 1, 3, dtype=dtype), torch.linspace(0.0, 1.0, 4))
        options = {"noise_type": "general", "seed": 3, "norm": None}
        if case == "Heun":  # (this double has Euler's general-noise launches only: Heun is seen asking for its own, with the matrix formed)
            with torch.no_grad(), pytest.raises(AttributeError, match="_sde_gn_heun_predict"):
                sdeint(*args, Heun, options=options)
            return
        with torch.no_grad():
            ys = sdeint(*args, Euler, options=options)
        assert ys.shape == (2, 4, 3) and bool(torch.isfinite(ys).all())
        assert len(be.launches) >= 3 and all(name.startswith("sde_gn_") for name in be.launches), be.launches
    finally:
        _hip._set_backend_for_testing(None)
