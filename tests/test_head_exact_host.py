"""The float32 statements of the two fused heads (tests/_head_exact.py) and the branch names of their plans (tests/_head_plans.py)
without a GPU: on integer operands the statements are the float64 composition exactly, they do tell one summation order from another,
and the shapes the GPU modules launch at the default settings reach every branch their coverage tests require (the plans are host
arithmetic, so a retune that moves a shape off its branch is named here too)."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _head_exact as E
from . import _head_plans as P

# rows, D (H), M (C), K
SHAPES = [(1, 1, 1, 1), (5, 3, 1, 4), (65, 3, 3, 5), (7, 2, 130, 12), (9, 4, 5, 33), (6, 2, 7, 136), (3, 2, 3, 256)]


def _reals(seed, *shapes):
    rs = np.random.RandomState(seed)
    return [rs.randn(*shape).astype(np.float32) for shape in shapes]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
@pytest.mark.parametrize("bias", [False, True], ids=["no-bias", "bias"])
def test_the_statements_are_the_float64_composition_on_integer_operands(shape, bias):
    rows, D, M, K = shape
    a, W, b = E.integer_operands(rows, D * M, K, bias)
    assert E.integer_condition(a, W, b) < 2.0 ** 24
    pre = E.pre_activations(a, W, b)
    assert np.array_equal(pre.astype(np.float64), a.astype(np.float64) @ W.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64)))
    w, y0, f, gy = _reals(sum(shape), (rows, M), (rows, D), (rows, D), (rows, D))
    assert np.array_equal(E.sde_forward(a, W, b, w, y0, f, 0.0625), E.sde_forward_float64(a, W, b, w, y0, f, 0.0625))
    assert np.array_equal(E.cde_forward(a, W, b, w), E.cde_forward_float64(a, W, b, w))
    s, gf = E.sde_backward(w, gy, 0.3)
    assert s.shape == (rows, D * M) and s.dtype == gf.dtype == np.float32
    assert np.array_equal(s.reshape(rows, D, M), (gy.astype(np.float64)[:, :, None] * w.astype(np.float64)[:, None, :]).astype(np.float32))
    assert np.array_equal(gf, (gy.astype(np.float64) * float(np.float32(0.3))).astype(np.float32))
    assert np.array_equal(E.cde_backward(w, gy), s)


def test_the_condition_refuses_what_is_not_an_integer_and_grows_with_the_operands():
    a, W, b = E.integer_operands(4, 6, 9, True)
    assert E.integer_condition(a, W, b) <= 9 * 9 + 3
    assert E.integer_condition(a * 1000, W * 1000, b) >= 2.0 ** 24 or float(np.abs(a).max()) == 0.0
    with pytest.raises(AssertionError, match="integer operands only"):
        E.integer_condition(a + np.float32(0.5), W, b)


def test_the_statements_tell_one_order_from_another():
    """What the bit-for-bit tests rely on: with real increments, the run of m summed descending, or started from +0 on the far side,
    gives other bits somewhere."""
    rows, D, M, K = 64, 4, 7, 12
    a, W, b = E.integer_operands(rows, D * M, K, True)
    w, y0, f = _reals(3, (rows, M), (rows, D), (rows, D))
    y1 = E.sde_forward(a, W, b, w, y0, f, 0.0625)
    flipped = E.sde_forward(a, W.reshape(D, M, K)[:, ::-1].reshape(D * M, K).copy(), b.reshape(D, M)[:, ::-1].reshape(-1).copy(),
                            w[:, ::-1].copy(), y0, f, 0.0625)
    assert not np.array_equal(y1, flipped) and np.allclose(y1, flipped, rtol=1e-4, atol=1e-4)
    p = E.pre_activations(a, W, b).reshape(rows, D, M) * w[:, None, :]
    other = y0 + (f * np.float32(0.0625) + E._ascending_sum(p, None))
    assert not np.array_equal(y1, other)


def test_the_gpu_modules_shapes_reach_every_reachable_branch():
    from . import test_gpu_cdehead as Tc
    from . import test_gpu_sdehead as Ts

    be = _hip.get_backend()
    for backward in (False, True):
        seen = set()
        for rows, D, M, K in [row[:4] for row in Ts.TABLE]:
            seen |= P.sde_features(_hip.sde_head_plan(rows, D, M, K, torch.float32, None), rows, D, M, K, backward)
        for shape, extra in ((Ts.MISALIGNED, dict(misalign=True)), (Ts.GF_NULL, dict(gf_null=True))):
            seen |= P.sde_features(_hip.sde_head_plan(*shape, torch.float32, None), *shape, backward, **extra)
        assert P.gaps(P.sde_required(backward), seen) == [], backward
        seen = set()
        for shape, mis in [(row[:4], False) for row in Tc.TABLE] + [(Tc.MISALIGNED[:4], True)]:
            seen |= P.cde_features(be._cde_head_plan(*shape, torch.float32, None), *shape, backward, mis)
        assert P.gaps(P.cde_required(backward), seen) == [], backward


def test_the_branch_names_of_a_few_plans():
    plan = lambda *shape: _hip.sde_head_plan(*shape, torch.float32, None)  # noqa: E731
    f = P.sde_features(plan(70, 2, 50, 12), 70, 2, 50, 12, True)
    assert {"inst:2x2", "no-lds", "no-lds-second-tile", "sliced", "sliced-two-tiles", "s-vec", "s-scalar-by-slice", "a:vec"} <= f
    assert "kq-short:2" not in f and "gf-null" not in f and "second-item" not in f
    f = P.sde_features(plan(33, 3, 3, 20), 33, 3, 3, 20, False, misalign=True)
    assert {"inst:8x2", "kq-short:8", "early-exit:8", "a:scalar-by-pointer", "W:scalar-by-pointer", "lds"} <= f and not f & P._S_STORES
    assert "early-exit:8" not in P.sde_features(plan(33, 5, 8, 33), 33, 5, 8, 33, False)
    f = P.sde_features(plan(64 * 4096 + 65, 2, 3, 5), 64 * 4096 + 65, 2, 3, 5, True, gf_null=True)
    assert {"second-item", "third-item", "second-item:lds", "absent-second-tile", "gf-null", "s-scalar-by-size"} <= f
    assert "second-item-sliced" not in f and "second-item:one-tile" not in f
