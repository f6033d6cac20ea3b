"""sdeint's reversible Heun steps and sdeint_adjoint without a GPU: the end-to-end cases of tests/_rheun_cases.py on the numpy double,
the launches of the forward and of the sweep, the double against tests/_rheun_oracle.py, and the C ABI of the new entry points of
include/xde_hip_sde.h (every call below is refused on the host before anything is enqueued, or has nothing to do)."""
import functools
import os

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip

from . import _rheun_oracle as RO
from . import _sde_oracle as SO
from ._rheun_cases import *  # noqa: F401,F403
from ._rheun_cases import REVERSE_BAR, _opts, _y0, diffusion, drift, sdeint, sdeint_adjoint, ReversibleHeun
from .test_srk_host import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHEUN_SYMBOLS = ("xde_sde_rheun_predict", "xde_sde_rheun_correct", "xde_sde_rheun_adjoint_stage", "xde_sde_rheun_adjoint_step")


@pytest.fixture
def dev(monkeypatch):
    from ._rheun_double import RheunDoubleBackend

    # (the draws of (seed, k) are the same arrays for every walk of a test: drawn once; the arrays are dropped with the fixture)
    monkeypatch.setattr(SO, "state_normals", functools.lru_cache(maxsize=512)(SO.state_normals))
    _hip._set_backend_for_testing(RheunDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def test_launches_of_the_forward_and_of_the_sweep(dev):
    """A forward step is predict and correct, with gradients or without; back-propagating through the steps is the EM backward twice per
    step (correct's, at half dt and s, then predict's); the adjoint's sweep is stage, step, predict, correct per step, and nothing else
    of the library's on the plain plan."""
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    n_steps = len(t) - 1
    fwd = ["sde_rheun_predict", "sde_rheun_correct"]
    with torch.no_grad():
        sdeint(drift, diffusion, y0, t, solver=ReversibleHeun, options=_opts(seed=1))
    assert be.launches == fwd * n_steps
    del be.launches[:]
    mu = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    g = lambda t_, y: y * mu  # noqa: E731
    sol = sdeint(drift, g, y0.clone().requires_grad_(True), t, solver=ReversibleHeun, options=_opts(seed=1))
    assert be.launches == fwd * n_steps
    del be.launches[:]
    sol.sum().backward()
    assert be.launches == ["sde_em_backward"] * (2 * n_steps)
    del be.launches[:]
    sol = sdeint_adjoint(drift, g, y0.clone().requires_grad_(True), t, solver=ReversibleHeun, options=_opts(seed=1), adjoint_params=(mu,))
    assert be.launches == fwd * n_steps
    del be.launches[:]
    sol.sum().backward()
    assert be.launches == ["sde_rheun_adjoint_stage", "sde_rheun_adjoint_step", "sde_rheun_predict", "sde_rheun_correct"] * n_steps


def test_the_double_states_the_kernels_op_order(dev):
    """The double's four methods against tests/_rheun_oracle.py on one step, both dtypes, both directions, dt < 0 and dt = 0, the null
    cotangents of the first backward step (the GPU test holds the kernels to the same statement)."""
    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        gen = torch.Generator().manual_seed(1)
        y0, yh0, f0, f1, g0, g1, ay, ayh, af, ag, v = ops = [torch.randn(3, 7, generator=gen, dtype=dtype) for _ in range(11)]
        Y, YH, F0, F1, G0, G1, AY, AYH, AF, AG, V = (x.numpy() for x in ops)
        for dt in (T(-0.0123), T(0.0)):
            s = float(SO.s_of(dt, T))
            z = SO.state_normals((3, 7), 5, 17, T)
            for d in (1, -1):
                out = torch.empty_like(y0)
                be._sde_rheun_predict(out, y0, yh0, f0, g0, float(dt), s, d, 5, 17)
                assert np.array_equal(out.numpy(), RO.predict(Y, YH, F0, G0, dt, z, T, d))
                if dt == 0:
                    assert np.array_equal(out.numpy(), (Y + Y) - YH)
                be._sde_rheun_correct(out, y0, f0, f1, g0, g1, float(dt), s, d, 5, 17)
                assert np.array_equal(out.numpy(), RO.correct(Y, F0, F1, G0, G1, dt, z, T, d))
                if dt == 0:
                    assert np.array_equal(out.numpy(), Y)
            bf, bg = torch.empty_like(y0), torch.empty_like(y0)
            for a, b, A, B in ((af, ag, AF, AG), (None, None, None, None)):
                be._sde_rheun_adjoint_stage(bf, bg, a, b, ay, float(dt), s, 5, 17)
                for got, want in zip((bf, bg), RO.adjoint_stage(A, B, AY, dt, z, T)):
                    assert np.array_equal(got.numpy(), want)
            outs = [torch.empty_like(y0) for _ in range(4)]
            for h, H in ((ayh, AYH), (None, None)):
                be._sde_rheun_adjoint_step(*outs, ay, h, v, float(dt), s, 5, 17)
                for got, want in zip(outs, RO.adjoint_step(AY, H, V, dt, z, T)):
                    assert np.array_equal(got.numpy(), want)
            if dt == 0:
                assert not outs[2].numpy().any() and not outs[3].numpy().any() and np.array_equal(outs[0].numpy(), AY + (V + V))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reverse_after_forward_returns_the_state(dev, dtype):
    from ._rheun_cases import reverse_after_forward

    reverse_after_forward(dev, dtype)


# ----------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------
def test_rheun_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    A = 0x10000
    directed = [("n", 8), ("dt", 0.1), ("s", 0.3), ("direction", 1), ("seed", 1), ("k", 0), ("dtype", 0)]
    plain = [("n", 8), ("dt", 0.1), ("s", 0.3), ("seed", 1), ("k", 0), ("dtype", 0)]
    common = [({}, dict(n=-1)), ({}, dict(dtype=2)), ({}, dict(dtype=-1)), ({}, dict(k=-1)), ({}, dict(k=1 << 32))]
    direction = [({}, dict(direction=0)), ({}, dict(direction=2)), ({}, dict(direction=-2))]

    def nulls(idx):
        return [({i: None}, {}) for i in idx]

    def misaligned(i, j):  # (pointer i two bytes off for fp32, pointer j four bytes off for fp64)
        return [({i: A * (i + 1) + 2}, {}), ({j: A * (j + 1) + 4}, dict(dtype=1))]

    cases = [("xde_sde_rheun_predict", 5, directed, nulls(range(5)) + common + direction + misaligned(0, 4)),
             ("xde_sde_rheun_correct", 6, directed, nulls(range(6)) + common + direction + misaligned(1, 5)),
             # (af1 or ag1 alone null is refused; both null is the first backward step)
             ("xde_sde_rheun_adjoint_stage", 5, plain, nulls(range(5)) + common + misaligned(0, 4) + [({2: None, 3: None, 4: None}, {})]),
             ("xde_sde_rheun_adjoint_step", 7, plain, nulls((0, 1, 2, 3, 4, 6)) + common + misaligned(0, 6) + [({5: None, 6: None}, {})])]
    run = {}
    for name, nptr, scalars, bad in cases:
        fn = run[name] = _entry(lib, name, nptr, scalars)
        for ptrs, kw in bad:
            for extra in ({}, dict(s=0.0, dt=0.0)):  # (the form without the generator checks the same)
                rc, msg = fn(ptrs, **dict(extra, **kw))
                assert rc == _hip.XDE_EBADARG, (name, ptrs, kw, rc, msg)
                assert name + ":" in msg, (ptrs, kw, msg)
        assert fn(n=0)[0] == _hip.XDE_OK  # n == 0: nothing to launch
    # the null cotangents of the first backward step are admitted
    assert run["xde_sde_rheun_adjoint_stage"]({2: None, 3: None}, n=0)[0] == _hip.XDE_OK
    assert run["xde_sde_rheun_adjoint_step"]({5: None}, n=0)[0] == _hip.XDE_OK
    # the error texts are the existing entry points', word for word, in their order (null, n / dtype / k, alignment) after the direction
    assert run["xde_sde_rheun_predict"](direction=0, n=-1)[1] == "xde_sde_rheun_predict: direction must be +1 or -1"
    assert run["xde_sde_rheun_predict"]({2: None}, n=-1)[1] == "xde_sde_rheun_predict: null pointer"
    assert run["xde_sde_rheun_correct"](n=-1)[1] == "xde_sde_rheun_correct: n < 0"
    assert run["xde_sde_rheun_adjoint_stage"](k=-1)[1] == "xde_sde_rheun_adjoint_stage: k out of range (0 <= k < 2^32)"
    assert run["xde_sde_rheun_adjoint_stage"]({2: None})[1] == "xde_sde_rheun_adjoint_stage: null pointer"
    assert run["xde_sde_rheun_adjoint_step"]({1: A * 2 + 2}, dtype=2)[1] == "xde_sde_rheun_adjoint_step: bad dtype"
    assert run["xde_sde_rheun_adjoint_step"]({1: A * 2 + 2})[1] == "xde_sde_rheun_adjoint_step: operand not aligned to its element type"


def test_the_header_the_prototypes_and_the_library_agree_on_the_rheun_entry_points():
    text = open(os.path.join(ROOT, "include", "xde_hip_sde.h")).read()
    assert "REVERSIBLE HEUN" in text
    lib = _hip.load_library()
    assert lib.xde_abi_version() == 6
    for sym in RHEUN_SYMBOLS:  # (the table against the header, parameter counts included: tests/test_cabi_headers.py)
        assert sym in _hip.HEADERS["xde_hip_sde.h"] and hasattr(lib, sym)


def test_the_rheun_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("sde" in m or "rheun" in m for m in pub)
    for m in ("_sde_rheun_predict", "_sde_rheun_correct", "_sde_rheun_adjoint_stage", "_sde_rheun_adjoint_step"):
        assert callable(getattr(_hip.HipBackend, m))


def test_rheun_is_importable_from_both_solver_packages():
    import paddlexde_amd
    from paddlexde_amd.solver import FixedSolver, ReversibleHeun as A
    from paddlexde_amd.solver.fixed_solver import ReversibleHeun as B

    assert A is B and issubclass(A, FixedSolver) and A.steps_sde
    for name in ("ReversibleHeun", "sdeint", "sdeint_adjoint", "Milstein", "SRK"):
        assert not hasattr(paddlexde_amd, name)  # (the top level keeps the reference's ODE / DDE names)
