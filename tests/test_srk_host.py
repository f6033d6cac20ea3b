"""sdeint's SRK steps without a GPU: the second draw's counter, the end-to-end cases of tests/_srk_cases.py on the numpy double, the
launches of a step, and the C ABI of the new entry points of include/xde_hip_sde.h (every call below is refused on the host before
anything is enqueued, or has nothing to do)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.functional import sdeint
from paddlexde_amd.xde.base_sde import BaseSDE

from . import _milstein_oracle as MO
from . import _sde_oracle as SO
from . import _srk_oracle as KO
from ._srk_cases import *  # noqa: F401,F403
from ._srk_cases import _opts, _y0, diffusion, drift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRK_SYMBOLS = ("xde_sde_srk_stage1", "xde_sde_srk_stage2", "xde_sde_srk_step", "xde_sde_srk_stage1_backward",
               "xde_sde_srk_stage2_backward", "xde_sde_srk_step_backward", "xde_sde_noise_draw")


@pytest.fixture
def dev(monkeypatch):
    from ._srk_double import SrkDoubleBackend

    # (the draws of (seed, k) are the same arrays for every walk of a test: drawn once.  A strong-order case walks 2^16 paths over up to
    # 256 steps three times per grid on two draws; the arrays are dropped with the fixture)
    monkeypatch.setattr(SO, "state_normals", functools.lru_cache(maxsize=512)(SO.state_normals))
    monkeypatch.setattr(KO, "state_normals", functools.lru_cache(maxsize=1024)(KO.state_normals))
    _hip._set_backend_for_testing(SrkDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the second draw
# ----------------------------------------------------------------------------------------------
def test_the_second_draw_is_the_counter_with_last_word_one(dev):
    seed, k = 0x0123_4567_89AB_CDEF, 41
    w = KO.words(3, seed, k, 1)
    for j in range(3):
        assert np.array_equal(w[j], SO.philox4x32_10(np.array([j, 0, k, 1], dtype=np.uint64), (0x89ABCDEF, 0x01234567)))
    assert np.array_equal(KO.words(5, seed, k, 0), SO.words(5, seed, k))
    be = _hip.get_backend()
    bits = torch.empty(10, dtype=torch.int32)
    be._sde_noise(bits, seed, k, bits=True, draw=1)
    assert np.array_equal(bits.numpy().view(np.uint32), w.reshape(-1)[:10])
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        z0, z0d, v = (torch.empty(11, dtype=dtype) for _ in range(3))
        be._sde_noise(z0, seed, k)
        be._sde_noise(z0d, seed, k, draw=0)
        be._sde_noise(v, seed, k, draw=1)
        assert torch.equal(z0, z0d) and not torch.equal(z0, v)
        assert np.array_equal(z0.numpy(), SO.normals(11, seed, k, T).astype(T))
        assert np.array_equal(v.numpy(), KO.normals(11, seed, k, T, 1).astype(T))
        u = SO.uniforms(w, T)  # (the pairs are (u0, u1), (u2, u3) for fp32, (u_a, u_b) for fp64, as for Z)
        v0, v1, _ = SO.box_muller(u[0, 0], u[0, 1])
        assert v.numpy()[0] == T(v0) and v.numpy()[1] == T(v1)


def test_the_weights_sum_to_the_increment():
    """e1 + e2 + e3 + e4 = w up to rounding, and the header's literals are the constants they name."""
    for T in (np.float32, np.float64):
        r3, third, two3, four3, five3 = KO.consts(T)
        eps = np.finfo(T).eps
        assert abs(float(r3) - 3.0**-0.5) <= eps and abs(float(third) - 1 / 3) <= eps and abs(float(two3) - 2 / 3) <= eps
        assert abs(float(four3) - 4 / 3) <= eps and abs(float(five3) - 5 / 3) <= eps
        z, v = KO.state_normals((4099,), 5, 3, T, 0), KO.state_normals((4099,), 5, 3, T, 1)
        dt = T(-0.0123)
        e = KO.weights(dt, z, v, T)
        w, _ = KO.wp(dt, z, v, T)
        assert np.abs(((e[0] + e[1]) + (e[2] + e[3])) - w).max() <= 64 * eps * np.abs(np.stack(e)).max()


# ----------------------------------------------------------------------------------------------
# the step
# ----------------------------------------------------------------------------------------------
def test_launches_of_a_step(dev):
    """Without gradients a step is the three forward launches and nothing else of the library's; with gradients the three backward
    launches appear once per step, in reverse."""
    be = _hip.get_backend()
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    n_steps = len(t) - 1
    fwd = ["sde_srk_stage1", "sde_srk_stage2", "sde_srk_step"]
    with torch.no_grad():
        sdeint(drift, diffusion, y0, t, solver=SRK, options=_opts(seed=1))
    assert be.launches == fwd * n_steps
    del be.launches[:]
    mu = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    sol = sdeint(drift, lambda t_, y: y * mu, y0.clone().requires_grad_(True), t, solver=SRK, options=_opts(seed=1))
    assert be.launches == fwd * n_steps
    del be.launches[:]
    sol.sum().backward()
    assert be.launches == ["sde_srk_step_backward", "sde_srk_stage2_backward", "sde_srk_stage1_backward"] * n_steps


def test_a_step_counts_one_nfe_and_evaluates_drift_twice_and_diffusion_four_times(dev):
    from paddlexde_amd.solver import SRK as S

    nf, ng = [], []
    y0 = _y0(torch.float64, dev, shape=(2, 3))
    t = torch.linspace(0.0, 1.0, 4, dtype=torch.float64)
    xde = BaseSDE(lambda t_, y: nf.append(float(t_)) or y * 0.5, lambda t_, y: ng.append(float(t_)) or y * 0.25, y0, t, seed=3)
    s = S(xde=xde, y0=y0, rtol=1e-7, atol=1e-9, norm=None)
    with torch.no_grad():
        s.integrate(t)
    assert (s.nfe, len(nf), len(ng)) == (3, 6, 12)
    h = 1.0 / 3
    assert np.allclose(nf[:2], [0.0, 0.75 * h], atol=1e-15) and np.allclose(ng[:4], [0.0, 0.25 * h, h, 0.25 * h], atol=1e-15)
    assert S.order == 1.5 and "2 drift and 4 diffusion" in S.__doc__


def test_the_double_states_the_kernels_op_order(dev):
    """The double's six methods against tests/_srk_oracle.py on one step, both dtypes, dt < 0 and dt = 0 (the GPU test holds the kernels
    to the same statement)."""
    be = _hip.get_backend()
    for dtype, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        g = torch.Generator().manual_seed(1)
        y0, a1, a2, b1, b2, b3, b4, g1, g2, g3 = (torch.randn(3, 7, generator=g, dtype=dtype) for _ in range(10))
        Y, A1, A2, B1, B2, B3, B4, H1, H2, H3 = (x.numpy() for x in (y0, a1, a2, b1, b2, b3, b4, g1, g2, g3))
        for dt in (T(-0.0123), T(0.0)):
            s, c, c3 = float(SO.s_of(dt, T)), float(MO.c_of(dt, T)), float(KO.c3_of(dt, T))
            z, v = KO.state_normals((3, 7), 5, 17, T, 0), KO.state_normals((3, 7), 5, 17, T, 1)
            o1, o2, o3, o4, y1 = (torch.empty_like(y0) for _ in range(5))
            be._sde_srk_stage1(o1, o2, o3, y0, a1, b1, float(dt), s, 5, 17)
            for got, want in zip((o1, o2, o3), KO.stage1(Y, A1, B1, dt, z, v, T)):
                assert np.array_equal(got.numpy(), want)
            be._sde_srk_stage2(o4, y0, a1, b1, b2, b3, float(dt), s)
            assert np.array_equal(o4.numpy(), KO.stage2(Y, A1, B1, B2, B3, dt, T))
            be._sde_srk_step(y1, y0, a1, a2, b1, b2, b3, b4, float(dt), s, c, c3, 5, 17)
            assert np.array_equal(y1.numpy(), KO.srk_step(Y, A1, A2, B1, B2, B3, B4, dt, z, v, T))
            if dt == 0:
                assert (c, c3) == (0.0, 0.0)
                for o in (o1, o2, o3, o4, y1):
                    assert np.array_equal(o.numpy(), Y)
            outs = [torch.empty_like(y0) for _ in range(6)]
            be._sde_srk_stage1_backward(*outs[:3], g1, g2, g3, float(dt), s, 5, 17)
            for got, want in zip(outs[:3], KO.stage1_backward(H1, H2, H3, dt, z, v, T)):
                assert np.array_equal(got.numpy(), want)
            be._sde_srk_stage2_backward(*outs[:4], g1, float(dt), s)
            for got, want in zip(outs[:4], KO.stage2_backward(H1, dt, T)):
                assert np.array_equal(got.numpy(), want)
            be._sde_srk_step_backward(*outs, g1, float(dt), s, c, c3, 5, 17)
            for got, want in zip(outs, KO.step_backward(H1, dt, z, v, T)):
                assert np.array_equal(got.numpy(), want)
                if dt == 0:
                    assert not got.numpy().any()


# ----------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------
def _entry(lib, sym, nptr, scalars):
    """``run(ptrs={index: pointer}, **scalars)`` calls ``sym`` with ``nptr`` distinct 16-byte aligned pointers that are never
    dereferenced (every call below is refused first, or has nothing to do) and returns (status, error text)."""

    def run(ptrs=None, **kw):
        p = [0x10000 * (i + 1) for i in range(nptr)]
        for i, val in (ptrs or {}).items():
            p[i] = val
        vals = dict(scalars, **kw)
        return getattr(lib, sym)(*p, *[vals[name] for name, _ in scalars], None), lib.xde_last_error().decode()

    return run


def test_srk_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    A = 0x10000
    noisy = [("n", 8), ("dt", 0.1), ("s", 0.3), ("seed", 1), ("k", 0), ("dtype", 0)]
    quiet = [("n", 8), ("dt", 0.1), ("s", 0.3), ("dtype", 0)]
    full = [("n", 8), ("dt", 0.1), ("s", 0.3), ("c", 1.5), ("c3", 1.6), ("seed", 1), ("k", 0), ("dtype", 0)]
    common = [({}, dict(n=-1)), ({}, dict(dtype=2)), ({}, dict(dtype=-1))]
    ks = [({}, dict(k=-1)), ({}, dict(k=1 << 32))]

    def nulls(idx):
        return [({i: None}, {}) for i in idx]

    def misaligned(i, j):  # (pointer i two bytes off for fp32, pointer j four bytes off for fp64)
        return [({i: A * (i + 1) + 2}, {}), ({j: A * (j + 1) + 4}, dict(dtype=1))]

    cases = [("xde_sde_srk_stage1", 6, noisy, nulls(range(6)) + common + ks + misaligned(3, 5)),
             ("xde_sde_srk_stage2", 6, quiet, nulls(range(6)) + common + misaligned(1, 5)),
             ("xde_sde_srk_step", 8, full, nulls(range(8)) + common + ks + misaligned(1, 7)),
             ("xde_sde_srk_stage1_backward", 6, noisy, nulls((3, 4, 5)) + common + ks + misaligned(0, 2)),
             # (the last ones: a group of outputs given in part)
             ("xde_sde_srk_stage2_backward", 5, quiet, nulls((4,)) + common + misaligned(0, 3) + [({1: None}, {}), ({2: None, 3: None}, {})]),
             ("xde_sde_srk_step_backward", 7, full, nulls((6,)) + common + ks + misaligned(0, 5)
              + [({0: None}, {}), ({3: None}, {}), ({2: None, 3: None, 4: None}, {})])]
    run = {}
    for name, nptr, scalars, bad in cases:
        fn = run[name] = _entry(lib, name, nptr, scalars)
        for ptrs, kw in bad:
            rc, msg = fn(ptrs, **kw)
            assert rc == _hip.XDE_EBADARG, (name, ptrs, kw, rc, msg)
            assert name + ":" in msg, (ptrs, kw, msg)
        assert fn(n=0)[0] == _hip.XDE_OK  # n == 0: nothing to launch
    noise = _entry(lib, "xde_sde_noise_draw", 1, [("n", 8), ("seed", 1), ("k", 0), ("draw", 1), ("mode", 0), ("dtype", 0)])
    for ptrs, kw in (({0: None}, {}), ({}, dict(n=-1)), ({}, dict(mode=2)), ({}, dict(mode=-1)), ({}, dict(draw=2)), ({}, dict(draw=-1)),
                     ({}, dict(dtype=2)), ({}, dict(k=1 << 32)), ({0: A + 4}, dict(dtype=1))):
        rc, msg = noise(ptrs, **kw)
        assert rc == _hip.XDE_EBADARG and "xde_sde_noise_draw:" in msg, (ptrs, kw, rc, msg)
    assert noise(n=0)[0] == _hip.XDE_OK and noise(n=0, draw=0)[0] == _hip.XDE_OK
    # the error texts are the existing entry points', word for word, and the checks come in their order (null, n / dtype / k, alignment)
    assert run["xde_sde_srk_stage1"](n=-1)[1] == "xde_sde_srk_stage1: n < 0"
    assert run["xde_sde_srk_step"](k=-1)[1] == "xde_sde_srk_step: k out of range (0 <= k < 2^32)"
    assert run["xde_sde_srk_step"]({2: None}, n=-1)[1] == "xde_sde_srk_step: null pointer"
    assert run["xde_sde_srk_step"]({1: A * 2 + 2}, dtype=2)[1] == "xde_sde_srk_step: bad dtype"
    assert run["xde_sde_srk_stage2"]({1: A * 2 + 2})[1] == "xde_sde_srk_stage2: operand not aligned to its element type"
    assert run["xde_sde_srk_step_backward"]({6: None})[1] == "xde_sde_srk_step_backward: null pointer (gy1)"
    # no output wanted: nothing to do
    assert run["xde_sde_srk_stage1_backward"]({0: None, 1: None, 2: None})[0] == _hip.XDE_OK
    assert run["xde_sde_srk_stage2_backward"]({i: None for i in range(4)})[0] == _hip.XDE_OK
    assert run["xde_sde_srk_step_backward"]({i: None for i in range(6)})[0] == _hip.XDE_OK


def test_the_header_the_prototypes_and_the_library_agree_on_the_srk_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xde_hip_sde.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for sym in SRK_SYMBOLS:  # (the table against the header, parameter counts included: tests/test_cabi_headers.py)
        assert sym in _hip.HEADERS["xde_hip_sde.h"] and hasattr(lib, sym)
    # the old generator entry point keeps its signature
    assert len(re.search(r"\bxde_sde_noise\s*\(([^)]*)\)", src).group(1).split(",")) == 7


def test_the_srk_backend_methods_are_private():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("sde" in m or "srk" in m for m in pub)
    for m in ("_sde_srk_stage1", "_sde_srk_stage2", "_sde_srk_step", "_sde_srk_stage1_backward", "_sde_srk_stage2_backward",
              "_sde_srk_step_backward"):
        assert callable(getattr(_hip.HipBackend, m))


def test_srk_is_importable_from_both_solver_packages():
    import paddlexde_amd
    from paddlexde_amd.solver import FixedSolver, SRK as A
    from paddlexde_amd.solver.fixed_solver import SRK as B

    assert A is B and issubclass(A, FixedSolver) and A.steps_sde
    assert not hasattr(paddlexde_amd, "SRK")  # (the top level keeps the reference's ODE / DDE names)
