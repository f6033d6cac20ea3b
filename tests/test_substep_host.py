"""Sub-stepping of the fixed-step solvers (step_size / grid_constructor) on the CPU double: the end-to-end cases of
tests/_substep_cases.py, the grid itself, the refusals, and the C ABI of xde_interp_rows without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from paddlexde_amd import RK4, Euler, _hip, odeint
from paddlexde_amd.solver.base_fixed_solver import step_size_grid
from paddlexde_amd.utils import _rms_norm
from paddlexde_amd.xde import BaseODE

from . import _substep_oracle as SO
from . import problems as P
from ._substep_cases import *  # noqa: F401,F403


@pytest.fixture
def dev():
    from ._substep_double import SubstepDoubleBackend

    _hip._set_backend_for_testing(SubstepDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the grid
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("t0, t1, h", [(0.0, 1.0, 0.1), (0.0, 1.0, 0.3), (0.3, 0.7, 0.1), (1.0, 2.44, 0.03), (0.0, 1.3000000715255737, 0.1),
                                       (1.0, 0.0, 0.1), (2.0, -1.0, 0.25), (0.0, 0.05, 0.1), (0.5, 0.5, 0.1), (0.0, 1.0, 1.0)])
def test_step_size_grid_is_the_reference_formula(dtype, t0, t1, h):
    t = np.array([t0, t1], dtype=dtype)
    got = step_size_grid(t, h)
    assert got.dtype == dtype
    assert np.array_equal(got, SO.grid_from_step_size(t, h))


def test_step_size_grid_random_sweep_is_strictly_monotone_with_exact_ends():
    rng = np.random.RandomState(11)
    overshoots = 0
    for dtype in (np.float32, np.float64):
        tt = dtype
        for _ in range(3000):
            t0 = tt(rng.choice([0.0, 0.1, 0.3, 1.0, -0.7]))
            h = tt(rng.choice([0.1, 0.01, 0.03, 0.07, 0.3, 0.2]))
            d = rng.choice([-1, 1])
            t1 = tt(t0 + tt(d) * tt(rng.randint(1, 50)) * h)
            t = np.array([t0, t1], dtype=dtype)
            niters = int(np.ceil((t1 - t0) / (tt(d) * h) + tt(1)))
            raw = np.arange(niters, dtype=dtype) * (tt(d) * h) + t0
            overshoots += int(np.any(d * (raw[1:-1] - t1) >= 0))
            g = step_size_grid(t, h)
            assert g[0] == t0 and g[-1] == t1
            assert np.all(d * np.diff(g) > 0)
    assert overshoots > 0  # (the sweep met the rounding case the deviation is for)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def _call(dev, **options):
    y0 = torch.tensor([[0.5, 0.1]], dtype=torch.float64)
    t = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64)
    return odeint(P.spiral_torch, y0, t, solver=RK4, options=dict({"norm": _rms_norm}, **options))


@pytest.mark.parametrize("h", [0.0, -0.1, float("nan"), float("inf"), np.float32(-1.0), torch.tensor([0.0]), [0.1, 0.2],
                               np.array([0.1, 0.2]), torch.tensor([0.1, 0.2]), []])
def test_refuses_a_bad_step_size(dev, h):
    with pytest.raises(ValueError, match="step_size"):
        _call(dev, step_size=h)


def test_refuses_both_options(dev):
    with pytest.raises(ValueError, match="mutually exclusive"):
        _call(dev, step_size=0.1, grid_constructor=lambda y, t: t)


@pytest.mark.parametrize("grid", [[0.1, 0.5, 1.0], [0.0, 0.5, 0.9]])
def test_refuses_grid_endpoints_other_than_t_span(dev, grid):
    with pytest.raises(AssertionError):
        _call(dev, grid_constructor=lambda y, t: torch.tensor(grid, dtype=torch.float64))


@pytest.mark.parametrize("grid", [[0.0, 0.6, 0.4, 1.0], [0.0, 0.5, 0.5, 1.0], [[0.0, 1.0]]])
def test_refuses_a_grid_that_is_not_strictly_monotone_or_not_1d(dev, grid):
    with pytest.raises(ValueError, match="grid"):
        _call(dev, grid_constructor=lambda y, t: torch.tensor(grid, dtype=torch.float64))


def test_refuses_a_non_monotone_t_span(dev):
    y0 = torch.tensor([[0.5, 0.1]], dtype=torch.float64)
    with pytest.raises(ValueError, match="monotone"):
        odeint(P.spiral_torch, y0, torch.tensor([0.0, 0.7, 0.4, 1.0], dtype=torch.float64), solver=RK4,
               options={"norm": _rms_norm, "step_size": 0.1})


def test_interp_empty_refuses_an_off_grid_output_before_anything_runs(dev):
    y0 = torch.tensor([[0.5, 0.1]], dtype=torch.float64)
    t = torch.tensor([0.0, 0.55, 1.0], dtype=torch.float64)
    s = Euler(xde=BaseODE(P.spiral_torch, y0=y0, t_span=t), y0=y0, rtol=1e-7, atol=1e-9, norm=_rms_norm, step_size=0.1, interp="")
    with pytest.raises(ValueError, match=r"0\.55.*interp=''"):
        s.integrate(t)
    assert s.nfe == 0


def test_adjoint_interval_replay_is_off_with_substeps(dev):
    y0 = torch.tensor([[0.5, 0.1]], dtype=torch.float64)
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    s = RK4(xde=BaseODE(P.spiral_torch, y0=y0, t_span=t), y0=y0, rtol=1e-7, atol=1e-9, norm=_rms_norm, step_size=0.1)
    assert not s.intervals_supported()


# ----------------------------------------------------------------------------------------------
# the C ABI of xde_interp_rows (no GPU: every call below is refused before anything is enqueued, or has n == 0)
# ----------------------------------------------------------------------------------------------
def test_interp_rows_validates_its_arguments_on_the_host():
    lib = _hip.load_library()
    A, B = 0x10000, 0x20000  # (never dereferenced: every call is refused first)

    def call(rows=(0x30000,), kinds=(0,), G=None, y_a=A, y_b=B, f_a=None, f_b=None, mode=0, outer=1, chunk=8, row_stride=8, dtype=0):
        G = len(rows or (0,)) if G is None else G
        r = (C.c_void_p * max(len(rows), 1))(*rows) if rows is not None else None
        k = (C.c_int * max(len(kinds), 1))(*kinds) if kinds is not None else None
        w = (C.c_double * (4 * max(len(rows or ()), 1)))()
        rc = lib.xde_interp_rows(r, k, w, G, y_a, y_b, f_a, f_b, mode, outer, chunk, row_stride, dtype, None)
        return rc, lib.xde_last_error().decode()

    bad = [dict(rows=None), dict(kinds=None), dict(y_a=None), dict(y_b=None), dict(rows=(None,)), dict(G=0), dict(G=9, rows=(0x30000,) * 9, kinds=(0,) * 9),
           dict(mode=2), dict(mode=1), dict(mode=1, f_a=A), dict(kinds=(3,)), dict(kinds=(-1,)), dict(dtype=2), dict(y_a=A + 2),
           dict(rows=(0x30004,), dtype=1), dict(outer=-1), dict(outer=2, row_stride=4)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == _hip.XDE_EBADARG, (kw, rc, msg)
        assert "xde_interp_rows" in msg, (kw, msg)
    assert call(outer=0)[0] == _hip.XDE_OK  # n == 0: nothing to launch
