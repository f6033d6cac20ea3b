"""Sub-stepping of the fixed-step solvers on the GPU: the end-to-end cases of tests/_substep_cases.py with the HIP backend, the graph
pipelines against "sync", and xde_interp_rows against numpy in the kernel's op order."""
import numpy as np
import pytest
import torch

from paddlexde_amd import RK4, Midpoint, _hip
from paddlexde_amd.solver.base_fixed_solver import FixedSolver, step_size_grid
from paddlexde_amd.utils import _rms_norm
from paddlexde_amd.xde import BaseODE

from . import problems as P
from ._substep_cases import *  # noqa: F401,F403
from ._substep_double import SubstepDoubleBackend

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    return "cuda:0"


@pytest.mark.parametrize("cls", [RK4, Midpoint])
@pytest.mark.parametrize("pipeline", ["graph", "auto"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_graph_pipelines_match_sync(cls, pipeline, dtype):
    """The captured step replayed over the grid, rows written after each replay outside the graph: bit-identical to "sync", same nfe."""
    y0 = torch.tensor([[2.0, 0.0]], dtype=dtype, device="cuda:0")
    t = torch.tensor([0.0, 0.013, 0.4, 0.4, 0.41, 0.42, 0.43, 0.44, 0.45, 0.46, 0.47, 0.48, 0.49, 1.25, 2.0, 3.0], dtype=dtype)
    out, nfe = {}, {}
    took = []
    for p in ("sync", pipeline):
        s = cls(xde=BaseODE(P.spiral_torch, y0=y0, t_span=t), y0=y0, rtol=1e-7, atol=1e-9, norm=_rms_norm, step_size=0.05, pipeline=p)
        inner = s._integrate_graph

        def spy(*a, **k):
            r = inner(*a, **k)
            took.append(p)
            return r

        s._integrate_graph = spy
        with torch.no_grad():
            out[p] = s.integrate(t).cpu()
        nfe[p] = s.nfe
    assert took == [pipeline]  # (the graph pipeline ran to the end: no fall-back to the eager loop)
    n_steps = len(step_size_grid(t.numpy(), 0.05)) - 1
    assert n_steps >= FixedSolver.AUTO_GRAPH_MIN_STEPS
    assert torch.equal(out["sync"], out[pipeline]) and nfe["sync"] == nfe[pipeline] == {RK4: 4, Midpoint: 2}[cls] * n_steps


def _operands(n_outer, L, D, dtype, misalign, seed):
    g = torch.Generator().manual_seed(seed)
    ops = []
    for _ in range(4):
        x = torch.randn(n_outer * L * D + 1, generator=g, dtype=dtype)
        x = (x[1:] if misalign else x[:-1]).reshape(n_outer, L, D)
        ops.append(x)
    return ops


@pytest.mark.parametrize("G", [1, 3, 8, 11])
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape, misalign", [((1, 1, 1), False), ((1, 1, 5), False), ((1, 1, 4099), False), ((1, 2, 4096), False),
                                             ((3, 2, 8), False), ((3, 2, 5), False), ((2, 1, 4099), True), ((3, 2, 8), True)])
def test_interp_rows_kernel_vs_numpy(G, cubic, dtype, shape, misalign):
    """xde_interp_rows against numpy in the kernel's op order, bit for bit: every row kind, rows strided into a [B, T*L, D] solution
    (B > 1), operands and rows at addresses that are not 16-byte aligned (the scalar path)."""
    B, L, D = shape
    T = G + 2
    ops_cpu = _operands(B, L, D, dtype, False, seed=G * 7 + L)
    rng = np.random.RandomState(G)
    kinds = [[_hip.XDE_ROW_INTERP, _hip.XDE_ROW_COPY_A, _hip.XDE_ROW_COPY_B][r % 3] for r in range(G)]
    weights = [tuple(rng.uniform(-1.5, 1.5, size=4)) for _ in range(G)]
    rows_idx = [int(j) for j in rng.permutation(T)[:G]]
    dev = torch.device("cuda:0")
    be = _hip.get_backend()

    def place(x):
        """``x`` on the device, 4 bytes off a 16-byte boundary when ``misalign``."""
        flat = torch.empty(x.numel() + 1, dtype=dtype, device=dev)
        y = (flat[1:] if misalign else flat[:-1]).view(x.shape)
        y.copy_(x)
        return y

    ops = [place(x) for x in ops_cpu]
    use = ops if cubic else ops[:2] + [None, None]
    if misalign:
        base = torch.zeros(B * T * L * D + 1, dtype=dtype, device=dev)[1:].view(B, T * L, D)
    else:
        base = torch.zeros(B, T * L, D, dtype=dtype, device=dev)
    dsts = [base.narrow(-2, j * L, L) for j in rows_idx]
    be._interp_rows(dsts, kinds, weights, *use)
    torch.cuda.synchronize()

    ref = torch.zeros(B, T * L, D, dtype=dtype)
    SubstepDoubleBackend()._interp_rows([ref.narrow(-2, j * L, L) for j in rows_idx], kinds, weights,
                                        *(ops_cpu if cubic else ops_cpu[:2] + [None, None]))
    assert torch.equal(base.cpu(), ref)
