"""The per-sample cases the host tests (numpy double) and the GPU tests share: the five-row problem ``y' = -lam (y - cos t)`` on
``[0, 2]`` with one ``lam`` per row, and its row-alone references from the CPU oracle, computed once per process."""
import functools

import numpy as np
import torch

from . import _rows_oracle as RO

LAM = (0.5, 2.0, 10.0, 50.0, 200.0)
Y0_ROW = (1.0, 0.5, -0.25)  # D = 3
RTOL, ATOL = 1e-5, 1e-7
_NP = {torch.float32: np.float32, torch.float64: np.float64}

# The bars of the end-to-end comparisons with the row-alone oracle: 16 x the largest deviation measured on the numpy double
# (DESIGN section 17).  The oracle takes its norms with numpy's pairwise sums, the kernels in THE ROW SUM's order, so the first steps
# (and with them the trajectories) differ in their last bits.
BAR = {torch.float64: 16 * 1.4e-14, torch.float32: 16 * 3.6e-6}
BAR_F32_STATE_F64_TIME = 16 * 7.0e-6  # (an fp32 state under fp64 times: measured 7.0e-6 on the double; fp64 under fp32 times holds BAR's fp64)


def y0_of(lam, dtype, dev="cpu"):
    return (torch.ones(len(lam), len(Y0_ROW), dtype=dtype) * torch.tensor(Y0_ROW, dtype=dtype)).to(dev)


def func_of(lam, dtype, dev="cpu"):
    """The batch's func: row r decays towards cos(t_r) at its own rate.  ``t`` is ``[rows, 1]`` under per_sample, 0-dim else."""
    lam_t = torch.tensor(lam, dtype=dtype, device=dev)[:, None]
    return lambda t, y: -lam_t * (y - torch.cos(t))


def np_func_of(lam, T):
    return lambda r: (lambda t, y: (-T(lam[r]) * (y - np.cos(t))).astype(T))


def t_of(dtype, n=5, t1=2.0, dev="cpu"):
    return torch.linspace(0.0, t1, n, dtype=dtype).to(dev)


@functools.lru_cache(maxsize=None)
def reference(lam, dtype, n=5, reverse=False, solver="dopri5", tdtype=None, **options):
    """``(solution [T, rows, 3], ((n_accept, n_reject), ...))`` of the rows solved alone by the oracle; ``dtype`` is the state dtype and,
    unless ``tdtype`` says otherwise, the time dtype."""
    T = _NP[dtype]
    tdtype = dtype if tdtype is None else tdtype
    t = t_of(tdtype, n).numpy()
    mk = np_func_of(lam, T)
    if reverse:  # the same problem in falling time: y' = +lam (y - cos t) run from 0 to -2 is its mirror image
        t = -t
        mk = lambda r: (lambda t_, y: (T(lam[r]) * (y - np.cos(t_))).astype(T))  # noqa: E731
    sol, counts = RO.solve_alone(mk, y0_of(lam, dtype).numpy(), t, solver, rtol=RTOL, atol=ATOL, options=dict(options, dtype=_NP[tdtype]))
    sol.setflags(write=False)
    return sol, tuple(counts)
