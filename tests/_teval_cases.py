"""The per-sample output-time cases the host tests (numpy double) and the GPU tests share: the five-row problem of
tests/_rows_cases.py solved JOINTLY over [0, 2] with seven times per row, the MLP problem of the gradient tests, and the reference
every comparison uses — the existing ``odeint`` on the sorted distinct union of all rows' times, gathered."""
import numpy as np
import torch

from paddlexde_amd import odeint
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _rows_cases as RC
from . import _teval_oracle as TO

_NP = {torch.float32: np.float32, torch.float64: np.float64}
T_END = 2.0


def five_row_times(tdtype, reverse=False, seed=3):
    """``tq [5, 7]`` on [0, 2] (negated: on [0, -2]) from a seed.  Row 0 has three times within 1e-3 (one step holds them all), row 1 a
    query at the start time and two equal neighbours, row 2 one at the end time; row 3 is padded from column 4 on, row 4 from column 2."""
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.05, 1.95, size=(5, 7)), axis=1)
    t[0, 1:4] = [0.4, 0.4004, 0.4008]
    t[0] = np.sort(t[0])
    t[1, 0] = 0.0
    t[1, 3] = t[1, 2]
    t[2, 6] = T_END
    t[3, 4:] = np.nan
    t[4, 2:] = np.nan
    return torch.tensor(-t if reverse else t, dtype=tdtype)


def five_row_problem(dtype, reverse=False, dev="cpu"):
    """``(func, y0, t_span ends)`` of the five-row problem solved jointly (``t`` is 0-dim); in falling time its mirror image."""
    f = RC.func_of(RC.LAM, dtype, dev)
    func = (lambda t, y: -f(-t, y)) if reverse else f
    return func, RC.y0_of(RC.LAM, dtype, dev), [0.0, -T_END if reverse else T_END]


def union_of(tq, t_span):
    """``(times, idx)``: the sorted distinct union of ``t_span``'s ends and every finite time, in the direction of integration, and
    ``idx[r, q]`` the position of ``tq[r, q]`` in it (-1 where that is NaN)."""
    a = tq.cpu().numpy()
    d = -1.0 if t_span[1] < t_span[0] else 1.0
    fin = ~np.isnan(a)
    ends = np.asarray(t_span, dtype=a.dtype)
    u = np.unique(np.concatenate([d * ends, d * a[fin]]))
    idx = np.where(fin, np.searchsorted(u, np.where(fin, d * a, u[0])), -1)
    return d * u, idx


def gather(union_sol, idx):
    """``[Q, rows, ...]`` from the union solve's ``[U, rows, ...]``: ``union_sol[idx[r, q], r]``, 0 where ``idx`` is -1."""
    rows, Q = idx.shape
    out = union_sol.new_zeros((Q, rows) + tuple(union_sol.shape[2:]))
    for r in range(rows):
        for q in range(Q):
            if idx[r, q] >= 0:
                out[q, r] = union_sol[int(idx[r, q]), r]
    return out


def solve_teval(func, y0, ends, tq, solver, tdtype, rtol=RC.RTOL, atol=RC.ATOL, **opt):
    """The solve through ``t_eval`` and the accepted steps ``[(t0, t1, dt)]`` its hook saw."""
    steps = []

    def hook(i, y0_, y1, ks, c):
        if c.accept:
            steps.append((float(c.t0), float(c.t1), float(c.dt_last)))

    t_span = torch.tensor(ends, dtype=tdtype, device=y0.device)
    sol = odeint(func, y0, t_span, solver, rtol=rtol, atol=atol, options=dict(opt, t_eval=tq, norm=_rms_norm, dtype=tdtype, _step_hook=hook))
    return sol, steps


def solve_union(func, y0, ends, tq, solver, tdtype, rtol=RC.RTOL, atol=RC.ATOL, **opt):
    """``(solution [U, rows, ...], idx)`` of the existing ``odeint`` on the union of the times."""
    times, idx = union_of(tq, ends)
    t = torch.tensor(times, dtype=tdtype, device=y0.device)
    return odeint(func, y0, t, solver, rtol=rtol, atol=atol, options=dict(opt, norm=_rms_norm, dtype=tdtype)), idx


def held_per_step(steps, tq, ends, tdtype):
    """``[[number of queries of row r inside step n] ...]`` by the oracle's MEMBERSHIP."""
    a = tq.cpu().numpy().astype(np.float64)
    cnt = (~np.isnan(a)).cumprod(axis=1).sum(axis=1)
    d = -1 if ends[1] < ends[0] else 1
    return [[len(TO.members(a[r], cnt[r], t0, t1, d, _NP[tdtype])) for r in range(a.shape[0])] for t0, t1, _ in steps]


class MLP(torch.nn.Module):
    """The func of the gradient tests: a 3 x 4 state."""

    def __init__(self, dtype=torch.float64, dim=4, hidden=16, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter((0.5 * torch.randn(hidden, dim, generator=g, dtype=torch.float64)).to(dtype))
        self.b1 = torch.nn.Parameter((0.1 * torch.randn(hidden, generator=g, dtype=torch.float64)).to(dtype))
        self.c1 = torch.nn.Parameter((0.3 * torch.randn(hidden, generator=g, dtype=torch.float64)).to(dtype))
        self.w2 = torch.nn.Parameter((0.5 * torch.randn(dim, hidden, generator=g, dtype=torch.float64)).to(dtype))

    def forward(self, t, y):
        return torch.tanh(y @ self.w1.t() + self.b1 + t * self.c1) @ self.w2.t()


MLP_ENDS = [0.0, 5.0]
# row 0: a query at the start, three inside the first steps, a long gap some step covers without a query, one at the end;
# row 1: equal neighbours, then padding; row 2: no observation at all
MLP_TIMES = [[0.0, 0.02, 0.0205, 0.021, 1.1, 5.0],
             [0.5, 0.5, 3.0, float("nan"), float("nan"), float("nan")],
             [float("nan")] * 6]


def mlp_y0(dtype, dev="cpu"):
    return torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4).to(dtype).to(dev)


def loss_of(sol, w):
    return (sol * w).sum() + (sol**2).sum() * 0.1


def loss_weights(sol):
    return torch.linspace(-1.0, 1.0, sol.numel(), dtype=sol.dtype, device=sol.device).reshape(sol.shape)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
