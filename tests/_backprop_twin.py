"""Eager torch twin of the reference's adaptive step, for checking options["backprop"] = "steps".

Restates paddlexde/solver/base_adaptive_solver_rk.py's step with the stages in a Python list and autograd flowing through every
k_j (what the reference's PaddleAssign achieves), dense output by the quartic of utils/ode_utils.py (interp_fit + interp_evaluate),
and the next step's k_0 = this step's last stage derivative.  It REPLAYS a given accepted step sequence [(t0, t1, dt)] instead of
running a controller, so a comparison isolates the gradient arithmetic from the step-size decisions.  Tableaus: oracle.xde_oracle.
"""
import torch

from oracle.xde_oracle import ADAPTIVE


def quartic(y0, y1, y_mid, f0, f1, dt, x):
    # interp_fit (ode_utils.py:44-49) + interp_evaluate (:69-77)
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    d = dt * f0
    return y0 + x * d + x**2 * c + x**3 * b + x**4 * a


def _t(v, dtype, dev):
    return v.to(dtype) if torch.is_tensor(v) else torch.tensor(v, dtype=dtype, device=dev)


def twin_odeint(func, y0, t_span, name, steps, first_dt=None):
    """Solution [T, *y0.shape] of the replayed solve, differentiable w.r.t. y0 and func's parameters.
    ``steps``: the accepted (t0, t1, dt) of a solve (e.g. from the product's record_trace / step hook).
    ``first_dt``: a tensor that replaces the first step size, graph included (the reference's select_initial_step is not
    no_grad); every later time is then ``t0 + dt`` of the step before, as in the reference's loop."""
    _, tab, mid = ADAPTIVE[name]
    ts = [float(t) for t in t_span]
    T = len(ts)
    d = 1.0 if T < 2 or ts[-1] >= ts[0] else -1.0
    dtype, dev = y0.dtype, y0.device
    rows = [y0]
    r = 1
    while r < T and d * ts[r] <= d * ts[0]:
        rows.append(y0)
        r += 1
    y = y0
    f = func(_t(ts[0], dtype, dev), y0)
    t_prev = None
    for n, (t0, t1, dt) in enumerate(steps):
        if first_dt is not None:
            dt = first_dt if n == 0 else dt
            t0 = ts[0] if n == 0 else t_prev
            t1 = t0 + dt
            t_prev = t1
        k = [f]
        for i, a in enumerate(tab.alpha):
            yi = y
            for j, bij in enumerate(tab.beta[i]):
                if bij != 0.0:
                    yi = yi + k[j] * (float(bij) * dt)
            ti = t1 if float(a) == 1.0 else t0 + float(a) * dt
            k.append(func(_t(ti, dtype, dev), yi))
        y1 = y
        y_mid = y
        for j in range(len(k)):
            if float(tab.c_sol[j]) != 0.0:
                y1 = y1 + k[j] * (float(tab.c_sol[j]) * dt)
            if float(mid[j]) != 0.0:
                y_mid = y_mid + k[j] * (float(mid[j]) * dt)
        while r < T and d * ts[r] <= d * float(t1):
            rows.append(quartic(y, y1, y_mid, k[0], k[-1], dt, (ts[r] - t0) / (t1 - t0)))
            r += 1
        y, f = y1, k[-1]
    assert r == T, "the step sequence ends before the last output time"
    return torch.stack(rows)
