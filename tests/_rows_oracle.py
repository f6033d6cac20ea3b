"""include/xde_hip_rows.h restated in numpy, op by op, including THE ROW SUM's order; the whole per-sample solve is
``oracle.xde_oracle.odeint`` called row by row (``solve_alone``).

``ctl`` below is any object whose attributes ``t, t_prev, h, h_used, ratio, nonfinite`` (float64 ``[rows]``), ``accept, done, status,
next_out, n_accept, n_reject, steps_in_interval`` (int32 ``[rows]``) and ``t_stage`` (``[S, rows]`` of the state dtype) are numpy arrays;
the functions write into them as the kernels do."""
import types

import numpy as np

from oracle import xde_oracle as O

F64 = ("t", "t_prev", "h", "h_used", "ratio", "nonfinite")
I32 = ("accept", "done", "status", "next_out", "n_accept", "n_reject", "steps_in_interval")
STATUS_OK, STATUS_DT_UNDERFLOW, STATUS_NONFINITE, STATUS_MAX_STEPS = 0, 1, 2, 3


def new_ctl(rows, n_stage, T):
    c = types.SimpleNamespace(**{n: np.zeros(rows, np.float64) for n in F64}, **{n: np.zeros(rows, np.int32) for n in I32})
    c.t_stage = np.zeros((n_stage, rows), T)
    return c


def copy_ctl(c):
    return types.SimpleNamespace(**{n: np.array(getattr(c, n)) for n in F64 + I32 + ("t_stage",)})


def _fmax(a, b):
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b)))


def lanes_of(D, T):
    """(W, C, G): elements of a chunk, chunks of a row, lanes of a row — a function of (D, dtype) only."""
    W = 4 if T == np.float32 else 2
    C = -(-D // W)
    G = 1
    while G < 256 and G < C:
        G <<= 1
    return W, C, G


def row_sum(q, T):
    """THE ROW SUM of the float64 terms ``q`` ``[rows, D]``: lane g sums the chunks g, g + G, ... in increasing d, sequentially from 0.0;
    then the pairwise tree over the lanes."""
    rows, D = q.shape
    W, C, G = lanes_of(D, T)
    iters = -(-C // G)
    pad = np.zeros((rows, iters * G * W), np.float64)
    pad[:, :D] = q
    pad = pad.reshape(rows, iters, G, W)
    valid = (np.arange(iters * G * W) < D).reshape(iters, G, W)
    S = np.zeros((rows, G), np.float64)
    with np.errstate(all="ignore"):
        for it in range(iters):
            for w in range(W):
                S = np.where(valid[it, :, w], S + pad[:, it, :, w], S)
        while S.shape[1] > 1:
            S = S[:, 0::2] + S[:, 1::2]
    return S[:, 0]


def norm_of(total, D, T):
    """xde_norm_result's RMS: |round_T(sqrt(round_T(sum / D)))|, as float64."""
    with np.errstate(all="ignore"):
        mean = (np.asarray(total, np.float64) / np.float64(D)).astype(T).astype(np.float64)
        return np.abs(np.sqrt(mean).astype(T).astype(np.float64))


def stage_combine(y0, ks, coef, ctl, coef2=None):
    """Kernel 1 on ``[rows, D]`` arrays: returns ``(out, out2)`` (``out2`` None without ``coef2``)."""
    T = y0.dtype.type
    dt = ctl.h.astype(T)[:, None]
    with np.errstate(all="ignore"):
        acc = ks[0] * (T(coef[0]) * dt)
        for j in range(1, len(ks)):
            acc = acc + ks[j] * (T(coef[j]) * dt)
        out = np.where(ctl.done[:, None] != 0, y0, y0 + acc)
        out2 = None
        if coef2 is not None:
            out2 = ks[0] * (dt * T(coef2[0]))
            for j in range(1, len(ks)):
                out2 = out2 + ks[j] * (dt * T(coef2[j]))
    return out, out2


def _pow(a, b):
    """pow_ of the device controller: the float64 power rounded once."""
    return type(a)(np.float64(a) ** np.float64(b))


def control_row(ctl, r, ratio, nonfinite, p, t_span, n_out, Y):
    """xde_rk_control's I-controller on row ``r`` (no step_t, no replay), as kernel 2's one lane runs it."""
    TT = np.float32 if p.time_dtype == 0 else np.float64
    d = TT(p.direction)
    with np.errstate(all="ignore"):
        t0, dt = TT(ctl.t[r]), TT(ctl.h[r])
        t1 = t0 + dt
        min_step, max_step = TT(p.min_step), TT(p.max_step)
        status = int(ctl.status[r])
        if nonfinite > 0 and status == STATUS_OK:
            status = STATUS_NONFINITE
        accept = 1 if ratio <= 1.0 else 0
        if d * dt > max_step:
            accept = 0
        if d * dt <= min_step:
            accept = 1
        if ratio == 0.0:
            dt_next = dt * TT(p.ifactor)
        else:
            dfactor = TT(1) if ratio < 1.0 else TT(p.dfactor)
            exponent = TT(1) / TT(p.order)
            factor = np.fmin(TT(p.ifactor), np.fmax(TT(p.safety) / _pow(TT(ratio), exponent), dfactor))
            dt_next = dt * TT(factor)
        mag = d * dt_next
        if mag == mag:
            mag = min(max(mag, min_step), max_step)
            dt_next = d * mag
        steps = int(ctl.steps_in_interval[r]) + 1
        if accept:
            ctl.n_accept[r] += 1
        else:
            ctl.n_reject[r] += 1
        t_new = t1 if accept else t0
        e = b = int(ctl.next_out[r])
        if accept:
            while e < n_out and d * TT(t_span[e]) <= d * t1:
                e += 1
        if e > b:
            steps = 0
        done = e >= n_out
        # plan_next on (t_new, dt_next)
        nt0, ndt = TT(t_new), TT(dt_next)
        nt1 = nt0 + ndt
        if not done:
            if not (d * (nt0 + ndt) > d * nt0) and status == STATUS_OK:
                status = STATUS_DT_UNDERFLOW
            if steps >= p.max_num_steps and status == STATUS_OK:
                status = STATUS_MAX_STEPS
        ctl.t_prev[r], ctl.t[r], ctl.h_used[r], ctl.h[r] = float(t0), float(t_new), float(dt), float(dt_next)
        ctl.ratio[r], ctl.nonfinite[r], ctl.accept[r], ctl.status[r], ctl.steps_in_interval[r] = ratio, nonfinite, accept, status, steps
        for i in range(ctl.t_stage.shape[0]):
            a = Y(p.alpha[i])
            ctl.t_stage[i, r] = Y(nt0) if done else (Y(nt1) if a == 1.0 else Y(nt0) + a * Y(ndt))


def norm_control(ks, c_err, e_pre, y0, y1, ctl, p, t_span, n_out):
    """Kernel 2 on ``[rows, D]`` arrays."""
    T = y0.dtype.type
    rows, D = y0.shape
    frozen = (ctl.done != 0) | (ctl.status != STATUS_OK)
    dt = ctl.h.astype(T)[:, None]
    with np.errstate(all="ignore"):
        e = ks[0] * (dt * T(c_err[0]))
        if e_pre is not None:
            e = e_pre + e
        for j in range(1, len(ks)):
            e = e + ks[j] * (dt * T(c_err[j]))
        tol = T(p.atol) + T(p.rtol) * _fmax(np.abs(y0), np.abs(y1))
        q = (e / tol).astype(np.float64)
        ratio = norm_of(row_sum(q * q, T), D, T)
    nf = (~np.isfinite(y0)).sum(axis=1)
    for r in range(rows):
        if frozen[r]:
            ctl.accept[r] = 0
        else:
            control_row(ctl, r, float(ratio[r]), float(nf[r]), p, t_span, n_out, T)


def quartic(y0, y1, f0, f1, ymid, x, dt):
    T = y0.dtype.type
    with np.errstate(all="ignore"):
        ca = T(2) * dt * (f1 - f0) - T(8) * (y1 + y0) + T(16) * ymid
        cb = dt * (T(5) * f0 - T(3) * f1) + T(18) * y0 + T(14) * y1 - T(32) * ymid
        cc = dt * (f1 - T(4) * f0) - T(11) * y0 - T(5) * y1 + T(16) * ymid
        cd = dt * f0
        total = y0 + x * cd
        xp = x * x
        total = total + xp * cc
        xp = xp * x
        total = total + xp * cb
        xp = xp * x
        total = total + xp * ca
    return total


def dense_commit(out, ks, mid, y0, y1, f1, ctl, p, t_span, n_out):
    """Kernel 3 on ``[rows, D]`` arrays (``out`` ``[n_out, rows, D]``); ``y0`` and ``ks[0]`` are committed in place."""
    T = y0.dtype.type
    TT = np.float32 if p.time_dtype == 0 else np.float64
    d = TT(p.direction)
    for r in range(y0.shape[0]):
        if not ctl.accept[r]:
            continue
        t0, t1 = TT(ctl.t_prev[r]), TT(ctl.t[r])
        dt = T(TT(ctl.h_used[r]))
        b = e = int(ctl.next_out[r])
        while e < n_out and d * TT(t_span[e]) <= d * t1:
            e += 1
        if e > b:
            with np.errstate(all="ignore"):
                acc = ks[0][r] * (dt * T(mid[0]))
                for j in range(1, len(ks)):
                    acc = acc + ks[j][r] * (dt * T(mid[j]))
                ymid = y0[r] + acc
                for j in range(b, e):
                    x = T((TT(t_span[j]) - t0) / (t1 - t0))
                    out[j, r] = quartic(y0[r], y1[r], ks[0][r], f1[r], ymid, x, dt)
        y0[r] = y1[r]
        ks[0][r] = f1[r]
        ctl.next_out[r] = e
        ctl.done[r] = 1 if e >= n_out else 0


def scaled_norm(a, b, y0, rtol, atol):
    """Kernel 4 on ``[rows, D]`` arrays: a float64 per row."""
    T = y0.dtype.type
    with np.errstate(all="ignore"):
        scale = T(atol) + np.abs(y0) * T(rtol)
        q = ((a - b if b is not None else a) / scale).astype(np.float64)
        return norm_of(row_sum(q * q, T), y0.shape[1], T)


def solve_alone(make_func, y0, t_span, solver, **kw):
    """The row-alone reference: ``oracle.xde_oracle.odeint`` on ``y0[r:r+1]`` for every row; ``make_func(r)`` is row r's numpy func.
    Returns ``(solution [T, rows, ...], [(n_accept, n_reject)] per row)``."""
    sols, counts = [], []
    for r in range(y0.shape[0]):
        sol, s = O.odeint(make_func(r), y0[r:r + 1], t_span, solver, return_solver=True, **kw)
        sols.append(sol)
        counts.append((s.n_accept, s.n_reject))
    return np.concatenate(sols, axis=1), counts
