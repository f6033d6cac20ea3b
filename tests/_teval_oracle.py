"""Numpy ORACLE of the two kernels of include/xde_hip_teval.h, written from the header as plain loops per (row, query): membership by
a linear scan (the kernels search), the quartic and the weights op by op.  The state dtype T is the arrays', the time dtype TT given.

Layouts as in the header: state operands ``[rows, D]``, ``out`` / ``g`` ``[Q, rows, D]``, ``tq`` float64 ``[rows, Q]``, ``cnt`` int32
``[rows]``.  Everything is written in place."""
import numpy as np


def members(tq_row, cnt, t0, t1, direction, TT):
    """MEMBERSHIP: the queries q of one row inside the step (t0, t1], in increasing q."""
    d = TT(direction)
    return [q for q in range(int(cnt)) if d * TT(t0) < d * TT(tq_row[q]) and d * TT(tq_row[q]) <= d * TT(t1)]


def frac(tq, t0, t1, T, TT):
    return T((TT(tq) - TT(t0)) / (TT(t1) - TT(t0)))


def dense(out, tq, cnt, ks, mid, y0, y1, f0, f1, t0, t1, dt, direction, TT):
    T = y0.dtype.type
    rows = y0.shape[0]
    dtT = T(TT(dt))
    for r in range(rows):
        qs = members(tq[r], cnt[r], t0, t1, direction, TT)
        if not qs:
            continue
        acc = ks[0][r] * (dtT * T(mid[0]))
        for j in range(1, len(ks)):
            acc = acc + ks[j][r] * (dtT * T(mid[j]))
        a0, a1, b0, b1 = y0[r], y1[r], f0[r], f1[r]
        ymid = a0 + acc
        ca = T(2) * dtT * (b1 - b0) - T(8) * (a1 + a0) + T(16) * ymid
        cb = dtT * (T(5) * b0 - T(3) * b1) + T(18) * a0 + T(14) * a1 - T(32) * ymid
        cc = dtT * (b1 - T(4) * b0) - T(11) * a0 - T(5) * a1 + T(16) * ymid
        cd = dtT * b0
        for q in qs:
            x = frac(tq[r, q], t0, t1, T, TT)
            total = a0 + x * cd
            xp = x * x
            total = total + xp * cc
            xp = xp * x
            total = total + xp * cb
            xp = xp * x
            total = total + xp * ca
            out[q, r] = total


def weights(x, dts):
    """``(p0 + pm, p1, pm, q0, q1)`` at fraction ``x``, in float64 in the header's order."""
    x, dts = np.float64(x), np.float64(dts)
    x2 = x * x
    x3 = x2 * x
    x4 = x3 * x
    p0 = 1.0 - 11.0 * x2 + 18.0 * x3 - 8.0 * x4
    p1 = -5.0 * x2 + 14.0 * x3 - 8.0 * x4
    pm = 16.0 * x2 - 32.0 * x3 + 16.0 * x4
    q0 = dts * (x - 4.0 * x2 + 5.0 * x3 - 2.0 * x4)
    q1 = dts * (x2 - 3.0 * x3 + 2.0 * x4)
    return (p0 + pm, p1, pm, q0, q1)


def cotangent(outs, g, tq, cnt, t0, t1, dt, direction, TT, acc_mask=0):
    T = g.dtype.type
    rows = g.shape[1]
    dts = np.float64(T(TT(dt)))
    for r in range(rows):
        qs = members(tq[r], cnt[r], t0, t1, direction, TT)
        for j, o in enumerate(outs):
            if o is None:
                continue
            acc = (acc_mask >> j) & 1
            if not qs:
                if not acc:
                    o[r] = T(0)
                continue
            w = [T(weights(frac(tq[r, q], t0, t1, T, TT), dts)[j]) for q in qs]
            s = g[qs[0], r] * w[0]
            if acc:
                s = o[r] + s
            for q, wq in zip(qs[1:], w[1:]):
                s = s + g[q, r] * wq
            o[r] = s
