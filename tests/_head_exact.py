"""The two fused heads (include/xde_hip_sdehead.h, include/xde_hip_cdehead.h) in float32 numpy, op by op in the headers' order, for
operands on which the headers' one unstated rounding cannot matter.

The headers state every op but the rounding inside one matrix instruction.  With ``a``, ``W`` and ``bias`` small integers such that

    max_{r, n}  sum_k |a[r, k]| |W[n, k]| + |bias[n]|  <  2^24                                     (``integer_condition``)

every partial sum over k, in any grouping, is an integer below 2^24: it is a float32, so ``pre`` is exact under ANY rounding and the
rest of the header — the products with the increments or with dX, the sequential sums in ascending m or c, the update — can be held
bit for bit.  That sees what an error bound cannot: a run added in another order, a carry on the wrong side, a misplaced element.

Nothing here needs a GPU.  ``*_float64`` are the same results composed differently — an exact float64 matrix product, then every later
op in float64 on float32 operands and rounded to float32 on its own (for +, - and * that is the float32 op: 53 >= 2 * 24 + 2) — and
exist so that the statements themselves can be checked (tests/test_head_exact_host.py)."""
import numpy as np

F32 = np.float32


def integer_operands(rows, N, K, bias, seed=0):
    """``a [rows, K]``, ``W [N, K]``, ``bias [N]`` (or None): integers uniform in {-3 .. 3} stored in float32."""
    rs = np.random.RandomState(1000003 * seed + 7919 * K + 31 * N + rows % 65521)
    draw = lambda *shape: rs.randint(-3, 4, size=shape).astype(F32)  # noqa: E731
    return draw(rows, K), draw(N, K), (draw(N) if bias else None)


def integer_condition(a, W, bias):
    """The left side of the condition above, computed exactly (float64 on integers far below 2^53)."""
    for x in (a, W) + (() if bias is None else (bias,)):
        assert x.dtype == F32 and np.array_equal(x, np.rint(x)), "integer operands only"
    mag = np.abs(a).astype(np.float64) @ np.abs(W).astype(np.float64).T
    return float((mag + (0.0 if bias is None else np.abs(bias).astype(np.float64))).max())


def pre_activations(a, W, bias):
    """``pre [rows, N]`` in float32 in the header's order: acc = +0; acc <- acc + (a_j W_j + a_{KH+j} W_{KH+j}) for ascending j, with
    KH = 4 ceil(K / 8) and +0 * +0 where KH + j >= K; then one add of the bias."""
    assert a.dtype == W.dtype == F32
    K = a.shape[1]
    KH = 4 * ((K + 7) // 8)
    acc = np.zeros((a.shape[0], W.shape[0]), dtype=F32)
    zero = np.zeros((), dtype=F32)
    for j in range(min(KH, K)):
        lo = a[:, j, None] * W[None, :, j]
        hi = a[:, KH + j, None] * W[None, :, KH + j] if KH + j < K else zero * zero
        acc = acc + (lo + hi)
    return acc if bias is None else acc + bias[None, :]


def _ascending_sum(p, start):
    """``(...(start + p[.., 0]) + p[.., 1]) + ...`` along the last axis in float32; ``start`` None: the sum starts from p[.., 0]."""
    acc = p[..., 0].copy() if start is None else F32(start) + p[..., 0]
    for m in range(1, p.shape[-1]):
        acc = acc + p[..., m]
    return acc


def sde_forward(a, W, bias, w, y0, f, dt):
    """``y1 [rows, D]`` of xde_sdehead_step with the identity activation; ``w [rows, M]`` are the increments s * Z."""
    rows, D = y0.shape
    M = w.shape[1]
    p = pre_activations(a, W, bias).reshape(rows, D, M) * w[:, None, :]
    return (y0 + f * F32(dt)) + _ascending_sum(p, None)


def sde_backward(w, gy1, dt):
    """``s_out [rows, D M]`` and ``gf [rows, D]`` of xde_sdehead_backward with the identity activation."""
    rows, D = gy1.shape
    return (gy1[:, :, None] * w[:, None, :]).reshape(rows, D * w.shape[1]), gy1 * F32(dt)


def cde_forward(a, W, bias, dX):
    """``out [B, H]`` of xde_cdehead_forward with the identity activation; ``dX [B, C]``."""
    B, C = dX.shape
    p = pre_activations(a, W, bias).reshape(B, W.shape[0] // C, C) * dX[:, None, :]
    return _ascending_sum(p, 0.0)


def cde_backward(dX, gout):
    """``s [B, H C]`` of xde_cdehead_backward with the identity activation."""
    B, H = gout.shape
    return (gout[:, :, None] * dX[:, None, :]).reshape(B, H * dX.shape[1])


# -- the same results composed in float64 --------------------------------------------------------------------------------------------
def _r(x):
    return x.astype(F32).astype(np.float64)


def _pre_float64(a, W, bias):
    pre = a.astype(np.float64) @ W.astype(np.float64).T  # (exact: integers)
    return pre if bias is None else pre + bias.astype(np.float64)[None, :]


def sde_forward_float64(a, W, bias, w, y0, f, dt):
    rows, D = y0.shape
    M = w.shape[1]
    pre, w, y0, f = _pre_float64(a, W, bias), w.astype(np.float64), y0.astype(np.float64), f.astype(np.float64)
    y1 = np.empty((rows, D), dtype=F32)
    for d in range(D):
        acc = None
        for m in range(M):
            p = _r(pre[:, d * M + m] * w[:, m])
            acc = p if acc is None else _r(acc + p)
        y1[:, d] = _r(_r(y0[:, d] + _r(f[:, d] * float(F32(dt)))) + acc)
    return y1


def cde_forward_float64(a, W, bias, dX):
    B, C = dX.shape
    H = W.shape[0] // C
    pre, dX = _pre_float64(a, W, bias), dX.astype(np.float64)
    out = np.empty((B, H), dtype=F32)
    for h in range(H):
        acc = np.zeros(B)
        for c in range(C):
            acc = _r(acc + _r(pre[:, h * C + c] * dX[:, c]))
        out[:, h] = acc
    return out
