"""Logsignature windows without a GPU: the C ABI of include/xde_hip_logsig.h (every call below is refused on the host before anything
is enqueued), the channel query, the double against the oracle, the cases of tests/_logsig_cases.py on the numpy double, gradients,
launch counts and what the public functions refuse."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd import interpolation as I
from paddlexde_amd.interpolation import LogsigWindowsFn, logsig_path, logsig_windows, logsignature_channels, window_times

from . import _logsig_oracle as LO
from ._logsig_cases import *  # noqa: F401,F403
from ._logsig_cases import CHEN_BAR, CHEN_MEASURED, chen_series

# the gradient of a weighted sum of logsig_path against the same formulas in framework ops, (2, 9, 3), L = 4, float64: the worst
# |difference| measured on the numpy double is 8.9e-16; the bar is 16 times that
PATH_GRAD_MEASURED = 8.9e-16


@pytest.fixture
def dev():
    from ._logsig_double import LogsigDoubleBackend

    _hip._set_backend_for_testing(LogsigDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_logsig.h
# ----------------------------------------------------------------------------------------------
def test_the_logsig_backend_methods_are_private_and_the_functions_are_exported():
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("logsig" in m for m in pub)
    for m in ("_logsig_windows", "_logsig_windows_backward"):
        assert callable(getattr(_hip.HipBackend, m))
    import paddlexde_amd

    for name in ("logsignature_channels", "logsig_windows", "logsig_path", "window_times"):
        assert name in I.__all__ and callable(getattr(I, name)) and not hasattr(paddlexde_amd, name)
    assert list(_hip.HEADERS)[-1] == "xde_hip_logsig.h" and list(_hip.HEADERS)[-2] == "xde_hip_rows.h" and _hip.ABI_VERSION == 6


def test_logsig_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    OUT, X, GX = (0x100000 * (i + 1) for i in range(3))  # (never dereferenced: every call is refused first)

    def fwd(out=OUT, x=X, B=2, T=9, C=3, L=4, depth=2, dtype=0):
        return lib.xde_logsig_windows(out, x, B, T, C, L, depth, dtype, None), lib.xde_last_error().decode()

    def bwd(gx=GX, gout=OUT, x=X, B=2, T=9, C=3, L=4, depth=2, dtype=0):
        return lib.xde_logsig_windows_backward(gx, gout, x, B, T, C, L, depth, dtype, None), lib.xde_last_error().decode()

    shape = [dict(B=0), dict(B=-1), dict(T=1), dict(T=0), dict(C=0), dict(C=513), dict(C=-2), dict(L=0), dict(L=-4), dict(depth=0),
             dict(depth=3), dict(depth=-1), dict(dtype=2), dict(dtype=-1),
             dict(B=1 << 40, T=1 << 9, C=2), dict(B=1 << 30, T=1 << 30, C=1),          # B T C past 2^48
             dict(B=1 << 30, T=257, C=512, L=1), dict(B=1 << 62, T=2, C=1)]  # B W K past 2^48 (B T C is not), and B alone
    cases = [(fwd, "xde_logsig_windows", [dict(out=None), dict(x=None)] + shape + [
        dict(out=OUT + 2), dict(x=X + 4, dtype=1), dict(out=X), dict(out=X + 2 * 9 * 3 * 4 - 4), dict(out=X - 2 * 2 * 6 * 4 + 4)]),
             (bwd, "xde_logsig_windows_backward", [dict(gx=None), dict(gout=None), dict(x=None)] + shape + [
                 dict(gx=GX + 1), dict(gout=OUT + 4, dtype=1), dict(x=X + 2), dict(gx=X), dict(gx=OUT + 2 * 2 * 6 * 4 - 4), dict(gx=X + 4)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert msg.startswith(name + ":"), (kw, msg)
    for fn in (fwd, bwd):
        assert "depth 2" in fn(depth=3)[1] and "not built" in fn(depth=3)[1]
        assert "B * W * K is too large (> 2^48)" in fn(B=1 << 30, T=257, C=512, L=1)[1]
        assert "B * T * C is too large (> 2^48)" in fn(B=1 << 40, T=1 << 9, C=2)[1]


def test_the_channel_query():
    lib = _hip.load_library()
    for C_, K in ((1, 1), (2, 3), (3, 6), (32, 528), (64, 2080), (512, 131328)):
        assert lib.xde_logsig_channels(C_, 2) == K == logsignature_channels(C_, 2) == logsignature_channels(C_) == LO.channels(C_, 2)
        assert lib.xde_logsig_channels(C_, 1) == C_ == logsignature_channels(C_, 1)
        assert LO.pair(C_, C_ - 2, C_ - 1) == K - 1 if C_ > 1 else True
    for C_, depth in ((0, 2), (513, 2), (3, 0), (3, 3), (-1, 1)):
        assert lib.xde_logsig_channels(C_, depth) == -1 and b"xde_logsig_channels" in lib.xde_last_error()
        with pytest.raises(ValueError):
            logsignature_channels(C_, depth)
    with pytest.raises(ValueError, match="depth 3 is not built"):
        logsignature_channels(3, 3)


# ----------------------------------------------------------------------------------------------
# the double states the header
# ----------------------------------------------------------------------------------------------
def test_the_double_states_the_header(dev):
    """The double's launches are the oracle's arrays; the oracle against an independent statement of the header's formulas (einsum
    over the steps, autograd for the cotangent) to rounding, and its level 1 and its n = 1 areas exactly."""
    be = _hip.get_backend()
    for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 4e-15)):
        for (B, Tn, C_, L), depth in [((2, 8, 3, 3), 2), ((2, 8, 3, 3), 1), ((1, 2, 2, 1), 2), ((3, 6, 1, 2), 2), ((2, 5, 4, 9), 2)]:
            gen = torch.Generator().manual_seed(Tn * 10 + C_)
            x = torch.randn(B, Tn, C_, generator=gen, dtype=torch.float64).to(dtype)
            W, K = LO.n_windows(Tn, L), LO.channels(C_, depth)
            out = torch.empty(B, W, K, dtype=dtype)
            be._logsig_windows(out, x, L, depth)
            assert np.array_equal(out.numpy(), LO.windows(x.numpy(), L, depth))
            gout = torch.randn(B, W, K, generator=gen, dtype=torch.float64).to(dtype)
            gx = torch.empty_like(x)
            be._logsig_windows_backward(gx, gout, x, L, depth)
            assert np.array_equal(gx.numpy(), LO.backward(gout.numpy(), x.numpy(), L, depth))
            xr = x.double().requires_grad_(True)
            ref = _framework_windows(xr, depth, L)
            (gref,) = torch.autograd.grad(ref, xr, gout.double())
            assert np.array_equal(out[..., :C_].numpy(), ref[..., :C_].detach().to(dtype).numpy())
            assert float((out.double() - ref.detach()).abs().max()) <= tol * 8 and float((gx.double() - gref).abs().max()) <= tol * 8
            if L == 1 and depth == 2:
                assert not out[..., C_:].any()
    assert be.launches == ["logsig_windows", "logsig_windows_backward"] * 10
    # a leading axis more or none: flattened into B
    x = torch.randn(2, 3, 7, 2, dtype=torch.float64)
    assert torch.equal(logsig_windows(x, 2, 3), logsig_windows(x.reshape(6, 7, 2), 2, 3).reshape(2, 3, 2, 3))
    assert torch.equal(logsig_windows(x[0, 0], 2, 3), logsig_windows(x, 2, 3)[0, 0])


def _framework_windows(x, depth, L):
    """The same formulas as framework ops: a diff, offsets from the window's first point, a product per window, the
    antisymmetrisation and the triangular gather."""
    Tn, C_ = x.shape[-2:]
    iu, ju = np.triu_indices(C_, 1)
    outs = []
    for t0, n in LO.spans(Tn, L):
        p = x[..., t0 : t0 + n + 1, :]
        l1 = p[..., n, :] - p[..., 0, :]
        if depth == 1:
            outs.append(l1)
            continue
        u, d = p[..., 1:n, :] - p[..., :1, :], p[..., 2:, :] - p[..., 1:n, :]
        M = torch.einsum("...ki,...kj->...ij", u, d)
        outs.append(torch.cat([l1, (0.5 * (M - M.transpose(-1, -2)))[..., iu, ju]], dim=-1))
    return torch.stack(outs, dim=-2)


def test_the_chen_bar_is_sixteen_times_the_figure_of_the_double(dev):
    x = chen_series()
    whole = LO.windows(x, 8, 2)[0, 0]
    a, b = LO.windows(x, 4, 2)[0]
    iu, ju = np.triu_indices(4, 1)
    err = np.abs(whole[4:] - (a[4:] + b[4:] + 0.5 * (a[iu] * b[ju] - a[ju] * b[iu]))).max()
    print("Chen on the oracle:", err)
    assert err <= CHEN_MEASURED and CHEN_BAR == 16 * CHEN_MEASURED


# ----------------------------------------------------------------------------------------------
# gradients
# ----------------------------------------------------------------------------------------------
def test_gradcheck_of_logsig_windows(dev):
    x = torch.randn(2, 7, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s: logsig_windows(s, 2, 3), (x,))
    assert torch.autograd.gradcheck(lambda s: logsig_windows(s, 1, 3), (x,))
    assert torch.autograd.gradcheck(lambda s: logsig_path(s, 2, 2), (x,))
    assert "logsig_windows_backward" in _hip.get_backend().launches


def test_the_gradient_of_a_weighted_sum_of_the_path_equals_the_framework_ops(dev):
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 9, 3, generator=gen, dtype=torch.float64)
    w = torch.randn(2, 3, 6, generator=gen, dtype=torch.float64)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got = logsig_path(a, 2, 4)
    inc = _framework_windows(b, 2, 4)
    want = torch.cat([torch.zeros_like(inc[..., :1, :]), torch.cumsum(inc, dim=-2)], dim=-2)
    assert got.shape == (2, 3, 6) and not got[:, 0].any() and float((got - want).detach().abs().max()) <= 16 * PATH_GRAD_MEASURED
    (got * w).sum().backward()
    (want * w).sum().backward()
    err = float((a.grad - b.grad).abs().max())
    print("path gradient against framework ops:", err)
    assert err <= 16 * PATH_GRAD_MEASURED


# ----------------------------------------------------------------------------------------------
# launch counts
# ----------------------------------------------------------------------------------------------
def test_one_launch_each_way_and_none_without_a_gradient(dev):
    be = _hip.get_backend()
    x = torch.randn(2, 9, 3, dtype=torch.float64)
    out = logsig_windows(x, 2, 4)
    assert be.launches == ["logsig_windows"] and not out.requires_grad
    del be.launches[:]
    xg = x.clone().requires_grad_(True)
    path = logsig_path(xg, 2, 4)
    assert be.launches == ["logsig_windows"]
    del be.launches[:]
    path.sum().backward()
    assert be.launches == ["logsig_windows_backward"] and xg.grad.shape == x.shape
    # an absent cotangent stays absent: nothing is launched for it
    del be.launches[:]
    out = logsig_windows(xg, 2, 4)
    assert LogsigWindowsFn.backward(out.grad_fn, None) == (None, None, None) and be.launches == ["logsig_windows"]
    # the forward saves the series only
    assert len(out.grad_fn.saved_tensors) == 1 and out.grad_fn.saved_tensors[0].data_ptr() == xg.data_ptr()


# ----------------------------------------------------------------------------------------------
# what is refused, before the first launch
# ----------------------------------------------------------------------------------------------
def test_refusals(dev):
    be = _hip.get_backend()
    x = torch.randn(2, 9, 3, dtype=torch.float64)
    for depth in (0, 3, 4, -1):
        with pytest.raises(ValueError, match="depth {} is not built".format(depth)):
            logsig_windows(x, depth, 4)
        with pytest.raises(ValueError, match="is not built"):
            logsig_path(x, depth, 4)
    with pytest.raises(ValueError, match="depth must be 1 or 2"):
        logsig_windows(x, 1.5, 4)
    with pytest.raises(ValueError, match="T >= 2"):
        logsig_windows(x[:, :1], 2, 1)
    for L in (0, -2, 1.5):
        with pytest.raises(ValueError, match="window_length must be an integer >= 1"):
            logsig_windows(x, 2, L)
        with pytest.raises(ValueError, match="window_length must be an integer >= 1"):
            window_times(torch.arange(9.0), L)
    with pytest.raises(ValueError, match="1 <= C <= 512"):
        logsig_windows(torch.zeros(1, 2, 513, dtype=torch.float64), 2, 1)
    with pytest.raises(ValueError, match=r"\[\.\.\., T, C\]"):
        logsig_windows(torch.zeros(5, dtype=torch.float64), 2, 1)
    for bad in (torch.zeros(2, 9, 3, dtype=torch.int64), torch.zeros(2, 9, 3, dtype=torch.float16), np.zeros((2, 9, 3))):
        with pytest.raises(TypeError, match="float32 or float64 tensor"):
            logsig_windows(bad, 2, 4)
    assert be.launches == []
    # a series that is not on a device, with the production backend
    _hip._set_backend_for_testing(None)
    with pytest.raises(_hip.XdeError, match="no CPU path"):
        logsig_windows(x, 2, 4)
    with pytest.raises(_hip.XdeError, match="no CPU path"):
        _hip.get_backend()._logsig_windows(torch.empty(2, 2, 6, dtype=torch.float64), x, 4, 2)


def test_window_times():
    t = torch.linspace(0.0, 1.0, 10)
    assert torch.equal(window_times(t, 4), t[[0, 4, 8, 9]]) and torch.equal(window_times(t, 3), t[[0, 3, 6, 9]])
    assert torch.equal(window_times(t, 1), t) and torch.equal(window_times(t, 50), t[[0, 9]])
    for L in (1, 3, 4, 9, 50):
        assert window_times(t, L).numel() == LO.n_windows(10, L) + 1
    with pytest.raises(ValueError, match="at least 2"):
        window_times(t[:1], 2)
