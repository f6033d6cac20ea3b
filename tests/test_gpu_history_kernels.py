"""GPU parity, kernel level, for the delay-equation history kernels: `xde_hermite_gather`, `xde_history_gather` (linear, bez) and
the workspace re-arm of `xde_lag_grad`, against the numpy statement of their contracts (tests/_cpu_double.py, the kernels' op order).

The gathers are element-wise: value AND derivative must be BIT-EXACT (`torch.equal`; the library is built with -ffp-contract=off), and
the scalar kernels must give the vector kernels' bits ("same results", include/xde_hip.h).  Cases are chosen for the branches of
csrc/xde_dense.hip (`xde_hermite_kernel`, `xde_hermite_vec_kernel`: HermiteLag's mode 1 / 2 rows, `zrow`, the 128-lag table) and
csrc/xde_history.hip (`make_lag`, `make_scales`, the `Tn - SPAN - 1` clamp, the lag tiles); tests/_history_grid.py holds the grid.
What the double itself is worth at those edges is pinned on the CPU by tests/test_history_double_host.py.

Mutation check (one arithmetic change at a time in a scratch build, each caught by assertion): `c2` / `c3` swapped in
`xde_hermite_vec_kernel` only — the scalar-path == vector-path assertion of test_gather_row_lengths_and_misaligned_operands (and every
cubic case against the double); `ts[mid] < tau` -> `<=` in `make_lag` — the on-knot lags of every linear / bez case, first at T = 2 / 4;
`r.h1` for `r.h2` in the vector Hermite kernel — the non-uniform grids (first at T = 3).

NOT tested: the 64-bit index branch of `xde_hermite_vec_kernel` (`total >= 2^31` vectors needs about 68 GB of outputs)."""
import numpy as np
import pytest
import torch

from paddlexde_amd import _hip
from paddlexde_amd.xde import HistoryIndex

from . import _history_grid as G
from ._cpu_double import NumpyDoubleBackend

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
WIDTH = {"f32": 4, "f64": 2}
ONE_PASS = 2048 * 256  # work items one pass of the grid-stride loop covers (grid_cap() workgroups of 256 lanes)


@pytest.fixture(scope="module")
def be():
    return _hip.get_backend()


@pytest.fixture(scope="module")
def dbl():
    return NumpyDoubleBackend()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _gpu_gather(be, dev, his, t, lags, method, entry="history"):
    """value, derivative of the GPU kernel as CPU tensors; the outputs start as NaN, so a row no lane wrote cannot compare equal."""
    h = torch.from_numpy(his).to(dev)
    shape = tuple(his.shape[:-2]) + (len(lags), his.shape[-1])
    val = torch.full(shape, float("nan"), dtype=h.dtype, device=dev)
    der = torch.full(shape, float("nan"), dtype=h.dtype, device=dev)
    if entry == "hermite":
        be.hermite_gather(val, der, h, torch.from_numpy(t).to(dev), torch.from_numpy(lags).to(dev))
    else:
        be.history_gather(val, der, h, torch.from_numpy(t).to(dev), torch.from_numpy(lags).to(dev), method)
    torch.cuda.synchronize()
    return val.cpu(), der.cpu()


def _dbl_gather(dbl, his, t, lags, method):
    shape = tuple(his.shape[:-2]) + (len(lags), his.shape[-1])
    val = torch.full(shape, float("nan"), dtype=torch.from_numpy(his).dtype)
    der = torch.full(shape, float("nan"), dtype=val.dtype)
    dbl.history_gather(val, der, torch.from_numpy(his), torch.from_numpy(t), torch.from_numpy(lags), method)
    return val, der


def _first_difference(a, b):
    ne = (a != b) | (a.isnan() != b.isnan())
    idx = ne.nonzero()
    return None if len(idx) == 0 else (tuple(int(i) for i in idx[0]), int(ne.sum()), float(a[tuple(idx[0])]), float(b[tuple(idx[0])]))


def _assert_same_bits(got, want, tag):
    for name, g, w in (("value", got[0], want[0]), ("derivative", got[1], want[1])):
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        assert torch.equal(g, w), (tag, name, "first difference (index, count, got, want):", _first_difference(g, w))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_gather_bit_exact_over_history_lengths_and_lag_kinds(be, dbl, dev, method, dtype):
    """T = the minimum, minimum + 1, 5, 24, 257 on uniform and non-uniform grids; lags below t[0], on EVERY knot, one ulp on either
    side of interior knots, inside the first / middle / last intervals, beyond t[-1]; scalar (D = 1, 3, 7) and vector (D = 4, 8)
    kernels.  The pool of T = 257 holds 289 lags: the scalar cubic kernel and the lag tiles of linear / bez."""
    for T in G.t_values(method):
        for uniform in (True, False):
            t = G.knots(T, uniform, NP[dtype])
            lags = G.lag_pool(t)
            for D in (1, 3, 7, 4, 8):
                his = G.history((3,), T, D, NP[dtype])
                want = _dbl_gather(dbl, his, t, lags, method)
                assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
                _assert_same_bits(_gpu_gather(be, dev, his, t, lags, method), want, (method, dtype, T, uniform, D))
                if method == "cubic":  # xde_hermite_gather called directly is the same launch
                    _assert_same_bits(_gpu_gather(be, dev, his, t, lags, method, entry="hermite"), want, ("hermite", dtype, T, uniform, D))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_gather_lag_counts_and_tiling(be, dbl, dev, method, dtype):
    """L = 0, 1, 127, 128, 129, 300 on the vector and the scalar path.  Above 128 lags the cubic method takes its scalar kernel and
    linear / bez are served in tiles of 128: a lag's bits must not depend on that — the first 128 lags of the 300 give, inside
    L = 300, exactly what they give as a launch of their own."""
    T = 24
    t = G.knots(T, False, NP[dtype])
    w = WIDTH[dtype]
    for D in (2 * w, 7):
        his = G.history((3,), T, D, NP[dtype])
        all_lags = G.lags_of_length(t, 300)
        for L in G.LAG_COUNTS:
            lags = all_lags[:L].copy()
            got = _gpu_gather(be, dev, his, t, lags, method)
            assert got[0].shape == (3, L, D)
            _assert_same_bits(got, _dbl_gather(dbl, his, t, lags, method), (method, dtype, D, L))
        whole = _gpu_gather(be, dev, his, t, all_lags, method)
        for lo, hi in ((0, 128), (128, 256), (256, 300)):
            part = _gpu_gather(be, dev, his, t, all_lags[lo:hi].copy(), method)
            _assert_same_bits((whole[0][:, lo:hi], whole[1][:, lo:hi]), part, (method, dtype, D, "tile", lo, hi))


def _offset_view(x, dev):
    """The same values one element into a larger buffer: 4 / 8 bytes past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_gather_row_lengths_and_misaligned_operands(be, dbl, dev, method, dtype):
    """D = 1, 3, 7 (scalar), 4, 8, 64, 256 (vector), fp64 also D = 2, 6 (vector).  Then the SAME data with `his`, `val` or `der` taken
    one element into a larger buffer: the launch falls to the scalar kernel, whose result must be the vector kernel's, bit for bit."""
    T = 24
    t = G.knots(T, False, NP[dtype])
    lags = G.lags_of_length(t, 40)
    td, ld = torch.from_numpy(t).to(dev), torch.from_numpy(lags).to(dev)
    w = WIDTH[dtype]
    for D in (1, 3, 7, 4, 8, 64, 256) + ((2, 6) if dtype == "f64" else ()):
        his = G.history((5,), T, D, NP[dtype])
        vec = _gpu_gather(be, dev, his, t, lags, method)
        h = torch.from_numpy(his).to(dev)
        # (the scalar kernel against the vector kernel FIRST: a defect in one of the two shows as such, whatever the double says)
        for which in ("his", "val", "der") if D % w == 0 else ():
            val = torch.full((5, len(lags), D), float("nan"), dtype=h.dtype, device=dev)
            der = torch.full_like(val, float("nan"))
            hh, vv, dd = (_offset_view(h, dev) if which == "his" else h), (_offset_view(val, dev) if which == "val" else val), (
                _offset_view(der, dev) if which == "der" else der)
            be.history_gather(vv, dd, hh, td, ld, method)
            torch.cuda.synchronize()
            _assert_same_bits((vv.cpu(), dd.cpu()), vec, (method, dtype, D, "scalar path ==", "vector path", which))
        _assert_same_bits(vec, _dbl_gather(dbl, his, t, lags, method), (method, dtype, D))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_gather_batches_beyond_one_pass_of_the_grid_stride_loop(be, dbl, dev, method, dtype):
    """outer = 0 and 1; the D3STN shape [9824, 12, 64] (3.6 passes of 2048 x 256 lanes in fp32, 7.2 in fp64); a scalar-path shape past
    one pass (D = 63).  Every element compared: a lane that strides wrongly writes a wrong row somewhere."""
    T = 24
    t = G.knots(T, False, NP[dtype])
    lags = G.lags_of_length(t, 12)
    w = WIDTH[dtype]
    for outer, D in ((0, 8), (1, 8), (1, 7), (9824, 64), (1100, 63)):
        work = outer * len(lags) * (D // w if D % w == 0 else D)
        if outer > 1:
            assert work > ONE_PASS
        his = G.history((outer,), T, D, NP[dtype])
        got = _gpu_gather(be, dev, his, t, lags, method)
        assert got[0].shape == (outer, 12, D)
        _assert_same_bits(got, _dbl_gather(dbl, his, t, lags, method), (method, dtype, outer, D))


def _lag_grad_close(got, want, dtype):
    # the bound of test_lag_gradient_reduction_at_odd_sizes: products in the state dtype, fp64 accumulation in another order
    return np.allclose(got, want, rtol=3e-6 if dtype == "f32" else 1e-13, atol=1e-6 if dtype == "f32" else 1e-13)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("method", G.METHODS)
def test_history_index_apply_and_backward_against_the_double(be, dbl, dev, method, dtype):
    """Through the product: `HistoryIndex.apply` (leading shapes (), (3,), (2, 5)) then `backward()` equals the double's
    `history_gather` + `lag_grad` on the same inputs — values bit for bit, the lag gradient to fp64-accumulation accuracy.  With 129
    and 300 lags too: `interp_method="linear"` / `"bez"` raised XdeError there (the kernel's table holds 128 lags; the entry point
    refused more instead of serving them in tiles), the reference and the double accept any number."""
    T, D = 24, 8
    t = G.knots(T, False, NP[dtype])
    for lead, L in (((), 11), ((3,), 11), ((2, 5), 11), ((3,), 129), ((2,), 300)):
        his = G.history(lead, T, D, NP[dtype])
        lags = G.lags_of_length(t, L)
        lg = torch.from_numpy(lags).to(dev).requires_grad_(True)
        y = HistoryIndex.apply(lg, torch.from_numpy(his).to(dev), torch.from_numpy(t).to(dev), method)
        val, der = _dbl_gather(dbl, his, t, lags, method)
        assert y.shape == lead + (L, D)
        assert torch.equal(y.detach().cpu(), val), (method, dtype, lead, L, _first_difference(y.detach().cpu(), val))
        wgt = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=y.dtype)
        (y * wgt.to(dev)).sum().backward()
        want = dbl.lag_grad(wgt, der).numpy()
        assert lg.grad.shape == lg.shape and lg.grad.dtype == lg.dtype
        assert _lag_grad_close(lg.grad.cpu().numpy(), want, dtype), (method, dtype, lead, L, np.abs(lg.grad.cpu().numpy() - want).max())


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_lag_grad_workspace_is_rearmed_between_mappings_of_one_lag_count(be, dbl, dev, dtype):
    """The binding keys `xde_lag_grad`'s workspace by (device, L, stream): launches with the same L but another `outer` / `D` share the
    arrival counters.  PLANE mapping (hundreds of workgroups), then ROWS mapping (12 x 9 workgroups, other shard populations), then PLANE
    again with few workgroups: the second and third results depend on the re-arm after a launch with another workgroup count."""
    L = 12
    rng = np.random.RandomState(5)
    for outer, D in ((1200, 16), (9, 2048), (37, 16), (1200, 16)):
        gy, de = rng.randn(outer, L, D).astype(NP[dtype]), rng.randn(outer, L, D).astype(NP[dtype])
        got = be.lag_grad(torch.from_numpy(gy).to(dev), torch.from_numpy(de).to(dev)).cpu().numpy()
        want = dbl.lag_grad(torch.from_numpy(gy), torch.from_numpy(de)).numpy()
        assert got.shape == (L,) and got.dtype == NP[dtype]
        assert _lag_grad_close(got, want, dtype), (outer, D, np.abs(got - want).max())
