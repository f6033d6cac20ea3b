"""Cases of the logsignature windows that run on the numpy double (tests/test_logsig_host.py) and on the GPU (tests/test_gpu_logsig.py)
through the ``dev`` fixture of each module: the algebra of the two levels (Chen's identity, reversal, translation, a straight line), the
vector-field contract of the log-ODE method against products of segment exponentials, and cdeint on the path."""
import numpy as np
import torch

from paddlexde_amd.functional import cdeint
from paddlexde_amd.interpolation import LinearInterpolation, logsig_path, logsig_windows
from paddlexde_amd.solver import RK4
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _logsig_oracle as LO

__all__ = ["test_chen_s_identity", "test_reversing_a_window_negates_both_levels", "test_a_translated_series_gives_the_same_bits",
           "test_a_straight_line_has_zero_areas_exactly", "test_the_bracket_columns_follow_the_log_ode_contract",
           "test_cdeint_on_the_logsig_path_equals_cdeint_on_the_oracle_s_path"]

# Chen's identity at C = 4, nine points: the figure of the CPU check the feature was specified with is 4.4e-16 (on chen_series() below the
# numpy double gives 1.1e-16 at level 1 and 5.6e-17 at level 2: DESIGN section 18); the bar is 16 times that figure
CHEN_MEASURED = 4.4e-16
CHEN_BAR = 16 * CHEN_MEASURED


def _wedge(a, b):
    iu, ju = np.triu_indices(a.shape[-1], 1)
    return a[..., iu] * b[..., ju] - a[..., ju] * b[..., iu]


def _windows(x, depth, L, dev):
    return logsig_windows(torch.from_numpy(np.ascontiguousarray(x)).to(dev), depth, L).cpu().numpy()


def chen_series():
    return np.cumsum(0.3 * np.random.RandomState(4).randn(1, 9, 4), axis=1)


def test_chen_s_identity(dev):
    """A series of nine points cut at its fifth: l1(whole) = l1a + l1b and A(whole) = A_a + A_b + (l1a ^ l1b) / 2, float64."""
    x = chen_series()
    whole = _windows(x, 2, 8, dev)[0, 0]
    a, b = _windows(x, 2, 4, dev)[0]
    assert whole.shape == (10,) and np.array_equal(_windows(x[:, :5], 2, 4, dev)[0, 0], a) and np.array_equal(_windows(x[:, 4:], 2, 4, dev)[0, 0], b)
    err1 = np.abs(whole[:4] - (a[:4] + b[:4])).max()
    err2 = np.abs(whole[4:] - (a[4:] + b[4:] + 0.5 * _wedge(a[:4], b[:4]))).max()
    print("Chen: level 1 {:.3g}, level 2 {:.3g} (bar {:.3g})".format(err1, err2, CHEN_BAR))
    assert err1 <= CHEN_BAR and err2 <= CHEN_BAR


def test_reversing_a_window_negates_both_levels(dev):
    """Level 1 exactly.  Level 2: both directions round the same exact area, each within (n + 2) eps of the sum S of the magnitudes
    of its terms (n - 1 additions, a product, a difference and the final rounding), so they differ by at most 2 (n + 2) eps S."""
    x = chen_series()
    fwd, rev = _windows(x, 2, 8, dev)[0, 0], _windows(x[:, ::-1], 2, 8, dev)[0, 0]
    assert np.array_equal(rev[:4], -fwd[:4])
    iu, ju = np.triu_indices(4, 1)
    S = np.zeros(6)
    for p in (x[0], x[0, ::-1]):
        u, d = np.abs(p[1:-1] - p[0]), np.abs(p[2:] - p[1:-1])
        S = np.maximum(S, 0.5 * (u[:, iu] * d[:, ju] + u[:, ju] * d[:, iu]).sum(axis=0))
    bar = 2 * (8 + 2) * np.finfo(np.float64).eps * S
    print("reversal: worst |sum| / bar = {:.3g}".format((np.abs(rev[4:] + fwd[4:]) / bar).max()))
    assert np.all(np.abs(rev[4:] + fwd[4:]) <= bar)


def test_a_translated_series_gives_the_same_bits(dev):
    """Entries on a grid of 1/64 below 8 and a shift by whole numbers: the shifted entries are exact in both dtypes, so every
    difference of two points has the same bits."""
    rs = np.random.RandomState(5)
    for T in (np.float32, np.float64):
        x = (rs.randint(-512, 512, size=(2, 7, 3)) / 64.0).astype(T)
        shift = np.array([3.0, -5.0, 16.0], dtype=T)
        assert np.array_equal(((x + shift) - shift), x)
        for L in (1, 3, 6):
            assert np.array_equal(_windows(x + shift, 2, L, dev), _windows(x, 2, L, dev)), (T, L)


def test_a_straight_line_has_zero_areas_exactly(dev):
    """p_k = a + k v on small whole numbers: u_k = k v and D_k = v exactly, and every term is k v_i v_j - k v_j v_i = 0."""
    for T in (np.float32, np.float64):
        a, v = np.array([1.0, -2.0, 3.0, 0.5], dtype=T), np.array([3.0, 1.0, -2.0, 0.25], dtype=T)
        x = (a + np.arange(9, dtype=T)[:, None] * v)[None]
        for L in (2, 8, 3):
            out = _windows(x, 2, L, dev)
            assert np.array_equal(out[..., 4:], np.zeros_like(out[..., 4:])), (T, L)
            assert np.array_equal(out[0, 0, :4], min(L, 8) * v)


def contract_errors(dev, sign=1.0):
    """C = 3, H = 3, A = 0.5 randn from RandomState(0), the path 0.8 (t, sin 3t, t cos 2t) on 65 uniform points of [0, 1]: the product
    of the per-window exponentials of ``sum_c l1_c A_c + sum_{i<j} out[pair] (A_j A_i - A_i A_j)`` against the product of the 64
    segment exponentials, in the spectral norm.  Returns {(depth, L): error}."""
    A = torch.from_numpy(0.5 * np.random.RandomState(0).randn(3, 3, 3))
    t = np.linspace(0.0, 1.0, 65)
    x = 0.8 * np.stack([t, np.sin(3 * t), t * np.cos(2 * t)], axis=-1)[None]
    iu, ju = np.triu_indices(3, 1)
    brackets = sign * torch.stack([A[j] @ A[i] - A[i] @ A[j] for i, j in zip(iu, ju)])
    fields = {1: A, 2: torch.cat([A, brackets])}

    def flow(inc, depth):
        z = torch.eye(3, dtype=torch.float64)
        for row in torch.from_numpy(inc):
            z = torch.linalg.matrix_exp(torch.einsum("k,khg->hg", row, fields[depth])) @ z
        return z

    exact = flow(_windows(x, 1, 1, dev)[0], 1)
    return {(depth, L): float(torch.linalg.matrix_norm(flow(_windows(x, depth, L, dev)[0], depth) - exact, 2))
            for depth, L in ((1, 8), (2, 8), (2, 4))}


def test_the_bracket_columns_follow_the_log_ode_contract(dev):
    """Depth 2 is second order in the window and far better than depth 1: the error at L = 4 is at most 1/8 of that at L = 8, and
    the depth-2 error at L = 8 at most 1/50 of the depth-1 error at L = 8 (the CPU figures the feature was specified with: 1/17.8
    and 1/168; with this seed on the numpy double: 1/18.1 and 1/171).  With the bracket's sign reversed both conditions fail."""
    e = contract_errors(dev)
    print("contract: depth 1 L 8 {:.3g}, depth 2 L 8 {:.3g}, depth 2 L 4 {:.3g}: ratios 1/{:.3g} and 1/{:.3g}".format(
        e[1, 8], e[2, 8], e[2, 4], e[2, 8] / e[2, 4], e[1, 8] / e[2, 8]))
    assert e[2, 4] <= e[2, 8] / 8 and e[2, 8] <= e[1, 8] / 50
    r = contract_errors(dev, sign=-1.0)
    assert not r[2, 4] <= r[2, 8] / 8 and not r[2, 8] <= r[1, 8] / 50


def integration_inputs():
    rs = np.random.RandomState(7)
    x = np.cumsum(0.2 * rs.randn(2, 17, 3), axis=1)
    a = 0.5 * rs.randn(4, 6)
    z0 = 1.0 + rs.rand(2, 4)
    return x, a, z0


def test_cdeint_on_the_logsig_path_equals_cdeint_on_the_oracle_s_path(dev):
    """cdeint(RK4, step_size = 1/2) on LinearInterpolation(logsig_path(x, 2, 4)) against the same call on the path built from the
    oracle's increments with the same framework ops: the transform is the oracle's bit for bit (measured on the double: 0), so the
    solutions are equal.  With differentiable=True the loss gradient reaches x."""
    x, a, z0 = (torch.from_numpy(v).to(dev) for v in integration_inputs())
    ts = torch.arange(5, dtype=torch.float64).to(dev)
    opts = {"norm": _rms_norm, "step_size": 0.5}
    field = lambda t, z: torch.tanh(z)[..., None] * a  # noqa: E731
    with torch.no_grad():
        got = cdeint(field, LinearInterpolation(logsig_path(x, 2, 4)), z0, ts, RK4, options=opts)
        inc = torch.from_numpy(LO.windows(x.cpu().numpy(), 4, 2)).to(dev)
        path = torch.cat([torch.zeros_like(inc[..., :1, :]), torch.cumsum(inc, dim=-2)], dim=-2)
        want = cdeint(field, LinearInterpolation(path), z0, ts, RK4, options=opts)
    assert got.numel() == 5 * 2 * 4 and torch.equal(got, want) and bool(torch.isfinite(got).all())
    x.requires_grad_(True)
    sol = cdeint(field, LinearInterpolation(logsig_path(x, 2, 4), differentiable=True), z0, ts, RK4, options=opts)
    (sol * sol).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert float(x.grad[:, 1:-1].abs().min()) > 0  # (every interior point moves some area)
