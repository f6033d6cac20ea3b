"""The T / lag grid of the history-gather tests (tests/test_gpu_history_kernels.py on the GPU, tests/test_history_double_host.py on the
CPU): knot grids, histories and lag lists chosen for the branches of csrc/xde_dense.hip (HermiteLag's mode 1 / 2 rows, `zrow`) and
csrc/xde_history.hip (`make_lag`, the `Tn - SPAN - 1` clamp of `scale1`).  Everything is rounded to the working dtype HERE, so both
sides of a comparison see the same inputs.  No repeated knots (zero spacing divides by zero in the reference too), nothing non-finite."""
import numpy as np

METHODS = ("cubic", "linear", "bez")
MIN_T = {"cubic": 2, "linear": 2, "bez": 4}
LAG_COUNTS = (0, 1, 127, 128, 129, 300)


def t_values(method):
    """The minimum T of the method, minimum + 1, 5, 24, 257."""
    m = MIN_T[method]
    return sorted({m, m + 1, 5, 24, 257})


def knots(T, uniform, dtype, seed=0):
    rng = np.random.RandomState(1000 + 7 * T + seed)
    t = 0.5 * np.arange(T, dtype=np.float64) - 1.25 if uniform else np.cumsum(rng.uniform(0.3, 1.7, size=T)) - 2.0
    t = t.astype(dtype)
    assert np.all(np.diff(t) > 0)
    return t


def history(lead, T, D, dtype, seed=0):
    """A smooth series plus noise, [*lead, T, D]: neighbouring rows differ (a wrong row shows), no element is tiny by construction."""
    rng = np.random.RandomState(2000 + 13 * T + D + seed)
    base = np.sin(0.37 * np.arange(T))[:, None] * np.linspace(0.5, 1.5, D)[None, :]
    return (base + 0.3 * rng.randn(*lead, T, D)).astype(dtype)


def lag_pool(t, seed=0):
    """Every kind of lag the index search and the clamps see, in the knots' dtype: below t[0]; exactly on every knot (t[0] and t[-1]
    included: bucketize is right=False, so a knot belongs to the interval on its left with s == 1); one ulp on either side of an
    interior knot; interior points; beyond t[-1] (the last interval extrapolated).  Unsorted, with repeats."""
    rng = np.random.RandomState(3000 + len(t) + seed)
    dtype = t.dtype.type
    T = len(t)
    h0, hl = float(t[1] - t[0]), float(t[-1] - t[-2])
    lags = [t[0] - dtype(0.5 * h0), t[0] - dtype(1e-3), t[-1] + dtype(0.9 * hl), t[-1] + dtype(2.1 * hl), np.nextafter(t[-1], dtype(np.inf)),
            np.nextafter(t[0], dtype(-np.inf)), np.nextafter(t[0], dtype(np.inf)), np.nextafter(t[-1], dtype(-np.inf))]
    lags += list(t)  # on every knot
    for j in sorted({1, T // 2, T - 2} & set(range(1, T - 1))):  # interior knots, one ulp away on either side
        lags += [np.nextafter(t[j], dtype(-np.inf)), np.nextafter(t[j], dtype(np.inf))]
    for j in sorted({0, 1, T // 2, T - 3, T - 2} & set(range(T - 1))):  # interior points of the first, middle and last intervals
        lags += [t[j] + dtype(x) * (t[j + 1] - t[j]) for x in (0.25, 0.5, 0.77)]
    lags = np.asarray(lags, dtype=t.dtype)
    lags = np.concatenate([lags, lags[:3]])  # repeats
    return lags[rng.permutation(len(lags))]


def lags_of_length(t, L, seed=0):
    """L lags: the pool (cycled when L is larger, cut when smaller — a cut keeps a shuffled sample of every kind), the rest uniform
    over [t[0] - 0.5 h, t[-1] + 0.9 h]."""
    pool = lag_pool(t, seed)
    if L <= len(pool):
        return pool[:L].copy()
    rng = np.random.RandomState(4000 + L + seed)
    lo, hi = float(t[0]) - 0.5 * float(t[1] - t[0]), float(t[-1]) + 0.9 * float(t[-1] - t[-2])
    return np.concatenate([pool, rng.uniform(lo, hi, size=L - len(pool)).astype(t.dtype)])
