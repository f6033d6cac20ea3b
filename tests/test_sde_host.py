"""sdeint without a GPU: the generator's restatement against its known answers, the counter layout, the end-to-end cases of
tests/_sde_cases.py on the numpy double, and the C ABI of include/xde_hip_sde.h (every call below is refused on the host before anything
is enqueued, or has n == 0)."""
import numpy as np
import pytest

from paddlexde_amd import _hip

from . import _sde_oracle as SO
from ._sde_cases import *  # noqa: F401,F403


@pytest.fixture
def dev():
    from ._sde_double import SdeDoubleBackend

    _hip._set_backend_for_testing(SdeDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


# ----------------------------------------------------------------------------------------------
# the generator
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", SO.KAT)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(x) for x in SO.philox4x32_10(np.array(counter, dtype=np.uint64), key)) == want


def test_words_put_j_k_and_the_seed_where_the_header_says():
    seed, k = 0x0123_4567_89AB_CDEF, 41
    w = SO.words(3, seed, k)
    for j in range(3):
        assert np.array_equal(w[j], SO.philox4x32_10(np.array([j, 0, k, 0], dtype=np.uint64), (0x89ABCDEF, 0x01234567)))
    big = (1 << 32) + 5  # (the counter's second word is j's high word)
    assert np.array_equal(SO.philox4x32_10(np.array([big & 0xFFFFFFFF, big >> 32, k, 0], dtype=np.uint64), (1, 2)),
                          SO.philox4x32_10(np.array([5, 1, k, 0], dtype=np.uint64), (1, 2)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_step_and_element_has_its_own_counter_and_words(dtype):
    """(k, e) -> (counter (j_lo, j_hi, k, 0), words): fp32 one word of j = e/4, fp64 a word pair of j = e/2; no two (k, e) share."""
    W = 4 if dtype == np.float32 else 2
    seen = set()
    for k in range(5):
        for e in range(4099):
            j = e // W
            ws = (e % 4,) if W == 4 else (2 * (e % 2), 2 * (e % 2) + 1)
            for wd in ws:
                key = (j & 0xFFFFFFFF, j >> 32, k, 0, wd)
                assert key not in seen
                seen.add(key)
    assert len(seen) == 5 * 4099 * (4 // W)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_uniforms_and_normals_follow_the_mapping(dtype):
    w = SO.words(4096, 3, 7)
    u = SO.uniforms(w, dtype)
    assert u.min() > 0 and u.max() <= 1
    if dtype == np.float32:
        assert np.array_equal(u, ((w.astype(np.int64) >> 8) + 1) * 2.0**-24)
    ends = SO.uniforms(np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32), dtype)
    eps = 2.0**-24 if dtype == np.float32 else 2.0**-53
    assert ends[0, 0] == eps and ends[0, -1] == 1.0
    z = SO.normals(9, 3, 7, dtype)  # (the pairs are (u0, u1), (u2, u3) for fp32, (u_a, u_b) for fp64)
    z0, z1, _ = SO.box_muller(u[0, 0], u[0, 1])
    assert z[0] == z0 and z[1] == z1
    # the tail bound: r is largest at the smallest u1
    r_max = float(np.sqrt(-2.0 * np.log(eps)))
    assert abs(r_max - (5.768 if dtype == np.float32 else 8.572)) < 1e-3


def test_the_double_draws_the_oracle_noise(dev):
    import torch

    be = _hip.get_backend()
    out = torch.empty(11, dtype=torch.float32)
    be._sde_noise(out, 5, 2)
    assert np.array_equal(out.numpy(), SO.normals(11, 5, 2, np.float32).astype(np.float32))
    bits = torch.empty(10, dtype=torch.int32)
    be._sde_noise(bits, 5, 2, bits=True)
    assert np.array_equal(bits.numpy().view(np.uint32), SO.words(3, 5, 2).reshape(-1)[:10])


# ----------------------------------------------------------------------------------------------
# the C ABI of include/xde_hip_sde.h
# ----------------------------------------------------------------------------------------------
def test_sde_entry_points_validate_their_arguments_on_the_host():
    lib = _hip.load_library()
    A, B, Cc, D = 0x10000, 0x20000, 0x30000, 0x40000  # (never dereferenced: every call is refused first)

    def step(y1=A, y0=B, f=Cc, g=D, n=8, k=0, dtype=0):
        return lib.xde_sde_em_step(y1, y0, f, g, n, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    def bwd(gf=A, gg=B, gy=Cc, n=8, k=0, dtype=0):
        return lib.xde_sde_em_backward(gf, gg, gy, n, 0.1, 0.3, 1, k, dtype, None), lib.xde_last_error().decode()

    def noise(out=A, n=8, k=0, mode=0, dtype=0):
        return lib.xde_sde_noise(out, n, 1, k, mode, dtype, None), lib.xde_last_error().decode()

    cases = [(step, "xde_sde_em_step", [dict(y1=None), dict(y0=None), dict(f=None), dict(g=None), dict(n=-1), dict(dtype=2),
                                        dict(dtype=-1), dict(k=-1), dict(k=1 << 32), dict(y0=B + 2), dict(g=D + 4, dtype=1)]),
             (bwd, "xde_sde_em_backward", [dict(gy=None), dict(n=-1), dict(dtype=2), dict(k=-1), dict(gf=A + 2)]),
             (noise, "xde_sde_noise", [dict(out=None), dict(n=-1), dict(mode=2), dict(mode=-1), dict(dtype=2), dict(k=1 << 32),
                                       dict(out=A + 4, dtype=1)])]
    for fn, name, bad in cases:
        for kw in bad:
            rc, msg = fn(**kw)
            assert rc == _hip.XDE_EBADARG, (name, kw, rc, msg)
            assert name in msg, (kw, msg)
        assert fn(n=0)[0] == _hip.XDE_OK  # n == 0: nothing to launch
    assert bwd(gf=None, gg=None)[0] == _hip.XDE_OK  # neither output wanted


def test_the_backend_methods_are_private():
    """The public methods of HipBackend are the contract tests/_cpu_double.py mirrors; the SDE entry points stay outside it."""
    pub = {m for m in dir(_hip.HipBackend) if not m.startswith("_")}
    assert not any("sde" in m for m in pub)
    for m in ("_sde_em_step", "_sde_em_backward", "_sde_noise"):
        assert callable(getattr(_hip.HipBackend, m))
