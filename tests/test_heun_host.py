"""Heun without a GPU: what the three Heun entry points of include/xde_hip_gn.h refuse on the host before anything is enqueued, and what
the solver class refuses before its first launch."""
import pytest
import torch

import paddlexde_amd
from paddlexde_amd import _hip
from paddlexde_amd.functional import odeint, sdeint, sdeint_adjoint
from paddlexde_amd.solver import FixedSolver, Heun

from . import _sde_cases as SC

Y1, A0, Y0, F0, F1, G = (0x100000 * (i + 1) for i in range(6))  # (never dereferenced: every call is refused first)
N = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32); g holds 3 times as many
SHAPE = [dict(rows=0), dict(D=0), dict(M=0), dict(D=(1 << 30) + 1), dict(M=(1 << 30) + 1), dict(rows=1 << 20, D=1 << 20, M=1 << 9), dict(k=-1),
         dict(k=1 << 32), dict(dtype=2)]


def _call(name, ptrs, scalars, **kw):
    a = dict(dict(rows=2, D=4, M=3, k=0, dtype=0, **ptrs), **kw)
    lib = _hip.load_library()
    rc = getattr(lib, name)(*[a[p] for p in ptrs], a["rows"], a["D"], a["M"], *scalars, 1, a["k"], a["dtype"], None)
    return rc, lib.xde_last_error().decode()


@pytest.mark.parametrize("name, ptrs, scalars, bad, nothing_to_do", [
    ("xde_sde_gn_heun_predict", dict(yp=Y1, a0=A0, y0=Y0, f0=F0, g0=G), (0.1, 0.3),
     [dict(yp=None), dict(a0=None), dict(y0=None), dict(f0=None), dict(g0=None), dict(f0=F0 + 2), dict(g0=G + 4, dtype=1), dict(a0=A0 + 1),
      dict(yp=Y0), dict(a0=Y1 + N - 4), dict(a0=F0 - 4), dict(yp=G + 3 * N - 4), dict(a0=G - N + 4)], []),
    ("xde_sde_gn_heun_correct", dict(y1=Y1, y0=Y0, f0=F0, f1=F1, a0=A0, g1=G), (0.1, 0.3),
     [dict(y1=None), dict(y0=None), dict(f0=None), dict(f1=None), dict(a0=None), dict(g1=None), dict(f1=F1 + 2), dict(y1=Y1 + 1),
      dict(y1=Y0 + 4), dict(y1=F0), dict(y1=F1 - 4), dict(y1=A0), dict(y1=G + 3 * N - 4)], []),
    ("xde_sde_gn_heun_backward", dict(gf=Y1, ga=A0, gg=G, gy=Y0, gc=F0), (0.1, 0.5, 0.3),
     [dict(gy=None, gc=None), dict(gy=None), dict(gy=None, gf=None), dict(gy=None, ga=None), dict(gc=F0 + 2), dict(gg=G + 4, dtype=1),
      dict(gf=Y0), dict(ga=Y1), dict(ga=F0 + 4), dict(gg=F0 - 3 * N + 4), dict(gg=Y1 + N - 4), dict(gf=G + 3 * N - 4)],
     [dict(gf=None, ga=None, gg=None), dict(gf=None, ga=None, gg=None, gy=None)])])
def test_heun_entry_points_validate_their_arguments_on_the_host(name, ptrs, scalars, bad, nothing_to_do):
    for kw in bad + SHAPE:
        rc, msg = _call(name, ptrs, scalars, **kw)
        assert rc == _hip.XDE_EBADARG and name in msg, (name, kw, rc, msg)
    for kw in nothing_to_do:  # (no output wanted: XDE_OK without a launch, but only after the checks)
        assert _call(name, ptrs, scalars, **kw)[0] == _hip.XDE_OK and _call(name, ptrs, scalars, rows=0, **kw)[0] == _hip.XDE_EBADARG, kw


def test_what_the_class_refuses_before_its_first_launch():
    assert issubclass(Heun, FixedSolver) and Heun.steps_sde and Heun.steps_matrix_noise and not Heun.steps_logqp
    assert not hasattr(paddlexde_amd, "Heun") and "STRATONOVICH" in Heun.__doc__
    y0, t = SC._y0(torch.float64, "cpu", shape=(2, 3)), torch.linspace(0.0, 1.0, 3, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="Heun steps SDEs only"):
        odeint(SC.drift, y0, t, solver=Heun)
    for noise_type, g, why in (("diagonal", SC.diffusion, "Euler and Milstein accumulate the KL term"),
                               ("general", lambda t_, y: y.unsqueeze(-1).expand(y.shape + (2,)), "linear solve")):
        for match, o in ((why, dict(logqp=True, prior_drift=SC.drift)), ("pipeline='graph'", dict(pipeline="graph")),
                         ("interp='cubic'", dict(interp="cubic", step_size=0.1))):
            with pytest.raises(NotImplementedError, match=match):
                sdeint(SC.drift, g, y0, t, solver=Heun, options=SC._opts(seed=1, noise_type=noise_type, **o))
        with pytest.raises(NotImplementedError):
            sdeint_adjoint(SC.drift, g, y0, t, solver=Heun, options=SC._opts(seed=1, noise_type=noise_type), adjoint_params=())
