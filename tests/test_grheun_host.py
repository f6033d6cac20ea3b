"""GeneralReversibleHeun without a GPU: what the four xde_sde_gn_rheun_* entry points of include/xde_hip_gn.h refuse on the host before
anything is enqueued, and what the solver class and sdeint_adjoint refuse or accept before the first launch."""
import pytest
import torch

import paddlexde_amd
from paddlexde_amd import _hip
from paddlexde_amd.functional import odeint, sdeint, sdeint_adjoint
from paddlexde_amd.solver import GeneralReversibleHeun, ReversibleHeun
from paddlexde_amd.solver import fixed_solver

from . import _sde_cases as SC

P = [0x100000 * (i + 1) for i in range(9)]  # (never dereferenced: every call is refused first, or has nothing to do)
N = 2 * 4 * 4  # bytes of a state operand at the default shape (fp32); a matrix holds 3 times as many
GN_SHAPE = [dict(rows=0), dict(D=0), dict(M=0), dict(M=(1 << 30) + 1), dict(rows=1 << 20, D=1 << 20, M=1 << 9), dict(k=-1), dict(k=1 << 32), dict(dtype=2)]
ENTRIES = {
    "xde_sde_gn_rheun_predict": (dict(yh1=P[0], a=P[1], y=P[2], yh0=P[3], f=P[4], g=P[5]),
                                 lambda a: (a["rows"], a["D"], a["M"], 0.1, 0.3, 1, a["k"], a["dtype"], None)),
    "xde_sde_gn_rheun_seam": (dict(y1=P[0], yh2=P[1], a1=P[2], y0=P[3], f0=P[4], f1=P[5], a0=P[6], yh1=P[7], g1=P[8]),
                              lambda a: (a["rows"], a["D"], a["M"], 0.1, 0.3, a["k"], 0.2, 0.4, a["k1"], 1, a["dtype"], None)),
    "xde_sde_gn_rheun_adjoint_stage": (dict(bf=P[0], bg=P[8], af1=P[1], c1=P[2], ay1=P[3]),
                                       lambda a: (a["rows"], a["D"], a["M"], 0.1, 0.3, a["k"], 0.4, a["k1"], 1, a["dtype"], None)),
    "xde_sde_gn_rheun_adjoint_step": (dict(ay0=P[0], ayh0=P[1], af0=P[2], c0=P[3], ay1=P[4], ayh1=P[5], v=P[6]),
                                      lambda a: (a["rows"] * a["D"], 0.1, a["dtype"], None)),
}


def _call(name, **kw):
    ptrs, tail = ENTRIES[name]
    a = dict(dict(rows=2, D=4, M=3, k=0, k1=1, dtype=0, **ptrs), **kw)
    lib = _hip.load_library()
    rc = getattr(lib, name)(*[a[p] for p in ptrs], *tail(a))
    return rc, lib.xde_last_error().decode()


@pytest.mark.parametrize("name, bad, nothing_to_do", [
    ("xde_sde_gn_rheun_predict", [dict(yh1=None), dict(a=None), dict(y=None), dict(yh0=None), dict(f=None), dict(g=None), dict(f=P[4] + 2),
                                  dict(g=P[5] + 4, dtype=1), dict(yh1=P[3]), dict(yh1=P[2] + N - 4), dict(a=P[5] + 3 * N - 4), dict(a=P[0])] + GN_SHAPE, []),
    ("xde_sde_gn_rheun_seam", [dict(y1=None), dict(yh2=None), dict(a1=None), dict(y0=None), dict(f0=None), dict(f1=None), dict(a0=None),
                               dict(yh1=None), dict(g1=None), dict(a0=P[6] + 1), dict(yh2=P[7]), dict(y1=P[3] + 4), dict(a1=P[6]), dict(yh2=P[0] + N - 4),
                               dict(a1=P[8] - N + 4), dict(k1=-1), dict(k1=1 << 32)] + GN_SHAPE, []),
    ("xde_sde_gn_rheun_adjoint_stage", [dict(bg=None), dict(ay1=None, c1=None, af1=None, bf=None), dict(ay1=None), dict(ay1=None, af1=None),
                                        dict(bf=None), dict(af1=None), dict(c1=None), dict(c1=P[2] + 2), dict(bf=P[3]), dict(bf=P[1] + 4), dict(bg=P[3] - 3 * N + 4),
                                        dict(bf=P[8] + 3 * N - 4), dict(k1=-1), dict(k1=1 << 32)] + GN_SHAPE, []),
    ("xde_sde_gn_rheun_adjoint_step", [dict(ay0=None), dict(ayh0=None), dict(af0=None), dict(c0=None), dict(ay1=None), dict(v=None), dict(v=P[6] + 2),
                                       dict(ay0=P[1]), dict(af0=P[4]), dict(c0=P[6] + N - 4), dict(ay0=P[4] + 4), dict(ayh0=P[5] - 4), dict(dtype=2), dict(rows=-1)],
     [dict(rows=0), dict(rows=0, ayh1=None), dict(rows=0, ay0=P[4], ayh0=P[5])])])
def test_entry_points_validate_their_arguments_on_the_host(name, bad, nothing_to_do):
    for kw in bad:
        rc, msg = _call(name, **kw)
        assert rc == _hip.XDE_EBADARG and name in msg, (name, kw, rc, msg)
    for kw in nothing_to_do:  # (XDE_OK without a launch, but only after the checks)
        assert _call(name, **kw)[0] == _hip.XDE_OK and _call(name, **dict(kw, v=None))[0] == _hip.XDE_EBADARG, kw


def test_what_the_class_and_the_adjoint_refuse_and_accept():
    G = GeneralReversibleHeun
    assert issubclass(G, ReversibleHeun) and G.steps_matrix_noise and not ReversibleHeun.steps_matrix_noise and not G.steps_logqp
    assert fixed_solver.GeneralReversibleHeun is G and not hasattr(paddlexde_amd, "GeneralReversibleHeun") and _hip.ABI_VERSION == 6
    y0, t = SC._y0(torch.float64, "cpu", shape=(2, 3)), torch.linspace(0.0, 1.0, 3, dtype=torch.float64)
    general = lambda t_, y: y.unsqueeze(-1).expand(y.shape + (2,))  # noqa: E731
    with pytest.raises(NotImplementedError, match="ReversibleHeun steps SDEs only"):
        odeint(SC.drift, y0, t, solver=G)
    for noise_type, g, why in (("diagonal", SC.diffusion, ReversibleHeun.logqp_refusal[:40]), ("general", general, "linear solve")):
        for match, o in ((why, dict(logqp=True, prior_drift=SC.drift)), ("pipeline='graph'", dict(pipeline="graph")),
                         ("interp='cubic'", dict(interp="cubic", step_size=0.1))):
            with pytest.raises(NotImplementedError, match=match):
                sdeint(SC.drift, g, y0, t, solver=G, options=SC._opts(seed=1, noise_type=noise_type, **o))
    # sdeint_adjoint takes the class with every noise type — the solve gets as far as the device check — and nothing else new
    for noise_type, g in (("diagonal", SC.diffusion), ("general", general), ("scalar", lambda t_, y: y.unsqueeze(-1))):
        with pytest.raises(_hip.XdeError):
            sdeint_adjoint(SC.drift, g, y0, t, solver=G, options=SC._opts(seed=1, noise_type=noise_type), adjoint_params=())
    with pytest.raises(NotImplementedError, match="general noise for them is a follow-up"):
        sdeint_adjoint(SC.drift, general, y0, t, solver=ReversibleHeun, options=SC._opts(seed=1, noise_type="general"), adjoint_params=())
