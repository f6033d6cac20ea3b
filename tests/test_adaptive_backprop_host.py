"""options["backprop"] of odeint on a box without a GPU: option routing and validation, the C entry points' argument checks, and the
whole "steps" sweep on CPU tensors through a numpy statement of the two backprop kernels, against the eager twin in fp64."""
import gc
import importlib
import warnings
import weakref

import pytest
import torch

from paddlexde_amd import AdaptiveHeun, Bosh3, Dopri5, Dopri8, Fehlberg2, RK4, _hip, odeint
from paddlexde_amd.utils.ode_utils import _rms_norm

from ._backprop_twin import twin_odeint

odeint_mod = importlib.import_module("paddlexde_amd.functional.odeint")

SOLVERS = [(Dopri5, "dopri5"), (Dopri8, "dopri8"), (Bosh3, "bosh3"), (Fehlberg2, "fehlberg2"), (AdaptiveHeun, "adaptive_heun")]


class MLP(torch.nn.Module):
    def __init__(self, dim=4, hidden=16, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter(0.5 * torch.randn(hidden, dim, generator=g, dtype=torch.float64))
        self.b1 = torch.nn.Parameter(0.1 * torch.randn(hidden, generator=g, dtype=torch.float64))
        self.c1 = torch.nn.Parameter(0.3 * torch.randn(hidden, generator=g, dtype=torch.float64))
        self.w2 = torch.nn.Parameter(0.5 * torch.randn(dim, hidden, generator=g, dtype=torch.float64))

    def forward(self, t, y):
        return torch.tanh(y @ self.w1.t() + self.b1 + t * self.c1) @ self.w2.t()


class Linear(torch.nn.Module):
    def __init__(self, dim=4, seed=1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(0.4 * torch.randn(dim, dim, generator=g, dtype=torch.float64) - 0.3 * torch.eye(dim, dtype=torch.float64))

    def forward(self, t, y):
        return y @ self.a.t()


T_OUT = [0.0, 0.02, 0.0205, 0.021, 1.1, 5.0]  # several rows inside the first steps; a long gap that some step covers without a row


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def run_steps(func, y0, t, solver, rtol=1e-5, atol=1e-7, **opts):
    steps = []

    def hook(i, y0_, y1, ks, c):
        if c.accept:
            steps.append((float(c.t0), float(c.t1), float(c.dt_last), int(c.out_begin), int(c.out_end)))

    y0 = y0.clone().requires_grad_()
    sol = odeint(func, y0, t, solver, rtol=rtol, atol=atol, options=dict(backprop="steps", norm=_rms_norm, dtype=y0.dtype, _step_hook=hook, **opts))
    w = torch.linspace(-1.0, 1.0, sol.numel(), dtype=sol.dtype, device=sol.device).reshape(sol.shape)
    params = [p for p in func.parameters()]
    loss = (sol * w).sum() + (sol**2).sum() * 0.1
    grads = torch.autograd.grad(loss, [y0] + params)
    return sol.detach(), grads, steps, w


def twin_grads(func, y0, t, name, steps, w):
    y0 = y0.clone().requires_grad_()
    sol = twin_odeint(func, y0, t, name, [(a, b, c) for a, b, c, _, _ in steps])
    loss = (sol * w).sum() + (sol**2).sum() * 0.1
    return sol.detach(), torch.autograd.grad(loss, [y0] + list(func.parameters()))


# -- validation and routing -----------------------------------------------------------------------------------------------------
def test_unknown_mode_and_fixed_adjoint_are_value_errors():
    y0 = torch.ones(2, 3)
    with pytest.raises(ValueError, match="backprop"):
        odeint(lambda t, y: -y, y0, torch.tensor([0.0, 1.0]), Dopri5, options={"norm": _rms_norm, "backprop": "through"})
    with pytest.raises(ValueError, match="odeint_adjoint"):
        odeint(lambda t, y: -y, y0, torch.tensor([0.0, 1.0]), RK4, options={"norm": _rms_norm, "backprop": "adjoint"})


def test_steps_refusals():
    f = MLP()
    y0 = torch.ones(2, 4, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="odeint_adjoint"):
        odeint(f, y0, t.clone().requires_grad_(), Dopri5, options={"norm": _rms_norm, "backprop": "steps"})
    with pytest.raises(NotImplementedError, match="tuple"):
        odeint(f, (y0, y0), t, Dopri5, options={"norm": _rms_norm, "backprop": "steps"})
    with pytest.raises(NotImplementedError, match="process_group"):
        odeint(f, y0, t, Dopri5, options={"norm": _rms_norm, "backprop": "steps", "process_group": object()})
    for pl in ("lag", "graph", "auto"):
        with pytest.raises(ValueError, match="sync"):
            odeint(f, y0, t, Dopri5, options={"norm": _rms_norm, "backprop": "steps", "pipeline": pl})


def test_key_absent_still_routes_to_the_adjoint_with_one_warning(monkeypatch):
    adj_mod = importlib.import_module("paddlexde_amd.functional.odeint_adjoint")

    calls = []
    monkeypatch.setattr(adj_mod, "odeint_adjoint", lambda *a, **k: calls.append(k) or "adjoint-result")
    monkeypatch.setattr(odeint_mod, "_ROUTE_WARNED", False)
    f = MLP()
    y0 = torch.ones(2, 4, dtype=torch.float64)
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert odeint(f, y0, t, Dopri5) == "adjoint-result"
        assert odeint(f, y0, t, Dopri5) == "adjoint-result"
    assert len(calls) == 2
    assert sum("odeint_adjoint" in str(w.message) for w in rec) == 1
    # the explicit choice: the same route, no warning
    monkeypatch.setattr(odeint_mod, "_ROUTE_WARNED", False)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert odeint(f, y0, t, Dopri5, options={"norm": _rms_norm, "backprop": "adjoint"}) == "adjoint-result"
    assert len(calls) == 3 and "backprop" not in calls[-1]["options"]
    assert not [w for w in rec if "odeint_adjoint" in str(w.message)]


def test_steps_without_a_gradient_is_a_plain_solve(cpu_double):
    f = MLP()
    y0 = torch.ones(3, 4, dtype=torch.float64)
    t = torch.tensor(T_OUT, dtype=torch.float64)
    with torch.no_grad():
        ref = odeint(f, y0, t, Dopri5)
    f.requires_grad_(False)
    out = odeint(f, y0, t, Dopri5, options={"norm": _rms_norm, "backprop": "steps"})  # nothing requires grad
    assert out.grad_fn is None and torch.equal(out, ref)
    f.requires_grad_(True)
    with torch.no_grad():
        out = odeint(f, y0.clone().requires_grad_(), t, Dopri5, options={"norm": _rms_norm, "backprop": "steps"})
    assert out.grad_fn is None and torch.equal(out, ref)
    assert "cotangent" not in cpu_double.launches


def test_steps_with_a_fixed_solver_is_accepted(cpu_double):
    f = MLP()
    y0 = torch.ones(3, 4, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64)
    a = odeint(f, y0, t, RK4, options={"norm": _rms_norm, "backprop": "steps"})
    b = odeint(f, y0, t, RK4)
    assert torch.equal(a, b) and a.grad_fn is not None


# -- the sweep against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", SOLVERS, ids=[n for _, n in SOLVERS])
@pytest.mark.parametrize("problem", ["mlp", "linear"])
def test_sweep_matches_the_twin_fp64(cpu_double, solver, name, problem):
    f = MLP() if problem == "mlp" else Linear()
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4)
    t = torch.tensor(T_OUT, dtype=torch.float64)
    sol, grads, steps, w = run_steps(f, y0, t, solver)
    assert any(oe - ob >= 2 for *_, ob, oe in steps), steps  # several rows inside one step
    assert any(oe == ob for *_, ob, oe in steps[:-1]), steps  # a step that covers none
    tsol, tgrads = twin_grads(f, y0, t, name, steps, w)
    assert rel(sol, tsol) <= 1e-12
    for a, b in zip(grads, tgrads):
        assert rel(a, b) <= 1e-12, (name, rel(a, b))


def test_sweep_reverse_time_fp64(cpu_double):
    f = MLP()
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4)
    t = torch.tensor([1.6, 1.5, 1.45, 0.7, 0.0], dtype=torch.float64)
    sol, grads, steps, w = run_steps(f, y0, t, Dopri5)
    _, tgrads = twin_grads(f, y0, t, "dopri5", steps, w)
    for a, b in zip(grads, tgrads):
        assert rel(a, b) <= 1e-12


def test_sweep_recomputes_the_forward_bit_for_bit(cpu_double):
    f = MLP()
    seen = []
    y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4)
    t = torch.tensor(T_OUT, dtype=torch.float64)
    for solver, _ in SOLVERS:
        seen.clear()
        run_steps(f, y0, t, solver, _backprop_probe=lambda n, y1, kept, ts: seen.append(torch.equal(y1, kept)))
        assert seen and all(seen)


def test_nothing_of_the_solve_outlives_backward_without_the_cycle_collector(cpu_double):
    """Every tensor an attempt made is released by reference counting alone once backward() has run and the result is gone (the
    stepper is a reference cycle: it must not be what keeps them)."""
    f = MLP()
    refs = []

    def hook(i, y0_, y1, ks, c):
        refs.extend(weakref.ref(x) for x in [y1] + list(ks[1:]))

    gc.collect()
    gc.disable()
    try:
        y0 = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).reshape(3, 4).requires_grad_()
        for solver, _ in SOLVERS:
            sol = odeint(f, y0, torch.tensor(T_OUT, dtype=torch.float64), solver,
                         options={"norm": _rms_norm, "backprop": "steps", "_step_hook": hook})
            sol.square().sum().backward()
            del sol
            assert refs and not [r for r in refs if r() is not None], solver
            refs.clear()
    finally:
        gc.enable()


# -- the C entry points without a GPU ---------------------------------------------------------------------------------------------
def test_backprop_symbols_exported_and_reject_bad_arguments():
    import ctypes as C

    lib = _hip.load_library()
    EB = _hip.XDE_EBADARG
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p).value
    xs = (C.c_void_p * 17)(*([p] * 17))
    cs = (C.c_double * 17)()
    assert lib.xde_stage_cotangent(None, None, xs, cs, None, 1, 8, 1, None) == EB
    assert lib.xde_stage_cotangent(p, None, None, cs, None, 1, 8, 1, None) == EB
    assert lib.xde_stage_cotangent(p, None, xs, cs, None, 0, 8, 1, None) == EB
    assert lib.xde_stage_cotangent(p, None, xs, cs, None, _hip.XDE_BP_MAX_X + 1, 8, 1, None) == EB
    assert lib.xde_stage_cotangent(p, p, xs, cs, None, 1, 8, 1, None) == EB  # out2 without coef2
    assert lib.xde_stage_cotangent(p, None, xs, cs, None, 1, 8, 7, None) == EB  # dtype
    assert lib.xde_stage_cotangent(p, None, xs, cs, None, 1, 8, 1, None) == EB  # out aliases x[0]
    assert b"alias" in lib.xde_last_error()
    outs = (C.c_void_p * 5)()
    assert lib.xde_dense_cotangent(None, p, cs, 1, 0, 8, 1, None) == EB
    assert lib.xde_dense_cotangent(outs, p, cs, 1, 0, 8, 1, None) == EB  # every output null
    outs[0] = p
    assert lib.xde_dense_cotangent(outs, None, cs, 1, 0, 8, 1, None) == EB
    assert lib.xde_dense_cotangent(outs, p, cs, 0, 0, 8, 1, None) == EB
    assert lib.xde_dense_cotangent(outs, p, cs, 1, 0, -1, 1, None) == EB
