"""End-to-end cases of the gradient with respect to the control path of cdeint, run on the numpy double (tests/test_cdegrad_host.py)
and on the GPU (tests/test_gpu_cdegrad.py) through the ``dev`` fixture of each module: ``series.grad`` through the steps of RK4 against
torch-CPU float64 autograd through a PLAIN-TORCH restatement of the same spline and ``einsum``, and the continuous adjoint against the
steps route.

The restatements know nothing of the kernels: the natural spline is the textbook one (per column: the nodes by the end rule, a dense
``torch.linalg.solve`` of the tridiagonal system, the textbook piecewise cubic); the linear and the cubic Hermite control are the
reference's formulas on the unit grid, where its scale conventions are exact."""
import numpy as np
import pytest
import torch

from paddlexde_amd.functional import cdeint, cdeint_adjoint
from paddlexde_amd.interpolation import CubicHermiteSpline, LinearInterpolation, NaturalCubicSpline
from paddlexde_amd.solver import RK4, Dopri5
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _spline_cases as SC
from ._cde_cases import B, C, H, T, _field, inputs
from .problems import parity_ok, worst

__all__ = ["test_series_grad_through_rk4_on_the_natural_control_equals_torch_autograd",
           "test_series_grad_through_rk4_on_the_linear_and_cubic_controls_equals_torch_autograd",
           "test_the_adjoint_gives_the_series_the_gradient_of_the_steps_route"]


class TorchNatural:
    """The natural cubic spline through the observed entries of ``series [B, Tn, C]`` (a float64 CPU tensor on the autograd graph) as
    plain torch ops."""

    def __init__(self, series, knots):
        self.cols = []
        t = knots.detach().double().cpu()
        for b in range(series.shape[0]):
            row = []
            for c in range(series.shape[2]):
                y = series[b, :, c]
                obs = torch.nonzero(~torch.isnan(y.detach())).reshape(-1).tolist()
                idx = sorted(set([0, series.shape[1] - 1] + obs))
                take = [k if k in obs else (obs[0] if k == 0 else obs[-1]) for k in idx]  # the end rule
                x, yn = t[idx], y[take]
                n = len(idx)
                A = torch.zeros(n, n, dtype=torch.float64)
                A[0, 0] = A[-1, -1] = 1.0
                rhs = [torch.zeros((), dtype=torch.float64)]
                for i in range(1, n - 1):
                    hl, hr = x[i] - x[i - 1], x[i + 1] - x[i]
                    A[i, i - 1], A[i, i], A[i, i + 1] = hl, 2.0 * (hl + hr), hr
                    rhs.append(6.0 * ((yn[i + 1] - yn[i]) / hr - (yn[i] - yn[i - 1]) / hl))
                rhs.append(torch.zeros((), dtype=torch.float64))
                row.append((x, yn, torch.linalg.solve(A, torch.stack(rhs))))
            self.cols.append(row)

    def _piece(self, x, y, M, tq, want):
        a = int(np.clip(np.searchsorted(x.numpy(), tq, side="right") - 1, 0, len(x) - 2))
        h, p, q = x[a + 1] - x[a], x[a + 1] - tq, tq - x[a]
        ca, cb = y[a] / h - M[a] * h / 6.0, y[a + 1] / h - M[a + 1] * h / 6.0
        if want == "val":
            return M[a] * p**3 / (6.0 * h) + M[a + 1] * q**3 / (6.0 * h) + ca * p + cb * q
        return -M[a] * p**2 / (2.0 * h) + M[a + 1] * q**2 / (2.0 * h) - ca + cb

    def at(self, tq, want):
        tq = float(tq)
        return torch.stack([torch.stack([self._piece(*col, tq, want) for col in row]) for row in self.cols])  # [B, C]


class TorchUnitGrid:
    """``X'(t)`` of the reference's LinearInterpolation / CubicHermiteSpline on the unit grid 0..Tn-1 as plain torch ops (index =
    clip(#{k < t} - 1, 0, Tn - 1); the cubic's node derivatives are one-sided differences, the last one repeated)."""

    def __init__(self, series, method):
        self.x, self.method, self.Tn = series, method, series.shape[1]

    def at(self, tq, want):
        assert want == "der"
        tq, Tn, x = float(tq), self.Tn, self.x
        i = int(np.clip(np.ceil(tq) - 1, 0, Tn - 1))
        i1 = min(i + 1, Tn - 1)
        if self.method == "linear":
            return x[:, i1] - x[:, i]
        s = tq - i
        d = lambda k: x[:, k + 1] - x[:, k] if k < Tn - 1 else x[:, Tn - 1] - x[:, Tn - 2]  # noqa: E731
        g0, g1, g2, g3 = 6 * s * s - 6 * s, -6 * s * s + 6 * s, 3 * s * s - 4 * s + 1, 3 * s * s - 2 * s
        return g0 * x[:, i] + g1 * x[:, i1] + g2 * d(i) + g3 * d(i + 1)


class _Composed(torch.nn.Module):
    """The CDE's vector field as framework ops on the CPU: einsum(F, X'(t)) with ``X`` one of the restatements above."""

    def __init__(self, field, X):
        super().__init__()
        self.field = field
        self.__dict__["X"] = X

    def forward(self, t, z):
        return torch.einsum("bhc,bc->bh", self.field(t, z), self.X.at(t, "der"))


def _rk4_classic(f, z0, ts):
    """The textbook RK4 walk over the grid ``ts`` (numpy float64) as plain torch ops on the CPU: ``[len(ts), B, H]``."""
    out, z = [z0], z0
    for t0, t1 in zip(ts[:-1], ts[1:]):
        h = t1 - t0
        k1 = f(t0, z)
        k2 = f(t0 + 0.5 * h, z + (0.5 * h) * k1)
        k3 = f(t0 + 0.5 * h, z + (0.5 * h) * k2)
        k4 = f(t1, z + h * k3)
        z = z + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out.append(z)
    return torch.stack(out)


def _models(dev, seed=3):
    """The field, and the linear layer that takes z0 from the control's first value; the same weights on ``dev`` and on the CPU."""
    torch.manual_seed(seed)
    init = torch.nn.Linear(C, H).double()
    there = torch.nn.Linear(C, H).double().to(dev)
    there.load_state_dict(init.state_dict())
    here_field = _field("cpu")
    return _field(dev), there, here_field, init


def _fine_grid(k64, substeps):
    fine = np.concatenate([np.linspace(k64[i], k64[i + 1], substeps, endpoint=False) for i in range(len(k64) - 1)] + [k64[-1:]])
    fine[::substeps] = k64  # (the knots themselves, bit for bit)
    return fine


def _weights(n):
    return torch.randn(n, B, H, generator=torch.Generator().manual_seed(1), dtype=torch.float64)


def test_series_grad_through_rk4_on_the_natural_control_equals_torch_autograd(dev):
    """cdeint(RK4) on NaturalCubicSpline(series.requires_grad_(), t, differentiable=True) over irregular knots with 20 % of the
    interior entries missing; the model takes z0 from X.evaluate(t0) through a linear layer, so the gather's transpose carries a term
    of the gradient too.  ``series.grad`` (and z0's layer's) against torch-CPU float64 autograd through the plain-torch restatement,
    the textbook RK4 walk (two steps per knot interval; options["variant"] = "classic") on the composed field in plain torch;
    parity_ok at its defaults.  Unobserved entries get exactly +0.  On a parent without the feature ``series.grad is None``."""
    x, kn, _, _ = SC.cde_problem(torch.float64)
    assert np.isnan(x).any()
    field, init, field_cpu, init_cpu = _models(dev)
    fine = _fine_grid(kn, 2)
    w = _weights(len(fine))
    rk4 = {"norm": _rms_norm, "dtype": torch.float64, "variant": "classic"}

    series = torch.from_numpy(x).to(dev).requires_grad_(True)
    knots = torch.from_numpy(kn).to(dev)
    X = NaturalCubicSpline(series, knots, differentiable=True)
    z0 = init(X.evaluate(knots[:1])[:, 0, :])
    sol = cdeint(field, X, z0, torch.from_numpy(fine).to(dev), RK4, options=rk4)
    (sol.reshape(len(fine), B, H) * w.to(dev)).sum().backward()
    assert series.grad is not None, "the series got no gradient through the differentiable control"

    ref = torch.from_numpy(x).requires_grad_(True)
    Xr = TorchNatural(ref, torch.from_numpy(kn))
    solr = _rk4_classic(_Composed(field_cpu, Xr), init_cpu(Xr.at(kn[0], "val")), fine)
    (solr * w).sum().backward()

    got, want = series.grad.cpu().numpy(), ref.grad.numpy()
    assert np.array_equal(got[np.isnan(x)], np.zeros(int(np.isnan(x).sum()))) and not np.signbit(got[np.isnan(x)]).any()
    print("series.grad, natural control through RK4: worst / bar = {:.3g}".format(worst(got, want)))
    assert np.abs(want).max() > 0 and parity_ok(got, want)
    for p, q in zip(list(init.parameters()) + list(field.parameters()), list(init_cpu.parameters()) + list(field_cpu.parameters())):
        assert parity_ok(p.grad.cpu().numpy(), q.grad.numpy())


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_series_grad_through_rk4_on_the_linear_and_cubic_controls_equals_torch_autograd(dev, method):
    """The same for LinearInterpolation / CubicHermiteSpline(differentiable=True) on the unit grid, z0 from the indexed series row
    through the linear layer (evaluate is refused on these: the value at a knot IS the series row)."""
    x, _, _ = inputs(torch.float64)
    field, init, field_cpu, init_cpu = _models(dev)
    fine = _fine_grid(np.arange(T, dtype=np.float64), 2)
    w = _weights(len(fine))
    rk4 = {"norm": _rms_norm, "dtype": torch.float64, "variant": "classic"}

    series = torch.from_numpy(x).to(dev).requires_grad_(True)
    X = {"linear": LinearInterpolation, "cubic": CubicHermiteSpline}[method](series, differentiable=True)
    sol = cdeint(field, X, init(series[:, 0, :]), torch.from_numpy(fine).to(dev), RK4, options=rk4)
    (sol.reshape(len(fine), B, H) * w.to(dev)).sum().backward()
    assert series.grad is not None, "the series got no gradient through the differentiable control"

    ref = torch.from_numpy(x).requires_grad_(True)
    solr = _rk4_classic(_Composed(field_cpu, TorchUnitGrid(ref, method)), init_cpu(ref[:, 0, :]), fine)
    (solr * w).sum().backward()
    got, want = series.grad.cpu().numpy(), ref.grad.numpy()
    print("series.grad, {} control through RK4: worst / bar = {:.3g}".format(method, worst(got, want)))
    assert np.abs(want).max() > 0 and parity_ok(got, want)


def test_the_adjoint_gives_the_series_the_gradient_of_the_steps_route(dev):
    """cdeint_adjoint(Dopri5) against cdeint(RK4) on the same problem (the natural control, irregular knots, 20 % missing, z0 through
    the gather), for ``series.grad``, z0's layer and the field's parameters, at the bar and with the settings of
    tests/_spline_e2e.py's adjoint-against-steps comparison: options["dtype"] = float64 and step_t = the knots,
    rtol 1e-9 / atol 1e-11 for the adjoint, 32 classic RK4 steps per knot interval; parity_ok at its defaults.  The coefficient
    backward launches ONCE per backward pass (asserted on the double's launch record where there is one)."""
    from paddlexde_amd import _hip

    x, kn, _, _ = SC.cde_problem(torch.float64)
    field, init, _, _ = _models(dev)
    params = list(init.parameters()) + list(field.parameters())
    knots = torch.from_numpy(kn).to(dev)
    fine = _fine_grid(kn, 32)
    w = _weights(len(kn)).to(dev)
    launches = getattr(_hip.get_backend(), "launches", None)

    def grads(route):
        series = torch.from_numpy(x).to(dev).requires_grad_(True)
        for p in params:
            p.grad = None
        X = NaturalCubicSpline(series, knots, differentiable=True)
        z0 = init(X.evaluate(knots[:1])[:, 0, :])
        if route == "steps":
            sol = cdeint(field, X, z0, torch.from_numpy(fine).to(dev), RK4,
                         options={"norm": _rms_norm, "dtype": torch.float64, "variant": "classic"}).reshape(len(fine), B, H)[::32]
        else:
            sol = cdeint_adjoint(field, X, z0, knots, solver=Dopri5, rtol=1e-9, atol=1e-11,
                                 options={"norm": _rms_norm, "dtype": torch.float64, "step_t": X.grid_points.cpu()},
                                 adjoint_options={"dtype": torch.float64})
        if launches is not None:
            del launches[:]
        (sol * w).sum().backward()
        if launches is not None:
            assert launches.count("spline_natural_coeffs_backward") == 1, route
            assert launches.count("spline_natural_gather_backward") == 1, route
            assert launches.count("cde_control_grad_natural") > 1, route
        return [series.grad.cpu().numpy()] + [p.grad.cpu().numpy().copy() for p in params]

    got, want = grads("adjoint"), grads("steps")
    for g, r in zip(got, want):
        print("adjoint against the steps route: worst / bar = {:.3g}".format(worst(g, r)))
        assert np.abs(r).max() > 0 and parity_ok(g, r)
