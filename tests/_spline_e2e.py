"""End-to-end cases of cdeint / cdeint_adjoint on the natural cubic spline control, run on the numpy double (tests/test_spline_host.py)
and on the GPU (tests/test_gpu_spline.py) through the ``dev`` fixture of each module: the closed form of the one-channel linear CDE on
irregular knots with missing values, and the gradients through the steps of RK4 against the continuous adjoint."""
import numpy as np
import pytest
import torch

from paddlexde_amd.functional import cdeint, cdeint_adjoint
from paddlexde_amd.interpolation import NaturalCubicSpline
from paddlexde_amd.solver import RK4, Dopri5
from paddlexde_amd.utils.ode_utils import _rms_norm

from . import _spline_cases as SC
from ._cde_cases import B, H, _field, _grads
from .problems import parity_ok, worst

__all__ = ["test_the_one_channel_linear_cde_follows_its_closed_form_on_irregular_knots_with_missing_values",
           "test_gradients_through_rk4_equal_the_continuous_adjoints"]

SUBSTEPS = 32  # RK4 steps per knot interval in the gradient case


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_one_channel_linear_cde_follows_its_closed_form_on_irregular_knots_with_missing_values(dev, dtype):
    """C = 1, F = a z has z_h(t) = z_h(t0) exp(a_h (X(t) - X(t0))) for ANY path X.  Dopri5 at its default tolerances on knots of
    spacing ratio 16 with 30 % of the interior entries missing, against X.evaluate, at the bar of the existing closed-form case
    (tests/_cde_cases.py: rtol 4e-3, atol 1e-8)."""
    series, kn, a, z0 = (torch.from_numpy(x).to(dev) for x in SC.cde_problem(dtype, channels=1, share=0.3))
    assert bool(torch.isnan(series).any())
    X = NaturalCubicSpline(series, kn)
    lo, hi = float(kn[0]), float(kn[-1])
    ts = torch.linspace(lo, hi, 10, dtype=dtype)
    ts[-1] = kn[-1].cpu()  # (the rounded end stays inside the interval)
    with torch.no_grad():
        sol = cdeint(lambda t, z: z[..., None] * a, X, z0, ts.to(dev), Dopri5)  # [10, B, H]
    Xe = X.evaluate(ts).cpu().numpy().astype(np.float64)[:, :, 0]  # [B, 10]
    want = z0.cpu().numpy()[None] * np.exp(a.cpu().numpy().astype(np.float64)[None, None, :, 0] * (Xe - Xe[:, :1]).T[:, :, None])
    got = sol.cpu().numpy()
    print("closed form on the natural control, {}: worst / bar = {:.3g}".format(dtype, worst(got, want, rtol=4e-3, atol=1e-8)))
    assert got.shape == (10, B, H) and parity_ok(got, want, rtol=4e-3, atol=1e-8)


def test_gradients_through_rk4_equal_the_continuous_adjoints(dev):
    """z0's gradient and every parameter's: cdeint(RK4) against cdeint_adjoint(Dopri5), float64, parity_ok at its defaults (the
    existing gradient case's bar).  The adjoint runs as DESIGN section 11 prescribes: options["dtype"] = float64 (for the adjoint's
    solve too) and step_t = the knots.  RK4 walks SUBSTEPS = 32 equal steps per knot interval (the knots are on its grid, and the loss
    reads the solution at the knots only) with the textbook tableau, options["variant"] = "classic": the default variant is the
    reference's, which converges with h^2 on a field that depends on time (measured on the double, this problem, against 256 steps:
    4.7e-4, 1.2e-4, 2.9e-5 at 16, 32, 64 steps; the classic tableau: 5.0e-7, 3.1e-8, 1.9e-9), so no affordable grid brings it
    within rtol 1e-5 of the continuous adjoint.  At 32 steps the classic walk is within 3.1e-8 of its limit.  The adjoint solves at
    rtol 1e-9, atol 1e-11: the two routes are different discretisations, so each has to be well inside the bar on its own, and at
    the default rtol 1e-7 the adjoint's own parameter gradients sit 1.3e-5 (relative) from their limit — 64 RK4 steps instead of 32
    leave that figure where it is, the tighter adjoint brings the worst gradient to 0.21 of the bar (numpy double, this CPU)."""
    series, kn, _, z0 = (torch.from_numpy(x).to(dev) for x in SC.cde_problem(torch.float64))
    X = NaturalCubicSpline(series, kn)
    field = _field(dev)
    k64 = kn.cpu().numpy()
    fine = np.concatenate([np.linspace(k64[i], k64[i + 1], SUBSTEPS, endpoint=False) for i in range(len(k64) - 1)] + [k64[-1:]])
    fine[::SUBSTEPS] = k64  # (the knots themselves, bit for bit)
    fine_t = torch.from_numpy(fine).to(dev)
    wts = torch.randn(len(k64), B, H, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    rk4 = {"norm": _rms_norm, "dtype": torch.float64, "variant": "classic"}
    steps = lambda z: (cdeint(field, X, z, fine_t, RK4, options=rk4).reshape(len(fine), B, H)[::SUBSTEPS] * wts).sum()  # noqa: E731
    kw = dict(solver=Dopri5, rtol=1e-9, atol=1e-11, options={"norm": _rms_norm, "dtype": torch.float64, "step_t": X.grid_points.cpu()},
              adjoint_options={"graph_func": False, "dtype": torch.float64})
    adjoint = lambda z: (cdeint_adjoint(field, X, z, kn, **kw) * wts).sum()  # noqa: E731
    got, want = _grads(steps, field, z0), _grads(adjoint, field, z0)
    assert len(got) == 5
    for g, w in zip(got, want):
        print("gradients on the natural control, rk4 against the adjoint: worst / bar = {:.3g}".format(worst(g, w)))
        assert np.abs(w).max() > 0 and parity_ok(g, w)
