"""The fixed-step solvers' walk (plain, step_size, grid_constructor) on the numpy double against what the commit named in
tests/golden/fixed_walk_parent.json computed: the same solution bits, nfe, launch sequence, gradients and hook arguments, case by case
(tests/golden/make_fixed_walk.py holds the table and the runner), and the per-step state idle again after every solve."""
import json

import pytest

from paddlexde_amd import _hip

from .golden import make_fixed_walk as M

with open(M.PATH) as _fh:
    GOLDEN = json.load(_fh)


@pytest.fixture
def dev():
    from ._sde_double import SdeDoubleBackend

    _hip._set_backend_for_testing(SdeDoubleBackend())
    try:
        yield "cpu"
    finally:
        _hip._set_backend_for_testing(None)


def test_the_table_covers_every_value_in_every_mode():
    assert sorted(GOLDEN["cases"]) == sorted(c["id"] for c in M.CASES) and len(GOLDEN["parent"]) == 40
    for mode in M.MODES:
        cs = [c for c in M.CASES if c["mode"] == mode]
        ode = [c for c in cs if c["kind"] == "ode"]
        assert {c["solver"] for c in ode} == set(M.SOLVERS)
        assert {c["interp"] for c in ode} == {"linear", "cubic", ""}
        assert {c["tt"] for c in ode} == {"f32", "f64"}
        assert {"desc", "repeated"} <= {c["span"] for c in ode}
        assert {(c["shape"], c["st"]) for c in ode} >= {("1x2", "f64"), ("1x3", "f32"), ("3x2x2", "f64"), ("3x2x2", "f32")}
        assert {c["grad"] for c in ode} >= {"none", "y0", "param"} and {c["hook"] for c in ode} == {False, True}
        assert any(c.get("raises") for c in ode)
        assert {c["kind"] for c in cs} == {"ode", "sde", "dde"}
    for c in M.CASES:
        times, grid = M.SPANS[c["span"]]
        assert len(times) <= 15 and (grid is None or len(grid) <= 41)


@pytest.mark.parametrize("case", M.CASES, ids=[c["id"] for c in M.CASES])
def test_walk_equals_the_parent(dev, case):
    got, s = M.run_case(case)
    want = GOLDEN["cases"][case["id"]]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], field
    assert ("error" in got) == bool(case.get("raises"))
    for name in M.IDLE_FIELDS:  # armed only while integrate() drives step()
        assert getattr(s, name) is None, name
