"""The refusals of the control kernels' 13 entry points (include/xde_hip_cde.h, xde_hip_spline.h, xde_hip_cdegrad.h) against
tests/golden/cde_arg_refusals_parent.json: the return code and the message, character for character, for every single fault the host
tests use and for every pair of faults of two different rules — so the message that wins when two arguments are wrong at once stays
the one the recorded commit gave (tests/golden/make_cde_arg_refusals.py holds the table and the caller).  No GPU: every call is
refused on the host or enqueues nothing."""
import json

import pytest

from paddlexde_amd import _hip

from .golden import make_cde_arg_refusals as M

with open(M.PATH) as _fh:
    GOLDEN = json.load(_fh)


def test_the_table_covers_the_three_headers():
    assert len(M.ENTRIES) == 13 and set(M.ENTRIES) == set(GOLDEN["cases"])
    assert set(M.ENTRIES) == set(_hip.HEADERS["xde_hip_cde.h"]) | set(_hip.HEADERS["xde_hip_spline.h"]) | set(_hip.HEADERS["xde_hip_cdegrad.h"])
    for name in M.ENTRIES:
        r = M.rules(name)
        assert {M.case_id(dict(a, **b)) for a in r.values() for b in r.values() if not set(a) & set(b)} <= set(GOLDEN["cases"][name])


@pytest.mark.parametrize("name", sorted(M.ENTRIES))
def test_every_recorded_refusal_replays_exactly(name):
    lib = _hip.load_library()
    want = GOLDEN["cases"][name]
    cases = M.cases(name)
    assert {M.case_id(c) for c in cases} == set(want)
    wrong = []
    for c in cases:
        rc, at = want[M.case_id(c)]
        # (a call that is not refused would go on to launch on the fake pointers: only the queries, which enqueue nothing, may succeed)
        assert rc != _hip.XDE_OK or name in M.QUERIES, (name, c)
        got = M.call(lib, name, c)
        if got != (rc, GOLDEN["messages"][at]):
            wrong.append((M.case_id(c), got, (rc, GOLDEN["messages"][at])))
    assert wrong == []
