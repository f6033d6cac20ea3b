"""The numpy double's step controller (tests/_cpu_double.py: `ctrl_init`, `rk_control`) held to the ORACLE's controller, attempt by
attempt, over the scripts of tests/_controller_scripts.py — no GPU.  tests/test_gpu_controller_kernels.py then holds the kernels to
the double bit for bit; together the two say that the kernels run the oracle's controller.

The oracle's `AdaptiveRKSolver` takes a `norm` callable: with `func = 0`, a one-element state, an explicit `first_step` and a `norm`
that returns the script's next ratio, its own control code (`_adaptive_step`, `step()`, the `step_t` bookkeeping) runs on prescribed
error ratios and records `(t0, dt, ratio, accept)` per attempt; the stage times are the times it hands to `func`.

The oracle has no reverse time, no replay table and makes no attempt after the last output: the reverse-time twin of every script
must be the exact negation of the forward run, and replay / after-done behaviour is stated here in plain Python without the double.
"""
import numpy as np
import pytest

from oracle import xde_oracle as xo
from paddlexde_amd import _hip

from . import _controller_scripts as S
from ._controller_drivers import SENTINEL, fields, run_double, same

TIME_FIELDS = ("t0", "t1", "dt", "dt_last", "t_plan")
NPT = S.TT


def run_oracle(s):
    """The oracle's controller over script `s`: (trace, stage times per attempt, error text or None, n_accept, n_reject)."""
    T, Y = NPT[s.tdt], NPT[s.sdt]
    used, times = [], []

    def norm(_x):
        r = Y(s.stated_ratio(len(used))[0])  # (IndexError past the script's end)
        used.append(r)
        return r

    def func(t, y):
        times.append(t)
        return np.zeros_like(y)

    o = xo.AdaptiveRKSolver(func, np.zeros(1, dtype=Y), 1e-3, 1e-6, method=s.method, norm=norm, first_step=s.first_step, step_t=s.step_t,
                            min_step=s.min_step, max_step=s.max_step, max_num_steps=s.max_num_steps, dtype=T, safety=s.safety,
                            ifactor=s.ifactor, dfactor=s.dfactor, controller="PI" if s.pi else "I", pi_beta=s.pi_beta)
    err = None
    try:
        o.integrate(np.asarray(s.t_span))
    except AssertionError as e:
        err = str(e)
    except IndexError:
        err = "script ran out"
    n_stage = len(s.alpha)
    per_attempt = [times[1 + i * n_stage : 1 + (i + 1) * n_stage] for i in range(len(o.trace))]  # (times[0]: f0 before the first step)
    return o.trace, per_attempt, err, o.n_accept, o.n_reject


ORACLE_SCRIPTS = [s for s in S.SCRIPTS if s.replay is None]


def test_ratio_filter_is_within_its_cap():
    """The fp32 draws the filter replaced (libm powf not the correctly rounded power): reported, and at most 1% of the draws."""
    st = S.FILTER_STATS
    print("fp32 draws filtered: {rejected} of {drawn}".format(**st))
    assert st["drawn"] > 1000 and st["rejected"] <= 0.01 * st["drawn"], st
    assert len(S.RANDOM) >= 200 and all(40 <= len(s.attempts) <= 80 for s in S.RANDOM)
    assert {(s.tdt, s.sdt) for s in S.RANDOM} == set(S.COMBOS)


@pytest.mark.parametrize("chunk", range(6))
def test_double_equals_oracle_attempt_by_attempt(chunk):
    """(t0, dt, ratio, accept) and the stage times of every attempt the oracle makes; n_accept / n_reject; the status mapping:
    `underflow in dt` <-> DT_UNDERFLOW and `max_num_steps exceeded` <-> MAX_STEPS on the attempt where the oracle asserts (and not
    before), a clean finish <-> done = 1 with STATUS_OK."""
    total = rejected = 0
    for s in ORACLE_SCRIPTS[chunk::6]:
        Y = NPT[s.sdt]
        trace, o_stage, err, n_acc, n_rej = run_oracle(s)
        blocks, stages = run_double(s)
        m = len(trace)
        assert m <= len(s.attempts), s.id
        for i, rec in enumerate(trace):
            before, after = blocks[i], blocks[i + 1]
            got = (before.t1, before.dt, after.ratio, bool(after.accept))
            assert same(tuple(rec), got), (s.id, i, tuple(rec), got)
            assert (after.t0, after.dt_last) == (rec.t0, rec.dt), (s.id, i)
            want_stage = np.array([Y(t) for t in o_stage[i]], dtype=Y)
            assert stages[i][: len(s.alpha)].tobytes() == want_stage.tobytes(), (s.id, i, stages[i], want_stage)
            assert (stages[i][len(s.alpha):] == SENTINEL).all(), s.id
            total += 1
            rejected += not rec.accept
        end = blocks[m]
        assert (end.n_accept, end.n_reject, end.n_steps) == (n_acc, n_rej, m), (s.id, err)
        had_nf = any(sum(nfs) > 0 for _v, nfs in s.attempts[:m])
        clean = _hip.STATUS_NONFINITE if had_nf else _hip.STATUS_OK
        if err is None:
            assert (end.done, end.status) == (1, clean), (s.id, end.done, end.status)
        else:
            want = {"underflow": _hip.STATUS_DT_UNDERFLOW, "max_num_steps": _hip.STATUS_MAX_STEPS, "script ran out": clean}
            key = next(k for k in want if err.startswith(k))
            assert (end.done, end.status) == (0, want[key]), (s.id, err, end.done, end.status)
            if m and not had_nf:
                assert blocks[m - 1].status == _hip.STATUS_OK, (s.id, "status set before the oracle asserts")
    assert total > 300 and rejected > 50, (total, rejected)


def test_witnesses_of_the_fixed_scripts():
    """Each fixed script reaches the branch it was written for (a table that drifted away from its purpose would test nothing)."""
    runs = {s.id: (s, run_double(s)[0]) for s in S.FIXED}

    def of(name, combo="[tf64-yf64]"):
        return runs[name + combo]

    for combo in ("[tf32-yf32]", "[tf32-yf64]", "[tf64-yf32]", "[tf64-yf64]"):
        s, b = of("forced_min_accept", combo)
        assert b[1].dt == s.min_step and (b[2].accept, b[2].ratio > 1, b[2].dt_last) == (1, True, s.min_step), combo
        s, b = of("forced_max_reject", combo)
        assert (b[1].accept, b[1].ratio < 1, b[1].dt) == (0, True, s.max_step) and b[2].accept == 1, combo
        s, b = of("step_t_inside_reject_and_row", combo)
        assert (b[0].on_step_t, b[0].next_step_index, b[0].dt) == (1, 2, 1 / 32), combo  # init: two entries skipped, first step clipped
        assert (b[1].accept, b[1].next_step_index) == (0, 2), combo  # rejected on a clipped step: the index stays
        rows = [x for x in b[1:] if x.out_end > x.out_begin]
        assert rows and rows[0].t1 == 0.25 and rows[0].next_step_index == 4, combo  # a row time equal to t1, reached by a clipped step
        assert max(x.next_step_index for x in b) == 4 and sum(x.on_step_t for x in b) >= 4, combo
        s, b = of("step_t_equal_to_step_end", combo)
        assert b[0].on_step_t == 0 and b[0].t_plan == 1 / 16, combo
        s, b = of("step_t_clamp", combo)
        assert b[0].on_step_t == 1 and b[1].accept == 1 and all(x.next_step_index == 0 for x in b), combo
        s, b = of("step_t_all_before_start", combo)
        assert b[0].next_step_index == 2 and not any(x.on_step_t for x in b), combo
        s, b = of("five_rows_in_one_step", combo)
        assert (b[1].out_begin, b[1].out_end) == (1, 6), combo
        s, b = of("repeated_rows", combo)
        assert b[0].next_out == 2 and (b[1].out_begin, b[1].out_end) == (2, 5), combo
        s, b = of("all_rows_at_start", combo)
        assert b[0].done == 1 and b[0].next_out == 3, combo
        s, b = of("max_steps_3", combo)
        assert [x.status for x in b].count(_hip.STATUS_MAX_STEPS) >= 1 and b[3].steps_in_interval == 0 and b[3].status == 0, combo
        s, b = of("max_steps_1", combo)
        assert [x.status for x in b[:4]] == [0, 0, 0, _hip.STATUS_MAX_STEPS], combo
        s, b = of("underflow_at_one", combo)
        assert b[-1].status == _hip.STATUS_DT_UNDERFLOW, combo
        s, b = of("sticky_nonfinite", combo)
        assert [x.status for x in b] == [0, 0, 0] + [_hip.STATUS_NONFINITE] * 5 and b[3].nonfinite == 2.0 and b[4].nonfinite == 0.0, combo
        s, b = of("pi_prev_floor_and_accept_only", combo)
        assert b[1].ratio_prev == float(NPT[s.sdt](S.G)) and b[4].ratio_prev == S.H and b[4].accept == 0 and b[5].dt == b[4].dt, combo
        s, b = of("pi_accepted_nan", combo)
        assert b[3].accept == 1 and b[3].ratio != b[3].ratio and b[3].ratio_prev == S.H, combo
        s, b = of("ring_wrap", combo)
        assert b[-1].seq == 48, combo
    for combo in ("[tf32-yf32]", "[tf32-yf64]"):
        s, b = of("underflow_at_zero", combo)
        first = next(i for i, x in enumerate(b) if x.status)
        assert first == 61 and b[first].status == _hip.STATUS_DT_UNDERFLOW and 0 < abs(b[first - 1].dt) < 1.2e-38, (combo, first)


@pytest.mark.parametrize("chunk", range(4))
def test_reverse_time_is_the_negated_forward_run(chunk):
    """`direction = -1` with negated tables: every time-like field and stage time is the exact negation of the forward run's, every
    other field is equal, after init and after every attempt."""
    for s in S.SCRIPTS[chunk::4]:
        fwd_b, fwd_s = run_double(s)
        rev_b, rev_s = run_double(s.reversed())
        for i, (a, b) in enumerate(zip(fwd_b, rev_b)):
            fa, fb = fields(a), fields(b)
            for f in fa:
                want = -fa[f] if f in TIME_FIELDS else fa[f]
                assert same(want, fb[f]), (s.id, i, f, fa[f], fb[f])
            n = len(s.alpha)
            assert np.array_equal(-fwd_s[i][:n], rev_s[i][:n], equal_nan=True), (s.id, i)


def test_replay_table_stated_without_the_double():
    """While the table lasts: attempt i's verdict is the table's, the next attempt's step is the table's next entry (the last entry's
    attempt keeps the controller's own next step); the error ratio stays the measured one; afterwards the controller decides."""
    for s in (x for x in S.FIXED if x.replay is not None):
        T = NPT[s.tdt]
        blocks, _ = run_double(s)
        n_rep = len(s.replay)
        assert blocks[0].dt == s.replay[0][0] != s.first_step, s.id
        t = T(s.t_span[0])
        for i in range(len(s.attempts)):
            c, ratio = blocks[i + 1], s.stated_ratio(i)[0]
            assert same(c.ratio, ratio) and c.n_steps == i + 1, (s.id, i)
            if i < n_rep:
                dt, acc = T(s.replay[i][0]), int(s.replay[i][1])
                t1 = T(t + dt) if acc else t
                assert (c.accept, c.t0, c.t1, c.dt_last) == (acc, float(t), float(t1), float(dt)), (s.id, i)
                if i + 1 < n_rep:
                    assert c.dt == s.replay[i + 1][0], (s.id, i)
                t = t1
            else:
                assert c.accept == int(ratio <= 1.0), (s.id, i)
        accepted_above_one = any(s.replay[i][1] and s.stated_ratio(i)[0] > 1 for i in range(min(n_rep, len(s.attempts))))
        rejected_below_one = any(not s.replay[i][1] and s.stated_ratio(i)[0] < 1 for i in range(min(n_rep, len(s.attempts))))
        assert accepted_above_one and rejected_below_one, s.id


def test_launches_after_done_are_no_ops():
    """After `done`: `seq` counts the launch, `accept = 0`, no rows (`out_begin = out_end = next_out`), every other field and the stage
    times as they were."""
    seen = 0
    for s in (x for x in S.FIXED if x.name in ("after_done", "all_rows_at_start")):
        blocks, stages = run_double(s)
        for i in range(1, len(blocks)):
            if not blocks[i - 1].done:
                continue
            seen += 1
            before, after = fields(blocks[i - 1]), fields(blocks[i])
            want = dict(before, seq=before["seq"] + 1, accept=0, out_begin=before["next_out"], out_end=before["next_out"])
            assert all(same(want[f], after[f]) for f in want), (s.id, i, want, after)
            assert stages[i].tobytes() == stages[i - 1].tobytes(), (s.id, i)
    assert seen >= 6 * 4
