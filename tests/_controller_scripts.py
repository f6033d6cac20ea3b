"""The case table of the step-controller tests (tests/test_controller_double_host.py, tests/test_gpu_controller_kernels.py): pure data,
no GPU import.

A SCRIPT prescribes everything one solve's controller launches see — the parameters, the output times, the forced step times, the
first step, optionally a replay table — and, per attempt, the per-segment sums (`vals`, `nfs`) a norm pass would have left.  With
`NORM_LINF`, `n_seg = 1` and `vals = [r]` the attempt's error ratio is `r` itself, so a script is a list of error ratios; the
oracle's `AdaptiveRKSolver` runs the same list through a `norm` callable that returns the next entry.  Every time-like value is rounded
to the script's time dtype here, as the host does before it hands them to the kernels.

RATIO POLICY (why a free-running comparison can be exact).  The step factor is `min(ifactor, max(safety / r**e, dfactor))`; `pow` is
the one operation whose result differs between implementations (device double pow, glibc pow, glibc powf: none correctly rounded).
  * fp64-time scripts use POW-FREE ratios only: 0, NaN, inf, exactly 1 (pow(1, e) == 1), or a ratio at least 1e-3 (relative) inside
    a range where the clamp decides: HOLD (factor exactly 1: `safety**(1/e) < r < 1`), GROW (factor exactly `ifactor`), SHRINK
    (factor exactly `dfactor`).  For the PI controller the ranges hold for every `ratio_prev` in [1e-4, 1], and exactly 1 is NOT
    pow-free (its factor is `safety * prev**beta`), so PI scripts in fp64 time do not use it.
  * fp32-time scripts also draw UNCLAMPED ratios.  The kernel's fp32 power is a double pow rounded once (the correctly rounded fp32
    power but for ~2^-29 of the cases); the double and the oracle use libm powf (numpy's scalar `float32 ** float32`).  A draw is kept
    only if libm powf returns the correctly rounded value (mpmath) for every power the draw can enter: `r**e`, for PI `r**alpha` and
    `r**beta` (an accepted ratio is the next attempt's `prev`).  Rejected draws are replaced from the same stream; `FILTER_STATS`
    counts them and the module asserts that at most 1% were rejected.
"""
import numpy as np
from mpmath import mp, mpf, power as _mp_power

TT = {"f32": np.float32, "f64": np.float64}
COMBOS = [("f32", "f32"), ("f32", "f64"), ("f64", "f32"), ("f64", "f64")]  # (time dtype, state dtype)
NORM_RMS, NORM_LINF = 0, 1
NO_LIMIT = 2**31 - 1

# alpha of the tableaus (oracle/xde_oracle.py ADAPTIVE; stated here so that this module stays data)
ALPHA = {
    "dopri5": (5, [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]),
    "bosh3": (3, [1 / 2, 3 / 4, 1.0]),
    "fehlberg2": (2, [1 / 2, 1.0]),
}
TRIPLES = [(0.9, 10.0, 0.2), (0.8, 3.0, 0.5)]  # (safety, ifactor, dfactor)
PI_BETA = 0.04

FILTER_STATS = {"drawn": 0, "rejected": 0, "mpmath": 0}
_cr_cache = {}


def _dopri8_alpha():
    from oracle import dopri8_data  # (coefficients only)

    return [float(a) for a in dopri8_data.ALPHA]


ALPHA["dopri8"] = (8, _dopri8_alpha())


def powf_is_correctly_rounded(r32, e32):
    """Whether libm's powf (numpy scalar `**`) returns the correctly rounded float32 power.  The correctly rounded value is the
    float64 pow (off by an ulp of float64 at most) rounded once, unless that lies within 2^-20 of a float32 ulp of a rounding
    midpoint: then mpmath at 120 bits, rounded once to 24, decides."""
    key = (float(r32), float(e32))
    hit = _cr_cache.get(key)
    if hit is None:
        with np.errstate(all="ignore"):
            x = np.float64(key[0]) ** np.float64(key[1])
            cr = np.float32(x)
            off = abs(float(x) - float(cr)) / float(np.spacing(cr))  # 0 .. 0.5 float32 ulp from the nearest float32
            if not np.isfinite(x) or abs(off - 0.5) < 2.0**-20:
                FILTER_STATS["mpmath"] += 1
                with mp.workprec(120):
                    y = _mp_power(mpf(key[0]), mpf(key[1]))
                with mp.workprec(24):
                    cr = np.float32(float(+y))
            hit = _cr_cache[key] = bool(np.float32(r32) ** np.float32(e32) == cr)
    return hit


class Script:
    """One scripted solve (see the module docstring).  `attempts`: list of (vals, nfs), each a list of `n_seg` floats."""

    def __init__(self, name, tdt, sdt, t_span, first_step, attempts, *, method="dopri5", triple=TRIPLES[0], min_step=0.0,
                 max_step=float("inf"), max_num_steps=NO_LIMIT, pi=False, norm_kind=NORM_LINF, seg_count=(1.0,), step_t=None,
                 replay=None, direction=1):
        T = TT[tdt]
        self.name, self.tdt, self.sdt, self.method = name, tdt, sdt, method
        self.order, self.alpha = ALPHA[method]
        self.safety, self.ifactor, self.dfactor = (float(T(x)) for x in triple)
        self.min_step, self.max_step = float(T(min_step)), float(T(max_step))
        self.max_num_steps, self.pi, self.pi_beta = int(max_num_steps), bool(pi), PI_BETA
        self.norm_kind, self.seg_count, self.n_seg = norm_kind, [float(c) for c in seg_count], len(seg_count)
        self.t_span = [float(T(t)) for t in t_span]
        self.step_t = None if step_t is None else [float(T(t)) for t in step_t]
        self.first_step = float(T(first_step))
        self.replay = None if replay is None else [(float(T(dt)), 1.0 if acc else 0.0) for dt, acc in replay]
        self.direction = direction
        self.attempts = [(list(map(float, v)), list(map(float, f))) for v, f in attempts]
        for v, f in self.attempts:
            assert len(v) == self.n_seg and len(f) == self.n_seg

    @property
    def id(self):
        return "{}[t{}-y{}{}]".format(self.name, self.tdt, self.sdt, "-rev" if self.direction < 0 else "")

    def reversed(self):
        """The reverse-time twin: every time-like input negated, `direction = -1` (the contract: the controller on the flipped problem)."""
        s = Script.__new__(Script)
        s.__dict__.update(self.__dict__)
        s.t_span = [-t for t in self.t_span]
        s.step_t = None if self.step_t is None else [-t for t in self.step_t]
        s.first_step = -self.first_step
        s.replay = None if self.replay is None else [(-dt, acc) for dt, acc in self.replay]
        s.direction = -self.direction
        return s

    def stated_ratio(self, i):
        """Attempt i's error ratio, stated from its sums: per segment `|Y(sqrt(Y(sum / count)))|` (RMS) or `|Y(max)|` (LINF) in the
        state dtype Y, then the maximum over the segments with a NaN winning.  Returns (ratio, per-segment ratios)."""
        Y = TT[self.sdt]
        per = []
        with np.errstate(all="ignore"):
            for v, n in zip(self.attempts[i][0], self.seg_count):
                r = Y(np.sqrt(Y(np.float64(v) / np.float64(n)))) if self.norm_kind == NORM_RMS else Y(v)
                per.append(float(abs(r)))
        ratio = per[0]
        for r in per[1:]:
            if ratio != ratio:
                break
            ratio = r if (r != r or r > ratio) else ratio
        return ratio, per


def build_params(hip, s, replay_ptr=None):
    """`xde_ctrl_params_t` of script `s` (`hip`: the paddlexde_amd._hip module; `replay_ptr`: where the caller put the replay table,
    as 2 * n_replay doubles, in the memory the backend reads)."""
    p = hip.XdeCtrlParams()
    p.rtol, p.atol = 1e-3, 1e-6
    p.min_step, p.max_step = s.min_step, s.max_step
    p.safety, p.ifactor, p.dfactor, p.order = s.safety, s.ifactor, s.dfactor, float(s.order)
    p.max_num_steps = s.max_num_steps
    p.time_dtype = hip.XDE_F32 if s.tdt == "f32" else hip.XDE_F64
    p.state_dtype = hip.XDE_F32 if s.sdt == "f32" else hip.XDE_F64
    p.direction, p.norm_kind, p.n_stage, p.n_seg = s.direction, s.norm_kind, len(s.alpha), s.n_seg
    p.n_step_t = 0 if s.step_t is None else len(s.step_t)
    p.pi_controller, p.pi_beta = int(s.pi), s.pi_beta
    for i, a in enumerate(s.alpha):
        p.alpha[i] = a
    for i, c in enumerate(s.seg_count):
        p.seg_count[i] = c
    if s.replay is not None:
        assert replay_ptr
        p.replay, p.n_replay = replay_ptr, len(s.replay)
    return p


def replay_flat(s):
    return [x for row in s.replay for x in row]


# ------------------------------------------------------------------------------------------------------------------------------
# the pow-free ratio classes
# ------------------------------------------------------------------------------------------------------------------------------
def ratio_ranges(order, triple, pi):
    """(hold_lo, grow_hi, shrink_lo): HOLD = (hold_lo, 1), GROW = (0, grow_hi], SHRINK = [shrink_lo, inf); each bound 1e-3 inside."""
    safety, ifactor, dfactor = triple
    if not pi:
        return safety**order * (1 + 1e-3), (safety / ifactor) ** order * (1 - 1e-3), (safety / dfactor) ** order * (1 + 1e-3)
    a = 1.0 / order - 0.75 * PI_BETA  # prev in [1e-4, 1]: prev**beta in [1e-4**beta, 1]
    lo = 1e-4**PI_BETA
    return safety ** (1 / a) * (1 + 1e-3), (safety * lo / ifactor) ** (1 / a) * (1 - 1e-3), (safety / dfactor) ** (1 / a) * (1 + 1e-3)


H, G, R = 0.875, 1e-30, 1e30  # HOLD, GROW, SHRINK for every tableau / triple / controller of this table (asserted below)
for _m, (_o, _a) in ALPHA.items():
    for _t in TRIPLES:
        for _pi in (False, True):
            _lo, _g, _s = ratio_ranges(_o, _t, _pi)
            assert _lo < H < 1 and G < _g and R > _s, (_m, _t, _pi)
NAN, INF = float("nan"), float("inf")


def _r(*ratios, nf=0.0):
    """Attempts of a one-segment LINF script from plain ratios."""
    return [([x], [nf]) for x in ratios]


def _fixed():
    out = []

    def add(name, t_span, first, attempts, combos=COMBOS, **kw):
        for tdt, sdt in combos:
            att = attempts(tdt, sdt) if callable(attempts) else attempts
            out.append(Script(name, tdt, sdt, t_span, first, att, **kw))

    # ---- ratio edges: exactly 0 (ifactor without pow), exactly 1 (accepted, dfactor NOT reset: factor = safety), one ulp below 1 (factor
    # 1), NaN (rejected, factor dfactor), +inf (rejected, factor dfactor)
    below = lambda sdt: float(np.nextafter(TT[sdt](1), TT[sdt](0)))
    above = lambda sdt: float(np.nextafter(TT[sdt](1), TT[sdt](2)))
    add("ratio_edges", [0.0, 100.0], 1 / 64, lambda tdt, sdt: _r(0.0, 1.0, H, below(sdt), NAN, INF, G, 1.0, NAN, 0.0, R, H))
    add("ratio_edges_bosh3", [0.0, 100.0], 1 / 64, lambda tdt, sdt: _r(1.0, 0.0, below(sdt), INF, NAN, 1.0, H), method="bosh3", triple=TRIPLES[1])
    # one ulp above 1 (rejected; the power is not 1): free-running in fp32 time (filtered below like every fp32 draw), and in fp64 time
    # with the next step clipped to min_step, which makes it independent of the power
    add("ratio_above_one", [0.0, 100.0], 1 / 64, lambda tdt, sdt: _r(above(sdt), H, above(sdt), 1.0), combos=COMBOS[:2])
    add("ratio_above_one_clipped", [0.0, 100.0], 1 / 64, lambda tdt, sdt: _r(above(sdt), above(sdt), H), min_step=0.015, max_step=1.0)
    # ---- several segments, one NaN segment: ratio_seg[] and the NaN-propagating max
    seg_attempts = [([4 * 0.25, 9 * 0.5625, 16 * 0.0625], [0.0] * 3), ([1.0, NAN, 1.0], [0.0] * 3), ([4e60, 9 * 0.5625, 1.0], [0.0] * 3),
                    ([0.0, 0.0, 0.0], [0.0] * 3), ([NAN, 4.0, INF], [0.0] * 3), ([1.0, 2.25, 16 * 0.5625], [0.0, 0.0, 0.0])]
    add("three_segments_rms", [0.0, 100.0], 1 / 64, seg_attempts, norm_kind=NORM_RMS, seg_count=(4.0, 9.0, 16.0))
    lin_attempts = [([0.25, H, 0.5], [0.0] * 3), ([0.5, NAN, R], [0.0] * 3), ([R, 0.0, G], [0.0] * 3), ([0.0, 0.0, 0.0], [0.0] * 3),
                    ([G, G, H], [0.0] * 3), ([H, INF, NAN], [0.0] * 3)]
    add("three_segments_linf", [0.0, 100.0], 1 / 64, lin_attempts, seg_count=(4.0, 9.0, 16.0))
    # ---- forced decisions: the clip makes dt exactly min_step, then `dt <= min_step` accepts a ratio above 1; a first step above
    # max_step is rejected with a ratio below 1
    add("forced_min_accept", [0.0, 1.0], 0.04, _r(R, R, NAN, H, G, G, H, R), min_step=0.01, max_step=0.2)
    add("forced_max_reject", [0.0, 1.0], 0.5, _r(H, H, G, H, R, H), min_step=0.01, max_step=0.2)
    # ---- step_t
    # entries at or before t_start (skipped by init); an entry inside the first step (clipped) whose attempt is REJECTED (the index
    # stays); the same entry met again and accepted; an entry that is also an output time (1/4: the row's time equals t1); the last
    # entry reached by a clipped step (the index is clamped at n_step_t - 1)
    add("step_t_inside_reject_and_row", [0.0, 0.25, 1.0], 1 / 16, _r(R, H, G, H, G, H, H, G, H, H, G, H),
        step_t=[-1.0, 0.0, 1 / 32, 0.25, 0.375])
    # an entry exactly equal to t0 + dt is not clipped (strict <)
    add("step_t_equal_to_step_end", [0.0, 1.0], 1 / 16, _r(H, H, G, H), step_t=[1 / 16])
    # one entry, met twice by clipped steps would need index n_step_t: more clipped steps than entries
    add("step_t_clamp", [0.0, 1.0], 1 / 16, _r(H, H, R, H, G, H, H), step_t=[1 / 32])
    add("step_t_all_before_start", [0.5, 1.0], 1 / 16, _r(H, H, G, H), step_t=[0.125, 0.25, 0.5])
    # ---- output times
    add("five_rows_in_one_step", [0.0, 0.01, 0.02, 0.03, 0.04, 0.05, 1.0], 1 / 16, _r(H, G, H, H))
    add("repeated_rows", [0.0, 0.0, 0.05, 0.05, 0.05, 0.5, 0.5], 1 / 16, _r(H, R, H, G, H, H))
    add("all_rows_at_start", [0.5, 0.5, 0.5], 1 / 16, _r(H, R, G))
    # ---- max_num_steps: 3 attempts without a row; the count restarts when a row is emitted
    add("max_steps_3", [0.0, 0.1, 0.2, 1.0], 0.04, _r(H, H, H, H, H, H, H, H, H, H), max_num_steps=3)
    add("max_steps_1", [0.0, 0.1, 0.2, 1.0], 0.1, _r(H, H, H, H, H), max_num_steps=1)
    # ---- dt underflow: ratio 1e30 from 1e-3; at t0 = 0 in fp32 time the steps run down through the subnormals
    add("underflow_at_zero", [0.0, 1.0], 1e-3, _r(*[R] * 66), combos=COMBOS[:2])
    add("underflow_at_one", [1.0, 2.0], 1e-3, _r(*[R] * 30))
    # ---- sticky status: a non-finite count in attempt 3, attempts go on
    add("sticky_nonfinite", [0.0, 100.0], 1 / 64, _r(H, G) + _r(H, nf=2.0) + _r(R, H, G, H))
    # ---- PI controller: ratio_prev floored at 1e-4 (accepted G), updated on accept only (the rejected R must not become `prev`: with it
    # the HOLD attempt that follows would grow by ifactor), not updated by an accepted NaN (forced by min_step)
    add("pi_prev_floor_and_accept_only", [0.0, 100.0], 1 / 64, _r(G, H, H, R, H, R, R, H, 0.0, H, G, H), pi=True)
    add("pi_accepted_nan", [0.0, 100.0], 0.04, _r(H, R, NAN, H, NAN, H, G, H), pi=True, min_step=0.01, max_step=10.0)
    # ---- replay table: shorter than the script (the controller takes over) and longer; a replayed accept with ratio > 1 and a
    # replayed reject with ratio < 1
    tab = [(1 / 64, 1), (1 / 32, 0), (1 / 128, 1), (1 / 16, 1)]
    add("replay_short", [0.0, 0.03125, 100.0], 1 / 8, _r(R, H, G, NAN, H, G, H, R), replay=tab)
    add("replay_long", [0.0, 0.03125, 100.0], 1 / 8, _r(R, H, G), replay=tab + [(1 / 4, 0), (1 / 2, 1)])
    # ---- launches after done
    add("after_done", [0.0, 0.05], 1 / 16, _r(H, H, R, G))
    # ---- the 16-slot mirror ring wrapped three times
    add("ring_wrap", [0.0, 1e6], 1 / 64, _r(*([H, G, R, H, R, H, 0.0, R] * 6)))
    return out


def _random(count=200, seed=20240607):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        tdt, sdt = COMBOS[i % 4]
        T, Y = TT[tdt], TT[sdt]
        method = ["dopri5", "bosh3", "dopri8", "fehlberg2"][(i // 4) % 4]
        order = ALPHA[method][0]
        triple = TRIPLES[(i // 16) % 2]
        pi = i % 5 == 0
        kw = {}
        if i % 7 == 0:
            kw.update(min_step=0.01 if not (pi and tdt == "f64") else 0.0, max_step=0.2)
        if i % 11 == 0:
            kw["max_num_steps"] = 3
        t_span = np.sort(np.concatenate([[0.0], rng.uniform(0, 4, 5)]))
        if i % 3 == 0:
            t_span[2] = t_span[1]
        step_t = None
        if i % 4 < 2 or i % 9 == 0:
            step_t = sorted(list(rng.uniform(-0.5, 4, 4)) + ([float(t_span[3])] if i % 2 == 0 else []) + ([0.0] if i % 6 == 0 else []))
        hold_lo, grow_hi, shrink_lo = ratio_ranges(order, triple, pi)
        if tdt == "f32":
            es = [T(1) / T(order)] if not pi else [T(1) / T(order) - T(0.75) * T(PI_BETA), T(PI_BETA)]
        n = int(rng.integers(40, 81))
        ratios = []
        while len(ratios) < n:
            u = rng.uniform()
            if tdt == "f32" and u < 0.4:  # unclamped
                r = Y(np.exp(rng.normal(0.0, 1.5)))
            elif u < 0.55:
                r = Y(rng.uniform(hold_lo * 1.01, 0.999))
            elif u < 0.70:
                r = Y(grow_hi * 10.0 ** -rng.uniform(0.01, 6))
            elif u < 0.90:
                r = Y(shrink_lo * 10.0 ** rng.uniform(0.01, 6))
            else:
                k = int(rng.integers(0, 5))
                if pi and tdt == "f64" and k == 1:  # (PI at ratio 1: safety * prev**beta, a power)
                    k = 4
                r = Y([0.0, 1.0, NAN, INF, float(np.nextafter(Y(1), Y(0)))][k])
            # the filter: unclamped draws; every draw of a PI script (a forced accept can make any of them `prev`, and then no
            # range above is clamped any more)
            if tdt == "f32" and (u < 0.4 or pi) and np.isfinite(r) and r > 0:
                FILTER_STATS["drawn"] += 1
                if not all(powf_is_correctly_rounded(T(r), e) for e in es):
                    FILTER_STATS["rejected"] += 1
                    continue
            ratios.append(float(r))
        out.append(Script("random{:03d}".format(i), tdt, sdt, t_span, 1e-2 * 10.0 ** -rng.uniform(0, 2), _r(*ratios), method=method,
                          triple=triple, pi=pi, step_t=step_t, **kw))
    return out


FIXED = _fixed()
RANDOM = _random()
SCRIPTS = FIXED + RANDOM

# the fp32-time fixed scripts obey the filter too (every finite ratio that is not clamped by construction)
for _s in FIXED:
    if _s.tdt == "f32" and _s.n_seg == 1:
        _T = TT["f32"]
        _es = [_T(1) / _T(_s.order)] if not _s.pi else [_T(1) / _T(_s.order) - _T(0.75) * _T(PI_BETA), _T(PI_BETA)]
        _lo, _g, _sh = ratio_ranges(_s.order, (_s.safety, _s.ifactor, _s.dfactor), _s.pi)
        for _v, _f in _s.attempts:
            if np.isfinite(_v[0]) and _v[0] > 0 and (_s.pi or _g < _v[0] <= _lo or 1 < _v[0] < _sh):
                assert all(powf_is_correctly_rounded(_T(TT[_s.sdt](_v[0])), _e) for _e in _es), (_s.id, _v[0])
assert powf_is_correctly_rounded(np.float32(1e-4), np.float32(PI_BETA))  # the floor of ratio_prev
assert FILTER_STATS["rejected"] <= 0.01 * max(FILTER_STATS["drawn"], 1), FILTER_STATS
