"""Generates tests/golden/cde_arg_refusals_parent.json: what the 13 entry points of include/xde_hip_cde.h, xde_hip_spline.h and
xde_hip_cdegrad.h answer to wrong arguments at the commit this is run at — per case the return code and the error message.  The cases
are every single fault the host tests use (tests/test_cde_host.py, test_spline_host.py, test_cdegrad_host.py) and every pair of one
representative fault of each of two different refusal rules, so the message that WINS when two arguments are wrong at once is on
record.  tests/test_cde_arg_refusals_host.py replays the table against the built library and requires equality, character for
character.  Every pointer is a fake, well-formed address that is never dereferenced: each call is refused on the host, or enqueues
nothing (the plan and workspace queries).

    python -m tests.golden.make_cde_arg_refusals        # at the commit whose refusals are the yardstick
"""
import ctypes
import itertools
import json
import os
import subprocess

from paddlexde_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "cde_arg_refusals_parent.json")

A = 0x10000  # pointer i of an entry point is A * (i + 1): 16-byte aligned, distinct
# kinds of pointer argument: required; may be null (`der`, one of `gval` / `gder`); the launch's time (null = the time is `t_host`); read
# for its alignment only (the plan queries' operand); the plan a query writes
REQ, OPT, TIME, ALIGN_ONLY, PLAN = "required", "optional", "time", "align_only", "plan"
_KINDS = (REQ, OPT, TIME, ALIGN_ONLY, PLAN)
_TIMED = [("t_host", 0.5), ("time_dtype", 1), ("B", 2), ("H", 3), ("C", 4), ("Tn", 5)]
_STREAM = [("stream", None)]
SIZES = ("B", "H", "C", "outer", "L", "D")

# name -> its arguments in the header's order: (name, kind) for a pointer, (name, good value) for a scalar
ENTRIES = {
    "xde_cde_contract": [("out", REQ), ("F", REQ), ("series", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED + [("method", 1), ("dtype", 0)] + _STREAM,
    "xde_cde_contract_backward": [("gF", REQ), ("gout", REQ), ("series", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED
    + [("method", 1), ("dtype", 0)] + _STREAM,
    "xde_cde_plan": [("backward", 0), ("big", ALIGN_ONLY), ("B", 2), ("H", 3), ("C", 4), ("dtype", 0), ("plan", PLAN)],
    "xde_spline_natural_coeffs": [("Y", REQ), ("M", REQ), ("series", REQ), ("knots", REQ), ("B", 2), ("Tn", 5), ("C", 4), ("dtype", 0)] + _STREAM,
    "xde_spline_natural_gather": [("val", REQ), ("der", OPT), ("Y", REQ), ("M", REQ), ("knots", REQ), ("tq", REQ), ("outer", 2), ("Tn", 5), ("L", 3),
                                  ("D", 4), ("dtype", 0)] + _STREAM,
    "xde_cde_contract_natural": [("out", REQ), ("F", REQ), ("Y", REQ), ("M", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED + [("dtype", 0)] + _STREAM,
    "xde_cde_contract_natural_backward": [("gF", REQ), ("gout", REQ), ("Y", REQ), ("M", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED
    + [("dtype", 0)] + _STREAM,
    "xde_cde_control_grad": [("gSeries", REQ), ("gout", REQ), ("F", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED + [("method", 1), ("dtype", 0)]
    + _STREAM,
    "xde_cde_control_grad_natural": [("gY", REQ), ("gM", REQ), ("gout", REQ), ("F", REQ), ("knots", REQ), ("t_dev", TIME)] + _TIMED + [("dtype", 0)]
    + _STREAM,
    "xde_cde_control_grad_plan": [("F", ALIGN_ONLY), ("B", 2), ("H", 3), ("C", 4), ("dtype", 0), ("plan", PLAN)],
    "xde_spline_natural_coeffs_backward": [("gSeries", REQ), ("gY", REQ), ("gM", REQ), ("series", REQ), ("knots", REQ), ("workspace", REQ), ("B", 2),
                                           ("Tn", 5), ("C", 4), ("dtype", 0)] + _STREAM,
    "xde_spline_natural_coeffs_backward_workspace_bytes": [("B", 2), ("Tn", 5), ("C", 4), ("dtype", 0)],
    "xde_spline_natural_gather_backward": [("gY", REQ), ("gM", REQ), ("gval", OPT), ("gder", OPT), ("knots", REQ), ("tq", REQ), ("outer", 2), ("Tn", 5),
                                           ("L", 3), ("D", 4), ("dtype", 0)] + _STREAM,
}
PLANS = {"xde_cde_plan": _hip.XdeCdePlan, "xde_cde_control_grad_plan": _hip.XdeCdeGradPlan}
QUERIES = tuple(PLANS) + ("xde_spline_natural_coeffs_backward_workspace_bytes",)  # enqueue nothing: the only calls that may succeed
SILENT = ("xde_spline_natural_coeffs_backward_workspace_bytes",)  # answers -1 and sets no message


def _is_ptr(kind):
    return isinstance(kind, str) and kind in _KINDS


def _pointers(name, *kinds):
    return [arg for arg, kind in ENTRIES[name] if _is_ptr(kind) and kind in kinds]


def _has(name, arg):
    return any(a == arg for a, _ in ENTRIES[name])


def case_id(case):
    """A fault is {argument: value}: None (a null pointer), "+n" (a pointer n bytes past its aligned address) or a scalar."""
    return ",".join("{}{}".format(k, v if isinstance(v, str) else "=null" if v is None else "={}".format(v)) for k, v in sorted(case.items()))


def rules(name):
    """One representative fault of each refusal rule the entry point has; two of them never touch the same argument unless they are two
    faults of the one `method` argument."""
    req, data = _pointers(name, REQ), _pointers(name, REQ, OPT, ALIGN_ONLY)
    r = {}
    if _pointers(name, PLAN):
        r["null"] = {"plan": None}
    elif req:
        r["null"] = {req[1]: None}
    r["sizes"] = {next(a for a, _ in ENTRIES[name] if a in SIZES): 0}
    if _has(name, "Tn"):
        r["Tn"] = {"Tn": 1}
    r["dtype"] = {"dtype": 2}
    if _has(name, "time_dtype"):
        r["time_dtype"] = {"time_dtype": 2}
        r["t_align"] = {"t_dev": "+4"}
    if _has(name, "method"):
        r.update(bezier={"method": 2}, natural_code={"method": 3}, unknown={"method": 7})
    if data:
        r["align"] = {data[0]: "+2"}
    return r


def singles(name):
    req, data = _pointers(name, REQ), _pointers(name, REQ, OPT, ALIGN_ONLY)
    out = [{p: None} for p in req + _pointers(name, PLAN)]
    if name == "xde_spline_natural_gather_backward":
        out.append({"gval": None, "gder": None})
    if name == "xde_cde_plan":
        out.append({"big": None})  # (succeeds: only the alignment of `big` is used)
    for p in data:
        out += [{p: "+2"}, {p: "+4", "dtype": 1}]
    out += [{p: "+1"} for p in data[:1]]
    for s in (a for a, _ in ENTRIES[name] if a in SIZES):
        out += [{s: 0}, {s: -1}]
    if _has(name, "Tn"):
        out += [{"Tn": 1}, {"Tn": 0}]
    out += [{"dtype": 2}, {"dtype": -1}, {"dtype": 3}]
    if _has(name, "method"):
        out += [{"method": m} for m in (2, 3, 4, 7, -1)]
    if req:
        out += [{req[0]: None, next(a for a, _ in ENTRIES[name] if a in SIZES): 0}]
        out += [{req[0]: None, "Tn": 1}] if _has(name, "Tn") else []
    if _has(name, "time_dtype"):
        out += [{"time_dtype": 2}, {"time_dtype": -1}]
        out += [dict(c, t_dev=None) for c in out]  # (with the time in device memory, and as a host number)
        out += [{"t_dev": "+2", "time_dtype": 0}, {"t_dev": "+4"}]
    return out


def cases(name):
    out = singles(name)
    for (_, a), (_, b) in itertools.combinations(sorted(rules(name).items()), 2):
        if not set(a) & set(b):
            out.append(dict(a, **b))
    ids = [case_id(c) for c in out]
    assert len(set(ids)) == len(ids), (name, sorted(i for i in ids if ids.count(i) > 1))
    return out


def call(lib, name, case):
    """-> (return code, message): the entry point with good arguments but for ``case``."""
    args, at = [], 0
    for arg, kind in ENTRIES[name]:
        if _is_ptr(kind):
            at += 1
            good = ctypes.byref(PLANS[name]()) if kind == PLAN else A * at
            fault = case.get(arg, "+0")
            args.append(None if fault is None else good if fault == "+0" else good + int(fault))
        else:
            args.append(case.get(arg, kind))
    rc = getattr(lib, name)(*args)
    # (a call that succeeds sets no message: the thread's last one is some earlier call's)
    return int(rc), "" if name in SILENT or rc == _hip.XDE_OK else lib.xde_last_error().decode()


def record():
    lib = _hip.load_library()
    messages, table = [], {}
    for name in ENTRIES:
        table[name] = {}
        for c in cases(name):
            rc, msg = call(lib, name, c)
            assert rc != _hip.XDE_OK or name in QUERIES, (name, c)  # (anything else would go on to launch on the fake pointers)
            if msg not in messages:
                messages.append(msg)
            table[name][case_id(c)] = [rc, messages.index(msg)]
    return messages, table


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(HERE))
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, check=True, capture_output=True, text=True).stdout.strip()
    messages, table = record()
    with open(PATH, "w") as fh:
        json.dump({"parent": commit, "messages": messages, "cases": table}, fh, indent=0, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print("wrote", PATH, "at", commit, "-", sum(len(v) for v in table.values()), "cases,", len(messages), "messages")
