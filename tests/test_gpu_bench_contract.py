"""The driver's contract for bench.py: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line with the
agreed keys (metric/value/unit/…/config.workload, roofline{bound,achieved,peak,unit,frac,traffic}, cpu_baseline{value,
unit,cores,kind,sample}) and times exactly K steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--batch", "4096", *extra],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_json_contract():
    j = _run("--pipeline", "lag", "--repeat-blocks", "2")  # (per-kernel HIP events need eager launches; "auto" replays a hipGraph at this small size)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 6 and j["warmup"] == 2
    assert j["higher_is_better"] is True and j["scaling"] == "weak" and j["vs_baseline"] is None
    assert j["dtype"] == "f32" and j["data"] == "synthetic" and "workload" in j["config"]
    assert j["unit"] == "states/s" and j["value"] > 0 and j["ms_per_step"] > 0
    assert abs(j["value"] - 4096 * 128 / (j["ms_per_step"] * 1e-3)) / j["value"] < 1e-6  # value = states per step / step time
    # warmup + steps attempted, nothing skipped (+ the untimed settle attempts of set-up: the allocator's pool at its steady state, and —
    # pipeline="auto" — the graph captured)
    assert j["solver"]["n_steps"] == 8 + j["solver"]["settle_steps"] and j["solver"]["settle_steps"] >= 32

    # VERDICT r04 (next 6): the same K-step block three times in one run (the first is `ms_per_step`), and what of a step is inside no kernel
    assert len(j["ms_per_step_blocks"]) == 3 and j["ms_per_step_blocks"][0] == j["ms_per_step"] and all(b > 0 for b in j["ms_per_step_blocks"])
    assert abs(j["gap_ms_per_step"] - (j["ms_per_step"] - j["solver_kernel_ms_per_step"] - j["func_ms_per_step"])) < 1e-9
    assert len(j["gap_ms_per_step_blocks"]) == 3 and j["func_ms_per_step"] > 0

    rf = j["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and rf["achieved"] > 0
    assert "traffic" in rf
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "states/s" and cb["value"] > 0 and cb["cores"] >= 1 and cb["sample"]


def test_bench_default_pipeline_settles_before_the_timed_region():
    j = _run("--no-cpu-baseline")
    assert j["config"]["pipeline"] == "auto -> graph" and j["solver"]["settle_steps"] >= 16
    assert j["solver"]["n_steps"] == 8 + j["solver"]["settle_steps"]


def test_bench_side_workloads_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--pipeline", "graph"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    for controller in ("I", "PI"):
        r64 = j["results"][controller + "/float64"]
        assert r64["n_reject"] > 0 and r64["finite"]


def _launch(env_extra, *args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)


def test_bench_gpus_2_starts_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher starts two ranks itself (rehearsed on this one-GPU box: both
    ranks on cuda:0, gloo) and prints ONE line that says n_gpus == 2 = config 4 split over two ranks, with the N=1 datum of the
    same global workload riding along."""
    r = _launch({"XDE_BENCH_REHEARSAL": "1"}, "--gpus", "2", "--steps", "5", "--warmup", "2")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 5 and j["scaling"] == "strong"
    assert j["config"]["global_batch"] == 524288 and j["config"]["rows_per_gpu"] == 262144 and j["config"]["dim"] == 64
    assert j["rccl_ranks"] == 0  # gloo rehearsal: no RCCL group was formed, and the line says so
    n1 = j["n1_same_workload"]
    assert n1["n_gpus"] == 1 and n1["global_batch"] == 524288 and n1["dim"] == 64 and n1["value"] > 0


def test_bench_gpus_2_refuses_on_a_one_gpu_box():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has two GPUs")
    r = _launch({"XDE_BENCH_REHEARSAL": "0"}, "--gpus", "2", "--steps", "5", "--warmup", "2")
    assert r.returncode != 0
    assert "refusing" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_rccl_group_of_one_reports_its_ranks():
    r = _launch({"XDE_BENCH_FORCE_DIST": "1"}, "--gpus", "1", "--steps", "6", "--warmup", "2", "--batch", "4096", "--pipeline", "lag", "--no-cpu-baseline",
                "--exchange", "rccl")
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert j["rccl_ranks"] == 1 and j["n_gpus"] == 1
    # BASELINE configs[3] names the RCCL all-reduce: its step time is a top-level key of every sharded line (here it IS the headline transport)
    assert j["rccl_allreduce_ms_per_step"] == j["ms_per_step"] and "headline" in j["rccl_allreduce_transport"]


def test_bench_parent_stops_a_job_that_never_finishes():
    """VERDICT r03 (weak 5): `self_launch` had no watchdog.  XDE_BENCH_TEST_HANG=1 makes rank 1 of a rehearsed 2-rank job sleep at the
    start of its set-up (rank 0 then waits for it inside the set-up's first collective): the parent's wall clock (XDE_BENCH_TIMEOUT) must end the job's whole process
    group, say which stage every rank was in, print no line, and exit 124."""
    import time

    t0 = time.time()
    r = _launch({"XDE_BENCH_REHEARSAL": "1", "XDE_BENCH_TIMEOUT": "30", "XDE_BENCH_TEST_HANG": "1"}, "--gpus", "2", "--steps", "5", "--warmup", "2", "--no-n1", "--no-ab")
    assert r.returncode == 124, (r.returncode, r.stderr[-2000:])
    assert time.time() - t0 < 200
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "still running after 30 s" in r.stderr and "rank 0: in stage" in r.stderr and "rank 1: in stage 'set-up + warm-up + timed region'" in r.stderr
    # (the parent returned 124 only after every process of the job's session was gone — bench_launch.wait_for_group_exit — so the next
    #  test's probe children cannot meet a killed rank that is still tearing its GPU context down: no sleep here)


def test_bench_n_rank_line_names_devices_transport_and_alternatives():
    """The N > 1 line says who ran where and how the norm sums travelled: per-rank device rows, what the negotiation tried, the probe's
    verdict, and short runs on the other transports (rehearsal: p2p — the fused launch — and the host-staged all-reduce)."""
    r = _launch({"XDE_BENCH_REHEARSAL": "1"}, "--gpus", "2", "--steps", "5", "--warmup", "2", "--no-n1")
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert [d["rank"] for d in j["devices"]] == [0, 1] and all("device" in d and "name" in d for d in j["devices"])
    rep = j["norm_exchange_report"]
    said = (rep, r.stderr[-1500:])  # (a failure here must explain itself: what the negotiation reported, what the ranks wrote)
    assert rep["asked"] == "auto" and rep["p2p_probe"]["ok"] is True and rep["tried"][0] == {"transport": "p2p", "adopted": True}, said
    assert "xde_p2p_rk_control" in j["norm_exchange"], said
    ab = j["exchange_ab"]
    assert ab["p2p"]["headline"] is True and ab["p2p"]["ms_per_step"] == j["ms_per_step"] and ab["allreduce"]["ms_per_step"] > 0, (ab, said)
    assert "rccl_allreduce_ms_per_step" in j and j["rccl_allreduce_ms_per_step"] is None  # (gloo rehearsal: there is no RCCL group to time)


def test_bench_two_rank_rehearsal_takes_the_settle_phase_too():
    """a real N-GPU run always takes the multi-rank settle path — the all-reduce(MAX) of the settle count, then
    hundreds of collective mailbox exchanges before the timed region — while a one-card rehearsal skips it by default.  Once, in the
    default suite, with the settle phase ON (a short one): the ranks agree on the number of attempts, the peer-to-peer transport is
    adopted and survives them, and the line counts them."""
    r = _launch({"XDE_BENCH_REHEARSAL": "1", "XDE_BENCH_SETTLE_IN_REHEARSAL": "1", "XDE_BENCH_SETTLE_MS": "30"}, "--gpus", "2", "--steps", "5",
                "--warmup", "2", "--no-n1", "--no-ab")
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    rep = j["norm_exchange_report"]
    said = (rep, r.stderr[-1500:])
    assert rep["p2p_probe"]["ok"] is True and rep["tried"][0] == {"transport": "p2p", "adopted": True}, said
    assert j["solver"]["settle_steps"] >= 32 and j["solver"]["n_steps"] == 7 + j["solver"]["settle_steps"], (j["solver"], said)
    assert j["n_gpus"] == 2 and j["value"] > 0


def test_bench_survives_a_peer_to_peer_probe_that_crashes():
    """The peer-to-peer transport makes its first contact with a machine in CHILD processes.  XDE_BENCH_TEST_PROBE_FAIL=1 makes rank 1's
    probe exit at once with a non-zero status (what a probe that dies would look like to its parent): its peers' probes then run out of partners, every
    rank hears that the probe failed, the job moves on to the next transport together (rehearsal: the host-staged all-reduce) and the line
    says what happened."""
    # (XDE_BENCH_STAGE_SCALE: the surviving probe waits for its partner until its rendezvous stage — 45 s — runs out; half of that here)
    r = _launch({"XDE_BENCH_REHEARSAL": "1", "XDE_BENCH_TEST_PROBE_FAIL": "1", "XDE_BENCH_STAGE_SCALE": "0.5"}, "--gpus", "2", "--steps", "5", "--warmup",
                "2", "--no-n1")
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    rep = j["norm_exchange_report"]
    assert rep["p2p_probe"]["ok"] is False and "rank 1's probe exited with" in rep["p2p_probe"]["why"]
    assert rep["tried"] == [{"transport": "allreduce", "adopted": True}] and "all-reduce" in j["norm_exchange"]
    assert j["n_gpus"] == 2 and j["value"] > 0 and "p2p" not in j["exchange_ab"]


def test_bench_extra_measurement_that_hangs_keeps_the_headline_and_exits_nonzero():
    """a watchdog expiry during an EXTRA stage (here the whole-`odeint()` calls, made to hang by a test hook) used to
    print the main line and exit 0 — a hang in the library's public path reported as success.  Now the line is still printed (the
    headline is never lost to an extra), carries `watchdog_expired` = the stage that ran out, and the process exits 75."""
    env = dict(os.environ, XDE_BENCH_TEST_HANG="extra", XDE_BENCH_STAGE_SCALE="0.05")  # (the extra stage gets 15 s, the timed region 30 s)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 75, (r.returncode, r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["watchdog_expired"] == "whole odeint() calls" and j["value"] > 0 and j["n_gpus"] == 1 and "odeint_ms_T2" not in j
    assert "stage 'whole odeint() calls' has run for" in r.stderr


def test_bench_dump_outputs_are_the_solved_state(tmp_path):
    """--dump-outputs writes the solver's state after exactly settle + W + K attempts: y agrees with the exact solution
    y0 exp(A^T t1) of the linear ODE at the dumped t1 (to the solver's global error: ~3e-4 of max|y| here, bar 2e-3, while y has moved
    ~1.4 max|y| from y0), and f = y A^T.  A second run with the same arguments and a 1 MB budget dumps one seeded sample of rows
    (rows.npy) for both arrays: the same attempts, the same values at those rows."""
    import numpy as np
    import torch

    def run(d, budget=None):
        env = dict(os.environ, **({"XDE_BENCH_DUMP_MAX_BYTES": str(budget)} if budget else {}))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--batch", "4096",
                            "--no-cpu-baseline", "--no-odeint", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                           env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert j["solver"]["n_steps"] == j["solver"]["settle_steps"] + 3 + 7 and "ms_per_step_blocks" in j and len(j["ms_per_step_blocks"]) == 1
        assert sum(f.stat().st_size for f in d.iterdir()) <= (budget or 64 * 10 ** 6)
        return j, {n: np.load(d / (n + ".npy")) for n in ("y", "f", "rows", "t")}

    j1, a = run(tmp_path / "whole")
    assert a["y"].shape == a["f"].shape == (4096, 128) and a["y"].dtype == a["f"].dtype == np.float32
    assert a["rows"].dtype == np.float64 and np.array_equal(a["rows"], np.arange(4096)) and a["t"].dtype == np.float64
    g = torch.Generator().manual_seed(1)
    U = 0.1 * torch.randn(128, 128, generator=g, dtype=torch.float32)
    AT = (U - U.T).T.double()
    y0 = torch.randn(4096, 128, generator=torch.Generator().manual_seed(0)).double()
    t1 = float(a["t"][1])
    assert t1 > 1.0 and a["t"][0] < t1 and a["t"][2] > 0
    exact = (y0 @ torch.linalg.matrix_exp(AT * t1)).numpy()
    scale = float(np.abs(exact).max())
    assert float(np.abs(a["y"] - exact).max()) <= 2e-3 * scale
    assert float(np.abs(a["y"] - y0.numpy()).max()) > 0.5 * scale  # (a dump of y0 fails the line above by far)
    f_ref = a["y"].astype(np.float64) @ AT.numpy()
    assert float(np.abs(a["f"] - f_ref).max()) <= 1e-5 * float(np.abs(f_ref).max())

    j2, b = run(tmp_path / "sampled", budget=10 ** 6)
    rows = b["rows"].astype(np.int64)
    assert 0 < len(rows) < 4096 and np.array_equal(rows, np.unique(rows)) and np.array_equal(b["rows"], rows)
    assert b["y"].shape == b["f"].shape == (len(rows), 128)
    assert j2["solver"]["n_steps"] == j1["solver"]["n_steps"] and np.allclose(b["t"], a["t"], rtol=1e-6, atol=0)
    for n in ("y", "f"):
        assert np.allclose(b[n], a[n][rows], rtol=1e-5, atol=1e-6 * float(np.abs(a[n]).max())), n
