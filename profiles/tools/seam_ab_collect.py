"""Summary of profiles/tools/seam_ab.sh's output directory: per workload every timed block of both builds (ms per attempted step),
medians, within-build spreads, and the verdict — a gain counts only if EVERY block of this tree is faster than EVERY block of the parent
and the medians differ by more than three times the larger within-build spread; and whether the two output dumps are bit-identical.

    python profiles/tools/seam_ab_collect.py OUT_DIR [DUMP_DIR] [> summary.json]
"""
import glob
import json
import os
import statistics
import sys

import numpy as np


def last_json_line(path):
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def main(out_dir, dump_dir=None):
    res = {}
    for side in ("parent", "this"):
        d = os.path.join(dump_dir or out_dir, "dump_" + side)
        if os.path.isdir(d):
            res.setdefault("dump", {})[side] = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}
    if "dump" in res and len(res["dump"]) == 2:
        a, b = res["dump"]["parent"], res["dump"]["this"]
        res["dump"] = {"files": sorted(a), "bit_identical": sorted(a) == sorted(b) and all(
            a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes() for f in a)}
    else:
        res.pop("dump", None)
    workloads = sorted({os.path.basename(p).rsplit("_", 2)[0] for p in glob.glob(os.path.join(out_dir, "*_this_*.json"))} - {"dump"})
    for w in workloads:
        rec = {}
        for side in ("parent", "this"):
            runs = [last_json_line(p) for p in sorted(glob.glob(os.path.join(out_dir, "{}_{}_*.json".format(w, side))))]
            blocks = [b for r in runs for b in r["ms_per_step_blocks"]]
            rec[side] = {"runs": [r["ms_per_step_blocks"] for r in runs], "median": statistics.median(blocks), "min": min(blocks),
                         "max": max(blocks), "spread": max(blocks) - min(blocks),
                         "kernels_us": {k: round(v["avg_us"], 2) for k, v in (runs[-1].get("kernels") or {}).items()}}
        p, t = rec["parent"], rec["this"]
        spread = max(p["spread"], t["spread"])
        rec["every_block_faster"] = t["max"] < p["min"]
        rec["median_gain_ms"] = p["median"] - t["median"]
        rec["median_gain_percent"] = 100.0 * (p["median"] - t["median"]) / p["median"]
        rec["three_spreads_ms"] = 3.0 * spread
        rec["gain_counts"] = bool(rec["every_block_faster"] and rec["median_gain_ms"] > 3.0 * spread)
        res[w] = rec
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main(*sys.argv[1:3])
