"""Run as a program: the CDE kernels on a grid of 8 workgroups with a 4 KiB streaming threshold,

    XDE_GRID_BLOCKS=8 XDE_NT_BYTES=4096 python -m tests._cde_grid_child

Both settings are read once per process, so they need a fresh one: tests/test_gpu_cde.py starts this module as a child.  With them a
SLICED launch exceeds the grid — the one plan the default settings cannot reach, because the slicing keeps B * S within the default
grid.  Small shapes (B = 3, H = 33; C = 5, 64, 260 and 2050; aligned and one element off; both methods, both dtypes) against the numpy
double bit for bit, and the union of their plans must show second and third work items on sliced launches in the LDS and no-LDS
families, and the streaming loads.  Prints one "FAIL ..." line per failure, then "CHILD DONE"; the exit status is the failure count.
"""
import sys

import torch


def main():
    from . import _cde_plans as P
    from ._cde_double import CdeDoubleBackend
    from .test_gpu_cde import _check, _query

    B, H = 3, 33
    failures = 0
    double = CdeDoubleBackend()
    for dtype, dt in ((torch.float32, "f32"), (torch.float64, "f64")):
        seen = {False: set(), True: set()}
        n = 0
        for C in (5, 64, 260, 2050):
            for misalign in (False, True):
                for backward in (False, True):
                    p = _query(backward, dt, B, H, C, misalign)
                    seen[backward] |= P.features(p, B, H, C, backward)
                    if p["S"] > 1 and p["items"] > 2 * p["blocks"]:
                        seen[backward].add("third-item-sliced")
                for method in ("linear", "cubic"):
                    try:
                        _check(double, dtype, method, B, H, C, Tn=(8, 3)[n % 2], t=(2, 5, 1, 4)[n % 4], form=n % 3, misalign=misalign)
                    except AssertionError as e:
                        failures += 1
                        print("FAIL", dt, method, C, misalign, str(e)[:300].replace("\n", " "), flush=True)
                    n += 1
        for backward in (False, True):
            need = {"second-item-sliced", "third-item-sliced", "second-item:lds", "second-item:nolds", "kernel:vec-lds", "kernel:scalar-lds",
                    "kernel:scalar-nolds"} | (set() if backward else {"nt", "single", "long"})
            for branch in sorted(need - seen[backward]):
                failures += 1
                print("FAIL", dt, "backward" if backward else "forward", "no shape reaches", branch, flush=True)
    torch.cuda.synchronize()
    print("CHILD DONE failures={}".format(failures), flush=True)
    return failures


if __name__ == "__main__":
    sys.exit(main())
