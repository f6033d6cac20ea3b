"""Run as a program: the two fused heads on a grid of 2 workgroups,

    XDE_GRID_BLOCKS=2 python -m tests._head_grid_child sde | cde

The setting is read once per process, so it needs a fresh one: tests/test_gpu_sdehead.py and tests/test_gpu_cdehead.py each start this
module as a child.  With it a SLICED launch exceeds the grid — the plan the default settings cannot reach, because the slicing keeps
the work items within the default grid — so a workgroup walks second and third items that are slices: the barrier before the LDS
refill, the tile parity carried from one item into the next, in both the LDS and the per-use families and (SDE) on the one-tile plan.
Small shapes, both directions, aligned and one element off 16 bytes, each against the header's float32 statement on integer operands
bit for bit and against the float64 bounds on random operands with tanh (the checks of the parent modules).  The union of the plans
must show the branches of ``_head_plans.child_required``.  Prints one "FAIL ..." line per failure, then "CHILD DONE"; the exit status
is the failure count.  A launch that raises ends the run there: nothing more is launched.
"""
import sys

import torch

# rows, D, M, K
SDE_SHAPES = (
    (130, 66, 1, 4),   # two slices of 33 d on three row tiles: six items, so second and third items that are slices, increments in LDS
    (70, 2, 50, 12),   # increments per use, a populated second tile, two slices on two row tiles
    (70, 3, 4, 136),   # the one-tile plan: three row tiles, unsliced
    (193, 3, 3, 5),    # four unsliced items of two tiles; the last has one row
)
# B, H, C, K, Tn, control
CDE_SHAPES = (
    (70, 5, 7, 20, 8, "cubic"),     # five slices on three batch tiles, dX in LDS
    (40, 3, 200, 12, 3, "linear"),  # C > 192: dX per use, three slices on two batch tiles
    (33, 2, 5, 72, 8, "natural"),   # the instantiation of 16, leaving its k-loop early
)


def _run(head, shapes, features, checks):
    """``features(shape, backward, misalign)``; ``checks(shape, misalign)`` -> (name, callable) pairs.  Returns the failure count, or
    None where a launch raised."""
    from . import _head_plans as P

    failures = 0
    seen = {False: set(), True: set()}
    for shape in shapes:
        for misalign in (False, True):
            for backward in (False, True):
                seen[backward] |= features(shape, backward, misalign)
            for name, check in checks(shape, misalign):
                try:
                    check()
                except AssertionError as e:
                    failures += 1
                    print("FAIL", head, shape, "misaligned" if misalign else "aligned", name, str(e)[:300].replace("\n", " "), flush=True)
                except Exception as e:  # noqa: BLE001  (a launch or the device failed: nothing more is launched)
                    print("FAIL", head, shape, "misaligned" if misalign else "aligned", name, "raised", repr(e)[:300].replace("\n", " "), flush=True)
                    return None
    for backward in (False, True):
        for branch in P.gaps(P.child_required(head), seen[backward]):
            failures += 1
            print("FAIL", head, "backward" if backward else "forward", "no shape reaches", branch, flush=True)
    return failures


def main(head):
    from paddlexde_amd import _hip

    be = _hip.get_backend()
    if head == "sde":
        from . import test_gpu_sdehead as T

        failures = _run(head, SDE_SHAPES, lambda shape, backward, mis: T.features(*shape, backward, misalign=mis),
                        lambda shape, mis: (("integers", lambda: T.check_integer_operands(be, *shape, True, misalign=mis)),
                                            ("bounds", lambda: T.check_bounds(be, shape + ("tanh", True), misalign=mis))))
    elif head == "cde":
        from . import test_gpu_cdehead as T

        row = lambda shape: shape + (True, "tanh", True)  # noqa: E731
        failures = _run(head, CDE_SHAPES, lambda shape, backward, mis: T.features(*shape[:4], backward, misalign=mis),
                        lambda shape, mis: (("integers", lambda: T.check_integer_operands(be, row(shape), misalign=mis)),
                                            ("bounds", lambda: T.check_bounds(be, row(shape), misalign=mis))))
    else:
        raise SystemExit("usage: python -m tests._head_grid_child sde | cde")
    if failures is None:
        return 1
    torch.cuda.synchronize()
    print("CHILD DONE failures={}".format(failures), flush=True)
    return failures


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
