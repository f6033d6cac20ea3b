"""Which code of xde_cde.hip a shape runs, read from the launch plan (xde_cde_plan, include/xde_hip_cde.h: the function the launchers
themselves use), and the table of shapes that tests/test_gpu_cde.py launches to reach every plan that the default settings can reach.

Nothing here names a tuning constant: ``features`` turns a plan into the names of the branches it takes, a row of ``TABLE`` states the
branches the row is there for, and ``coverage_gaps`` lists the branches no shape reaches.  After a retune that moves a shape off its
branch, the row (or the coverage) fails with the branch's name.  No GPU is needed for any of it: the plan is host arithmetic.
"""
import collections

KERNELS = tuple("{}-{}".format(v, k) for v in ("vec", "scalar") for k in ("lds", "nolds", "grouped"))


def features(p, B, H, C, backward):
    """The branches a launch with plan ``p`` (a dict of xde_cde_plan_t's fields) takes, by name:

    kernel:<vec|scalar>-<lds|nolds|grouped>   the instantiation
    single | long                             forward: one lane holds a whole row's share, or strides along the row
    sliced | unsliced                         a batch row's H rows are dealt to several work items, or not
    short-last-slice                          sliced, and the last slice is shorter than the others
    short-last-group                          grouped, and the last item holds fewer batch rows than the others
    second-pass:<single|long|backward>        a work item has more rows than the workgroup covers in one pass: the reload of the
                                              single path, the row loop of the long path and of the backward kernel
    second-pass-in-a-slice                    ... where that work item is a slice
    short-last-pass                           ... and the last pass is not full
    second-item:<lds|nolds|grouped>           more work items than workgroups: a workgroup takes another item (a barrier, then the
                                              LDS table is refilled, in the two LDS families)
    second-item-sliced                        ... where the items are slices
    idle-teams                                forward, long path: the largest item has fewer rows than the workgroup has row teams, so
                                              whole teams (R = 64: whole waves) have no row and run ahead to the next item
    nt                                        forward: F is read with the streaming policy
    """
    family = "grouped" if p["grouped"] else ("lds" if p["lds"] else "nolds")
    path = "backward" if backward else ("single" if p["single"] else "long")
    sliced = p["S"] > 1
    f = {"kernel:{}-{}".format("vec" if p["vec"] else "scalar", family), "sliced" if sliced else "unsliced"}
    if not backward:
        f.add(path)
    rows = p["Hc"] if sliced else min(p["Gb"], B) * H  # rows of the largest work item
    if rows > p["rows_per_pass"]:
        f.add("second-pass:" + path)
        if sliced:
            f.add("second-pass-in-a-slice")
        if rows % p["rows_per_pass"]:
            f.add("short-last-pass")
    if path == "long" and rows < p["rows_per_pass"]:
        f.add("idle-teams")
    if p["items"] > p["blocks"]:
        f.add("second-item:" + family)
        if sliced:
            f.add("second-item-sliced")
    if sliced and H % p["Hc"]:
        f.add("short-last-slice")
    if p["grouped"] and B % p["Gb"]:
        f.add("short-last-group")
    if p["nt"]:
        f.add("nt")
    return f


def required(backward):
    """What the union of the suite's shapes must reach, per dtype and direction.  (``nt`` is a load policy: the backward kernel only
    stores the big operand, and its plan never sets it.)"""
    need = {"kernel:" + k for k in KERNELS} | {"second-item:lds", "second-item:grouped", "second-item:nolds", "short-last-slice",
                                               "short-last-group"}
    return need | ({"second-pass:backward"} if backward else {"second-pass:single", "second-pass:long", "nt"})


# label: the feature the row is there for; shape: (B, H, C), or one per dtype; misalign: the operands one element off 16 bytes;
# fwd / bwd: the branches the launch must take (features' names), or one set per dtype
Row = collections.namedtuple("Row", "label shape misalign fwd bwd")


def _both(x):
    return x if isinstance(x, dict) else {"f32": x, "f64": x}


TABLE = (
    Row("single path, second row pass, unsliced (a short last pass)", (1024, 70, 64), False,
        {"kernel:vec-lds", "single", "unsliced", "second-pass:single", "short-last-pass"}, {"unsliced", "second-pass:backward"}),
    Row("second row pass inside a slice", (128, 136, 256), False,
        {"f32": {"single", "second-pass:single", "second-pass-in-a-slice"}, "f64": {"long", "second-pass:long", "second-pass-in-a-slice"}},
        {"second-pass:backward", "second-pass-in-a-slice"}),
    Row("long path, second row pass, unsliced", (1024, 9, 260), False,
        {"long", "unsliced", "second-pass:long", "short-last-pass"}, {"unsliced", "second-pass:backward"}),
    Row("vector LDS kernel, second item", (2100, 600, 4), False,
        {"f32": {"kernel:vec-lds", "second-item:lds"}, "f64": {"kernel:vec-lds", "second-item:lds", "second-pass:single"}},
        {"kernel:vec-lds", "second-item:lds", "second-pass:backward"}),
    # (where the barrier before the LDS refill matters most: three of four waves have no row of the first item and are at the refill for
    # the second while the fourth still reads the table)
    Row("long path, second item, idle teams ahead at the LDS refill", (3000, 1, 2048), False,
        {"kernel:vec-lds", "long", "second-item:lds", "idle-teams"}, {"kernel:vec-lds", "second-item:lds"}),
    Row("scalar LDS kernel (C is no whole vector), second item", (2100, 600, 3), True,
        {"kernel:scalar-lds", "second-item:lds"}, {"kernel:scalar-lds", "second-item:lds", "second-pass:backward"}),
    Row("scalar LDS kernel (one element off 16 bytes), second item", (2100, 600, 4), True,
        {"kernel:scalar-lds", "second-item:lds"}, {"kernel:scalar-lds", "second-item:lds", "second-pass:backward"}),
    Row("scalar LDS kernel, second item and second row pass together", (2100, 1100, 1), False,
        {"kernel:scalar-lds", "second-item:lds", "second-pass:single", "short-last-pass"},
        {"kernel:scalar-lds", "second-item:lds", "second-pass:backward"}),
    Row("vector grouped kernel, a short last group", (2049, 3, 8), False,
        {"kernel:vec-grouped", "short-last-group"}, {"kernel:vec-grouped", "short-last-group"}),
    Row("vector grouped kernel, second item", {"f32": (4200, 256, 8), "f64": (4200, 128, 8)}, False,
        {"kernel:vec-grouped", "second-item:grouped"}, {"kernel:vec-grouped", "second-item:grouped", "second-pass:backward"}),
    Row("vector no-LDS kernel", (2, 3, 2052), False, {"kernel:vec-nolds", "long"}, {"kernel:vec-nolds"}),
    Row("vector no-LDS kernel, second item", (2100, 2, 2052), False,
        {"kernel:vec-nolds", "second-item:nolds"}, {"kernel:vec-nolds", "second-item:nolds"}),
    Row("scalar no-LDS kernel, second item", (2100, 1, 2050), True,
        {"kernel:scalar-nolds", "second-item:nolds"}, {"kernel:scalar-nolds", "second-item:nolds"}),
    Row("streaming loads of F (it is exactly 64 MiB)", {"f32": (1024, 256, 64), "f64": (1024, 128, 64)}, False,
        {"kernel:vec-lds", "nt", "second-pass:single"}, {"kernel:vec-lds", "second-pass:backward"}),
)
ROW_IDS = tuple(r.label for r in TABLE)


def row_case(row, dt):
    """(B, H, C), forward branches, backward branches of ``row`` for ``dt`` ("f32" | "f64")."""
    return _both(row.shape)[dt], _both(row.fwd)[dt], _both(row.bwd)[dt]


# the shapes the other tests of tests/test_gpu_cde.py launch, as (B, H, C, misalign)
GRID_SHAPES = tuple((B, H, C, mis) for C in (1, 3, 4, 5, 64, 260) for H in (1, 7, 33) for B in (1, 3) for mis in (False, True))
ITEM_SHAPES = ((2100, 1, 3, False), (2101, 1, 3, False), (4200, 512, 1, False))
TABLE_SHAPES = ((2, 3, 2050, False), (2, 3, 2050, True))


def suite_shapes(dt):
    return GRID_SHAPES + ITEM_SHAPES + TABLE_SHAPES + tuple(row_case(r, dt)[0] + (r.misalign,) for r in TABLE)


def coverage_gaps(query, dt):
    """``query(backward, dt, B, H, C, misalign)`` -> plan dict.  The branches of ``required`` that no shape of the suite reaches, as
    "forward: <branch>" / "backward: <branch>" (empty when the suite reaches every reachable plan)."""
    gaps = []
    for backward in (False, True):
        seen = set()
        for B, H, C, mis in suite_shapes(dt):
            seen |= features(query(backward, dt, B, H, C, mis), B, H, C, backward)
        gaps += ["{}: {}".format("backward" if backward else "forward", b) for b in sorted(required(backward) - seen)]
    return gaps
