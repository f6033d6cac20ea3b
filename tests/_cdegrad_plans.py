"""Which code of xde_cdegrad.hip's control-gradient kernel a shape runs, read from the launch plan (xde_cde_control_grad_plan,
include/xde_hip_cdegrad.h: the function the launcher itself uses), and the table of shapes tests/test_gpu_cdegrad.py launches to reach
every branch the default settings can reach.  In the manner of tests/_cde_plans.py: nothing here names a tuning constant; no GPU is
needed, the plan is host arithmetic."""
import collections


def features(p, B, H, C, dt):
    """The branches a launch with plan ``p`` (a dict of xde_cdegrad_plan_t's fields) takes, by name:

    kernel:<vec|scalar>     the instantiation (per dtype and control): 16-byte vector or scalar loads of F
    tree | no-tree          several partial sums over h meet in the LDS tree, or H == 1 has the one
    row-loop                a lane adds more than one row of F
    ragged-partials         H is no multiple of the partials: some have one row fewer
    chunked                 a batch row has more vectors than the workgroup has lanes along c: it is walked in chunks
    short-last-chunk        ... and the last chunk is not full
    idle-lanes              a batch row has fewer vectors than lanes along c
    ragged-vector           scalar path: C is no multiple of the vector width, the last lane's vector is partly past C
    strided                 more batch rows than workgroups: a workgroup takes a second batch row
    """
    W = 4 if dt == "f32" else 2
    NV = -(-C // W)
    f = {"kernel:" + ("vec" if p["vec"] else "scalar"), "tree" if p["P"] > 1 else "no-tree"}
    if p["rows"] > 1:
        f.add("row-loop")
    if H % p["P"]:
        f.add("ragged-partials")
    if p["chunks"] > 1:
        f.add("chunked")
        if NV % p["CL"]:
            f.add("short-last-chunk")
    elif NV < p["CL"]:
        f.add("idle-lanes")
    if C % W:
        f.add("ragged-vector")
    if p["strided"]:
        f.add("strided")
    assert p["blocks"] == min(B, p["blocks"]) and p["P"] * p["CL"] == 256
    return f


REQUIRED = {"kernel:vec", "kernel:scalar", "tree", "no-tree", "row-loop", "ragged-partials", "chunked", "short-last-chunk", "idle-lanes",
            "ragged-vector", "strided"}

# label: what the row is there for; shape (B, H, C); misalign: F one element off 16 bytes; features: the branches it must take
Row = collections.namedtuple("Row", "label shape misalign features")
TABLE = (
    Row("one row, one channel: no tree, idle lanes", (1, 1, 1), False, {"kernel:scalar", "no-tree", "idle-lanes", "ragged-vector"}),
    Row("vector loads, a full tree, one row per partial", (3, 32, 64), False, {"kernel:vec", "tree"}),
    Row("vector loads, the row loop with ragged partials", (3, 33, 64), False, {"kernel:vec", "tree", "row-loop", "ragged-partials"}),
    Row("a short tree (H = 7 of 8 partials)", (3, 7, 5), False, {"kernel:scalar", "tree", "ragged-partials", "ragged-vector"}),
    Row("scalar loads because F is one element off 16 bytes", (3, 7, 4), True, {"kernel:scalar", "tree"}),
    Row("a batch row walked in chunks, the last one short", (3, 512, 260), False, {"kernel:vec", "chunked", "short-last-chunk", "row-loop"}),
    Row("C beyond any on-chip table, scalar, chunked", (2, 33, 2050), True, {"kernel:scalar", "chunked", "row-loop"}),
    Row("no tree and chunks: H = 1 leaves every lane along c", (3, 1, 2050), False, {"no-tree", "chunked"}),
    Row("more batch rows than workgroups", (2100, 7, 3), False, {"strided", "kernel:scalar"}),
    Row("more batch rows than workgroups, an odd count, vector loads", (2101, 1, 4), False, {"strided", "kernel:vec", "no-tree"}),
)
ROW_IDS = tuple(r.label for r in TABLE)

# the shapes the other tests of tests/test_gpu_cdegrad.py launch, as (B, H, C, misalign)
GRID_SHAPES = tuple((B, H, C, mis) for C in (1, 3, 4, 5, 64, 260) for H in (1, 7, 33, 512) for B in (1, 3) for mis in (False, True))


def suite_shapes():
    return GRID_SHAPES + tuple(r.shape + (r.misalign,) for r in TABLE)


def coverage_gaps(query, dt):
    """``query(dt, B, H, C, misalign)`` -> plan dict.  The branches of ``REQUIRED`` that no shape of the suite reaches."""
    seen = set()
    for B, H, C, mis in suite_shapes():
        seen |= features(query(dt, B, H, C, mis), B, H, C, dt)
    return sorted(REQUIRED - seen)
