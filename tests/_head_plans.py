"""Which code of xde_sdehead.hip / xde_cdehead.hip a launch runs, read from its plan (xde_sdehead_plan / xde_cdehead_plan: the
functions the launchers themselves use), the shape, the direction and the placement of the operands.

``sde_features`` / ``cde_features`` turn a launch into the names of the branches it takes; ``gaps`` lists the branches of a required
set that no launch of a list reaches.  After a retune that moves a shape off its branch, the coverage tests of
tests/test_gpu_sdehead.py and tests/test_gpu_cdehead.py (and of tests/_head_grid_child.py) fail with the branch's name.  No GPU is
needed for any of it: the plans are host arithmetic.

The names (``R`` = the plan's kq_regs, ``T`` = the SDE head's tiles):

    inst:<R>x<T> | inst:<R>          the kernel instantiation
    kq-short:<R>                     kq < R: the lane's last vectors of k are +0 padding
    early-exit:<R>                   ... and the k-loop's break leaves before its last group of GROUP vectors (R = 8: after the first)
    a:vec, W:vec                     16-byte loads of a and W; else  a:scalar-by-K  (K % 4 != 0)  or  a:scalar-by-pointer
    s-vec | s-scalar-by-pointer | s-scalar-by-size   backward: the stores of s, decided at the launch
    s-scalar-by-slice                backward: s-vec at the launch, but a slice starts at n % 4 != 0 and stores by element
    lds | no-lds                     the increments (the dX tile) are in LDS, or made per use
    no-lds-second-tile               SDE: per-use increments where some item's second tile has rows
    partial-last-tile                the last row (batch) tile is not full
    absent-second-tile               SDE, two tiles: the last item's second tile has no row
    run-cut-by-chunk                 a run of m (of c) crosses a wave's chunk inside a pass
    run-cut-by-pass                  ... crosses a pass: the carry
    run-longer-than-pass             ... is longer than a pass: the carry is taken up and left again by one pass
    sliced, short-last-slice         D (H) is dealt to several work items; the last slice is shorter
    sliced-two-tiles                 sliced, with at least two row (batch) tiles
    second-item, third-item          more work items than workgroups (than twice the workgroups): the grid-stride loop
    second-item:<lds|no-lds>         ... by family (lds: the barrier before the refill)
    second-item:one-tile             SDE: ... on the one-tile plan
    second-item-sliced, third-item-sliced, second-item-sliced:<lds|no-lds>
    gf-null                          SDE backward without gf
"""
GROUP = 4  # 16-byte vectors of W requested ahead (kSdeHeadQB, kHeadQB): the granularity of the k-loop's exit


def _k_features(f, inst, p, K, misalign):
    R, kq = p["kq_regs"], p["kq"]
    f.add("inst:" + inst)
    if kq < R:
        f.add("kq-short:{}".format(R))
        if -(-kq // GROUP) * GROUP < R:
            f.add("early-exit:{}".format(R))
    for name in ("a", "W"):
        f.add(name + (":scalar-by-K" if K % 4 else ":scalar-by-pointer" if misalign else ":vec"))


def _s_features(f, N, run, S, per_slice, misalign):
    """``N`` = D M (H C), ``run`` = M (C), ``per_slice`` = Dc (Hc)."""
    if N % 4:
        f.add("s-scalar-by-size")
    elif misalign:
        f.add("s-scalar-by-pointer")
    else:
        f.add("s-vec")
        if any((part * per_slice * run) % 4 for part in range(S)):
            f.add("s-scalar-by-slice")


def _run_features(f, run, lengths, tile_n, pass_n):
    """``lengths``: the n of each kind of slice (a slice starts on a run, and its chunks and passes on the slice's start)."""
    if run > pass_n:
        f.add("run-longer-than-pass")
    for name, step in (("run-cut-by-chunk", tile_n), ("run-cut-by-pass", pass_n)):
        if run > 1 and any(b % run and (step == pass_n or b % pass_n) for n in lengths for b in range(step, n, step)):
            f.add(name)


def _item_features(f, p, sliced, one_tile=False):
    family = "lds" if "lds" in f else "no-lds"
    for nth, k in (("second", 1), ("third", 2)):
        if p["items"] > k * p["blocks"]:
            f.add(nth + "-item")
            if sliced:
                f.add(nth + "-item-sliced")
    if "second-item" in f:
        f.add("second-item:" + family)
        if one_tile:
            f.add("second-item:one-tile")
        if sliced:
            f.add("second-item-sliced:" + family)


def _slice_features(f, S, total, per_slice, tiles):
    if S > 1:
        f.add("sliced")
        if tiles >= 2:
            f.add("sliced-two-tiles")
        if total % per_slice:
            f.add("short-last-slice")


def _slice_lengths(S, total, per_slice, run):
    return {per_slice * run, (total - (S - 1) * per_slice) * run}


def sde_features(p, rows, D, M, K, backward, misalign=False, gf_null=False):
    """The branches a launch of the SDE head with plan ``p`` (a dict of xde_sdehead_plan_t's fields) takes; ``misalign``: a, W and s
    are contiguous but one element off 16 bytes."""
    f = set()
    _k_features(f, "{}x{}".format(p["kq_regs"], p["tiles"]), p, K, misalign)
    f.add("lds" if p["lds_w"] else "no-lds")
    tile_r = p["tile_r"]
    tiles = -(-rows // tile_r)
    last = rows - (tiles - 1) * tile_r  # rows of the last item
    if last < tile_r:
        f.add("partial-last-tile")
    if p["tiles"] == 2 and last <= tile_r // 2:
        f.add("absent-second-tile")
    if not p["lds_w"] and p["tiles"] == 2 and rows > tile_r // 2:
        f.add("no-lds-second-tile")
    _run_features(f, M, _slice_lengths(p["S"], D, p["Dc"], M), p["tile_n"], p["pass_n"])
    _slice_features(f, p["S"], D, p["Dc"], tiles)
    _item_features(f, p, p["S"] > 1, one_tile=p["tiles"] == 1)
    if backward:
        _s_features(f, D * M, M, p["S"], p["Dc"], misalign)
        if gf_null:
            f.add("gf-null")
    return f


def cde_features(p, B, H, C, K, backward, misalign=False):
    """The branches a launch of the CDE head with plan ``p`` (a dict of xde_cdehead_plan_t's fields) takes."""
    f = set()
    _k_features(f, str(p["kq_regs"]), p, K, misalign)
    f.add("lds" if p["lds_dx"] else "no-lds")
    tiles = -(-B // p["tile_b"])
    if B % p["tile_b"]:
        f.add("partial-last-tile")
    _run_features(f, C, _slice_lengths(p["S"], H, p["Hc"], C), p["tile_n"], p["pass_n"])
    _slice_features(f, p["S"], H, p["Hc"], tiles)
    _item_features(f, p, p["S"] > 1)
    if backward:
        _s_features(f, H * C, C, p["S"], p["Hc"], misalign)
    return f


_COMMON = {"a:vec", "W:vec", "a:scalar-by-K", "W:scalar-by-K", "a:scalar-by-pointer", "W:scalar-by-pointer", "lds", "no-lds",
           "partial-last-tile", "run-cut-by-chunk", "run-cut-by-pass", "run-longer-than-pass", "sliced", "sliced-two-tiles",
           "short-last-slice"}
_S_STORES = {"s-vec", "s-scalar-by-pointer", "s-scalar-by-size", "s-scalar-by-slice"}
_SDE_K = {"inst:2x2", "inst:8x2", "inst:16x2", "inst:32x1", "kq-short:2", "kq-short:8", "kq-short:16", "kq-short:32", "early-exit:8",
          "early-exit:16", "early-exit:32"}
_CDE_K = {"inst:1", "inst:2", "inst:4", "inst:8", "inst:16", "inst:32", "kq-short:4", "kq-short:8", "kq-short:16", "kq-short:32",
          "early-exit:16", "early-exit:32"}


def sde_required(backward):
    """What the shapes tests/test_gpu_sdehead.py launches at the default settings must reach together, per direction: everything the
    default grid can reach.  (A sliced launch beyond the grid is the child's: ``child_required``.)"""
    need = _COMMON | _SDE_K | {"no-lds-second-tile", "absent-second-tile", "second-item", "third-item", "second-item:lds"}
    return need | (_S_STORES | {"gf-null"} if backward else set())


def cde_required(backward):
    need = _COMMON | _CDE_K | {"second-item", "third-item", "second-item:lds"}
    return need | (_S_STORES if backward else set())


def child_required(head):
    """What the shapes of tests/_head_grid_child.py must reach together on its small grid, per direction."""
    need = {"second-item-sliced", "third-item-sliced", "second-item:lds", "second-item:no-lds", "second-item-sliced:lds",
            "second-item-sliced:no-lds", "a:scalar-by-pointer", "W:scalar-by-pointer"}
    return need | ({"second-item:one-tile"} if head == "sde" else set())


def gaps(required, seen):
    return sorted(required - seen)
