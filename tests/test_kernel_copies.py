"""Register copies in the shipped parity kernel's path loop, checked at build time (CPU; hipcc
cross-compiles gfx950).  A v_mov merges a value defined under one predicate with an old or default
value for the lanes that skipped the block: it computes nothing and costs VALU issue cycles, the
kernel's bound (DESIGN §5.5, §10 "copies").  The kernel is compiled with -DRTZIG_MARKS=1 and the
Makefile's flags, sample_kernel_bvh<true,false,false> is split at its ";@R <region>" markers in
program order, and v_mov_b64 + v_mov_b32 are counted per region against a budget: the count this
form of the source compiles to.  A count above its budget names the region that regressed.

region        parent (v_mov_b64 + v_mov_b32)   now
trips         16 + 9                            3 + 0
seed           6 + 1                            6 + 1   (all seven initialise a fresh lane's state)
scat_finish    6 + 0                            6 + 0
walk_setup     4 + 2                            3 + 1
dielectric     4 + 1                            3 + 0
lam_metal      3 + 0                            3 + 0
always         2 + 4                            2 + 4
handout        0 + 12                           0 + 8
"""
import collections

from abi_support import kernel_build

KERNEL = "_ZN3rtk17sample_kernel_bvhILb1ELb0ELb0E"

# region: (budget, the parent's count)
BUDGET = {
    "trips": (3, 25),
    "seed": (7, 7),
    "scat_finish": (6, 6),
    "walk_setup": (4, 6),
    "dielectric": (3, 5),
    "lam_metal": (3, 3),
    "always": (6, 6),
    "handout": (8, 12),
}


def _copies():
    lines = kernel_build.assembly("rt_kernel.hip", ("-DRTZIG_MARKS=1",))
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL))
    counts, region = collections.Counter(), "prologue"
    for l in lines[start + 1:]:
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            break
        if t.startswith(";@R "):
            region = t[4:].strip()
        elif t.startswith(("v_mov_b64", "v_mov_b32")):
            counts[region] += 1
    return counts


def test_path_loop_copies_within_budget():
    counts = _copies()
    assert counts["trips"] + counts["seed"] > 0, "no region markers found in the marked build"
    over = {r: {"count": counts[r], "budget": b, "parent": p} for r, (b, p) in BUDGET.items() if counts[r] > b}
    assert not over, over
