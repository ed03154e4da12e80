"""The case table of the hoisting tests (tests/test_contraction_hoist_plan.py, tests/test_gpu_contract_hoist.py): small
networks written by hand in which some steps and permutes do not depend on the slice assignment.  No GPU and no device
import.  A case is a `tests.mode_cases.Case`, so the fills, the einsum reference and the bounds of that module apply.

Every network is sliced over u (3) and w (2), each held by two tensors and summed, and p (2), which the output holds (a
block per value of p, visited once per value of (u, w): beta = 1 from the second visit on): 12 assignments.

    kept_first   T0 (m, c) T1 (c, k) are slice-free and contracted first: Z (m, k), kept.  Y (k, n) = T2 T3 depends on u
                 and w; the consumer Z Y, both operands in the arena, has Z as its first operand and sizes (M, N, K).
    kept_second  T1 (k, c) T2 (c, n) give Z (k, n), kept; the consumer T0 Z reads the sliced leaf T0 (u, w, m, k) in place
                 as its first operand and Z as its second.
                 Both in each shape class at its edge: tiled 64 x 64 x 33 and 65 x 65 x 48, dot with K = 512, stream.
    chain        T0 T1 -> Z1, T2 Z1 -> Z2: two hoisted steps, Z1 a temporary of the hoisted phase, Z2 kept.
    leaf_permute the slice-free leaf T1 (n, h, k) holds the batch axis h in the middle: its layout permute is hoisted, and
                 no step is.
    arena_permute  the kept Z (a, b, d) is summed over b, its middle axis, by its consumer: permuted arena to arena first.
    range        kept_first in the stream class over assignments 1 .. 10: off 0 and off every multiple of 5.
"""
from __future__ import annotations

import numpy as np

from tests import mode_cases as mc
from tnco_amd import contraction as ctr

SLICES = ("p", "u", "w")
SLICE_DIMS = dict(p=2, u=3, w=2)
N_ASSIGNMENTS = 12
BATCHES = (1, 5, 64)
EDGES = {"tiled-64-64-33": (64, 64, 33), "tiled-65-65-48": (65, 65, 48), "dot-3-5-512": (3, 5, 512), "stream-7-9-11": (7, 9, 11)}


def _case(name, ts, dims, output, path, slice_range=None):
    dims = {**SLICE_DIMS, **dims}
    return mc.Case(name, tuple(ts), tuple(dims.items()), tuple(output), tuple(path), SLICES, "float32", "uniform", slice_range)


def kept_first(name, sizes, slice_range=None):
    M, N, K = sizes
    ts = [("m", "c"), ("c", "k"), ("u", "k", "e"), ("u", "w", "e", "n"), ("p", "w", "n", "z")]
    # Z = T0 T1 | Y = T2 T3 | R = Z Y | T4 R
    return _case(name, ts, dict(m=M, n=N, k=K, c=3, e=2, z=2), ("p", "m", "z"), [(0, 1), (0, 1), (1, 2), (0, 1)], slice_range)


def kept_second(name, sizes):
    M, N, K = sizes
    ts = [("u", "w", "m", "k"), ("k", "c"), ("c", "n"), ("p", "u", "n", "y"), ("w", "y", "z")]
    # Z = T1 T2 | R = T0 Z | Q = T3 T4 | R Q
    return _case(name, ts, dict(m=M, n=N, k=K, c=3, y=2, z=2), ("p", "m", "z"), [(1, 2), (0, 3), (0, 1), (0, 1)])


def chain(name):
    ts = [("a", "b"), ("b", "c"), ("c", "d"), ("u", "w", "d", "e"), ("u", "w", "p", "e", "a")]
    # Z1 = T0 T1 | Z2 = T2 Z1 | Y = T3 T4 | Z2 Y
    return _case(name, ts, dict(a=5, b=4, c=6, d=7, e=3), ("p",), [(0, 1), (0, 3), (0, 1), (0, 1)])


def leaf_permute(name):
    ts = [("u", "w", "h", "m", "k"), ("n", "h", "k"), ("u", "w", "p", "n", "z")]
    return _case(name, ts, dict(h=3, m=5, n=6, k=7, z=2), ("p", "h", "m", "z"), [(0, 1), (0, 1)])


def arena_permute(name):
    ts = [("a", "b", "c"), ("c", "d"), ("u", "w", "b", "n"), ("u", "w", "p", "n", "a")]
    # Z (a, b, d) = T0 T1 | R = T2 Z over b | T3 R
    return _case(name, ts, dict(a=4, b=5, c=3, d=6, n=7), ("p", "d"), [(0, 1), (0, 2), (0, 1)])


# name -> (case, (steps hoisted, permutes hoisted), the shape class of the step that reads the kept tensor)
TABLE = {}
for _edge, _sizes in EDGES.items():
    TABLE[f"kept-first-{_edge}"] = (kept_first(f"kept-first-{_edge}", _sizes), (1, 0), _edge.split("-")[0])
    TABLE[f"kept-second-{_edge}"] = (kept_second(f"kept-second-{_edge}", _sizes), (1, 0), _edge.split("-")[0])
TABLE["chain"] = (chain("chain"), (2, 0), "stream")
TABLE["leaf-permute"] = (leaf_permute("leaf-permute"), (0, 1), "stream")
TABLE["arena-permute"] = (arena_permute("arena-permute"), (1, 1), "stream")
TABLE["range-1-11"] = (kept_first("range-1-11", EDGES["stream-7-9-11"], (1, 11)), (1, 0), "stream")

NAMES = tuple(TABLE)
TILED = tuple(n for n in NAMES if TABLE[n][2] == "tiled")


def case(name, dtype="float32"):
    return TABLE[name][0].with_(dtype=dtype)


def brute_force_flags(c, p):
    """(step flags, permute flags) restated from the definition: the set of leaves below each operand of each step,
    intersected with the holders of sliced indices.  The source of a permute of group -1 is the leaf its row names; a row
    of group k moves the operand of step k that the step then reads at the row's destination."""
    holders = {t for t, xs in enumerate(c.ts_inds) if set(xs) & set(c.slices)}
    free = lambda leaves: int(bool(c.slices) and not leaves & holders)  # noqa: E731
    below = [frozenset([t]) for t in range(len(c.ts_inds))]
    step_flags, perm_flags = [], [None] * len(p.perms)
    for r, row in enumerate(p.perms):
        if row[0] == 0:
            perm_flags[r] = int(free(frozenset([int(row[1])])) and row[2] == 1)
    for k, (a, b) in enumerate(c.path):
        a, b = sorted((a, b))
        lb, la = below.pop(b), below.pop(a)
        below.append(la | lb)
        step_flags.append(free(la | lb))
        for side, leaves in enumerate((la, lb)):
            for r, row in enumerate(p.perms):
                if row[6] == k and row[0] == 1 and p.steps[k][4 * side] == 1 and row[3] == p.steps[k][4 * side + 1]:
                    assert perm_flags[r] is None
                    perm_flags[r] = free(leaves)
    assert None not in perm_flags
    return step_flags, perm_flags


def _flags(p):
    if p.hoisted is None:
        return np.zeros(len(p.steps), np.int64), np.zeros(len(p.perms), np.int64)
    return p.step_hoist, p.perm_hoist


def launch_counts(p):
    """(once, per): the kernel launches, in KERNEL_PATHS order, of the hoisted phase of a call and of one assignment (of
    one group of a slice batch): a gather launch per permute group that has rows of the kind, every step in its slot."""
    step_flags, perm_flags = _flags(p)
    counts = [dict.fromkeys(ctr.KERNEL_PATHS, 0), dict.fromkeys(ctr.KERNEL_PATHS, 0)]  # [per, once]
    for g in set(p.perms[:, 6].tolist()):
        for kind in set(perm_flags[p.perms[:, 6] == g].tolist()):
            counts[kind]["gather"] += 1
    for sig, f in zip(mc.signature(p), step_flags):
        counts[int(f)][mc.kernel_slot(sig)] += 1
    return tuple(tuple(c[name] for name in ctr.KERNEL_PATHS) for c in (counts[1], counts[0]))


def mixed_groups(p):
    """Permute groups with hoisted rows and others: two gather launches where the plain plan has one."""
    _, perm_flags = _flags(p)
    return sum(len(set(perm_flags[p.perms[:, 6] == g].tolist())) == 2 for g in set(p.perms[:, 6].tolist()))


def side_counts(p):
    """(once, per) of the launches beside kernel_launches: dict(narrow=, split=), the narrowing passes of a scaled plan
    (a stored step each) and the split-kernel launches of compute="bf16x3" (a tiled-class step each)."""
    step_flags, _ = _flags(p)
    out = []
    for kind in (1, 0):
        picked = [k for k in range(len(p.steps)) if step_flags[k] == kind]
        narrow = sum(p.stage_refs[k] >= 0 for k in picked) if p.scaling is not None else 0
        split = sum(mc.signature(p)[k][0] == "tiled" for k in picked) if p.compute is not None else 0
        out.append(dict(narrow=int(narrow), split=int(split)))
    return tuple(out)
