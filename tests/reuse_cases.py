"""The case table of the reuse tests (tests/test_contraction_reuse_plan.py, tests/test_gpu_contract_reuse.py): small
networks written by hand in which the steps and permutes depend on subsets of the sliced indices.  No GPU and no device
import.  A case is a `tests.mode_cases.Case`, so the fills, the einsum reference and the bounds of that module apply.

Every network is sliced over p (2), which the output holds (a block per value of p), and over u (3) and w (2), both
summed.  The first tensor holds p, u appears before w: the default order is (p, u, w), places 6, 2, 1, 12 assignments.
A tensor below which only u is sliced has period 2 (6 runs of 12), only p: 6 (2 runs), none: 12 (1 run).

    kept_first   Z (m, k) = T1 T2 depends on u; Y (k, n) = T3 T4 on w; the consumer Z Y, period 1, reads the kept Z as its
                 first operand and has the sizes (M, N, K).
    kept_second  the same with the consumer Y Z: Z (k, n), kept, is its second operand.
                 Both in each shape class at its edge: tiled 64 x 64 x 33 and 65 x 65 x 48, dot with K = 512, stream.
    nested       Z1 = T0 T1 depends on p (period 6), Z2 = T2 Z1 on p and u (period 2), Q = T3 T4 and the last step Q Z2 on
                 everything: two kept tensors, the inner one written again while the outer one stays.
    nested_deep  nested with one more step on p: Z0 = T0 T1 is a temporary of the slowest phase, Z1 = T2 Z0 its kept
                 tensor.  The plan gives the room of Z0 to Z2, the kept tensor of the faster phase on p and u: a slower
                 phase's temporary on a faster phase's kept buffer.
    two_kept     Z1 = T1 T2 and Z2 = T3 T4 both depend on u and both are kept, for two steps of period 1: two kept tensors
                 of one phase, of 30 elements each.
    chain        X1 = T1 T2 and X2 = X1 T3 both depend on u: X1 is a temporary of that phase, X2 is kept; beside them the
                 slice-free pair F = T5 T6 (1 run), kept for a step of period 1, and V = T4 T7 on w.
    leaf_gather  the leaf T1 (m, u, k) is not dense after slicing and depends on u only: its slice-start gather has period
                 2 and its copy is kept.
    arena_permute  the kept Z (a, b, d), period 2, is summed over b, its middle axis, by its consumer V Z (V = T3 T4 on w):
                 permuted arena to arena first, at period 2, the copy kept.
    both_permuted  Z (a, b, d), on u, and Y (n1, b, n2), on w, are both summed over their middle axis by Z Y: two permutes
                 of one group, of periods 2 and 1.  With `indirect=True` Y, as fast as the step, is read in place; the
                 permute of Z, slower than the step, stays and its copy is kept.  Tiled 65 x 65 x 33 and stream.
    range-*      kept_first (stream) and nested over the assignments 1 .. 10 and 3 .. 8: the first assignment runs
                 everything, and multiples of 2 and of 6 fall inside the range.
"""
from __future__ import annotations

import numpy as np

from tests import mode_cases as mc
from tnco_amd import contraction as ctr

SLICES = ("p", "u", "w")
SLICE_DIMS = dict(p=2, u=3, w=2)
N_ASSIGNMENTS = 12
ORDERS = (None, "reversed", "reuse")  # "reversed": the default order back to front, for the cases of this table ("w", "u", "p")
ORDER_IDS = ("default", "w-u-p", "greedy")
EDGES = {"tiled-64-64-33": (64, 64, 33), "tiled-65-65-48": (65, 65, 48), "dot-3-5-512": (3, 5, 512), "stream-7-9-11": (7, 9, 11)}


def _case(name, ts, dims, output, path, slice_range=None):
    dims = {**SLICE_DIMS, **dims}
    return mc.Case(name, tuple(ts), tuple(dims.items()), tuple(output), tuple(path), SLICES, "float32", "uniform", slice_range)


def kept_first(name, sizes, slice_range=None):
    M, N, K = sizes
    ts = [("p", "n", "z"), ("u", "m", "c"), ("u", "c", "k"), ("w", "k", "e"), ("w", "e", "n")]
    # Z = T1 T2 | Y = T3 T4 | R = Z Y | T0 R
    return _case(name, ts, dict(m=M, n=N, k=K, c=3, e=2, z=2), ("p", "m", "z"), [(1, 2), (1, 2), (1, 2), (0, 1)], slice_range)


def kept_second(name, sizes):
    M, N, K = sizes
    ts = [("p", "n", "z"), ("u", "k", "c"), ("u", "c", "n"), ("w", "m", "e"), ("w", "e", "k")]
    # Y = T3 T4 | Z = T1 T2 | R = Y Z | T0 R
    return _case(name, ts, dict(m=M, n=N, k=K, c=3, e=2, z=2), ("p", "m", "z"), [(3, 4), (1, 2), (1, 2), (0, 1)])


def nested(name, slice_range=None):
    ts = [("p", "a", "b"), ("p", "b", "c"), ("u", "c", "d"), ("u", "w", "d", "a", "y"), ("w", "y")]
    # Z1 = T0 T1 | Z2 = T2 Z1 | Q = T3 T4 | Q Z2
    return _case(name, ts, dict(a=5, b=4, c=6, d=7, y=3), ("p", "y"), [(0, 1), (0, 3), (0, 1), (0, 1)], slice_range)


def nested_deep(name):
    ts = [("p", "a", "b"), ("p", "b", "e"), ("p", "e", "c"), ("u", "c", "d"), ("u", "w", "d", "a", "y"), ("w", "y")]
    # Z0 = T0 T1 | Z1 = T2 Z0 | Z2 = T3 Z1 | Q = T4 T5 | Q Z2
    return _case(name, ts, dict(a=5, b=4, c=6, d=7, e=4, y=3), ("p", "y"), [(0, 1), (0, 4), (0, 3), (0, 1), (0, 1)])


def two_kept(name):
    ts = [("p", "a", "d", "z"), ("u", "a", "c"), ("u", "c", "b"), ("u", "d", "e"), ("u", "e", "f"), ("w", "b", "g"), ("w", "g", "f")]
    # Z1 = T1 T2 | Z2 = T3 T4 | Y = T5 T6 | R1 = Z1 Y | R2 = Z2 R1 | T0 R2
    path = [(1, 2), (1, 2), (1, 2), (1, 3), (1, 2), (0, 1)]
    return _case(name, ts, dict(a=5, b=6, c=3, d=6, e=2, f=5, g=4, z=2), ("p", "z"), path)


def chain(name):
    ts = [("p", "a", "y"), ("u", "a", "b"), ("u", "b", "c"), ("c", "d"), ("w", "d", "e", "x"), ("e", "f"), ("f", "g"), ("w", "x")]
    # X1 = T1 T2 | X2 = X1 T3 | F = T5 T6 | V = T4 T7 | X3 = X2 V | X4 = X3 F | T0 X4
    path = [(1, 2), (1, 6), (2, 3), (1, 2), (1, 3), (1, 2), (0, 1)]
    return _case(name, ts, dict(a=5, b=4, c=6, d=7, e=3, f=4, g=5, y=2, x=2), ("p", "y", "g"), path)


def leaf_gather(name):
    ts = [("p", "u", "w", "n", "z"), ("m", "u", "k"), ("w", "k", "n")]
    return _case(name, ts, dict(m=5, n=6, k=7, z=2), ("p", "m", "z"), [(1, 2), (0, 1)])


def arena_permute(name):
    ts = [("p", "n", "a"), ("u", "a", "b", "c"), ("u", "c", "d"), ("w", "b", "n", "x"), ("w", "x")]
    # Z (a, b, d) = T1 T2 | V = T3 T4 | R = V Z over b | T0 R over n, a
    return _case(name, ts, dict(a=4, b=5, c=3, d=6, n=7, x=2), ("p", "d"), [(1, 2), (1, 2), (1, 2), (0, 1)])


def both_permuted(name, sizes):
    a, d, b, n1, n2 = sizes
    ts = [("p", "a", "n1", "z"), ("u", "a", "b", "c"), ("u", "c", "d"), ("w", "n1", "b", "e"), ("w", "e", "n2")]
    # Z (a, b, d) = T1 T2 | Y (n1, b, n2) = T3 T4 | R = Z Y over b, M = a d, N = n1 n2 | T0 R
    return _case(name, ts, dict(a=a, d=d, b=b, n1=n1, n2=n2, c=3, e=2, z=2), ("p", "z", "d", "n2"), [(1, 2), (1, 2), (1, 2), (0, 1)])


# name -> (case, (steps, permutes) with a period above 1 in the default order, the shape class of the step that reads
# the kept tensor)
TABLE = {}
for _edge, _sizes in EDGES.items():
    TABLE[f"kept-first-{_edge}"] = (kept_first(f"kept-first-{_edge}", _sizes), (1, 0), _edge.split("-")[0])
    TABLE[f"kept-second-{_edge}"] = (kept_second(f"kept-second-{_edge}", _sizes), (1, 0), _edge.split("-")[0])
TABLE["nested"] = (nested("nested"), (2, 0), "stream")
TABLE["nested-deep"] = (nested_deep("nested-deep"), (3, 0), "stream")
TABLE["two-kept"] = (two_kept("two-kept"), (2, 0), "stream")
TABLE["chain"] = (chain("chain"), (3, 0), "stream")
TABLE["leaf-gather"] = (leaf_gather("leaf-gather"), (0, 1), "stream")
TABLE["arena-permute"] = (arena_permute("arena-permute"), (1, 1), "stream")
TABLE["both-permuted-tiled-65-65-33"] = (both_permuted("both-permuted-tiled-65-65-33", (13, 5, 33, 5, 13)), (1, 1), "tiled")
TABLE["both-permuted-stream-6-6-5"] = (both_permuted("both-permuted-stream-6-6-5", (3, 2, 5, 2, 3)), (1, 1), "stream")
TABLE["range-1-11"] = (kept_first("range-1-11", EDGES["stream-7-9-11"], (1, 11)), (1, 0), "stream")
TABLE["range-3-9"] = (kept_first("range-3-9", EDGES["stream-7-9-11"], (3, 9)), (1, 0), "stream")
TABLE["nested-range-1-11"] = (nested("nested-range-1-11", (1, 11)), (2, 0), "stream")
TABLE["nested-range-3-9"] = (nested("nested-range-3-9", (3, 9)), (2, 0), "stream")

NAMES = tuple(TABLE)
TILED = tuple(n for n in NAMES if TABLE[n][2] == "tiled")
# indirect=True: one operand folded at its step's period, and a slower source that stays a permute and is kept
INDIRECT = ("both-permuted-tiled-65-65-33", "both-permuted-stream-6-6-5", "arena-permute", "nested")


def case(name, dtype="float32"):
    return TABLE[name][0].with_(dtype=dtype)


def order_kw(c, order):
    if order == "reversed":
        return dict(slice_order=tuple(reversed(c.plan().slice_inds)))
    return {} if order is None else dict(slice_order=order)


def runs(period, lo, hi):
    """The assignments of [lo, hi) at which an item of that period runs, counted one by one."""
    return sum(a == lo or a % period == 0 for a in range(lo, hi))


def deps(c, p):
    """(per step, per permute row) the sliced indices held by the leaves below the item, from the definition: the
    source of a permute of group -1 is the leaf its row names; an arena row of group k moves the operand of step k that
    the step then reads at the row's destination."""
    cut = [frozenset(x for x in xs if x in c.slices) for xs in c.ts_inds]
    below = list(cut)
    step_dep, perm_dep = [], [None] * len(p.perms)
    for r, row in enumerate(p.perms):
        if row[0] == ctr.LEAF:
            perm_dep[r] = cut[int(row[1])]
    for k, (a, b) in enumerate(c.path):
        a, b = sorted((a, b))
        db, da = below.pop(b), below.pop(a)
        below.append(da | db)
        step_dep.append(da | db)
        for side, dep in enumerate((da, db)):
            for r, row in enumerate(p.perms):
                if row[6] == k and row[0] == ctr.ARENA and p.steps[k][4 * side] == ctr.ARENA and row[3] == p.steps[k][4 * side + 1]:
                    assert perm_dep[r] is None
                    perm_dep[r] = dep
    assert None not in perm_dep
    return step_dep, perm_dep


def needed(p, dep):
    """The assignments of the whole run at which an item below which `dep` is sliced has to run again: the first, and
    every one that gives an index of `dep` another value than the assignment before."""
    place = [int(np.prod(p.slice_dims[s + 1:], dtype=np.int64)) for s in range(len(p.slice_dims))]
    digits = lambda a: tuple((a // place[s]) % p.slice_dims[s] for s, x in enumerate(p.slice_inds) if x in dep)  # noqa: E731
    return [a for a in range(p.n_slices) if a == 0 or digits(a) != digits(a - 1)]


def periods(p):
    if p.step_period is None:
        return np.ones(len(p.steps), np.int64), np.ones(len(p.perms), np.int64)
    return p.step_period, p.perm_period


def predicted(p):
    """What a run of the plan launches and multiplies, from the periods and the range alone: dict(kernel=, indirect=,
    narrow=, split=, matrix=, launches=, macs=), kernel in KERNEL_PATHS and indirect in INDIRECT_KERNEL_PATHS order.  A
    gather launch per permute group and period that has rows, every step in the slot of its class, each as often as its
    period is due."""
    step_per, perm_per = periods(p)
    lo, hi = p.slice_range
    kernel = dict.fromkeys(ctr.KERNEL_PATHS, 0)
    through = dict.fromkeys(ctr.INDIRECT_KERNEL_PATHS, 0)
    narrow = split = matrix = macs = 0
    for g, per in {(int(g), int(q)) for g, q in zip(p.perms[:, 6], perm_per)}:
        kernel["gather"] += runs(per, lo, hi)
    for k, (sig, per) in enumerate(zip(mc.signature(p), step_per)):
        n = runs(int(per), lo, hi)
        folded = p.ind_steps is not None and (p.ind_steps[k][0] >= 0 or p.ind_steps[k][3] >= 0)
        if folded:
            through["ix_" + sig[0]] += n
        else:
            kernel[mc.kernel_slot(sig)] += n
        narrow += n * int(p.scaling is not None and p.stage_refs[k] >= 0)
        split += n * int(p.compute == "bf16x3" and sig[0] == "tiled")
        matrix += n * int(p.compute == "matrix" and sig[0] == "tiled")
        macs += n * int(np.prod(p.steps[k][10:14], dtype=np.int64))
    out = dict(kernel=tuple(kernel[q] for q in ctr.KERNEL_PATHS), indirect=tuple(through[q] for q in ctr.INDIRECT_KERNEL_PATHS),
               narrow=narrow, split=split, matrix=matrix, macs=macs)
    out["launches"] = sum(out["kernel"]) + sum(out["indirect"]) + narrow
    return out
