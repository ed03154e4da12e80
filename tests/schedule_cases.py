"""The case table of the schedule tests (tests/test_contraction_schedule_plan.py, tests/test_gpu_contract_schedules.py,
tools/fuzz_contract.py): the random networks of tests/mode_cases.py and a few more, for the ways of running a plan that
change *when* and *from where* a step runs -- `hoist=True`, `reuse=True`, `slice_order=`, `indirect=True` -- and for
`compute="matrix"` fed by them.  No GPU and no device import.

The hand-made tables of those features (tests/hoist_cases.py, tests/reuse_cases.py, tests/indirect_cases.py,
tests/matrix_cases.py) share one structure: sliced over p = 2, u = 3, w = 2, filled "uniform", the kept tensor read by a
stream-class step.  What they do not vary is the schedule a plan nobody drew gives: how many phases, which buffer of
which phase lies where, which operand of which class reads a kept tensor, what is folded beside what is kept.
`coverage(case, plans)` names that, item by item of REQUIRED_SCHEDULE, and `CASES = mode_cases.CASES + EXTRA` reaches
every item in a real and in a complex dtype (tests/test_contraction_schedule_plan.py asserts it item by item).

EXTRA: seeds of `mode_cases.generate` found by tools/find_schedule_cases.py, and networks written by hand (`fed`) for what
the generator does not reach under `mode_cases.caps`: a tiled-class step that reads a kept, a hoisted or a folded
operand.  At most 16, at most 3 sliced indices each.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import mode_cases as mc
from tests import reuse_cases as rc
from tnco_amd import contraction as ctr

BATCHES = (3, 64)  # slice_batch= beside hoist=True
BATCH = 3  # slice_batch= beside indirect=True and compute="matrix"
ORDERS = (None, "reversed", "reuse")  # slice_order= beside reuse=True (tests/reuse_cases.py order_kw)
DTYPES = tuple(np.dtype(d).name for d in mc.DTYPES)  # compute="matrix" runs a case in all of them
MAX_EXTRA = 16
MAX_SLICED = 3  # of an EXTRA case: at most 3 orders of the sliced indices, a reference each


class Plans:
    """The plans of a case in the modes the device test runs it in, each made once: `plain`, `hoist`, `reuse[order]`,
    `indirect`, `indirect_hoist`, `indirect_reuse[order]`."""

    def __init__(self, case):
        self.case = case

    @functools.cached_property
    def plain(self):
        return self.case.plan()

    @functools.cached_property
    def hoist(self):
        return self.case.plan(hoist=True)

    @functools.cached_property
    def reuse(self):
        return {o: self.case.plan(reuse=True, **rc.order_kw(self.case, o)) for o in ORDERS}

    @functools.cached_property
    def indirect(self):
        return self.case.plan(indirect=True)

    @functools.cached_property
    def indirect_hoist(self):
        return self.case.plan(indirect=True, hoist=True)

    @functools.cached_property
    def indirect_reuse(self):
        return {o: self.case.plan(indirect=True, reuse=True, **rc.order_kw(self.case, o)) for o in (None, "reuse")}


def operands(p, k):
    """(kind, ref, elements) of the two operands of step k."""
    st = [int(v) for v in p.steps[k]]
    H, M, N, K = st[10:14]
    return (st[0], st[1], H * M * K), (st[4], st[5], H * K * N)


def kept_reads(p):
    """(step, side, period of the writer) of every read of a kept tensor of a reusing plan: an arena operand that is an
    entry of `p.kept`, read by a step that runs more often than the entry's writer."""
    out = []
    for k in range(len(p.steps)):
        for side, (kind, ref, numel) in enumerate(operands(p, k)):
            for entry, per in zip(p.kept, p.kept_period):
                if kind == ctr.ARENA and entry == (ref, numel) and p.step_period[k] < per:
                    out.append((k, side, int(per)))
    return out


def hoisted_reads(p):
    """(step, side) of every read of a kept tensor of a hoisting plan by a step of the assignments."""
    return [(k, side) for k in range(len(p.steps)) if not p.step_hoist[k]
            for side, (kind, ref, numel) in enumerate(operands(p, k)) if kind == ctr.ARENA and (ref, numel) in p.kept]


def written(p):
    """(offset, elements, period) of every arena buffer that a step or a permute of a reusing plan writes."""
    out = [(int(st[9]), int(st[10] * st[11] * st[12]), int(per)) for st, per in zip(p.steps, p.step_period) if st[8] == ctr.ARENA]
    return out + [(int(r[3]), int(r[5]), int(per)) for r, per in zip(p.perms, p.perm_period) if r[2] == ctr.ARENA]


def kept_on_a_slower_temporary(p):
    """A kept tensor lies where an item of a slower phase writes something that is not kept: arena ranges of two items
    with different periods overlap (`nested_deep` of tests/reuse_cases.py)."""
    for (off, numel), per in zip(p.kept, p.kept_period):
        for o, n, q in written(p):
            if q > per and (o, n) not in p.kept and o < off + numel and off < o + n:
                return True
    return False


def phases(p):
    return len(set(p.step_period.tolist()) | set(p.perm_period.tolist()) | {1})


def largest_period_below_the_count(p):
    below = [int(q) for q in list(p.step_period) + list(p.perm_period) if 1 < q < p.n_slices]
    return max(below, default=None)


def folds(p):
    """(step, side, class, H > 1, kind of the operand) of every folded operand of a plan."""
    if p.ind_steps is None:
        return []
    sig = mc.signature(p)
    return [(k, side, sig[k][0], sig[k][3], int(p.steps[k][4 * side]), int(p.steps[k][4 * side + 1]))
            for k, row in enumerate(p.ind_steps) for side in (0, 1) if row[3 * side] >= 0]


_KEPT = [f"kept:{c}:{s}" for c in mc.CLASSES for s in ("first", "second")] + ["kept:H>1"]
_PHASES = ["phases>=3", "phases>=4", "kept-on-a-slower-temporary", "permute-period>1:leaf-arena",
           "permute-period>1:arena-arena", "permute-group:two-periods"]
_SLICES = ["reused-step-on-a-dimension-1-slice", "range-off-zero:reused:off-the-period", "ragged-count:hoisted",
           "order:reuse-has-fewer", "order:named-has-more"]
_FOLDS = ["fold:sliced-leaf", "fold:arena", "fold:H>1"] + [f"fold:{c}" for c in mc.CLASSES] + \
    ["fold:first", "fold:second", "fold:both", "fold:hoist-takes-one", "fold:beside-a-kept-permute"]
_MATRIX = [f"matrix:form{a}{b}" for a in (0, 1) for b in (0, 1)] + \
    ["matrix:H>1:arena-arena", "matrix:H>1:leaf", "matrix:reads-hoisted", "matrix:reads-kept"]
_FILLS = [f"fill:{f}:{w}" for f in mc.FILLS for w in ("reuses", "folds")]
REQUIRED_SCHEDULE = tuple(_KEPT + _PHASES + _SLICES + _FOLDS + _MATRIX + _FILLS)


def coverage(case, plans=None):
    """The items of REQUIRED_SCHEDULE that the case reaches, from its plans alone."""
    P = plans or Plans(case)
    got = set()
    side_name = ("first", "second")
    # reuse=True: in each of the orders the device test runs
    for order, p in P.reuse.items():
        sig = mc.signature(p)
        for k, side, _ in kept_reads(p):
            got.add(f"kept:{sig[k][0]}:{side_name[side]}")
            if sig[k][3]:
                got.add("kept:H>1")
            if sig[k][0] == "tiled" and order is None:  # (matrix mode runs beside reuse=True in the default order)
                got.add("matrix:reads-kept")
        if phases(p) >= 3:
            got.add("phases>=3")
        if phases(p) >= 4:
            got.add("phases>=4")
        if kept_on_a_slower_temporary(p):
            got.add("kept-on-a-slower-temporary")
        slow = p.perms[p.perm_period > 1]
        if ((slow[:, 0] == ctr.LEAF) & (slow[:, 2] == ctr.ARENA)).any():
            got.add("permute-period>1:leaf-arena")
        if ((slow[:, 0] == ctr.ARENA) & (slow[:, 2] == ctr.ARENA)).any():
            got.add("permute-period>1:arena-arena")
        if any(len(set(p.perm_period[p.perms[:, 6] == g].tolist())) > 1 for g in set(p.perms[:, 6].tolist())):
            got.add("permute-group:two-periods")
        step_dep, _ = rc.deps(case, p)
        if any(per > 1 and any(case.dim[x] == 1 for x in dep) for per, dep in zip(p.step_period, step_dep)):
            got.add("reused-step-on-a-dimension-1-slice")
        big = largest_period_below_the_count(p)
        if p.slice_range[0] > 0 and p.reused[0] > 0 and big is not None and p.slice_range[0] % big:
            got.add("range-off-zero:reused:off-the-period")
    default = P.reuse[None]
    if P.reuse["reuse"].slice_inds != default.slice_inds and P.reuse["reuse"].macs < default.macs:
        got.add("order:reuse-has-fewer")
    if P.reuse["reversed"].macs > default.macs:
        got.add("order:named-has-more")
    if any(p.reused[0] > 0 for p in P.reuse.values()):
        got.add(f"fill:{case.fill}:reuses")
    # hoist=True
    n = case.n_assignments()
    if all(n % b for b in BATCHES) and P.hoist.hoisted != (0, 0):
        got.add("ragged-count:hoisted")
    sig = mc.signature(P.hoist)
    if any(sig[k][0] == "tiled" for k, _ in hoisted_reads(P.hoist)):
        got.add("matrix:reads-hoisted")
    # indirect=True: alone, and what the other two keywords change of it
    for k, side, cls, batch, kind, ref in folds(P.indirect):
        got.add(f"fold:{cls}")
        got.add(f"fold:{side_name[side]}")
        if batch:
            got.add("fold:H>1")
        if kind == ctr.ARENA:
            got.add("fold:arena")
        elif P.indirect.leaf_sl[ref][0] > 0:
            got.add("fold:sliced-leaf")
    if any(a and b for a, b in _folded_sides(P.indirect)):
        got.add("fold:both")
    if P.indirect_hoist.indirect != P.indirect.indirect:
        got.add("fold:hoist-takes-one")
    for p in P.indirect_reuse.values():
        for k, (a, b) in enumerate(_folded_sides(p)):
            if a == b:
                continue
            kind, ref, numel = operands(p, k)[int(a)]  # (the operand that is not folded)
            copies = (p.perms[:, 2] == ctr.ARENA) & (p.perms[:, 3] == ref) & (p.perms[:, 5] == numel)
            if kind == ctr.ARENA and (ref, numel) in p.kept and (p.perm_period[copies] > p.step_period[k]).any():
                got.add("fold:beside-a-kept-permute")
    if P.indirect.indirect > 0:
        got.add(f"fill:{case.fill}:folds")
    # compute="matrix": the tiled-class steps
    for cls, form_a, form_b, batch, ka, kb in mc.signature(P.plain):
        if cls != "tiled":
            continue
        got.add(f"matrix:form{form_a}{form_b}")
        if batch and ka == kb == "arena":
            got.add("matrix:H>1:arena-arena")
        if batch and "leaf" in (ka, kb):
            got.add("matrix:H>1:leaf")
    return got


def _folded_sides(p):
    if p.ind_steps is None:
        return [(False, False)] * len(p.steps)
    return [(bool(r[0] >= 0), bool(r[3] >= 0)) for r in p.ind_steps]


def tiled_steps(p):
    return sum(s[0] == "tiled" for s in mc.signature(p))


def fed(name, sizes, H, leaf_first, dtype, fill):
    """A network written by hand for a tiled-class step with a batch axis h (H) that reads a sliced leaf in place and a
    slice-free intermediate: the leaf L holds (u, w, h, ...) with the sliced axes outermost, Z = T1 T2 holds no sliced
    index -- hoisted under `hoist=True`, kept at the period of the whole run under `reuse=True` -- and the step L Z
    (`leaf_first`: Z is its second operand, [h][k][n]) or Z L (Z its first, [h][m][k]) has the sizes (M, N, K).  The last
    tensor takes the result to the output.  Sliced over u (2) and w (5), both summed, and p (2), which the output holds:
    20 assignments, no multiple of either slice batch."""
    M, N, K = sizes
    if leaf_first:
        ts = [("u", "w", "h", "m", "k"), ("h", "k", "c"), ("c", "n"), ("p", "u", "n", "z")]
        output = ("p", "h", "m", "z")
    else:
        ts = [("h", "m", "c"), ("c", "k"), ("u", "w", "h", "k", "n"), ("p", "u", "m", "z")]
        output = ("p", "h", "n", "z")
    path = [(1, 2), (0, 2), (0, 1)] if leaf_first else [(0, 1), (0, 2), (0, 1)]
    dims = dict(u=2, w=5, p=2, h=H, m=M, n=N, k=K, c=3, z=2)
    return mc.Case(name, tuple(ts), tuple(dims.items()), output, tuple(path), ("p", "u", "w"), np.dtype(dtype).name, fill)


HAND = {
    "fed-leaf-first-h2": dict(sizes=(64, 65, 33), H=2, leaf_first=True),
    "fed-leaf-second-h3": dict(sizes=(65, 64, 40), H=3, leaf_first=False),
}
# (a seed of `mode_cases.generate` or a name of HAND, dtype, fill)
EXTRA_TABLE = (
    ("fed-leaf-first-h2", "float64", "normal"),
    ("fed-leaf-second-h3", "complex64", "uniform"),
    (6, "complex128", "normal"),  # four phases; a kept tensor as the second operand of a dot-class step
    (36, "complex64", "uniform"),  # a reused step above a sliced index of dimension 1
    (1665, "complex128", "normal"),  # a kept tensor as the first operand of a tiled-class step
)


def make(key, dtype, fill):
    if isinstance(key, str):
        return fed(key, dtype=dtype, fill=fill, **HAND[key])
    return mc.generate(key, dtype, fill)


EXTRA = tuple(make(*row) for row in EXTRA_TABLE)
CASES = mc.CASES + EXTRA
IDS = tuple(f"{c.name}-{c.dtype}" for c in CASES)
