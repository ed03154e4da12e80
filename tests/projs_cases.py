"""The case table of the projection tests on multi-step networks (tests/test_contraction_projs_cases_plan.py,
tests/test_gpu_contract_projs_cases.py, tools/fuzz_contract.py --projs): networks with sparse output indices that are
contracted at given assignments of them (`sparse_inds=` / `projs=` of tnco_amd/contraction.py), written by hand and
random.  No GPU and no device import.

tests/test_gpu_contract_rows.py holds the edges of the three row-mapped kernels on one-step networks, where both
operands are leaves and the result is the output.  What it cannot vary is the *plan*: an operand that lies in the arena
with a row axis of its own, written by a row step, a folded step or a permute; a map from many rows to few; an operand
with one row beside one with rows; the row step as the last step under a summed slice and under block placement.
`coverage(case, plan)` reads those items from `plan.row_steps`, `plan.ops`, `plan.steps` and `plan.perms`, and the table
below reaches every item of REQUIRED in a real and in a complex dtype (tests/test_contraction_projs_cases_plan.py
asserts it item by item).  Every item can be planned, the arena-to-arena permute of a tensor with a row axis
too (`plan` permutes an arena operand whose layout does not fit, contraction.py `permute(T, target, ...)` with
target = ra + h + xs + s_order: the row axis stays outermost), so nothing was taken out of the list.

The words of the items: a step is *plain* when neither operand has a row axis, *folded* when only the first operand has
rows, stored [r][m][k] with H = 1 (one ordinary GEMM with R M rows), a *row step* otherwise.  A step goes to the
row-mapped kernel of its class when R > 1 or it has a map (csrc/contract.hip, run_step); every other step runs the plain
kernels.  An *arena operand* is an intermediate: the result of an earlier step (permuted or not).

A case is cheap by construction (`caps`): 4 to 8 leaves of at most 2^18 elements, 1 to 64 slice assignments, at most
5 10^7 multiply-adds over all of them, an arena of at most 2^22 elements, an output of at most 2^18 elements, and a
single-precision dtype only where `mode_cases.kt(plan)` <= contract_cases.KT_SINGLE (the rule of the row tests).

The projections of a case (`Case.projs()`) are seeded from its name: `projs_spec` a count (rows drawn with
replacement, and the last row a copy of the first whenever the count is above 2), "all" (every assignment of the sparse
indices once, shuffled) or ("distinct", n) (n of those).

The reference (`reference`) is numpy's einsum of the whole network in float64 / complex128, pairwise along the case's
own path, at the projections: every leaf is indexed at `projs` in its own sparse axes first, so that the einsum has one
batch axis of P entries instead of the product of the sparse dimensions (einsum, then index, gives the same numbers;
tests/test_contraction_projs_cases_plan.py holds the two against each other where the dense result is small).  Nothing
of tnco_amd.contraction takes part in it.
"""
from __future__ import annotations

import itertools
import math
import zlib
from dataclasses import dataclass

import numpy as np

from tests import contract_cases as cc
from tests import mode_cases as mc
from tests.mode_cases import _greedy_path, _random_path, klass, kt, summed_assignments
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn

DTYPES = mc.DTYPES
SINGLES = mc.SINGLES
FILLS = mc.FILLS
PROJ = ctr.PROJ
CLASSES = mc.CLASSES
P_CHOICES = (1, 7, 40)

MAX_LEAF = mc.MAX_LEAF
MAX_ARENA = mc.MAX_ARENA
MAX_MACS = mc.MAX_MACS
MAX_OUT = mc.MAX_OUT
MAX_ASSIGNMENTS = 64


@dataclass(frozen=True)
class Case:
    name: str
    ts_inds: tuple
    dims: tuple  # ((index, dimension), ...)
    output_inds: tuple
    sparse: tuple  # the sparse indices in column order of projs
    projs_spec: object  # a count, "all" or ("distinct", n)
    path: tuple
    slices: tuple
    slice_range: tuple
    dtype: str
    fill: str

    @property
    def dim(self):
        return dict(self.dims)

    def shapes(self):
        d = self.dim
        return [tuple(d[x] for x in xs) for xs in self.ts_inds]

    def n_assignments(self):
        lo, hi = self.slice_range or (0, math.prod(self.dim[x] for x in self.slices))
        return hi - lo

    def projs(self):
        """[P, len(sparse)] int64, seeded from the name."""
        d = self.dim
        every = np.array(list(itertools.product(*(range(d[x]) for x in self.sparse))), np.int64).reshape(-1, len(self.sparse))
        rng = np.random.RandomState(zlib.crc32(("projs " + self.name).encode()) % (1 << 31))
        if self.projs_spec == "all":
            return every[rng.permutation(len(every))]
        if isinstance(self.projs_spec, tuple):
            return every[rng.permutation(len(every))[:self.projs_spec[1]]]
        out = every[rng.randint(0, len(every), self.projs_spec)]
        if len(out) > 2:
            out[-1] = out[0]  # a duplicate row
        return out

    def plan(self, projs=None, sparse=None, slice_range=None):
        return ctr.plan(list(self.path), self.ts_inds, self.shapes(), self.output_inds, slices=self.slices,
                        slice_range=slice_range or self.slice_range, dtype=np.dtype(self.dtype),
                        sparse_inds=self.sparse if sparse is None else sparse, projs=self.projs() if projs is None else projs)

    def dense_plan(self):
        return ctr.plan(list(self.path), self.ts_inds, self.shapes(), self.output_inds, slices=self.slices,
                        slice_range=self.slice_range, dtype=np.dtype(self.dtype))

    def with_(self, **kw):
        return Case(**{**self.__dict__, **kw})

    def paste(self):
        """The case as a line of Python."""
        return (f"Case({self.name!r}, {self.ts_inds!r}, {self.dims!r}, {self.output_inds!r}, {self.sparse!r}, "
                f"{self.projs_spec!r}, {self.path!r}, {self.slices!r}, {self.slice_range!r}, {self.dtype!r}, {self.fill!r})")


def fill(case):
    """The leaves of a case in its dtype (the two fills of tests/mode_cases.py)."""
    return mc.fill(case)


def _wide(a):
    return np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64)


def reference(case, p, arrays, projs=None):
    """(the sum over the plan's assignments at every projection, the same of the moduli), float64 / complex128, axes in
    p.inds order: ("proj",) + the others."""
    projs = case.projs() if projs is None else np.asarray(projs)
    col = {x: j for j, x in enumerate(p.sparse_inds)}
    ts, wide = [], []
    for xs, a in zip(case.ts_inds, arrays):
        a, held = _wide(a), [x for x in xs if x in col]
        if held:  # [P][its other axes]: the leaf at each projection's values of the sparse indices it holds
            a = np.moveaxis(a, [xs.index(x) for x in held], range(len(held)))[tuple(projs[:, col[x]] for x in held)]
            xs = (PROJ,) + tuple(x for x in xs if x not in col)
        ts.append(tuple(xs))
        wide.append(a)
    sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in ts for x in xs))}
    shape = (len(projs),) + tuple(p.shape[1:])
    whole = p.slice_range == (0, p.n_slices)
    order = ["einsum_path"] + [tuple(sorted(step)) for step in case.path]
    out = []
    for ws in (wide, [np.abs(w) for w in wide]):
        if whole:
            args = [q for w, xs in zip(ws, ts) for q in (w, [sym[x] for x in xs])]
            out.append(np.einsum(*args, [sym[x] for x in p.inds], optimize=order).reshape(shape))
            continue
        total = np.zeros(shape, ws[0].dtype)
        rest = [x for x in p.inds if x not in p.slice_inds]
        for sid in range(*p.slice_range):
            at = {x: (sid // math.prod(p.slice_dims[s + 1:])) % p.slice_dims[s] for s, x in enumerate(p.slice_inds)}
            args = [q for w, xs in zip(ws, ts)
                    for q in (w[tuple(at.get(x, slice(None)) for x in xs)], [sym[x] for x in xs if x not in at])]
            total[tuple(at.get(x, slice(None)) for x in p.inds)] += np.einsum(*args, [sym[x] for x in rest], optimize=order)
        out.append(total)
    return tuple(out)


def dense_reference(case, p, arrays, projs=None):
    """The same numbers the plain way: the einsum of the whole network with every sparse index as an axis (the
    `reference` of tests/mode_cases.py), then indexed at the projections.  For small dense results."""
    projs = case.projs() if projs is None else np.asarray(projs)
    q = case.dense_plan() if p.slice_range == (case.slice_range or (0, p.n_slices)) else ctr.plan(
        list(case.path), case.ts_inds, case.shapes(), case.output_inds, slices=case.slices, slice_range=p.slice_range)
    out = []
    for z in mc.reference(case, q, arrays):
        front = [q.inds.index(x) for x in p.sparse_inds]
        z = np.moveaxis(z, front, range(len(front)))
        assert tuple(x for x in q.inds if x not in p.sparse_inds) == p.inds[1:]
        out.append(z[tuple(projs.T)])
    return tuple(out)


def bound(case, p, mag):
    """(c kt + 2) u mag: the plain bound of tests/mode_cases.py."""
    return mc.plain_bound(case, p, mag)


# ---- what the plan's tables say of every step

def row_slot(R, H, M, N, K):
    """The name in contraction.ROW_KERNEL_PATHS of a row step: the dispatch of csrc/contract.hip launch_rows_gemm (the
    classes of launch_gemm, the dot class counting R and H in its outputs)."""
    return "rows_" + klass(R * H, M, N, K)


def is_row_launch(rw):
    """The step goes to a row-mapped kernel: R > 1 or a map."""
    return int(rw[0]) > 1 or int(rw[2]) >= 0 or int(rw[4]) >= 0


def launches_per_assignment(p):
    """(kernel_launches, row_kernel_launches) of one slice assignment, from the tables: a gather launch per permute
    group, a step with R > 1 or a map in the row slot of its class, every other step, folded ones included, in its
    plain slot."""
    plain = dict.fromkeys(ctr.KERNEL_PATHS, 0)
    rows = dict.fromkeys(ctr.ROW_KERNEL_PATHS, 0)
    plain["gather"] = len(set(p.perms[:, 6].tolist()))
    for st, rw in zip(p.steps, p.row_steps):
        H, M, N, K = (int(v) for v in st[10:14])
        if is_row_launch(rw):
            rows[row_slot(int(rw[0]), H, M, N, K)] += 1
            continue
        cls = klass(H, M, N, K)
        form_a, form_b = int(st[3] != 1), int(st[7] != 1)  # (A [m][k]: sk == 1; B [k][n]: sn == 1)
        plain[cls if cls != "tiled" else ctr.KERNEL_PATHS[1 + 2 * (form_a == 0) + (form_b == 0)]] += 1
    return tuple(plain[n] for n in ctr.KERNEL_PATHS), tuple(rows[n] for n in ctr.ROW_KERNEL_PATHS)


def step_table(case, p):
    """Per step a dict: kind ("plain", "folded", "row"), cls (of the kernel that runs it), launch ("rows" or "plain"),
    and per side: src (("leaf", t) or ("step", j)), has_rows, arena (an intermediate), rows, map (None or the int32
    entries), stride (the operand's row stride is not 0), permuted (an arena-to-arena permute ran ahead of the step);
    and `feeds`, the step that reads the result (None: the output)."""
    live = [dict(src=("leaf", t), has_rows=p.leaf_rows[t] is not None) for t in range(len(case.ts_inds))]
    out = []
    for k, ((a, b), st, rw, op) in enumerate(zip(case.path, p.steps, p.row_steps, p.ops)):
        a, b = sorted((a, b))
        B, A = live.pop(b), live.pop(a)
        H, M, N, K = (int(v) for v in st[10:14])
        R = int(rw[0])
        sides = []
        for side, T in enumerate((A, B)):
            rows, at = int(rw[1 + 2 * side]), int(rw[2 + 2 * side])
            ref = int(st[4 * side + 1])
            group = p.perms[(p.perms[:, 6] == k) & (p.perms[:, 0] == ctr.ARENA) & (p.perms[:, 2] == ctr.ARENA) &
                            (p.perms[:, 3] == ref)]
            sides.append(dict(T, arena=T["src"][0] == "step", rows=rows, map=None if at < 0 else p.row_maps[at:at + R],
                              stride=not (at < 0 and rows == 1), permuted=len(group) > 0 and int(st[4 * side]) == ctr.ARENA))
        if not (A["has_rows"] or B["has_rows"]):
            kind = "plain"
        else:
            kind = "folded" if op["folded"] else "row"
        launch = "rows" if is_row_launch(rw) else "plain"
        out.append(dict(kind=kind, launch=launch, cls=klass(R * H, M, N, K) if launch == "rows" else klass(H, M, N, K),
                        A=sides[0], B=sides[1], H=H, R=R, form=(op["form_a"], op["form_b"]), feeds=None,
                        last=int(st[8]) == ctr.OUT))
        live.append(dict(src=("step", k), has_rows=A["has_rows"] or B["has_rows"]))
    for k, s in enumerate(out):
        for side in ("A", "B"):
            if s[side]["src"][0] == "step":
                out[s[side]["src"][1]]["feeds"] = k
    return out


REQUIRED = tuple(
    [f"rows_{c}:arena-map-{w}" for c in CLASSES for w in ("A", "B", "both")] +
    [f"rows_{c}:arena-rows-in-place" for c in CLASSES] +
    [f"rows_{c}:one-row-{w}" for c in CLASSES for w in ("A", "B")] + ["one-row:arena"] +
    [f"rows_{c}:H>1" for c in CLASSES] +
    [f"rows_tiled:form{a}{b}:arena" for a in (0, 1) for b in (0, 1)] +
    ["arena-map-repeats-rows", "row-step-feeds-row-step", "folded-reads-arena-rows", "folded-feeds-row-step",
     "plain-step-ahead-of-row-step", "arena-permute-of-row-tensor", "last:row-step-beta1", "last:row-step-blocks",
     "last:folded", "sliced-leaf-with-rows-gathered", "P=1", "duplicate-projection", "row_of_proj-not-monotone",
     "result-only-proj", "sparse-hyper-index-on-3-tensors"])


def coverage(case, p):
    """The items of REQUIRED that the case reaches."""
    got = set()
    table = step_table(case, p)
    for s in table:
        cls, A, B = s["cls"], s["A"], s["B"]
        if s["launch"] == "rows":
            mapped = [T["arena"] and T["has_rows"] and T["map"] is not None for T in (A, B)]
            if mapped[0] and not mapped[1]:
                got.add(f"rows_{cls}:arena-map-A")
            if mapped[1] and not mapped[0]:
                got.add(f"rows_{cls}:arena-map-B")
            if all(mapped):
                got.add(f"rows_{cls}:arena-map-both")
            for T, other, w in ((A, B, "A"), (B, A, "B")):
                if T["arena"] and T["map"] is None and T["stride"] and T["rows"] == s["R"] > 1:
                    got.add(f"rows_{cls}:arena-rows-in-place")
                if not T["stride"] and s["R"] > 1 and other["arena"] and other["has_rows"]:
                    got.add(f"rows_{cls}:one-row-{w}")
                    if T["arena"]:
                        got.add("one-row:arena")
                if T["arena"] and T["map"] is not None and s["R"] > T["rows"] and \
                        len(set(T["map"].tolist())) < len(T["map"]):
                    got.add("arena-map-repeats-rows")
                if T["permuted"] and T["has_rows"] and T["arena"]:
                    got.add("arena-permute-of-row-tensor")
            if s["H"] > 1:
                got.add(f"rows_{cls}:H>1")
            if cls == "tiled" and ((A["arena"] and A["has_rows"]) or (B["arena"] and B["has_rows"])):
                got.add("rows_tiled:form%d%d:arena" % s["form"])
        else:
            for T in (A, B):
                if T["permuted"] and T["has_rows"] and T["arena"]:
                    got.add("arena-permute-of-row-tensor")
        nxt = table[s["feeds"]] if s["feeds"] is not None else None
        if nxt is not None and nxt["launch"] == "rows" and nxt["kind"] == "row":
            if s["kind"] == "row" and s["launch"] == "rows":
                got.add("row-step-feeds-row-step")
            if s["kind"] == "folded":
                got.add("folded-feeds-row-step")
            if s["kind"] == "plain":
                got.add("plain-step-ahead-of-row-step")
        if s["kind"] == "folded" and A["arena"]:
            got.add("folded-reads-arena-rows")
    last = table[-1]
    if last["kind"] == "row" and last["launch"] == "rows":
        if summed_assignments(p) > 1:
            got.add("last:row-step-beta1")
        if mc._blocks_of(p, *p.slice_range) > 1:
            got.add("last:row-step-blocks")
    if last["kind"] == "folded":
        got.add("last:folded")
    for t, rows in enumerate(p.leaf_rows):
        if rows is not None and p.leaf_sl[t, 0] > 0 and p.slice_range[1] - p.slice_range[0] > 1 and \
                ((p.perms[:, 0] == ctr.LEAF) & (p.perms[:, 1] == t) & (p.perms[:, 6] == -1)).any():
            got.add("sliced-leaf-with-rows-gathered")
    projs = case.projs()
    n_rows, row_of_proj = p.out_rows
    if len(projs) == 1:
        got.add("P=1")
    if n_rows < len(projs):
        got.add("duplicate-projection")
    if (np.diff(row_of_proj) < 0).any():
        got.add("row_of_proj-not-monotone")
    if p.inds == (PROJ,):
        got.add("result-only-proj")
    if any(sum(x in xs for xs in case.ts_inds) >= 3 for x in case.sparse):
        got.add("sparse-hyper-index-on-3-tensors")
    return got


def caps(case):
    """The limits of a case that are broken, as strings; empty: the case is within all of them."""
    bad = []
    if not 4 <= len(case.ts_inds) <= 8:
        bad.append("leaves")
    if any(math.prod(s) > MAX_LEAF for s in case.shapes()):
        bad.append("leaf size")
    if not 1 <= case.n_assignments() <= MAX_ASSIGNMENTS:
        bad.append("assignments")
    if not 1 <= len(case.projs()) <= 64:
        bad.append("projections")
    try:
        p = case.plan()
    except (ValueError, NotImplementedError) as e:
        return bad + [str(e)]
    if p.macs > MAX_MACS:
        bad.append("multiply-adds")
    if p.arena_elems > MAX_ARENA:
        bad.append("arena")
    if p.out_numel > MAX_OUT or math.prod(p.shape) > MAX_OUT:
        bad.append("output size")
    if np.dtype(case.dtype) in SINGLES and kt(p) > cc.KT_SINGLE:
        bad.append("single precision beyond KT_SINGLE")
    return bad


def generate(seed, dtype=None, fill=None):
    """The case of a seed, or None when the network the seed gives is beyond the caps.  Deterministic: numpy's frozen
    RandomState stream and the project's own generators.  A single-precision dtype whose kt is beyond KT_SINGLE is
    widened to the double one of its kind."""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(4, 9))
    choices = mc.DIM_SETS[int(rng.randint(len(mc.DIM_SETS)))]
    if rng.randint(2):
        n += n % 2
        ts, _, _ = syn.random_regular_tn(n, seed=seed)
        n_inds = 1 + max(x for xs in ts for x in xs)
        dims = [int(choices[int(rng.randint(len(choices)))]) for _ in range(n_inds)]
    else:
        ts, dims, _ = syn.random_hyper_tn(n, n + int(rng.randint(0, n // 2 + 1)), k=3, n_output=0, seed=seed,
                                          dims_choices=choices)
    ts, dims = [[int(x) for x in xs] for xs in ts], [int(d) for d in dims]
    small = [d for d in choices if d <= 8] or [min(choices)]
    n_out = int(rng.randint(3, 7))
    opened = []
    for t in rng.choice(n, size=int(rng.randint(1, min(n, n_out) + 1)), replace=False):  # open indices
        ts[int(t)].append(len(dims))
        opened.append(len(dims))
        dims.append(int(small[int(rng.randint(len(small)))]))
    held = sorted({x for xs in ts for x in xs})
    shared = [x for x in held if x not in opened]
    more = rng.choice(shared, size=min(len(shared), n_out - len(opened)), replace=False) if n_out > len(opened) else []
    output = opened + [int(x) for x in more]
    n_sparse = min(int(rng.randint(2, 5)), len(output))
    hyper = [x for x in shared if sum(x in xs for xs in ts) >= 3]
    sparse = []
    if hyper:  # a sparse hyper-index held by three tensors where the generator offers one
        sparse.append(int(hyper[int(rng.randint(len(hyper)))]))
        if sparse[0] not in output:
            output.append(sparse[0])
    others = [x for x in output if x not in sparse]
    sparse += [int(x) for x in rng.choice(others, size=min(len(others), n_sparse - len(sparse)), replace=False)]
    sparse = [int(x) for x in rng.permutation(sparse)]
    ts = tuple(tuple(xs) for xs in ts)
    path = _random_path(len(ts), seed) if rng.randint(2) else _greedy_path(ts)
    free = [x for x in held if x not in sparse]
    slices = tuple(sorted(int(x) for x in rng.choice(free, size=min(len(free), int(rng.randint(1, 4))), replace=False)))
    total = math.prod(dims[x] for x in slices)
    slice_range = None
    if total > 3 and rng.randint(4) == 0:
        slice_range = (1 + int(rng.randint(2)), total - int(rng.randint(2)))
    spec = P_CHOICES[int(rng.randint(len(P_CHOICES)))]
    if math.prod(dims[x] for x in sparse) > 1 << 16:  # (Case.projs lists every assignment of the sparse indices)
        return None
    case = Case(f"seed-{seed}", ts, tuple((x, dims[x]) for x in held), tuple(sorted(output)), tuple(sparse), spec,
                tuple((int(a), int(b)) for a, b in path), slices, slice_range,
                np.dtype(dtype if dtype is not None else DTYPES[seed % 4]).name, fill or FILLS[(seed // 4) % 2])
    bad = caps(case)
    if bad == ["single precision beyond KT_SINGLE"]:
        case = case.with_(dtype={"float32": "float64", "complex64": "complex128"}[case.dtype])
        bad = caps(case)
    return None if bad else case


# which sparse indices the two branches hold: (branch 1, branch 2)
ROWS = {"both": (("s",), ("t",)), "a": (("s",), ("s", "t")), "b": (("s", "t"), ("t",)), "one-a": ((), ("t",)),
        "one-b": (("s",), ())}
SLICINGS = {  # the dimensions of the sliced (p, u, w)
    "puw": (2, 3, 2),  # 12 assignments, 6 added into every element of 2 blocks
    "u": (1, 2, 1),  # 2, both added into the one block
    "pu": (3, 2, 1),  # 6, three blocks
    "puw24": (2, 3, 4),  # 24
}


def two_branches(name, form, sizes, H, rows, dtype, fill, projs=11, sparse=None, stored=None, cut="puw", slice_range=None,
                 s_on_t1=False, st=(5, 3), inner=2):
    """A network written by hand, the two branches of `mode_cases.two_branches` with sparse indices: Z1 = T0 T1 with axes
    [rows of ROWS[rows][0]]([h], i0, i1) and Z2 = T2 T3 with [rows of ROWS[rows][1]]([h], j0, j1), both in the arena, and
    the step Z1 Z2 in the memory order `form` with sizes (M, N, K) and a batch axis h of dimension H (1: none): R the
    distinct rows of projs in the sparse indices of both, and the maps ROWS[rows] asks for.  T0 and T2 hold the sparse
    indices, and the sliced p and u behind them: their gathers run per assignment.  Sliced over u (held by T0 and T2,
    summed), w (held by T1 and T3, summed) and p (an axis of T0 and of the output: blocks that are revisited), of the
    dimensions SLICINGS[cut].  `s_on_t1`: T1 holds s too (a sparse hyper-index on three tensors; T0 T1 is then a row step).  `stored`: a fifth
    tensor takes the row step's result from the arena on to a last step -- "n": T4 (n, z), no sparse index, so Z is read
    in place with a null map beside an operand with one row; "v": T4 (v, n, z) with a third sparse index v, so Z is read
    through a map that repeats rows; "m": T4 (m, z), which Z's layout does not fit, so Z is permuted in the arena."""
    M, N, K = sizes
    fa, fb = form
    sa, sb = ROWS[rows]
    i0, i1 = ("k", "m") if fa else ("m", "k")
    j0, j1 = ("n", "k") if fb else ("k", "n")
    h = ("h",) if H > 1 else ()
    cut_inds, (dp, du, dw) = ("p", "u", "w"), SLICINGS[cut]
    ts = [sa + ("p", "u") + h + (i0, "c"), (("s",) if s_on_t1 else ()) + ("w", "c", i1), sb + ("u",) + h + (j0, "e"),
          ("w", "e", j1)]
    dims = dict(s=st[0], t=st[1], p=dp, u=du, w=dw, h=H, m=M, n=N, k=K, c=inner, e=inner)
    path = [(0, 1), (0, 1), (0, 1)]
    held = tuple(dict.fromkeys(sa + sb))
    output = held + ("p",) + h + ("m", "n")
    if stored:
        path = [(0, 1), (0, 1), (1, 2), (0, 1)]  # (T4 stays first: it is the first operand of the last step)
        dims["z"] = 3
        if stored == "v":
            ts.append(("v", "n", "z"))
            dims["v"] = 4
            held = held + ("v",)
            output = held + ("p",) + h + ("m", "z")
        elif stored == "n":
            ts.append(("n", "z"))
            output = held + ("p",) + h + ("m", "z")
        else:
            ts.append(("m", "z"))
            output = held + ("p",) + h + ("n", "z")
    if H == 1:
        del dims["h"]
    if "s" not in held:
        del dims["s"]
    if "t" not in held:
        del dims["t"]
    return Case(name, tuple(ts), tuple(dims.items()), output, tuple(sparse or held), projs, tuple(path), cut_inds, slice_range,
                np.dtype(dtype).name, fill)


TILED_A, TILED_B = (64, 64, 33), (65, 65, 48)
DOT, STREAM = (4, 5, 512), (9, 7, 5)
# networks written by hand: the step Z1 Z2 in each row class at its smallest edge (the sizes of
# tests/test_gpu_contract_rows.py), with every combination of maps, rows in place and one-row operands on arena operands
HAND = {
    # tiled: the four layouts, 64 x 64 x 33 and 65 x 65 x 48, H in {1, 3}
    "tiled-both-00": dict(form=(0, 0), sizes=TILED_A, H=1, rows="both", sparse=("t", "s")),
    "tiled-both-11-h3": dict(form=(1, 1), sizes=TILED_B, H=3, rows="both", cut="u", projs=7),
    "tiled-a-01": dict(form=(0, 1), sizes=TILED_B, H=1, rows="a", cut="pu"),
    "tiled-a-10": dict(form=(1, 0), sizes=TILED_A, H=1, rows="a", sparse=("t", "s"), slice_range=(5, 11)),
    "tiled-b-10": dict(form=(1, 0), sizes=TILED_B, H=1, rows="b", cut="u"),
    "tiled-b-01-h3": dict(form=(0, 1), sizes=TILED_A, H=3, rows="b", cut="u", projs=7),
    "tiled-one-a-00": dict(form=(0, 0), sizes=TILED_B, H=1, rows="one-a", cut="pu"),
    "tiled-one-a-11": dict(form=(1, 1), sizes=TILED_A, H=1, rows="one-a", projs="all"),
    "tiled-one-b-10": dict(form=(1, 0), sizes=TILED_A, H=1, rows="one-b", cut="pu"),
    "tiled-one-b-00-h3": dict(form=(0, 0), sizes=TILED_A, H=3, rows="one-b", cut="u", projs="all"),
    # dot 4 x 5 x 512
    "dot-both": dict(form=(0, 0), sizes=DOT, H=1, rows="both", sparse=("t", "s"), cut="pu"),
    "dot-both-h3": dict(form=(0, 1), sizes=DOT, H=3, rows="both", cut="u", projs=("distinct", 9)),
    "dot-a": dict(form=(0, 1), sizes=DOT, H=1, rows="a", cut="pu"),
    "dot-a-h3": dict(form=(1, 0), sizes=DOT, H=3, rows="a", cut="u"),
    "dot-b": dict(form=(0, 0), sizes=DOT, H=1, rows="b", cut="pu", projs="all"),
    "dot-b-10": dict(form=(1, 0), sizes=DOT, H=1, rows="b", cut="u"),
    "dot-one-a": dict(form=(0, 0), sizes=DOT, H=1, rows="one-a", cut="pu"),
    "dot-one-a-h3": dict(form=(0, 1), sizes=DOT, H=3, rows="one-a", cut="u"),
    "dot-one-b-10": dict(form=(1, 0), sizes=DOT, H=1, rows="one-b", cut="pu"),
    "dot-one-b-h3": dict(form=(0, 0), sizes=DOT, H=3, rows="one-b", cut="u"),
    # stream 9 x 7 x 5
    "stream-both": dict(form=(0, 0), sizes=STREAM, H=1, rows="both", sparse=("t", "s"), cut="puw24"),
    "stream-both-h3": dict(form=(1, 1), sizes=STREAM, H=3, rows="both", projs=2),
    "stream-a": dict(form=(0, 1), sizes=STREAM, H=1, rows="a", s_on_t1=True),
    "stream-a-h3": dict(form=(1, 0), sizes=STREAM, H=3, rows="a", s_on_t1=True, projs=("distinct", 13)),
    "stream-b": dict(form=(0, 0), sizes=STREAM, H=1, rows="b", projs=1),
    "stream-b-h3": dict(form=(1, 1), sizes=STREAM, H=3, rows="b", projs=1),
    "stream-one-a": dict(form=(0, 0), sizes=STREAM, H=1, rows="one-a"),
    "stream-one-a-h3": dict(form=(0, 1), sizes=STREAM, H=3, rows="one-a"),
    "stream-one-b-10": dict(form=(1, 0), sizes=STREAM, H=1, rows="one-b"),
    "stream-one-b-h3": dict(form=(0, 0), sizes=STREAM, H=3, rows="one-b"),
    # the last step folded (only Z1 has rows, [r][m][k], H = 1): a plain GEMM that reads a row tensor from the arena
    "tiled-last-folded": dict(form=(0, 0), sizes=TILED_A, H=1, rows="one-b", cut="pu"),
    "stream-last-folded": dict(form=(0, 1), sizes=STREAM, H=1, rows="one-b"),
    # stored: the row step's result goes on from the arena
    "tiled-stored-n": dict(form=(0, 1), sizes=TILED_A, H=1, rows="both", stored="n", sparse=("t", "s")),
    "stream-stored-n-h3": dict(form=(1, 0), sizes=STREAM, H=3, rows="both", stored="n"),
    "dot-stored-v": dict(form=(0, 0), sizes=DOT, H=1, rows="both", stored="v", cut="pu", projs=24, sparse=("v", "t", "s")),
    "stream-stored-v-h3": dict(form=(0, 0), sizes=STREAM, H=3, rows="both", stored="v", projs=40),
    "tiled-stored-m": dict(form=(1, 1), sizes=TILED_A, H=1, rows="both", stored="m", cut="pu"),
    "stream-stored-m-h3": dict(form=(0, 1), sizes=STREAM, H=3, rows="a", stored="m"),
}

# (a name of HAND, dtype), the fills alternating, or a seed of `generate` (dtype and fill are the seed's own).  Every pair
# of hand cases that reaches the same items has one real and one complex dtype, and every class runs in all four
TABLE = (
    ("tiled-both-00", "float32"), ("tiled-both-11-h3", "complex64"), ("tiled-a-01", "complex128"), ("tiled-a-10", "float64"),
    ("tiled-b-10", "complex64"), ("tiled-b-01-h3", "float32"), ("tiled-one-a-00", "complex128"),
    ("tiled-one-a-11", "float32"), ("tiled-one-b-10", "float64"), ("tiled-one-b-00-h3", "complex64"),
    ("dot-both", "float32"), ("dot-both-h3", "complex128"), ("dot-a", "complex64"), ("dot-a-h3", "float64"),
    ("dot-b", "float64"), ("dot-b-10", "complex64"), ("dot-one-a", "complex128"), ("dot-one-a-h3", "float32"),
    ("dot-one-b-10", "float32"), ("dot-one-b-h3", "complex64"),
    ("stream-both", "float64"), ("stream-both-h3", "complex64"), ("stream-a", "complex128"), ("stream-a-h3", "float32"),
    ("stream-b", "float32"), ("stream-b-h3", "complex128"), ("stream-one-a", "complex64"), ("stream-one-a-h3", "float64"),
    ("stream-one-b-10", "float64"), ("stream-one-b-h3", "complex128"),
    ("tiled-last-folded", "float32"), ("stream-last-folded", "complex64"),
    ("tiled-stored-n", "float64"), ("stream-stored-n-h3", "complex64"), ("dot-stored-v", "complex128"),
    ("stream-stored-v-h3", "float32"), ("tiled-stored-m", "complex64"), ("stream-stored-m-h3", "float64"),
    4, 6, 16, 47, 48, 59, 78, 80, 89, 100, 124, 183, 192, 242, 264, 296, 346, 357, 440, 547, 628, 638, 646, 673,
)


def make(row, k=0):
    if isinstance(row, tuple):
        return two_branches("hand-" + row[0], dtype=row[1], fill=FILLS[k % 2], **HAND[row[0]])
    return generate(row)


CASES = tuple(make(row, k) for k, row in enumerate(TABLE))
IDS = tuple(f"{c.name}-{c.dtype}" for c in CASES)
BY_NAME = {c.name: c for c in CASES}
