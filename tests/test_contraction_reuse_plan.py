"""`reuse=True` and `slice_order=` in the plan (tnco_amd/contraction.py), without a GPU: the period of every step and
permute against the definition, what the keywords refuse, what a call then costs in multiply-adds, how "reuse" orders
the sliced indices, and -- with a numpy interpreter of the plan's tables on one flat arena -- that the phases never step
on each other.

The interpreter runs the loop as the library does: at every assignment the phases that are due, the slowest first, each
in path order.  Before a phase of period P runs it fills with NaN every element outside the kept buffers of periods above
P -- what that phase and the faster ones may use -- and after an assignment everything outside the kept buffers; with
scaling it fills a step's staging buffer with NaN before the step's result is written.  A buffer that overlaps a kept
one of a slower phase, a kept tensor read before it is written or after something else was, or an operand released too
early would leave a NaN in the result, which is held to numpy's einsum of the whole network in double precision."""
import itertools
import math

import numpy as np
import pytest

from tests import mode_cases as mc
from tests import reuse_cases as rc
from tests import schedule_cases as sc
from tnco_amd import contraction as ctr

TABLES = ("leaf_numel", "leaf_sl", "perms", "steps")
OLD = [(n, rc.case(n)) for n in rc.NAMES] + [(i, c) for i, c in zip(mc.IDS, mc.CASES)]
ALL = OLD + [(f"{c.name}-{c.dtype}", c) for c in sc.EXTRA]
IDS = [n for n, _ in ALL]


def same_plan(p, q):
    return all(np.array_equal(getattr(p, t), getattr(q, t)) and getattr(p, t).dtype == getattr(q, t).dtype for t in TABLES) and \
        (p.arena_elems, p.out_numel, p.macs_per_slice, p.macs, p.peak_device_bytes, p.ops, p.inds, p.shape, p.slice_range,
         p.slice_inds, p.slice_dims, p.block_inds) == \
        (q.arena_elems, q.out_numel, q.macs_per_slice, q.macs, q.peak_device_bytes, q.ops, q.inds, q.shape, q.slice_range,
         q.slice_inds, q.slice_dims, q.block_inds)


@pytest.mark.parametrize("mode", [dict(), dict(hoist=True), dict(indirect=True), dict(storage="float16", scaling="tensor")],
                         ids=["plain", "hoist", "indirect", "scaled"])
@pytest.mark.parametrize("name,case", ALL, ids=IDS)
def test_without_the_keywords_nothing_changes(name, case, mode):
    if "storage" in mode:
        case = case.with_(dtype="complex64" if np.dtype(case.dtype).kind == "c" else "float32")
    p, q = case.plan(**mode), case.plan(reuse=None, slice_order=None, **mode)
    assert same_plan(p, q)
    assert q.reused is None and q.step_period is None and q.perm_period is None and q.kept_period == ()
    assert p.kept == q.kept and p.hoisted == q.hoisted and p.indirect == q.indirect
    if p.ind_steps is not None:
        assert np.array_equal(p.ind_steps, q.ind_steps) and np.array_equal(p.ind_maps, q.ind_maps)
    if p.scaling is not None:
        assert np.array_equal(p.stage_refs, q.stage_refs)
    # reuse changes where things lie and how often they run, not what a step is
    r = case.plan(reuse=True, **{k: v for k, v in mode.items() if k != "hoist"})
    assert np.array_equal(r.steps[:, 10:14], p.steps[:, 10:14]) and r.macs_per_slice == p.macs_per_slice
    assert [{k: v for k, v in op.items() if not k.startswith("ind_")} for op in r.ops] == \
        [{k: v for k, v in op.items() if not k.startswith("ind_")} for op in p.ops]
    if "indirect" not in mode:
        assert sorted(map(tuple, r.perms[:, 4:].tolist())) == sorted(map(tuple, p.perms[:, 4:].tolist()))


def test_no_reuse_possible_gives_the_plain_plan():
    c = rc.case("kept-first-stream-7-9-11")
    unsliced = c.with_(slices=())
    p = unsliced.plan(reuse=True)
    assert same_plan(p, unsliced.plan()) and p.reused == (0, 0) and p.kept == () and (p.step_period == 1).all()
    assert same_plan(unsliced.plan(reuse=True, indirect=True), unsliced.plan(indirect=True))
    # every leaf holds the fastest index: every period is 1
    ts = (("u", "w", "a", "b"), ("w", "b", "c"), ("u", "w", "c", "d"), ("w", "d", "a"))
    every = mc.Case("every", ts, tuple(dict(u=2, w=3, a=4, b=5, c=3, d=2).items()), (), ((0, 1), (0, 1), (0, 1)), ("u", "w"),
                    "float64", "uniform")
    for mode in (dict(), dict(indirect=True)):
        p = every.plan(reuse=True, **mode)
        assert same_plan(p, every.plan(**mode)) and p.reused == (0, 0) and p.kept == () and (p.step_period == 1).all()
        assert p.indirect == every.plan(**mode).indirect
    # a single leaf gathered into the output
    p = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), reuse=True)
    assert p.reused == (0, 0) and same_plan(p, ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",)))


@pytest.mark.parametrize("order", rc.ORDERS, ids=rc.ORDER_IDS)
@pytest.mark.parametrize("name,case", ALL, ids=IDS)
def test_periods_are_those_of_the_definition(name, case, order):
    p = case.plan(reuse=True, **rc.order_kw(case, order))
    step_dep, perm_dep = rc.deps(case, p)
    for per, dep in list(zip(p.step_period, step_dep)) + list(zip(p.perm_period, perm_dep)):
        assert rc.needed(p, dep) == [a for a in range(p.n_slices) if a % int(per) == 0], (per, dep)
    assert p.step_period.dtype == p.perm_period.dtype == np.int64
    assert p.reused == (int((p.step_period > 1).sum()), int((p.perm_period > 1).sum()))
    if p.n_slices > 1 and len(p.steps):
        assert p.step_period[-1] == 1
    if name in rc.TABLE and order is None:
        assert p.slice_inds == ("p", "u", "w") and p.reused == rc.TABLE[name][1]
    # within a permute group the rows of one period are together, the slowest first, and the groups are still sorted
    assert (np.diff(p.perms[:, 6]) >= 0).all()
    for g in set(p.perms[:, 6].tolist()):
        assert (np.diff(p.perm_period[p.perms[:, 6] == g]) <= 0).all()
    # kept: what a faster item reads of a slower one
    assert len(p.kept) == len(p.kept_period) and all(q > 1 for q in p.kept_period)


def test_the_cases_hold_what_they_are_for():
    sig = lambda n, k: mc.signature(rc.case(n).plan(reuse=True))[k][0]  # noqa: E731
    for n in rc.NAMES:
        if n.startswith("kept-"):
            p = rc.case(n).plan(reuse=True)
            assert sig(n, 2) == rc.TABLE[n][2]
            side = 0 if n.startswith("kept-first") else 1  # (the step on u: the first of the path, or the second)
            assert p.step_period[side] == 2 and p.steps[2][4 * side] == ctr.ARENA
            assert (int(p.steps[2][4 * side + 1]), int(p.steps[side][10:13].prod())) in p.kept
            assert sorted(p.step_period.tolist()) == [1, 1, 1, 2] and p.kept_period == (2,)
            assert tuple(int(v) for v in p.steps[2][11:14]) == rc.EDGES[n.split("-", 2)[2]]
    p = rc.case("nested").plan(reuse=True)
    assert p.step_period.tolist() == [6, 2, 1, 1] and sorted(p.kept_period) == [2, 6]
    p = rc.case("nested-deep").plan(reuse=True)  # (the slowest phase's temporary where the faster phase keeps its result)
    assert p.step_period.tolist() == [6, 6, 2, 1, 1] and p.kept_period == (6, 2) and p.steps[0][9] == p.steps[2][9] == p.kept[1][0]
    p = rc.case("two-kept").plan(reuse=True)
    assert p.step_period.tolist() == [2, 2, 1, 1, 1, 1] and p.kept_period == (2, 2) and p.kept[0][0] != p.kept[1][0]
    p = rc.case("chain").plan(reuse=True)
    assert p.step_period.tolist() == [2, 2, 12, 1, 1, 1, 1] and sorted(p.kept_period) == [2, 12]
    p = rc.case("leaf-gather").plan(reuse=True)
    assert p.perm_period.tolist().count(2) == 1 and p.perms[p.perm_period == 2][0][[0, 6]].tolist() == [ctr.LEAF, -1]
    p = rc.case("arena-permute").plan(reuse=True)
    row = p.perms[p.perm_period == 2][0]
    assert row[0] == ctr.ARENA and row[2] == ctr.ARENA and (int(row[3]), int(row[5])) in p.kept
    # another order, other periods: under (w, u, p) the steps on u keep period 2 and the step on p becomes every assignment's
    p = rc.case("nested").plan(reuse=True, slice_order=("w", "u", "p"))
    assert p.slice_inds == ("w", "u", "p") and p.slice_dims == (2, 3, 2) and p.step_period.tolist() == [1, 1, 2, 1]
    p = rc.case("chain").plan(reuse=True, slice_order=("w", "u", "p"))
    assert p.step_period.tolist() == [2, 2, 12, 6, 2, 2, 1]


@pytest.mark.parametrize("order", rc.ORDERS, ids=rc.ORDER_IDS)
@pytest.mark.parametrize("name,case", ALL, ids=IDS)
def test_macs_are_those_of_the_enumeration(name, case, order):
    p = case.plan(reuse=True, **rc.order_kw(case, order))
    lo, hi = p.slice_range
    step_dep, _ = rc.deps(case, p)
    each = [int(r[10]) * int(r[11]) * int(r[12]) * int(r[13]) for r in p.steps]
    # an item runs at the first assignment of the range and wherever an index below it changes
    want = sum(m * len({lo} | {a for a in rc.needed(p, dep) if lo <= a < hi}) for m, dep in zip(each, step_dep))
    assert p.macs == want == rc.predicted(p)["macs"]
    assert p.macs <= case.plan(hoist=True).macs <= case.plan().macs
    if order == "reuse":
        assert p.macs <= case.plan(reuse=True).macs
        if p.slice_inds != case.plan().slice_inds:
            assert p.macs < case.plan(reuse=True).macs


def greedy_rule(case):
    """slice_order="reuse" restated: the fastest place first; of the indices left the one with the least multiply-adds in
    the steps not yet covered that hold it, ties to the later one in the default order."""
    p = case.plan()
    step_dep, _ = rc.deps(case, p)
    each = [int(np.prod(r[10:14], dtype=np.int64)) for r in p.steps]
    left, covered, fastest_first = list(p.slice_inds), set(), []
    while left:
        best = None
        for x in left:
            cost = sum(m for k, (m, d) in enumerate(zip(each, step_dep)) if k not in covered and x in d)
            if best is None or cost <= best[0]:
                best = (cost, x)
        fastest_first.append(best[1])
        left.remove(best[1])
        covered |= {k for k, d in enumerate(step_dep) if best[1] in d}
    return tuple(reversed(fastest_first))


@pytest.mark.parametrize("name", ["nested", "chain", "arena-permute", "kept-first-stream-7-9-11", "nested-range-3-9"])
def test_the_reuse_order_is_the_greedy_rule(name):
    case = rc.case(name)
    by_order = {o: case.plan(reuse=True, slice_order=o).macs for o in itertools.permutations(rc.SLICES)}
    default, greedy = case.plan().slice_inds, greedy_rule(case)
    p = case.plan(reuse=True, slice_order="reuse")
    assert p.slice_inds == (greedy if by_order[greedy] < by_order[default] else default)
    assert p.macs == by_order[p.slice_inds] <= by_order[default]
    assert same_plan(p, case.plan(reuse=True, slice_order=p.slice_inds))
    print(name, default, greedy, by_order)


def test_the_reuse_order_moves_something():
    moved = [c.plan(reuse=True, slice_order="reuse").slice_inds != c.plan().slice_inds for _, c in OLD]
    assert sum(moved) >= 3  # (a count: over the list it was written for)
    for _, c in ALL:
        assert c.plan(reuse=True, slice_order="reuse").slice_inds == \
            (greedy_rule(c) if c.plan(reuse=True, slice_order=greedy_rule(c)).macs < c.plan(reuse=True).macs else c.plan().slice_inds)


def test_a_named_order_renumbers_the_assignments():
    c = rc.case("nested")
    p, q = c.plan(), c.plan(slice_order=("w", "u", "p"))
    assert q.slice_inds == ("w", "u", "p") and q.slice_dims == (2, 3, 2) and q.block_inds == ("p",) and p.block_inds == ("p",)
    assert same_plan(c.plan(slice_order=("p", "u", "w")), p) and same_plan(c.plan(slice_order=["p", "u", "w"]), p)
    # the slot of a sliced axis of a leaf is its position in the order
    for t, xs in enumerate(c.ts_inds):
        cut = [x for x in xs if x in c.slices]
        assert q.leaf_sl[t, 1:1 + len(cut)].tolist() == [q.slice_inds.index(x) for x in cut]
    assert q.macs == p.macs and q.reused is None


def test_refusals_and_their_order():
    c = rc.case("kept-first-stream-7-9-11")
    args = (list(c.path), c.ts_inds, c.shapes(), c.output_inds)
    kw = dict(slices=c.slices, dtype=np.float32)
    order_text = "'slice_order' must be None, 'reuse' or every sliced index once."
    for bad in (False, 1, 0, "yes", 2.0, np.True_):
        with pytest.raises(ValueError, match="'reuse' must be None or True"):
            ctr.plan(*args, reuse=bad, **kw)
    with pytest.raises(ValueError) as e:
        ctr.plan(*args, reuse=True, hoist=True, **kw)
    assert str(e.value) == "'reuse' includes 'hoist': give one of them."
    with pytest.raises(NotImplementedError, match="'slice_batch' is not supported with 'reuse'"):
        ctr.plan(*args, reuse=True, slice_batch=4, **kw)
    with pytest.raises(NotImplementedError, match="'path_kernel' is not supported with 'reuse'"):
        ctr.plan(*args, reuse=True, path_kernel=4, **kw)
    # the order: value, hoist, slice_batch, path_kernel, projections; the checks of the other keywords come first
    with pytest.raises(ValueError, match="'reuse' must be None or True"):
        ctr.plan(*args, reuse=False, hoist=True, slice_batch=4, **kw)
    with pytest.raises(ValueError, match="'reuse' includes 'hoist'"):
        ctr.plan(*args, reuse=True, hoist=True, slice_batch=4, **kw)
    with pytest.raises(NotImplementedError, match="'hoist' is not supported with 'path_kernel'"):
        ctr.plan(*args, reuse=True, hoist=True, path_kernel=4, **kw)
    with pytest.raises(ValueError, match="'path_kernel' and 'slice_batch' are exclusive"):
        ctr.plan(*args, reuse=True, path_kernel=4, slice_batch=2, **kw)
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.plan(*args, reuse=True, hoist=False, **kw)
    with pytest.raises(ValueError, match="'indirect' must be None or True"):
        ctr.plan(*args, reuse=3, indirect=False, **kw)
    with pytest.raises(ValueError, match="'scaling' needs 'storage'"):
        ctr.plan(*args, reuse="x", scaling="tensor", **kw)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    projs = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    with pytest.raises(NotImplementedError, match="projections are not supported with 'reuse'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), reuse=True, **projs)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'slice_order'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), slice_order=(), **projs)
    with pytest.raises(ValueError, match="'reuse' must be None or True"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), reuse=0, **projs)
    # slice_order
    for bad in ("greedy", "", ("p", "u"), ("p", "u", "w", "w"), ("p", "u", "x"), ("p", "p", "u"), 3, ["p", ["u"], "w"], ()):
        with pytest.raises(ValueError) as e:
            ctr.plan(*args, slice_order=bad, reuse=True, **kw)
        assert str(e.value) == order_text, bad
    with pytest.raises(ValueError, match="slice_order='reuse' needs reuse=True"):
        ctr.plan(*args, slice_order="reuse", **kw)
    with pytest.raises(ValueError, match="'reuse' must be None or True"):  # (reuse is checked before slice_order)
        ctr.plan(*args, slice_order="reuse", reuse=False, **kw)
    # contract and contract_results refuse before any device use: no library is loaded for these
    arrays = [np.zeros(s, np.float32) for s in c.shapes()]
    call = lambda **k: ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, **k)  # noqa: E731
    with pytest.raises(ValueError, match="'reuse' must be None or True"):
        call(reuse=False)
    with pytest.raises(ValueError, match="'reuse' includes 'hoist'"):
        call(reuse=True, hoist=True)
    with pytest.raises(NotImplementedError, match="'slice_batch' is not supported with 'reuse'"):
        call(reuse=True, slice_batch=2)
    with pytest.raises(ValueError) as e:
        call(slice_order=("p", "u"))
    assert str(e.value) == order_text
    with pytest.raises(ValueError, match="slice_order='reuse' needs reuse=True"):
        call(slice_order="reuse")
    with pytest.raises(ValueError, match="'reuse' must be None or True"):
        ctr.contract_results(None, None, None, None, reuse="True")
    with pytest.raises(ValueError, match="'reuse' includes 'hoist'"):
        ctr.contract_results(None, None, None, None, reuse=True, hoist=True)
    with pytest.raises(NotImplementedError, match="'path_kernel' is not supported with 'reuse'"):
        ctr.contract_results(None, None, None, None, reuse=True, path_kernel=8)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'reuse'"):
        ctr.contract_results(None, None, None, None, reuse=True, projs=np.zeros((1, 1), np.int64))
    with pytest.raises(NotImplementedError, match="projections are not supported with 'slice_order'"):
        ctr.contract_results(None, None, None, None, slice_order=("a",), projs=np.zeros((1, 1), np.int64))
    with pytest.raises(ValueError, match="slice_order='reuse' needs reuse=True"):
        ctr.contract_results(None, None, None, None, slice_order="reuse")


def test_the_result_and_the_plan_have_the_new_fields():
    r = ctr.ContractionResult((), None, 0, 1, 0)
    assert r.reused is None
    p = rc.case("nested").plan(reuse=True)
    assert p.reused == (2, 0) and len(p.kept) == 2 and p.hoisted is None and p.step_hoist is None
    # the kept buffers cost arena: the plan says how much
    assert p.arena_elems >= sum(-(-n // ctr.ALIGN) * ctr.ALIGN for _, n in p.kept)
    assert p.peak_device_bytes - rc.case("nested").plan().peak_device_bytes == 4 * (p.arena_elems - rc.case("nested").plan().arena_elems)


def interpret(case, p, arrays):
    """The plan's tables run with numpy on one flat arena, in double precision (module docstring)."""
    wide = np.complex128 if any(np.iscomplexobj(a) for a in arrays) else np.float64
    leaves = [np.ascontiguousarray(a, wide).reshape(-1) for a in arrays]
    arena = np.full(max(p.arena_elems, 1), np.nan, wide)
    n_blocks = math.prod(p.shape[p.inds.index(x)] for x in p.block_inds)
    block = p.out_numel // n_blocks
    out = np.zeros(p.out_numel, wide)
    place = [math.prod(p.slice_dims[s + 1:]) for s in range(len(p.slice_dims))]
    step_per, perm_per = rc.periods(p)
    phases = sorted(set(step_per.tolist()) | set(perm_per.tolist()) | {1}, reverse=True)

    def outside_kept_above(per):
        mask = np.ones(len(arena), bool)
        for (off, numel), q in zip(p.kept, p.kept_period):
            if q > per:
                mask[off:off + numel] = False
        return mask

    def slice_offset(leaf, sid):
        ls = p.leaf_sl[leaf]
        return sum(((sid // place[int(ls[1 + j])]) % p.slice_dims[int(ls[1 + j])]) * int(ls[1 + ctr.MAX_AXES + j])
                   for j in range(int(ls[0])))

    def gather(row, sid, out_off):
        nd = int(row[4])
        dims, strides = row[8:8 + nd], row[8 + ctr.MAX_AXES:8 + ctr.MAX_AXES + nd]
        idx = np.zeros(tuple(int(d) for d in dims), np.int64)
        for k in range(nd):
            shape = [1] * nd
            shape[k] = int(dims[k])
            idx = idx + (np.arange(int(dims[k])) * int(strides[k])).reshape(shape)
        idx = idx.reshape(-1)
        if row[0] == ctr.LEAF:
            vals = leaves[int(row[1])][idx + slice_offset(int(row[1]), sid)]
        else:
            vals = arena[idx + int(row[1])]
        if row[2] == ctr.ARENA:
            arena[int(row[3]):int(row[3]) + int(row[5])] = vals
        else:
            out[out_off:out_off + block] = vals

    def operand(kind, ref, sid, H, R, Kc, sr, sk, tabs):
        """[H][R][Kc] of a batch operand: dense, rows sr and columns sk apart, or through its three offset tables."""
        base = leaves[int(ref)][slice_offset(int(ref), sid):] if kind == ctr.LEAF else arena[int(ref):]
        if tabs is not None:
            th, tr, tk = (p.ind_maps[int(o):int(o) + n] for o, n in zip(tabs, (H, R, Kc)))
            return base[th.reshape(-1, 1, 1) + tr.reshape(1, -1, 1) + tk.reshape(1, 1, -1)]
        idx = (np.arange(H) * R * Kc).reshape(-1, 1, 1) + (np.arange(R) * sr).reshape(1, -1, 1) + (np.arange(Kc) * sk).reshape(1, 1, -1)
        return base[idx]

    def step(k, sid, out_off, beta):
        st = [int(v) for v in p.steps[k]]
        H, M, N, K = st[10:14]
        ix = None if p.ind_steps is None else p.ind_steps[k]
        ta = ix[0:3] if ix is not None and ix[0] >= 0 else None  # (A: h, m, k)
        tb = ix[[3, 5, 4]] if ix is not None and ix[3] >= 0 else None  # (B: h, k, n; taken here as [h][n][k])
        A = operand(st[0], st[1], sid, H, M, K, st[2], st[3], ta)
        Bm = operand(st[4], st[5], sid, H, N, K, st[7], st[6], tb)
        if p.scaling is not None and p.stage_refs[k] >= 0:
            arena[int(p.stage_refs[k]):int(p.stage_refs[k]) + 2 * H * M * N] = np.nan
        Cm = np.einsum("hmk,hnk->hmn", A, Bm).reshape(-1)
        if st[8] == ctr.ARENA:
            arena[st[9]:st[9] + H * M * N] = Cm
        else:
            out[out_off:out_off + block] = out[out_off:out_off + block] + Cm if beta else Cm

    visited = set()
    for sid in range(*p.slice_range):
        blk = 0
        for x in p.block_inds:
            s = p.slice_inds.index(x)
            blk = blk * p.slice_dims[s] + (sid // place[s]) % p.slice_dims[s]
        for per in phases:
            if sid != p.slice_range[0] and sid % per:
                continue
            arena[outside_kept_above(per)] = np.nan
            for g in [-1] + list(range(len(p.steps))):
                for r in np.nonzero((p.perms[:, 6] == g) & (perm_per == per))[0]:
                    gather(p.perms[r], sid, blk * block)
                if g >= 0 and step_per[g] == per:
                    step(g, sid, blk * block, blk in visited)
        visited.add(blk)
        arena[outside_kept_above(0)] = np.nan
    return ctr._host_layout(p, out)


@pytest.mark.parametrize("mode", [dict(), dict(storage="float16", scaling="tensor"), dict(indirect=True)],
                         ids=["plain", "scaled", "indirect"])
@pytest.mark.parametrize("order", rc.ORDERS, ids=rc.ORDER_IDS)
@pytest.mark.parametrize("name,case", ALL, ids=IDS)
def test_the_tables_interpreted_on_one_arena_give_the_einsum(name, case, order, mode):
    c32 = case.with_(dtype="complex64" if np.dtype(case.dtype).kind == "c" else "float32")
    p = c32.plan(reuse=True, **rc.order_kw(case, order), **mode)
    arrays = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in mc.fill(case)]
    ref, mag = mc.reference(c32, p, arrays)
    got = interpret(c32, p, arrays)
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{name}: a buffer was read that nothing valid was in"
    assert (np.abs(got - ref) <= 1e-12 * mc.kt(p) * mag).all()
    if name in rc.TABLE and order is None:
        # the plain plan of the same case passes through the same interpreter with no kept buffer at all
        q = c32.plan(**mode)
        assert q.kept == () and np.allclose(interpret(c32, q, arrays), got, rtol=1e-12, atol=0)


def test_indirect_folds_at_the_steps_period_only():
    """An operand is folded iff its tables are small enough, its source is not slice-free and has the period of the step;
    the permute of a slower source stays, runs at the source's period, and its copy is kept."""
    folded = kept_permutes = 0
    for name, case in ALL:
        plain, p = case.plan(reuse=True), case.plan(reuse=True, indirect=True)
        step_dep, perm_dep = rc.deps(case, p)
        assert p.step_period.tolist() == plain.step_period.tolist() and p.macs == plain.macs
        slower = 0
        for r, row in enumerate(p.perms):
            k = int(row[6])  # (an arena-to-arena permute feeds the step of its group)
            if k < 0 or row[2] != ctr.ARENA:
                continue
            size_ok = 8 * sum(int(v) for v in _groups(p, k, row)) <= p.dtype.itemsize * int(row[5])
            if size_ok:  # it stayed a permute although its tables would be small: slower than its step, or slice-free
                # (slice-free: a sliced index of dimension 1 never changes and is no dependency)
                assert p.perm_period[r] > p.step_period[k] or not any(case.dim[x] > 1 for x in perm_dep[r]), (name, r)
                slower += int(p.perm_period[r] > p.step_period[k])
                if p.perm_period[r] > p.step_period[k]:
                    assert (int(row[3]), int(row[5])) in p.kept
        if (name, case) in OLD:  # (the counts: over the list they were written for)
            folded, kept_permutes = folded + p.indirect, kept_permutes + slower
    assert folded >= 10 and kept_permutes >= 3


def _groups(p, k, row):
    """H + M + K (or H + K + N) of the operand of step k that the permute row writes."""
    st = p.steps[k]
    side = 0 if st[0] == ctr.ARENA and st[1] == row[3] else 1
    return (st[10], st[13], st[12] if side else st[11])
