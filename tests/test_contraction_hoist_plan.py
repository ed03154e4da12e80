"""`hoist=True` in the plan (tnco_amd/contraction.py), without a GPU: which steps and permutes are flagged, what the
keyword refuses, what a call then costs in multiply-adds, launches and device memory, and -- with a numpy interpreter of
the plan's tables on one flat arena -- that the hoisted phase and the assignments never step on each other.

The interpreter runs the hoisted items once, then every assignment of the range; it fills the whole arena with NaN
before the hoisted phase and everything outside the kept buffers with NaN after each assignment, and with scaling it
fills a step's staging buffer with NaN before the step's result is written.  A buffer of an assignment that overlaps a
kept one, a kept tensor read before it is written, or an operand that the plan released too early would leave a NaN in
the result, which is held to numpy's einsum of the whole network in double precision."""
import math

import numpy as np
import pytest

from tests import hoist_cases as hc
from tests import mode_cases as mc
from tests import schedule_cases as sc
from tnco_amd import contraction as ctr

TABLES = ("leaf_numel", "leaf_sl", "perms", "steps")
ALL = [(n, hc.case(n)) for n in hc.NAMES] + [(i, c) for i, c in zip(sc.IDS, sc.CASES)]  # (mode_cases.CASES and EXTRA)


def same_plan(p, q):
    return all(np.array_equal(getattr(p, t), getattr(q, t)) and getattr(p, t).dtype == getattr(q, t).dtype for t in TABLES) and \
        (p.arena_elems, p.out_numel, p.macs_per_slice, p.macs, p.peak_device_bytes, p.ops, p.inds, p.shape, p.slice_range) == \
        (q.arena_elems, q.out_numel, q.macs_per_slice, q.macs, q.peak_device_bytes, q.ops, q.inds, q.shape, q.slice_range)


@pytest.mark.parametrize("name,case", ALL, ids=[n for n, _ in ALL])
def test_without_the_keyword_nothing_changes(name, case):
    p, q = case.plan(), case.plan(hoist=None)
    assert same_plan(p, q)
    assert q.hoisted is None and q.step_hoist is None and q.perm_hoist is None and q.kept == () and q.hoisted_macs == 0
    assert p.macs == p.macs_per_slice * case.n_assignments()
    # the rows of the permute table are in the order of the plan without the keyword unless a group mixes the two kinds
    h = case.plan(hoist=True)
    assert sorted(map(tuple, h.perms[:, 4:].tolist())) == sorted(map(tuple, p.perms[:, 4:].tolist()))
    assert np.array_equal(h.steps[:, 10:14], p.steps[:, 10:14]) and h.macs_per_slice == p.macs_per_slice


def test_nothing_to_hoist_gives_the_plain_plan():
    c = hc.case("kept-first-stream-7-9-11")
    unsliced = c.with_(slices=())
    p = unsliced.plan(hoist=True)
    assert same_plan(p, unsliced.plan()) and p.hoisted == (0, 0) and not p.step_hoist.any() and not p.perm_hoist.any()
    # every leaf holds a sliced index
    ts = (("u", "a", "b"), ("u", "b", "c"), ("w", "c", "d"), ("w", "d", "a"))
    every = mc.Case("every", ts, tuple(dict(u=2, w=3, a=4, b=5, c=3, d=2).items()), (), ((0, 1), (0, 1), (0, 1)), ("u", "w"),
                    "float64", "uniform")
    p = every.plan(hoist=True)
    assert same_plan(p, every.plan()) and p.hoisted == (0, 0) and p.kept == () and p.hoisted_macs == 0
    # a single leaf gathered into the output
    p = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), hoist=True)
    assert p.hoisted == (0, 0) and same_plan(p, ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",)))


@pytest.mark.parametrize("name,case", ALL, ids=[n for n, _ in ALL])
def test_flags_are_those_of_the_definition(name, case):
    p = case.plan(hoist=True)
    steps, perms = hc.brute_force_flags(case, p)
    assert p.step_hoist.tolist() == steps and p.perm_hoist.tolist() == perms
    assert p.hoisted == (sum(steps), sum(perms))
    if name in hc.TABLE:
        assert p.hoisted == hc.TABLE[name][1]
    # within a permute group the hoisted rows come first, and the groups are still sorted
    assert (np.diff(p.perms[:, 6]) >= 0).all()
    for g in set(p.perms[:, 6].tolist()):
        flags = p.perm_hoist[p.perms[:, 6] == g]
        assert (np.diff(flags) <= 0).all()


def test_the_random_networks_do_hoist_something():
    hoisted = [c.plan(hoist=True).hoisted for c in mc.CASES]
    assert sum(h[0] > 0 for h in hoisted) >= 3 and sum(h[1] > 0 for h in hoisted) >= 3, hoisted


def test_refusals_and_their_order():
    c = hc.case("kept-first-stream-7-9-11")
    args = (list(c.path), c.ts_inds, c.shapes(), c.output_inds)
    kw = dict(slices=c.slices, dtype=np.float32)
    for bad in (False, 1, 0, "yes", 2.0, np.True_):
        with pytest.raises(ValueError, match="'hoist' must be None or True"):
            ctr.plan(*args, hoist=bad, **kw)
    with pytest.raises(NotImplementedError, match="'hoist' is not supported with 'path_kernel'"):
        ctr.plan(*args, hoist=True, path_kernel=4, **kw)
    # the value is checked before the combination, and the checks of the other keywords come first
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.plan(*args, hoist=False, path_kernel=4, **kw)
    with pytest.raises(ValueError, match="'path_kernel' and 'slice_batch' are exclusive"):
        ctr.plan(*args, hoist=True, path_kernel=4, slice_batch=2, **kw)
    with pytest.raises(ValueError, match="'slice_batch' must be"):
        ctr.plan(*args, hoist=False, slice_batch=0, **kw)
    with pytest.raises(ValueError, match="'scaling' needs 'storage'"):
        ctr.plan(*args, hoist="x", scaling="tensor", **kw)
    with pytest.raises(TypeError, match="with 'compute' the compute dtype"):
        ctr.plan(*args, hoist=True, path_kernel=4, compute="bf16x3", slices=c.slices, dtype=np.float64)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    projs = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    with pytest.raises(NotImplementedError, match="projections are not supported with 'hoist'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), hoist=True, **projs)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'path_kernel'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), hoist=True, path_kernel=2, **projs)
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), hoist=0, **projs)
    # contract and contract_results refuse before any device use: no library is loaded for these
    arrays = [np.zeros(s, np.float32) for s in c.shapes()]
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, hoist=False)
    with pytest.raises(NotImplementedError, match="'hoist' is not supported with 'path_kernel'"):
        ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, hoist=True, path_kernel=2)
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.contract_results(None, None, None, None, hoist="True")
    with pytest.raises(NotImplementedError, match="'hoist' is not supported with 'path_kernel'"):
        ctr.contract_results(None, None, None, None, hoist=True, path_kernel=8)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'hoist'"):
        ctr.contract_results(None, None, None, None, hoist=True, projs=np.zeros((1, 1), np.int64))


@pytest.mark.parametrize("name,case", ALL, ids=[n for n, _ in ALL])
def test_macs_and_launches_per_call(name, case):
    p0, p = case.plan(), case.plan(hoist=True)
    n = case.n_assignments()
    each = [int(r[10]) * int(r[11]) * int(r[12]) * int(r[13]) for r in p.steps]
    once = sum(m for m, f in zip(each, p.step_hoist) if f)
    assert p.hoisted_macs == once and p.macs == once + n * (sum(each) - once) == p0.macs - (n - 1) * once
    # launches: what runs once and what runs per assignment are together what the plain plan runs per assignment, but
    # for a permute group with rows of both kinds, which is a launch of either kind
    h_once, h_per = hc.launch_counts(p)
    _, per = hc.launch_counts(p0)
    assert per == mc.launches_per_assignment(p0)
    mixed = hc.mixed_groups(p)
    assert tuple(a + b for a, b in zip(h_once, h_per)) == (per[0] + mixed,) + per[1:]
    assert sum(h_once[1:]) == p.hoisted[0]
    if name in hc.TABLE:
        assert mixed == 0  # (so that a hoisted run is the plain one minus (assignments - 1) x the hoisted share)


@pytest.mark.parametrize("mode", [dict(), dict(slice_batch=5), dict(storage="float16", scaling="tensor"),
                                  dict(storage="bfloat16", scaling="tensor", slice_batch=5)],
                         ids=["plain", "batch", "scaled", "scaled-batch"])
@pytest.mark.parametrize("name", hc.NAMES)
def test_peak_device_bytes_term_by_term(name, mode):
    case = hc.case(name, "complex64")
    p = case.plan(hoist=True, **mode)
    # the arena: the furthest end of any buffer the tables name, every buffer a whole number of ALIGN elements
    up = lambda v: -(-v // ctr.ALIGN) * ctr.ALIGN  # noqa: E731
    ends = [int(r[3]) + up(int(r[5])) for r in p.perms if r[2] == ctr.ARENA]
    ends += [int(r[9]) + up(int(r[10] * r[11] * r[12])) for r in p.steps if r[8] == ctr.ARENA]
    if p.scaling:
        ends += [int(s) + up(2 * int(r[10] * r[11] * r[12])) for s, r in zip(p.stage_refs, p.steps) if s >= 0]
    assert p.arena_elems == max(ends)
    B = p.slice_batch or 1
    item, held = 8, (4 if "storage" in mode else 8)
    leaves = held * int(p.leaf_numel.sum())
    arena = held * p.arena_elems * B
    out = item * p.out_numel
    tables = 8 * (p.leaf_sl.size + p.perms.size + 2 * p.leaf_numel.size)
    scale = 4 * (len(p.leaf_numel) + 2 * len(p.steps)) * B if p.scaling else 0
    stage = item * B * (p.out_numel // 2) if "slice_batch" in mode else 0  # (p, of dimension 2, selects the block)
    assert p.peak_device_bytes == leaves + arena + out + tables + scale + stage
    ctr.check_memory(p, p.peak_device_bytes)
    with pytest.raises(RuntimeError):
        ctr.check_memory(p, p.peak_device_bytes - 1)


def interpret(case, p, arrays):
    """The plan's tables run with numpy on one flat arena, in double precision (module docstring)."""
    wide = np.complex128 if any(np.iscomplexobj(a) for a in arrays) else np.float64
    leaves = [np.ascontiguousarray(a, wide).reshape(-1) for a in arrays]
    arena = np.full(max(p.arena_elems, 1), np.nan, wide)
    n_blocks = math.prod(p.shape[p.inds.index(x)] for x in p.block_inds)
    block = p.out_numel // n_blocks
    out = np.zeros(p.out_numel, wide)
    place = [math.prod(p.slice_dims[s + 1:]) for s in range(len(p.slice_dims))]
    hoisting = p.hoisted is not None
    step_h = p.step_hoist if hoisting else np.zeros(len(p.steps), np.int64)
    perm_h = p.perm_hoist if hoisting else np.zeros(len(p.perms), np.int64)
    outside = np.ones(len(arena), bool)
    for off, numel in p.kept:
        outside[off:off + numel] = False

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

    def operand(kind, ref, sid, H, R, Kc, sr, sk):
        """[H][R][Kc] of a dense batch operand whose rows are sr and columns sk apart."""
        base = leaves[int(ref)][slice_offset(int(ref), sid):] if kind == ctr.LEAF else arena[int(ref):]
        idx = (np.arange(H) * R * Kc).reshape(-1, 1, 1) + (np.arange(R) * sr).reshape(1, -1, 1) + (np.arange(Kc) * sk).reshape(1, 1, -1)
        return base[idx]

    def step(k, sid, out_off, beta):
        st = [int(v) for v in p.steps[k]]
        H, M, N, K = st[10:14]
        A = operand(st[0], st[1], sid, H, M, K, st[2], st[3])
        Bm = operand(st[4], st[5], sid, H, N, K, st[7], st[6])
        if p.scaling is not None and p.stage_refs[k] >= 0:
            arena[int(p.stage_refs[k]):int(p.stage_refs[k]) + 2 * H * M * N] = np.nan
        Cm = np.einsum("hmk,hnk->hmn", A, Bm).reshape(-1)
        if st[8] == ctr.ARENA:
            arena[st[9]:st[9] + H * M * N] = Cm
        else:
            out[out_off:out_off + block] = out[out_off:out_off + block] + Cm if beta else Cm

    def run(sid, out_off, beta, hoisted):
        for g in [-1] + list(range(len(p.steps))):
            for r in np.nonzero((p.perms[:, 6] == g) & (perm_h == hoisted))[0]:
                gather(p.perms[r], sid, out_off)
            if g >= 0 and step_h[g] == hoisted:
                step(g, sid, out_off, beta)

    if hoisting and any(p.hoisted):
        run(p.slice_range[0], 0, 0, 1)
    visited = set()
    for sid in range(*p.slice_range):
        blk = 0
        for x in p.block_inds:
            s = p.slice_inds.index(x)
            blk = blk * p.slice_dims[s] + (sid // place[s]) % p.slice_dims[s]
        run(sid, blk * block, blk in visited, 0)
        visited.add(blk)
        arena[outside] = np.nan
    return ctr._host_layout(p, out)


@pytest.mark.parametrize("mode", [dict(), dict(storage="float16", scaling="tensor")], ids=["plain", "scaled"])
@pytest.mark.parametrize("name,case", ALL, ids=[n for n, _ in ALL])
def test_the_tables_interpreted_on_one_arena_give_the_einsum(name, case, mode):
    c32 = case.with_(dtype="complex64" if np.dtype(case.dtype).kind == "c" else "float32")
    p = c32.plan(hoist=True, **mode)
    arrays = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in mc.fill(case)]
    ref, mag = mc.reference(c32, p, arrays)
    got = interpret(c32, p, arrays)
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{name}: a buffer was read that nothing valid was in"
    assert (np.abs(got - ref) <= 1e-12 * mc.kt(p) * mag).all()
    # after an assignment the arena holds the kept buffers and nothing else that anything reads: the plain plan of the
    # same case passes through the same interpreter with no kept buffer at all
    if name in hc.TABLE:
        q = c32.plan(**mode)
        assert q.kept == () and np.array_equal(interpret(c32, q, arrays), got)
