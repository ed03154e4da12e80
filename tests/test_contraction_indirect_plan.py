"""`indirect=True` in the plan (tnco_amd/contraction.py), without a GPU: which operands are folded, that every other
decision of a step stays the plain plan's, what the keyword refuses, what a call then costs in device memory, and -- with
the numpy interpreter of tests/indirect_cases.py, which reads a folded operand through `ind_maps` on one flat arena that
is NaN outside live buffers -- that the tables give numpy's einsum of the whole network in double precision."""
import numpy as np
import pytest

from tests import indirect_cases as ic
from tests import mode_cases as mc
from tests import schedule_cases as sc
from tnco_amd import contraction as ctr

TABLES = ("leaf_numel", "leaf_sl", "perms", "steps")
ONE = [(f"{n}-{f}", ic.case(n, f)) for n, f in ic.ONE_STEP]
CHAINS = list(ic.CHAINS.items())
MODE = [(i, c) for i, c in zip(sc.IDS, sc.CASES)]  # (mode_cases.CASES and EXTRA)
ALL = ONE + CHAINS + MODE
ids = lambda rows: [n for n, _ in rows]  # noqa: E731


@pytest.mark.parametrize("hoist", [None, True], ids=["plain", "hoist"])
@pytest.mark.parametrize("name,case", ALL, ids=ids(ALL))
def test_without_the_keyword_nothing_changes(name, case, hoist):
    p, q = case.plan(hoist=hoist), case.plan(hoist=hoist, indirect=None)
    for t in TABLES:
        assert getattr(p, t).tobytes() == getattr(q, t).tobytes() and getattr(p, t).dtype == getattr(q, t).dtype, t
    assert (p.arena_elems, p.peak_device_bytes, p.macs, p.ops) == (q.arena_elems, q.peak_device_bytes, q.macs, q.ops)
    assert q.indirect is None and q.ind_steps is None and q.ind_maps is None
    assert all("ind_a" not in op for op in q.ops)


@pytest.mark.parametrize("hoist", [None, True], ids=["plain", "hoist"])
@pytest.mark.parametrize("name,case", ALL, ids=ids(ALL))
def test_every_other_decision_of_a_step_is_the_plain_plans(name, case, hoist):
    p0, p = case.plan(hoist=hoist), case.plan(hoist=hoist, indirect=True)
    assert len(p.ops) == len(p0.ops) and p.inds == p0.inds and p.shape == p0.shape
    for op0, op in zip(p0.ops, p.ops):
        assert all(op[q] == op0[q] for q in ("h", "x", "y", "s", "H", "M", "N", "K"))
    assert [s[0] for s in mc.signature(p)] == [s[0] for s in mc.signature(p0)]
    assert np.array_equal(p.steps[:, 10:14], p0.steps[:, 10:14]) and p.macs == p0.macs
    assert len(p.perms) == len(p0.perms) - p.indirect
    sides = ic.folded_sides(p)
    assert p.indirect == sum(a + b for a, b in sides) == sum(op["ind_a"] + op["ind_b"] for op in p.ops)
    # a folded operand has both stride columns 0 and keeps its kind and ref; the others keep their form
    for st, st0, op, (fa, fb) in zip(p.steps, p0.steps, p.ops, sides):
        assert (tuple(st[2:4]) == (0, 0)) == fa and (tuple(st[6:8]) == (0, 0)) == fb
        assert (fa or tuple(st[2:4]) == tuple(st0[2:4])) and (fb or tuple(st[6:8]) == tuple(st0[6:8]))
        assert op["ind_a"] == fa and op["ind_b"] == fb
    if not p.indirect:  # the tables of the plan without the keyword
        assert p.ind_steps is None and p.ind_maps is None and p.peak_device_bytes == p0.peak_device_bytes
        assert all(getattr(p, t).tobytes() == getattr(p0, t).tobytes() for t in TABLES)
        return
    assert p.ind_steps.shape == (len(p.steps), ctr.IND_W) and p.ind_steps.dtype == p.ind_maps.dtype == np.int64
    # every table lies inside the pool with the extent of its role, and the tables of an operand are one permutation of it
    for st, row, (fa, fb) in zip(p.steps, p.ind_steps, sides):
        H, M, N, K = (int(v) for v in st[10:14])
        for side, f, ext in ((0, fa, (H, M, K)), (1, fb, (H, K, N))):
            o = row[3 * side:3 * side + 3]
            if not f:
                assert (o == -1).all()
                continue
            t = [p.ind_maps[int(a):int(a) + e] for a, e in zip(o, ext)]
            assert all(len(q) == e and (q >= 0).all() for q, e in zip(t, ext))
            reach = (t[0].reshape(-1, 1, 1) + t[1].reshape(1, -1, 1) + t[2].reshape(1, 1, -1)).reshape(-1)
            assert len(set(reach.tolist())) == H * M * N * K // (M if side else N)
            if st[4 * side] == ctr.ARENA:  # the tensor as the step before left it: dense
                assert sorted(reach.tolist()) == list(range(len(reach)))


@pytest.mark.parametrize("name,case", ALL, ids=ids(ALL))
def test_rule_a_no_hoisted_permute_is_folded(name, case):
    p0, p = case.plan(hoist=True), case.plan(hoist=True, indirect=True)
    # the hoisted permutes are those of the plan without the keyword, row for row; only others are gone
    hoisted0 = sorted(map(tuple, p0.perms[p0.perm_hoist == 1][:, 4:].tolist()))
    assert sorted(map(tuple, p.perms[p.perm_hoist == 1][:, 4:].tolist())) == hoisted0
    assert p.hoisted == p0.hoisted and np.array_equal(p.step_hoist, p0.step_hoist)
    assert len(p0.perms) - len(p.perms) == p.indirect == int((p0.perm_hoist == 0).sum()) - int((p.perm_hoist == 0).sum())
    if name in ic.CHAIN_FOLDS:
        assert (case.plan(indirect=True).indirect, p.indirect) == ic.CHAIN_FOLDS[name]


def test_rule_b_from_both_sides():
    # an outer product with K = 1, the operands interleaved with a summed-out axis of dimension 1
    ts, shapes = [("i1", "k", "i2"), ("j1", "k", "j2")], [(3, 1, 4), (5, 1, 2)]
    folded = {}
    for dtype in ic.DTYPES:
        p = ctr.plan([(0, 1)], ts, shapes, ("i1", "i2", "j1", "j2"), dtype=np.dtype(dtype), indirect=True)
        assert (p.ops[0]["M"], p.ops[0]["N"], p.ops[0]["K"]) == (12, 10, 1)
        folded[dtype] = (p.ops[0]["ind_a"], p.ops[0]["ind_b"], len(p.perms))
    # A: 8 (1 + 12 + 1) = 112 bytes of tables against 12 elements; B: 8 (1 + 1 + 10) = 96 against 10
    assert folded["float32"] == folded["complex64"] == (False, False, 2)
    assert folded["float64"] == (False, False, 2)
    assert folded["complex128"] == (True, True, 0)
    # the limit itself, M = 2, K = 3 in float64: 8 (1 + 2 + 3) = 48 = 8 x 6 is folded; the same tables against the 24
    # bytes of the float32 copy are not
    ts, shapes = [("i1", "k", "i2"), ("k", "j")], [(2, 3, 1), (3, 5)]
    assert ctr.plan([(0, 1)], ts, shapes, dtype=np.float64, indirect=True).indirect == 1
    assert ctr.plan([(0, 1)], ts, shapes, dtype=np.float32, indirect=True).indirect == 0
    # one element more of tables: M = 2, K = 2, 8 (1 + 2 + 2) = 40 against 8 x 4 = 32, and against 16 x 4 = 64
    ts, shapes = [("i1", "k", "i2"), ("k", "j")], [(2, 2, 1), (2, 5)]
    assert ctr.plan([(0, 1)], ts, shapes, dtype=np.float64, indirect=True).indirect == 0
    assert ctr.plan([(0, 1)], ts, shapes, dtype=np.complex128, indirect=True).indirect == 1


@pytest.mark.parametrize("mode", [dict(), dict(slice_batch=5), dict(hoist=True), dict(hoist=True, slice_batch=5)],
                         ids=["plain", "batch", "hoist", "hoist-batch"])
@pytest.mark.parametrize("name,case", CHAINS, ids=ids(CHAINS))
def test_peak_device_bytes_term_by_term(name, case, mode):
    case = case.with_(dtype="complex64")
    p = case.plan(indirect=True, **mode)
    assert p.indirect > 0
    up = lambda v: -(-v // ctr.ALIGN) * ctr.ALIGN  # noqa: E731
    ends = [int(r[3]) + up(int(r[5])) for r in p.perms if r[2] == ctr.ARENA]
    ends += [int(r[9]) + up(int(r[10] * r[11] * r[12])) for r in p.steps if r[8] == ctr.ARENA]
    assert p.arena_elems == max(ends + [0])
    B = p.slice_batch or 1
    block = p.out_numel // int(np.prod([p.shape[p.inds.index(x)] for x in p.block_inds]))
    leaves, arena, out = 8 * int(p.leaf_numel.sum()), 8 * p.arena_elems * B, 8 * p.out_numel
    tables = 8 * (p.leaf_sl.size + p.perms.size + 2 * p.leaf_numel.size)
    stage = 8 * B * block if "slice_batch" in mode else 0
    indirect = 8 * (p.ind_steps.size + p.ind_maps.size)
    assert p.ind_maps.size == sum(sum(ext) for st, (fa, fb) in zip(p.steps, ic.folded_sides(p))
                                  for f, ext in ((fa, (st[10], st[11], st[13])), (fb, (st[10], st[13], st[12]))) if f)
    assert p.peak_device_bytes == leaves + arena + out + tables + stage + indirect
    # the permute that is gone took its buffer with it
    q = case.plan(**mode)
    assert p.arena_elems <= q.arena_elems
    ctr.check_memory(p, p.peak_device_bytes)
    with pytest.raises(RuntimeError):
        ctr.check_memory(p, p.peak_device_bytes - 1)


def _no_gpu(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)


def test_refusals_their_texts_and_their_order(monkeypatch):
    _no_gpu(monkeypatch)
    c = ic.case("reordered")
    args = (list(c.path), c.ts_inds, c.shapes(), c.output_inds)
    kw = dict(slices=c.slices, dtype=np.float32)
    value = "'indirect' must be None or True."
    for bad in (False, 1, 0, "yes", 2.0, np.True_):
        with pytest.raises(ValueError, match=value):
            ctr.plan(*args, indirect=bad, **kw)
    texts = dict(storage="'storage' is not supported with 'indirect'.", compute="'compute' is not supported with 'indirect'.",
                 path_kernel="'path_kernel' is not supported with 'indirect'.")
    modes = dict(storage="float16", compute="matrix", path_kernel=4)
    for name, text in texts.items():
        with pytest.raises(NotImplementedError, match=text):
            ctr.plan(*args, indirect=True, **{name: modes[name]}, **kw)
        with pytest.raises(ValueError, match=value):  # the value before the combination
            ctr.plan(*args, indirect=False, **{name: modes[name]}, **kw)
    # in this order: storage, compute, path_kernel, projs -- where the checks of the other keywords let both through
    with pytest.raises(NotImplementedError, match=texts["compute"]):
        ctr.plan(*args, indirect=True, compute="bf16x3", **kw)
    # the checks of the other keywords come first
    with pytest.raises(ValueError, match="'compute' and 'storage' are exclusive"):
        ctr.plan(*args, indirect=True, compute="matrix", storage="float16", **kw)
    with pytest.raises(NotImplementedError, match="'storage' is not supported with 'path_kernel'"):
        ctr.plan(*args, indirect=True, storage="float16", path_kernel=4, **kw)
    with pytest.raises(NotImplementedError, match="'compute' is not supported with 'path_kernel'"):
        ctr.plan(*args, indirect=True, compute="matrix", path_kernel=4, **kw)
    with pytest.raises(NotImplementedError, match="'hoist' is not supported with 'path_kernel'"):
        ctr.plan(*args, indirect=True, hoist=True, path_kernel=4, **kw)
    with pytest.raises(ValueError, match="'hoist' must be None or True"):
        ctr.plan(*args, indirect="x", hoist=False, **kw)
    with pytest.raises(ValueError, match="'slice_batch' must be"):
        ctr.plan(*args, indirect=False, slice_batch=0, **kw)
    with pytest.raises(TypeError, match="with 'compute' the compute dtype"):
        ctr.plan(*args, indirect=True, compute="bf16x3", slices=c.slices, dtype=np.float64)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    projs = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    with pytest.raises(NotImplementedError, match="projections are not supported with 'indirect'."):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), indirect=True, **projs)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'hoist'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), indirect=True, hoist=True, **projs)
    with pytest.raises(NotImplementedError, match="projections are not supported with 'storage'"):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), indirect=True, storage="float16", dtype=np.float32, **projs)
    with pytest.raises(ValueError, match=value):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), indirect=0, **projs)
    # it works with slices, a range, a batch and hoisting, in the four dtypes
    for dtype in ic.DTYPES:
        p = ctr.plan(*args, slices=c.slices, slice_range=(1, 5), slice_batch=5, hoist=True, indirect=True, dtype=np.dtype(dtype))
        assert p.indirect == 1 and p.slice_batch == 4 and p.hoisted == (0, 1)
    # contract and contract_results refuse before any device use
    arrays = [np.zeros(s, np.float32) for s in c.shapes()]
    with pytest.raises(ValueError, match=value):
        ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, indirect=False)
    for name, text in texts.items():
        with pytest.raises(NotImplementedError, match=text):
            ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, indirect=True, **{name: modes[name]})
        with pytest.raises(NotImplementedError, match=text):
            ctr.contract_results(None, None, None, None, indirect=True, **{name: modes[name]})
    with pytest.raises(ValueError, match=value):
        ctr.contract_results(None, None, None, None, indirect="True")
    with pytest.raises(NotImplementedError, match="projections are not supported with 'indirect'."):
        ctr.contract_results(None, None, None, None, indirect=True, projs=np.zeros((1, 1), np.int64))
    with pytest.raises(AssertionError, match="the device was reached"):
        ctr.contract(list(c.path), c.ts_inds, arrays, c.output_inds, slices=c.slices, indirect=True)


def test_the_result_has_the_new_fields_before_the_last_one():
    import dataclasses
    fields = [f.name for f in dataclasses.fields(ctr.ContractionResult)]
    assert fields[-3:] == ["indirect", "indirect_launches", "matrix_launches"]
    r = ctr.ContractionResult((), None, 0, 1, 0)
    assert r.indirect is None and r.indirect_launches == (0, 0, 0)
    assert ctr.INDIRECT_KERNEL_PATHS == ("ix_tiled", "ix_dot", "ix_stream")


@pytest.mark.parametrize("hoist", [None, True], ids=["plain", "hoist"])
@pytest.mark.parametrize("name,case", ALL, ids=ids(ALL))
def test_the_tables_interpreted_on_one_arena_give_the_einsum(name, case, hoist):
    p = case.plan(hoist=hoist, indirect=True)
    arrays = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in mc.fill(case)]
    ref, mag = mc.reference(case, p, arrays)
    got = ic.interpret(p, arrays)
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{name}: a buffer was read that nothing valid was in"
    assert (np.abs(got - ref) <= 1e-12 * mc.kt(p) * mag).all()


def test_the_networks_fold_arena_operands_and_sliced_leaves():
    arena = leaf = dense_leaf = 0
    for case in mc.CASES:
        for hoist in (None, True):
            p = case.plan(hoist=hoist, indirect=True)
            for st, sides in zip(p.steps, ic.folded_sides(p)):
                for side, f in enumerate(sides):
                    if not f:
                        continue
                    kind, ref = int(st[4 * side]), int(st[4 * side + 1])
                    arena += kind == ctr.ARENA
                    n_cut = int(p.leaf_sl[ref, 0]) if kind == ctr.LEAF else 0
                    if n_cut:  # dense after slicing: every sliced axis lies outside the kept elements
                        cut_dims = [p.slice_dims[int(s)] for s in p.leaf_sl[ref, 1:1 + n_cut]]
                        cut_strides = p.leaf_sl[ref, 1 + ctr.MAX_AXES:1 + ctr.MAX_AXES + n_cut]
                        leaf += 1
                        dense_leaf += bool((cut_strides >= int(p.leaf_numel[ref]) // int(np.prod(cut_dims))).all())
    # arena operands, sliced leaves, and among those leaves that are not dense after slicing (a sliced axis inside)
    assert arena >= 10 and leaf >= 10 and leaf - dense_leaf >= 3, (arena, leaf, dense_leaf)
    # the chain of tests/batch_cases.py: its gathered leaf B (k, t, j), not dense after slicing over t, is folded
    p = ic.case("chain-stream-stream").plan(indirect=True)
    assert ic.folded_sides(p)[0] == (False, True) and p.steps[0, 4] == ctr.LEAF and p.steps[0, 5] == 1 and len(p.perms) == 0
    # and the intermediate of `reordered` is read by the next step in another order
    p = ic.case("reordered").plan(indirect=True)
    assert ic.folded_sides(p)[1][1] and p.steps[1, 4] == ctr.ARENA and p.steps[1, 5] == p.steps[0, 9]
