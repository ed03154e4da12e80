"""The plan side of the gather, reduce and narrowing cases (tests/gather_cases.py), without a GPU.

Every case records what it is for -- the rows of `perms` it must give (source kind, destination kind, ndim, numel,
group), the elements of a block of the output, the elements of every stored step result, the shape class of every step
-- and that is asserted from plan()'s tables, so a planner change that moves a case off its edge fails here and does
not quietly test less on the device.  The table as a whole must hold every combination the device tests are for.  Each
case is replayed by the numpy interpreter of the tables (tests/test_contraction_plan.py) and must give the expected
bytes, and the same replay with one of three planted defects -- a row that stops after its first trip, two strides of
a row swapped, a narrowing pass without its tail -- must not: the comparison of the device tests has teeth.
"""
import math

import numpy as np
import pytest

from tests import gather_cases as gc
from tests.test_contraction_plan import _gather, _interpret
from tnco_amd import contraction as ctr

_FILLED = {}


def filled(case, dtype):
    """(leaves, expected result, expected exponents) of a run, computed once and never written to."""
    key = (case.name, np.dtype(dtype))
    if key not in _FILLED:
        arrays = gc.fill(case, dtype)
        want, exps = gc.expected(case, dtype, arrays)
        for a in arrays + [want]:
            a.setflags(write=False)
        _FILLED[key] = (arrays, want, exps)
    return _FILLED[key]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def block_numel(p) -> int:
    return p.out_numel // math.prod(p.slice_dims[p.slice_inds.index(x)] for x in p.block_inds)


def stored_numel(p) -> tuple:
    return tuple(int(r[10] * r[11] * r[12]) for r in p.steps if r[8] == ctr.ARENA)


def row_kinds(p) -> tuple:
    return tuple((int(r[0]), int(r[2]), int(r[4]), int(r[5]), int(r[6])) for r in p.perms)


@pytest.mark.parametrize("case,dtype", gc.RUNS, ids=gc.RUN_IDS)
def test_every_case_plans_as_recorded(case, dtype):
    p = case.plan(dtype)
    assert row_kinds(p) == case.rows
    assert block_numel(p) == (case.block_numel if case.block_numel is not None else p.out_numel)
    assert stored_numel(p) == case.stored
    assert tuple(gc.klass(*(int(v) for v in r[11:14])) for r in p.steps) == case.classes
    assert set(p.inds) == set(case.out_inds) and p.slice_inds == case.slices
    assert p.slice_range == (case.assignments().start, case.assignments().stop)
    assert (p.storage, p.scaling) == (case.storage, case.scaling)
    for r in p.perms:  # every dimension of a row is in the tables as given: dimension-1 axes are not dropped
        assert math.prod(int(d) for d in r[8:8 + int(r[4])]) == int(r[5])
    # the batched runs: the tables of the plain plan, the group the keyword asks for, and memory under the cap
    assert p.peak_device_bytes <= gc.MEMORY_CAP
    for keyword, value in case.batching:
        q = case.plan(dtype, **{keyword: value})
        assert getattr(q, keyword) == min(value, len(case.assignments()))
        assert np.array_equal(q.perms, p.perms) and np.array_equal(q.steps, p.steps)
        assert p.peak_device_bytes < q.peak_device_bytes <= gc.MEMORY_CAP, (keyword, value, q.peak_device_bytes)
    assert bool(case.bites) or not case.large
    assert set(case.bites) <= set(gc.DEFECTS)


def test_the_table_holds_every_combination_the_device_tests_are_for():
    plans = [(c, c.plan(d)) for c, d in gc.RUNS]
    rows = [(c, r) for c, p in plans for r in p.perms]
    for src, dst in ((ctr.LEAF, ctr.OUT), (ctr.LEAF, ctr.ARENA), (ctr.ARENA, ctr.ARENA)):
        assert any(r[0] == src and r[2] == dst and r[5] > gc.TRIP for _, r in rows), (src, dst)
        # ... in storage mode too, where another kernel moves the 16-bit values (leaf -> output: widened, also scaled)
        assert dst == src or any(r[0] == src and r[2] == dst and r[5] > gc.TRIP and c.storage for c, r in rows), (src, dst)
    assert any(c.scaling and r[2] == ctr.OUT and r[5] > gc.TRIP for c, r in rows)
    assert any(r[4] == 0 and r[5] == 1 for _, r in rows)
    assert any(r[4] == ctr.MAX_AXES and r[5] > 3 * gc.TRIP and 1 in r[8:8 + ctr.MAX_AXES].tolist() for _, r in rows)
    # a second trip that covers a part of the grid only, and a sliced leaf whose blocks are placed
    assert any(gc.TRIP < r[5] < 2 * gc.TRIP and r[2] == ctr.OUT for _, r in rows)
    assert any(r[2] == ctr.OUT and c.slices and c.slice_range and r[5] < gc.TRIP for c, r in rows)
    # one launch -- the rows of one group -- with sizes on both sides of one block, the larger above a trip; run
    # unbatched, as a slice batch and in the path kernel
    two = [c for c, p in plans for g in set(p.perms[:, 6].tolist())
           if p.perms[p.perms[:, 6] == g][:, 5].max() > gc.TRIP and p.perms[p.perms[:, 6] == g][:, 5].min() <= gc.BLOCK]
    assert {k for c in two for k, _ in c.batching} == {"slice_batch", "path_kernel"}
    assert any(c.storage for c in two) and any(not c.storage for c in two)
    # an arena -> arena row above a trip inside the path kernel
    assert any(r[0] == r[2] == ctr.ARENA and r[5] > gc.TRIP and ("path_kernel", 1) in c.batching for c, r in rows)
    # both reduce kernels on a block above a trip: members that share a block, one block, a block per assignment
    for keyword in ("slice_batch", "path_kernel"):
        big = [(c, p) for c, p in plans if block_numel(p) > gc.TRIP and any(k == keyword for k, _ in c.batching)]
        n_blocks = {p.out_numel // block_numel(p) for c, p in big if c.group == "reduce"}
        assert n_blocks == {1, 3, 12}, (keyword, n_blocks)
        groups = {v for c, _ in big if c.group == "reduce" for k, v in c.batching if k == keyword}
        assert {1, 5} < groups and max(groups) >= 64
        assert any(c.slice_range and c.slice_range[0] % v for c, _ in big for k, v in c.batching if k == keyword)
        assert {np.dtype(d) for c, _ in big for d in c.run_dtypes()} >= {np.dtype(np.float32), np.dtype(np.complex128)}
    # the narrowing pass: parts on both sides of a trip, n % 4 of 0 and of 2, tail only; both classes of the stored step
    scaled = [(c, p, (2 if p.dtype.kind == "c" else 1) * n) for c, p in plans if c.scaling for n in stored_numel(p)]
    for storage in gc.STORAGES:
        for cplx in "fc":
            n_parts = {n for c, p, n in scaled if c.storage == storage and p.dtype.kind == cplx}
            assert min(n_parts) < 4 and any(4 < n < 8 for n in n_parts) and max(n_parts) > gc.NARROW_TRIP
            assert any(n > gc.NARROW_TRIP and n % 4 == 2 for n in n_parts)
            assert {c.classes[0] for c, p, n in scaled if c.storage == storage and p.dtype.kind == cplx
                    and n > gc.NARROW_TRIP} == {"stream", "tiled"}
        assert any(n % 4 == 0 for c, p, n in scaled if c.storage == storage)
        assert any(n > gc.NARROW_TRIP and ("slice_batch", 2) in c.batching and len(c.assignments()) == 2
                   for c, p, n in scaled if c.storage == storage)


# --- the replay, sound and with a planted defect ----------------------------------------------------------------------
def one_trip(row, src, base):
    """A gather that never takes `e += gridDim.x * blockDim.x`: what lies beyond the first trip is not written."""
    vals = _gather(row, src, base)
    vals[gc.TRIP:] = 0
    return vals


def swapped_strides(row, src, base):
    """A gather that reads the last two axes of a dimension above 1 with each other's stride."""
    P = ctr.MAX_AXES
    axes = [k for k in range(int(row[4])) if row[8 + k] > 1][-2:]
    if len(axes) < 2:
        return _gather(row, src, base)
    row = row.copy()
    row[8 + P + axes[0]], row[8 + P + axes[1]] = row[8 + P + axes[1]], row[8 + P + axes[0]]
    reach = base + sum(int(row[8 + k] - 1) * int(row[8 + P + k]) for k in range(int(row[4]))) + 1
    if reach > src.size:  # (the wrong strides may leave the source: zeros there)
        src = np.concatenate([src, np.zeros(reach - src.size, src.dtype)])
    return _gather(row, src, base)


def replay(case, dtype, defect=None):
    """(the case replayed from its tables in the axis order of case.out_inds, the exponents of the stored tensors)."""
    arrays, _, _ = filled(case, dtype)
    p = case.plan(dtype)
    leaves, exps = list(arrays), []
    if case.scaling is not None:  # the leaves as the engine holds them
        held = [ctr.scale_to_storage(a, case.storage) for a in arrays]
        leaves, exps = [v for v, _ in held], ([held[0][1]] if not case.path else [])
    elif case.storage is not None:
        leaves = [ctr.round_to_storage(a, case.storage) for a in arrays]

    def store(k, z):
        if case.storage is None:
            return z
        if case.scaling is None:
            return ctr._from_storage_bits(ctr._storage_bits(z, case.storage, check=False), case.storage, z)
        kept, e = ctr.scale_to_storage(z, case.storage)
        exps.append(e)
        if defect == "no_tail":
            kept = kept.copy()
            x = kept.view(np.float32)
            x[x.size // 4 * 4:] = 0
        return kept

    gather = dict(one_trip=one_trip, swapped_strides=swapped_strides).get(defect, _gather)
    got = _interpret(p, leaves, gather=gather, store=store)
    return got.transpose([p.inds.index(x) for x in case.out_inds]), exps


@pytest.mark.parametrize("case,dtype", gc.RUNS, ids=gc.RUN_IDS)
def test_the_replay_of_the_tables_gives_the_expected_bytes(case, dtype):
    arrays, want, want_exps = filled(case, dtype)
    got, exps = replay(case, dtype)
    assert got.dtype == want.dtype == dtype and got.shape == want.shape
    assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want))
    if case.scaling is not None:
        assert exps == want_exps and len(exps) == (len(case.assignments()) if case.path else 1)
    # an element that no assignment writes is zero in the expectation; every other one is not
    written = np.zeros(want.shape, bool)
    for sid in case.assignments():
        written[tuple(gc.digits(case, sid).get(x, slice(None)) for x in case.out_inds)] = True
    assert np.array_equal(want != 0, written)


@pytest.mark.parametrize("defect", gc.DEFECTS)
@pytest.mark.parametrize("case,dtype", gc.RUNS, ids=gc.RUN_IDS)
def test_a_planted_defect_changes_the_bytes_of_the_cases_it_bears_on(case, dtype, defect):
    _, want, _ = filled(case, dtype)
    got, _ = replay(case, dtype, defect)
    assert np.array_equal(bits(got), bits(want)) == (defect not in case.bites), (case.name, defect)


def test_every_large_case_fails_under_a_defect():
    large = [c for c in gc.CASES if c.large]
    assert len(large) >= 20 and all(c.bites for c in large)
    assert {d for c in large for d in c.bites} == set(gc.DEFECTS)
    # a gather above a trip fails under both gather defects, a stored tensor above a trip without its tail
    for c in large:
        p = c.plan(c.run_dtypes()[0])
        if len(p.perms) and p.perms[:, 5].max() > gc.TRIP:
            assert {"one_trip", "swapped_strides"} <= set(c.bites), c.name
        if c.scaling and c.stored and max(c.stored) * (2 if p.dtype.kind == "c" else 1) > gc.NARROW_TRIP:
            assert "no_tail" in c.bites, c.name
