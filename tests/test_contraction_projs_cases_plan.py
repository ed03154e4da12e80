"""The case table of the projection tests (tests/projs_cases.py) on the CPU: every case stays within the caps, the table
reaches every item of `projs_cases.REQUIRED` in a real and in a complex dtype -- asserted item by item, naming the
cases, so that an edit of the table cannot lose one silently -- and a seed-named case is what the generator gives.

The bound of tests/test_gpu_contract_projs_cases.py is shown here to be one that a correct contraction meets on these
inputs, and one that a wrong one does not: the plan's tables are replayed by the numpy interpreter of
tests/test_contraction_projs_plan.py in the case's own dtype, float32 and complex64 included, and held element by element
to |got - ref| <= (c kt + 2) u mag against `projs_cases.reference`; then four defects are planted, each into a copy of the
tables of every case that has the feature, and the replay must leave the bound in at least one element:

    one entry of `row_maps` set to another valid row of its operand;
    a row operand read at row 0 for every r;
    two entries of `row_of_proj` that name different rows swapped;
    one product dropped from one step (the largest of one element of the last step, in the first assignment).
"""
import copy

import numpy as np
import pytest

from tests import projs_cases as pc
from tests.test_contraction_projs_plan import _interpret

_REFERENCE = {}


def reference_of(case):
    """(plan, leaves, reference, magnitude, bound) of a case, computed once and left unchanged."""
    if case not in _REFERENCE:
        p, arrays = case.plan(), pc.fill(case)
        ref, mag = pc.reference(case, p, arrays)
        _REFERENCE[case] = (p, arrays, ref, mag, pc.bound(case, p, mag))
        for a in arrays + [ref, mag]:
            a.setflags(write=False)
    return _REFERENCE[case]


def outside(got, ref, bound):
    """The elements beyond the bound; one that is not a number is beyond it."""
    return ~(np.abs(got.astype(ref.dtype) - ref) <= bound)


def replay_case(case):
    """The replay of the case's tables in its own dtype against the bound of the device test: the largest
    error / bound.  Also what `tools/fuzz_contract.py --projs --cpu-only` runs."""
    p, arrays, ref, mag, bound = reference_of(case) if case in pc.CASES else _fresh(case)
    got = _interpret(p, arrays)
    assert got.dtype == np.dtype(case.dtype) and got.shape == ref.shape == p.shape
    assert np.isfinite(got).all()
    bad = outside(got, ref, bound)  # (a bound of 0: a block that no assignment of a partial slice_range visits stays 0)
    assert not bad.any(), f"{case.name}: the replay leaves the bound in {int(bad.sum())} elements"
    err = np.abs(got.astype(ref.dtype) - ref)
    return float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())


def _fresh(case):
    p, arrays = case.plan(), pc.fill(case)
    ref, mag = pc.reference(case, p, arrays)
    return p, arrays, ref, mag, pc.bound(case, p, mag)


def test_the_table_is_a_fixed_list_of_distinct_cases():
    assert len(set(pc.IDS)) == len(pc.IDS) == len(pc.CASES)
    per_dtype = {np.dtype(d).name: sum(c.dtype == np.dtype(d).name for c in pc.CASES) for d in pc.DTYPES}
    assert min(per_dtype.values()) >= len(pc.CASES) // 4 - 2, per_dtype
    assert {c.fill for c in pc.CASES} == set(pc.FILLS)
    seeds = [row for row in pc.TABLE if not isinstance(row, tuple)]
    assert len(seeds) >= 8
    for k, (row, case) in enumerate(zip(pc.TABLE, pc.CASES)):  # the generator is deterministic
        assert pc.make(row, k) == case
        if not isinstance(row, tuple):
            assert case.name == f"seed-{row}" and case == pc.generate(row)
    assert 2 in {c.n_assignments() for c in pc.CASES} and 24 in {c.n_assignments() for c in pc.CASES}
    assert any(c.slice_range and c.slice_range[0] > 0 for c in pc.CASES if c.name.startswith("hand-"))
    assert {len(c.projs()) for c in pc.CASES} >= set(pc.P_CHOICES)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_a_case_is_within_the_caps(case):
    assert pc.caps(case) == []
    p = case.plan()
    assert 4 <= len(case.ts_inds) <= 8 and int(p.leaf_numel.max()) <= 1 << 18
    assert 1 <= p.slice_range[1] - p.slice_range[0] <= 64 and p.macs <= 5 * 10 ** 7
    assert p.arena_elems <= 1 << 22 and p.out_numel <= 1 << 18
    assert len(p.steps) == len(case.ts_inds) - 1 and not set(case.sparse) & set(case.slices)
    plain, rows = pc.launches_per_assignment(p)
    assert sum(plain) + sum(rows) == len(p.steps) + len(set(p.perms[:, 6].tolist()))
    if case.name.startswith("seed-"):
        projs = case.projs()
        assert len(projs) in pc.P_CHOICES and 3 <= len(case.output_inds) <= 7 and 2 <= len(case.sparse) <= 4
        assert len(projs) <= 2 or (projs[-1] == projs[0]).all()


def _reached(cases):
    got = {}
    for c in cases:
        for item in pc.coverage(c, reference_of(c)[0]):
            got.setdefault(item, []).append(f"{c.name}-{c.dtype}")
    return got


@pytest.mark.parametrize("item", pc.REQUIRED)
def test_the_table_reaches(item):
    real = _reached(c for c in pc.CASES if np.dtype(c.dtype).kind == "f")
    cplx = _reached(c for c in pc.CASES if np.dtype(c.dtype).kind == "c")
    assert item in real, f"no case of a real dtype reaches '{item}'"
    assert item in cplx, f"no case of a complex dtype reaches '{item}'"
    print(f"{item}: {', '.join(real[item][:3])}; {', '.join(cplx[item][:3])}")


def test_every_row_slot_runs_with_an_arena_operand():
    """The point of the table: launches of each of the three row-mapped kernels with an intermediate as an operand."""
    count = dict.fromkeys(pc.CLASSES, 0)
    for c in pc.CASES:
        p = reference_of(c)[0]
        for s in pc.step_table(c, p):
            if s["launch"] == "rows" and (s["A"]["arena"] or s["B"]["arena"]):
                count[s["cls"]] += c.n_assignments()
    assert min(count.values()) > 0, count


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_the_replay_in_the_case_dtype_is_inside_the_bound(case):
    ratio = replay_case(case)
    print(f"{case.name} {case.dtype}: replay, largest error / bound {ratio:.4f} (kt {pc.kt(reference_of(case)[0])})")


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_the_reference_is_the_dense_einsum_at_the_projections(case):
    p, arrays, ref, mag, _ = reference_of(case)
    if np.prod([case.dim[x] for x in case.sparse], dtype=np.int64) * int(np.prod(p.shape[1:], dtype=np.int64)) > 1 << 21:
        return  # (the dense result is large: the generator's 520 or 600 on a sparse index)
    dense, dense_mag = pc.dense_reference(case, p, arrays)
    np.testing.assert_allclose(ref, dense, rtol=1e-12, atol=1e-13 * float(mag.max()))
    np.testing.assert_allclose(mag, dense_mag, rtol=1e-12)


# ---- the bound has teeth

def _row_operands(p, need_map):
    """(step, side) of every operand of a row step that has two rows or more (and, `need_map`, a map)."""
    for k, rw in enumerate(p.row_steps):
        for side in (0, 1):
            if int(rw[0]) > 1 and int(rw[1 + 2 * side]) > 1 and (int(rw[2 + 2 * side]) >= 0 or not need_map):
                yield k, side


def plant_wrong_map_entry(p):
    k, side = next(_row_operands(p, True))
    q = copy.copy(p)
    q.row_maps = p.row_maps.copy()
    at, rows = int(p.row_steps[k, 2 + 2 * side]), int(p.row_steps[k, 1 + 2 * side])
    q.row_maps[at] = (q.row_maps[at] + 1) % rows
    return q


def plant_row_zero(p):
    k, side = next(_row_operands(p, False))
    q = copy.copy(p)
    R = int(p.row_steps[k, 0])  # a map of R zeros, appended to the pool
    q.row_steps = p.row_steps.copy()
    q.row_steps[k, 2 + 2 * side] = p.row_maps.size
    q.row_maps = np.concatenate([p.row_maps, np.zeros(R, np.int32)])
    return q


def plant_swapped_projections(p):
    n_rows, row_of_proj = p.out_rows
    row_of_proj = row_of_proj.copy()
    j = int(np.argmax(row_of_proj != row_of_proj[0]))
    row_of_proj[[0, j]] = row_of_proj[[j, 0]]
    q = copy.copy(p)
    q.out_rows = (n_rows, row_of_proj)
    return q


def _defect_cases(feature):
    return [pytest.param(c, id=i) for c, i in zip(pc.CASES, pc.IDS) if feature(c.plan())]


def _assert_caught(case, q, what):
    p, arrays, ref, mag, bound = reference_of(case)
    bad = outside(_interpret(q, arrays), ref, bound)
    assert bad.any(), f"{case.name}: {what} stays inside the bound in every element"


@pytest.mark.parametrize("case", _defect_cases(lambda p: any(True for _ in _row_operands(p, True))))
def test_a_wrong_map_entry_leaves_the_bound(case):
    _assert_caught(case, plant_wrong_map_entry(reference_of(case)[0]), "a wrong map entry")


@pytest.mark.parametrize("case", _defect_cases(lambda p: any(True for _ in _row_operands(p, False))))
def test_an_operand_read_at_row_zero_leaves_the_bound(case):
    _assert_caught(case, plant_row_zero(reference_of(case)[0]), "an operand read at row 0 for every r")


@pytest.mark.parametrize("case", _defect_cases(lambda p: len(set(p.out_rows[1].tolist())) > 1))
def test_two_projections_swapped_leave_the_bound(case):
    _assert_caught(case, plant_swapped_projections(reference_of(case)[0]), "two rows of the result swapped")


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_a_dropped_product_leaves_the_bound(case, monkeypatch):
    """The interpreter multiplies with numpy.matmul, once per step and assignment: the call of the last step in the first
    assignment gets the largest product of its element (0, 0, 0, 0) taken out again."""
    p, arrays, ref, mag, bound = reference_of(case)
    matmul, calls = np.matmul, []

    def dropping(a, b):
        z = matmul(a, b)
        calls.append(1)
        if len(calls) == len(p.steps):
            products = a[0, 0, 0, :] * b[0, 0, :, 0]
            z[0, 0, 0, 0] -= products[int(np.argmax(np.abs(products)))]
        return z

    monkeypatch.setattr(np, "matmul", dropping)
    got = _interpret(p, arrays)
    monkeypatch.undo()
    assert len(calls) == len(p.steps) * case.n_assignments()
    assert outside(got, ref, bound).any(), f"{case.name}: a dropped product stays inside the bound in every element"
