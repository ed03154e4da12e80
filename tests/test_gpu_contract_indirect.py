"""Operands read in place (`contract(..., indirect=True)`, csrc/contract_indirect.h, tnco_hip_contract_set_indirect) on
the device.

The contract of the feature is bit equality with `indirect=None`: every case of tests/indirect_cases.py is run without
and with the keyword -- the one-step networks folded on A alone, on B alone and on both, in the four dtypes; the chains
also with slice_batch 1, 5 and 64 and with hoist=True, unbatched and in batches of 5 -- and the bytes of the result, the
multiply-adds and every launch count are compared: the launches are computed from the two plans
(tests/indirect_cases.py launch_counts), a step with a folded operand in its slot of `indirect_launches` and in none of
`kernel_launches`, and the gather launches lower by the permute groups that the folded permutes emptied.

Two equal wrong answers would pass that, so the result is also held, element by element, to numpy's einsum of the
network in double precision under (c kt + 2) u (|A| |B|), the bound of the plain kernels (tests/mode_cases.py
plain_bound; inputs uniform in (0.5, 1.5), no cancellation)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import indirect_cases as ic
from tests import mode_cases as mc

pytestmark = pytest.mark.gpu

CHAIN_SETTINGS = [dict()] + [dict(slice_batch=B) for B in ic.BATCHES] + [dict(hoist=True), dict(hoist=True, slice_batch=5)]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


@functools.lru_cache(maxsize=None)
def leaves_and_reference(name, fold, dtype):
    """(the leaves, the einsum of the network in double precision, the same of the moduli): computed once per case."""
    case = ic.case(name, fold, dtype)
    arrays = mc.fill(case)
    for a in arrays:
        a.setflags(write=False)
    ref, mag = mc.reference(case, case.plan(), arrays)
    return arrays, ref, mag


def total(counts, G):
    once, per = counts
    return tuple(tuple(a + G * b for a, b in zip(o, q)) for o, q in zip(once, per))


def check(ctr, name, fold, dtype, settings, folds=None):
    case = ic.case(name, fold, dtype)
    arrays, ref, mag = leaves_and_reference(name, fold, dtype)
    n = case.n_assignments()

    def call(**kw):
        return ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices,
                            slice_range=case.slice_range, **kw)

    r = None
    for kw in settings:
        what = f"{case.name} {dtype} {kw}"
        p0, p = case.plan(**kw), case.plan(indirect=True, **kw)
        assert p.indirect > 0 and (folds is None or p.indirect == folds[bool(kw.get("hoist"))]), what
        base, r = call(**kw), call(indirect=True, **kw)
        G = ic.groups(n, kw.get("slice_batch"))
        assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.dtype(dtype), what
        assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the run without indirect"
        assert r.indirect == p.indirect and base.indirect is None, what
        plain0, through0 = total(ic.launch_counts(p0), G)
        plain, through = total(ic.launch_counts(p), G)
        assert base.kernel_launches == plain0 and base.indirect_launches == through0 == (0, 0, 0), what
        assert r.kernel_launches == plain and r.indirect_launches == through, what
        # the gathers: lower by the permute groups that are gone; the steps: those with a folded operand left their slots
        assert base.kernel_launches[0] - r.kernel_launches[0] == plain0[0] - plain[0] > 0, what
        assert sum(base.kernel_launches[1:]) - sum(r.kernel_launches[1:]) == sum(r.indirect_launches) > 0, what
        assert r.batch_launches == base.batch_launches == (G if "slice_batch" in kw else 0), what
        assert r.launches == sum(r.kernel_launches) + sum(r.indirect_launches) + r.batch_launches < base.launches, what
        assert r.macs == base.macs == p.macs and r.n_slices == base.n_slices == n, what
        assert r.hoisted == base.hoisted == p.hoisted and r.slice_batch == base.slice_batch, what
        assert r.row_kernel_launches == (0, 0, 0) and r.path_launches == (0, 0), what
        # the library and the plan count the same change (a handle whose plan needs no arena holds one element of one)
        empty = np.dtype(dtype).itemsize * ((p.arena_elems == 0) - (p0.arena_elems == 0))
        assert r.peak_device_bytes - base.peak_device_bytes == p.peak_device_bytes - p0.peak_device_bytes + empty, what
    again = call(indirect=True, **settings[-1])
    assert np.array_equal(bits(again.array), bits(r.array)), f"{case.name}: a second call differs"
    err = np.abs(np.asarray(r.array).astype(ref.dtype) - ref)
    limit = mc.plain_bound(case, case.plan(), mag)
    print(f"{case.name} {dtype}: largest error / bound {float((err / limit).max()):.4f}")
    assert r.array.shape == ref.shape and not np.isnan(r.array).any() and (err <= limit).all(), (case.name, dtype)


@pytest.mark.parametrize("dtype", ic.DTYPES)
@pytest.mark.parametrize("name,fold", ic.ONE_STEP, ids=[f"{n}-{f}" for n, f in ic.ONE_STEP])
def test_a_step_that_reads_in_place_is_the_permuted_step_bit_for_bit(ctr, name, fold, dtype):
    sliced = ic.SHAPES[name][4]
    check(ctr, name, fold, dtype, [dict(), dict(slice_batch=5)] if sliced else [dict()])


def test_the_second_trip_of_the_stream_loop(ctr):
    check(ctr, ic.SECOND_TRIP, "a", "float32", [dict()])


@pytest.mark.parametrize("dtype", ic.DTYPES)
@pytest.mark.parametrize("name", ic.CHAINS)
def test_a_chain_in_batches_and_hoisted(ctr, name, dtype):
    check(ctr, name, None, dtype, CHAIN_SETTINGS, ic.CHAIN_FOLDS[name])


def test_nothing_folded_runs_as_without_the_keyword(ctr):
    case = mc.CASES[mc.IDS.index("hand-tiled-11-h2-complex64")]
    assert case.plan(indirect=True).indirect == 0
    arrays = mc.fill(case)
    call = lambda **kw: ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds,  # noqa: E731
                                     slices=case.slices, **kw)
    base, r = call(), call(indirect=True)
    assert np.array_equal(bits(r.array), bits(base.array)) and r.indirect == 0 and base.indirect is None
    assert r.kernel_launches == base.kernel_launches and r.launches == base.launches and r.indirect_launches == (0, 0, 0)
    assert r.peak_device_bytes == base.peak_device_bytes


def test_the_setter_validates_the_tables(ctr):
    """Through the ABI: tables that could send a lane outside its operand are refused with a text of their own, so are
    handles in a mode the kernels do not serve, and a handle that a refused call was made on runs as if it had not been."""
    from tnco_amd import _lib
    L = _lib.load()
    i64 = lambda v: np.ascontiguousarray(v, np.int64)  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    err = lambda: L.tnco_hip_last_error().decode()  # noqa: E731

    def handle(p):
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        del keep
        return h

    def refused(h, steps, maps, text):
        steps, maps = i64(steps), i64(maps)
        assert L.tnco_hip_contract_set_indirect(h, ptr(steps), maps.size, ptr(maps)) == _lib.EINVAL, text
        assert text in err(), (text, err())

    case = ic.case("reordered", None, "float64")
    arrays = mc.fill(case)
    p0, p = case.plan(), case.plan(indirect=True)
    assert ic.folded_sides(p) == [(False, True), (False, True)]  # the leaf (j1, k, j2), then the intermediate
    steps, maps = p.ind_steps, p.ind_maps
    want = ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices, indirect=True)
    h = handle(p)
    try:
        out = np.empty(p.out_numel, p.dtype)
        leaves = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        assert L.tnco_hip_contract_run(h, leaves, ptr(out)) == _lib.EINVAL  # folded operands and no tables yet
        assert "call tnco_hip_contract_set_indirect before the run" in err()
        bad = steps.copy()
        bad[0, 5] = maps.size  # the n table of step 0 starts at the end of the pool
        refused(h, bad, maps, "step 0: an offset table lies outside the pool.")
        bad = steps.copy()
        bad[1, 4] = -1  # two tables of three
        refused(h, bad, maps, "step 1: an offset table lies outside the pool.")
        bad = steps.copy()
        bad[1, 3:6] = -1  # no tables for an operand with both strides 0
        refused(h, bad, maps, "step 1: an operand with both strides 0 needs its tables.")
        bad = steps.copy()
        bad[0, 0:3] = bad[0, 3:6]  # tables for an operand that has strides
        refused(h, bad, maps, "step 0: both stride columns of a folded operand must be 0.")
        off = maps.copy()
        off[steps[0, 4] + 1] = -1
        refused(h, steps, off, "step 0: an offset table has a negative entry.")
        # the leaf of step 0 has 3 x 6 x 7 = 126 elements: an entry of 126, and entries whose sum is 126
        k_tab, n_tab = int(steps[0, 4]), int(steps[0, 5])
        off = maps.copy()
        off[n_tab + 2] = 126
        refused(h, steps, off, "step 0: an offset table reaches beyond its operand.")
        off = maps.copy()
        off[k_tab + 1] = 36  # (inside the leaf by itself)
        assert max(off[k_tab:k_tab + 6]) + max(off[n_tab:n_tab + 21]) == 126
        refused(h, steps, off, "step 0: an offset table reaches beyond its operand.")
        off = maps.copy()
        off[int(steps[1, 5])] = p.arena_elems  # the intermediate of step 1, in the arena
        refused(h, steps, off, "step 1: an offset table reaches beyond its operand.")
        assert L.tnco_hip_contract_set_indirect(h, None, maps.size, ptr(i64(maps))) == _lib.EINVAL
        assert L.tnco_hip_contract_set_indirect(h, ptr(i64(steps)), 5, None) == _lib.EINVAL
        # the handle is as it was: it takes the good tables and gives the bytes of the call through contract()
        got = ctr._run_handle(L, h, p, [np.ascontiguousarray(a) for a in arrays], None)
        h = None
        assert np.array_equal(bits(got.array), bits(want.array)) and got.indirect_launches == want.indirect_launches
    finally:
        if h is not None:
            L.tnco_hip_contract_destroy(h)
    # a handle with tables refuses the modes, and a handle in a mode refuses the tables
    h = handle(p)
    try:
        assert L.tnco_hip_contract_set_indirect(h, ptr(i64(steps)), maps.size, ptr(i64(maps))) == _lib.OK
        assert L.tnco_hip_contract_set_matrix(h, 1) == _lib.EINVAL
        assert "matrix mode is not supported with indirect operands" in err()
        assert L.tnco_hip_contract_set_path_kernel(h, 4) == _lib.EINVAL
        assert "a path kernel is not supported with indirect operands" in err()
        assert L.tnco_hip_contract_set_slice_batch(h, 5) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(h)
    p32 = case.with_(dtype="float32").plan(indirect=True)  # (a compute mode takes float32 and complex64 plans only)
    h = handle(p32)
    try:
        assert L.tnco_hip_contract_set_indirect(h, ptr(i64(p32.ind_steps)), p32.ind_maps.size,
                                                ptr(i64(p32.ind_maps))) == _lib.OK
        assert L.tnco_hip_contract_set_compute(h, 1) == _lib.EINVAL
        assert "a compute mode is not supported with indirect operands" in err()
        assert L.tnco_hip_contract_set_compute(h, 0) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(h)
    none = np.full((len(p0.steps), ctr.IND_W), -1, np.int64)
    for setter, arg, text in ((L.tnco_hip_contract_set_matrix, 1, "matrix mode is not supported with indirect operands."),
                              (L.tnco_hip_contract_set_path_kernel, 4, "a path kernel is not supported with indirect operands.")):
        h = handle(p0)
        try:
            assert setter(h, arg) == _lib.OK
            refused(h, none, maps, text)
        finally:
            L.tnco_hip_contract_destroy(h)
    h = handle(case.with_(dtype="float32").plan())
    try:
        assert L.tnco_hip_contract_set_compute(h, 1) == _lib.OK
        refused(h, none, maps, "a compute mode is not supported with indirect operands.")
    finally:
        L.tnco_hip_contract_destroy(h)
    h = handle(case.with_(dtype="float32").plan(storage="float16"))
    try:
        refused(h, none, maps, "indirect operands need a plain dtype.")
    finally:
        L.tnco_hip_contract_destroy(h)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    h = handle(rows)
    try:
        refused(h, none[:1], maps, "row axes are not supported with indirect operands.")
    finally:
        L.tnco_hip_contract_destroy(h)
    # all -1 on a handle without folded operands: it runs as one on which the call was never made
    h = handle(p0)
    try:
        assert L.tnco_hip_contract_set_indirect(h, ptr(none), 0, None) == _lib.OK
        assert L.tnco_hip_contract_set_matrix(h, 1) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(h)
    assert L.tnco_hip_contract_set_indirect(None, None, 0, None) == _lib.EINVAL
    counts = np.zeros(3, np.int64)
    assert L.tnco_hip_contract_indirect_launches(None, ptr(counts)) == _lib.EINVAL
