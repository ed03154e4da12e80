"""Hoisting (`contract(..., hoist=True)`, csrc/contract.hip tnco_hip_contract_set_hoist) on the device.

The contract of the feature is bit equality with `hoist=None`: every case of tests/hoist_cases.py is run unbatched and
with slice_batch 1, 5 and 64, each time without and with the keyword, and the bytes of the result, the exponents (under
scaling), the multiply-adds and every launch count are compared.  With G groups of assignments (G = the assignments when
unbatched) a hoisted run launches what the plain one launches minus (G - 1) times the hoisted share, which is computed
from the plan (tests/hoist_cases.py launch_counts, side_counts), and its multiply-adds are the plain ones minus
(assignments - 1) times those of the hoisted steps.

Two equal wrong answers would pass that, so the hoisted result is also held, element by element, to numpy's einsum of
the network in double precision under the bound of the mode's own tests (tests/mode_cases.py: plain_bound, split_bound,
storage_bound; inputs uniform in (0.5, 1.5), no cancellation)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import hoist_cases as hc
from tests import mode_cases as mc

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64", "complex64", "complex128")
HALF_MODES = [dict(storage="float16"), dict(storage="bfloat16"), dict(compute="bf16x3"),
              dict(storage="float16", scaling="tensor"), dict(storage="bfloat16", scaling="tensor")]
HALF_IDS = ["float16", "bfloat16", "bf16x3", "float16-scaled", "bfloat16-scaled"]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def free_leaf(case):
    return next(t for t, xs in enumerate(case.ts_inds) if not set(xs) & set(case.slices))


@functools.lru_cache(maxsize=None)
def leaves_and_reference(name, dtype, storage=None, planted=False):
    """(the leaves, the einsum of the network in double precision, the same of the moduli): computed once per case."""
    case = hc.case(name, dtype)
    arrays = mc.fill(case, storage)
    if planted:  # one element of a slice-free leaf 64 times the others: the kept tensor's largest part is that much larger
        t = free_leaf(case)
        arrays[t] = arrays[t].copy()
        arrays[t].reshape(-1)[0] *= 64  # (exact in either storage type)
    for a in arrays:
        a.setflags(write=False)
    ref, mag = mc.reference(case, case.plan(), arrays)
    return arrays, ref, mag


def check(ctr, name, dtype, mode, bound, storage=None, planted=False):
    case = hc.case(name, dtype)
    arrays, ref, mag = leaves_and_reference(name, dtype, storage, planted)
    n = case.n_assignments()
    p = case.plan(hoist=True, **mode)
    assert p.hoisted == hc.TABLE[name][1] and hc.mixed_groups(p) == 0
    once, per = hc.launch_counts(p)
    side_once, side_per = hc.side_counts(p)

    def call(**kw):
        return ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices,
                            slice_range=case.slice_range, **mode, **kw)

    r = None
    for B in (None,) + hc.BATCHES:
        kw = {} if B is None else dict(slice_batch=B)
        what = f"{name} {dtype} {mode} {kw}"
        base, r = call(**kw), call(hoist=True, **kw)
        G = n if B is None else -(-n // min(B, n))  # groups of assignments: the launches of a step of the loop
        assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.dtype(dtype), what
        assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the run without hoist"
        assert r.exponents == base.exponents and (r.exponents is not None) == ("scaling" in mode), what
        assert r.hoisted == p.hoisted and base.hoisted is None, what
        assert r.n_slices == base.n_slices == n and r.slice_batch == base.slice_batch, what
        # the plain run launches everything once per group; the hoisted one its share once
        assert base.kernel_launches == tuple((a + b) * G for a, b in zip(once, per)), what
        assert r.kernel_launches == tuple(v - (G - 1) * s for v, s in zip(base.kernel_launches, once)), what
        assert r.kernel_launches == tuple(a + b * G for a, b in zip(once, per)), what
        assert r.narrow_launches == base.narrow_launches - (G - 1) * side_once["narrow"], what
        assert r.narrow_launches == side_once["narrow"] + G * side_per["narrow"], what
        assert r.split_launches == base.split_launches - (G - 1) * side_once["split"], what
        assert r.split_launches == side_once["split"] + G * side_per["split"], what
        assert r.batch_launches == base.batch_launches == (0 if B is None else G), what
        assert r.macs == base.macs - (n - 1) * p.hoisted_macs == p.macs and (p.hoisted_macs > 0) == (p.hoisted[0] > 0), what
        assert r.launches == sum(r.kernel_launches) + r.narrow_launches + r.batch_launches, what
        assert (r.launches < base.launches) == (G > 1), what
        assert r.row_kernel_launches == (0, 0, 0) and r.path_launches == (0, 0), what
        # the library and the plan count the same change of the arena (kept buffers can move its peak)
        assert r.peak_device_bytes - base.peak_device_bytes == \
            case.plan(hoist=True, **mode, **kw).peak_device_bytes - case.plan(**mode, **kw).peak_device_bytes, what
    again = call(hoist=True, slice_batch=hc.BATCHES[-1])
    assert np.array_equal(bits(again.array), bits(r.array)) and again.exponents == r.exponents, f"{name}: a second call differs"
    got = call(hoist=True)
    err = np.abs(np.asarray(got.array).astype(ref.dtype) - ref)
    limit = bound(case, case.plan(), mag)
    print(f"{name} {dtype} {mode}: largest error / bound {float((err / limit).max()):.4f}")
    assert got.array.shape == ref.shape and not np.isnan(got.array).any() and (err <= limit).all(), (name, dtype, mode)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_a_hoisted_run_is_the_plain_run_bit_for_bit(ctr, name, dtype):
    check(ctr, name, dtype, {}, mc.plain_bound)


@pytest.mark.parametrize("dtype", ("float32", "complex64"))
@pytest.mark.parametrize("mode", HALF_MODES, ids=HALF_IDS)
@pytest.mark.parametrize("name", hc.TILED)
def test_a_kept_tensor_feeds_the_matrix_cores(ctr, name, mode, dtype):
    storage, scaled = mode.get("storage"), "scaling" in mode
    if storage is None:
        check(ctr, name, dtype, mode, mc.split_bound)
        return
    bound = lambda case, p, mag: mc.storage_bound(case, p, mag, storage)  # noqa: E731
    got = check(ctr, name, dtype, mode, bound, storage=storage, planted=scaled)
    if scaled:  # the kept tensor is the result of step 0: its exponent is its own, not that of a tensor of (0.5, 1.5) sums
        case = hc.case(name, dtype)
        slot = len(case.ts_inds)
        assert case.plan(hoist=True, **mode).step_hoist[0] == 1 and got.exponents[slot] != 0
        arrays, _, _ = leaves_and_reference(name, dtype, storage, False)
        flat = ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices, hoist=True, **mode)
        assert got.exponents[slot] > flat.exponents[slot]


def test_nothing_to_hoist_runs_as_without_the_keyword(ctr):
    case = hc.case("kept-first-stream-7-9-11", "complex64").with_(slices=())
    arrays = mc.fill(case)
    call = lambda **kw: ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, **kw)  # noqa: E731
    base, r = call(), call(hoist=True)
    assert np.array_equal(bits(r.array), bits(base.array)) and r.hoisted == (0, 0) and base.hoisted is None
    assert r.kernel_launches == base.kernel_launches and r.launches == base.launches and r.macs == base.macs
    a = mc.fill(case)[2]
    one = ctr.contract([], [case.ts_inds[2]], [a], slices=("u",), hoist=True)
    assert one.hoisted == (0, 0) and np.array_equal(bits(one.array), bits(ctr.contract([], [case.ts_inds[2]], [a], slices=("u",)).array))


@pytest.mark.parametrize("dtype", ("float32", "complex128"))
@pytest.mark.parametrize("name", ("kept-first-stream-7-9-11", "arena-permute", "leaf-permute", "chain"))
def test_hoist_flags_are_the_two_period_schedule(ctr, name, dtype):
    """Through the ABI: the plan's flags given to tnco_hip_contract_set_hoist, and given to tnco_hip_contract_set_reuse as
    periods (the number of assignments for a flag, 1 for none), run the same launches on the same bytes.  What the flags
    refuse beyond the periods stays: an unflagged permute of a kept tensor."""
    from tnco_amd import _lib
    L = _lib.load()
    i64 = lambda v: np.ascontiguousarray(v, np.int64)  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    case = hc.case(name, dtype)
    p = case.plan(hoist=True)
    assert p.hoisted == hc.TABLE[name][1]
    flags = (i64(p.step_hoist), i64(p.perm_hoist))
    reads = [(st[0], st[1]) for st, f in zip(p.steps, flags[0]) if f] + [(st[4], st[5]) for st, f in zip(p.steps, flags[0]) if f]
    reads += [(row[0], row[1]) for row, f in zip(p.perms, flags[1]) if f]
    if any(kind == ctr.LEAF and p.leaf_sl[ref][0] != 0 for kind, ref in reads):
        pytest.skip("a hoisted item reads a leaf whose sliced axes have dimension 1: flags refuse it, periods do not")
    n = int(np.prod(list(hc.SLICE_DIMS.values())))
    assert n == hc.N_ASSIGNMENTS == case.n_assignments()
    periods = tuple(np.where(f == 1, n, 1).astype(np.int64) for f in flags)
    arrays = [np.ascontiguousarray(a, p.dtype) for a in mc.fill(case)]
    leaves = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])

    def handle():
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        del keep
        return h

    def run(h):
        out, stats, counts = np.empty(p.out_numel, p.dtype), np.zeros(4, np.int64), np.zeros(len(ctr.KERNEL_PATHS), np.int64)
        _lib.check(L.tnco_hip_contract_run(h, leaves, ptr(out)))
        _lib.check(L.tnco_hip_contract_stats(h, ptr(stats)))
        _lib.check(L.tnco_hip_contract_kernel_launches(h, ptr(counts)))
        return out, int(stats[0]), int(stats[1]), tuple(counts.tolist())

    by_flags, by_periods = handle(), handle()
    try:
        _lib.check(L.tnco_hip_contract_set_hoist(by_flags, ptr(flags[0]), ptr(flags[1])))
        _lib.check(L.tnco_hip_contract_set_reuse(by_periods, ptr(periods[0]), ptr(periods[1])))
        a, b = run(by_flags), run(by_periods)
        assert np.array_equal(bits(a[0]), bits(b[0])), f"{name} {dtype}: the bytes differ"
        assert a[1] == b[1] == p.macs and a[2] == b[2] == sum(a[3]) and a[3] == b[3], (name, dtype, a[1:], b[1:])
        via = ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices, hoist=True)
        assert np.array_equal(bits(a[0]), bits(via.array)) and a[3] == via.kernel_launches, (name, dtype)
        if name == "arena-permute":  # the permute of the kept tensor, unflagged: its source stays kept under periods
            assert flags[1].tolist() == [1] and p.perms[0][0] == ctr.ARENA
            assert L.tnco_hip_contract_set_hoist(by_flags, ptr(flags[0]), ptr(i64([0]))) == _lib.EINVAL
            assert L.tnco_hip_last_error() == b"a permute and the item that writes its source must both be hoisted or both not."
            assert run(by_flags)[1:] == a[1:]  # (the refusal leaves the flags as they were)
            assert L.tnco_hip_contract_set_reuse(by_periods, ptr(periods[0]), ptr(i64([1]))) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(by_flags)
        L.tnco_hip_contract_destroy(by_periods)


def test_the_setter_validates_the_flags(ctr):
    """Through the ABI: flags that do not describe slice-independent work are refused, and so are handles with row axes
    or a path kernel."""
    from tnco_amd import _lib
    L = _lib.load()
    i64 = lambda v: np.ascontiguousarray(v, np.int64)  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def handle(p):
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        del keep
        return h

    for name in ("kept-first-stream-7-9-11", "arena-permute", "leaf-permute", "chain"):
        p = hc.case(name).plan(hoist=True)
        S, P = len(p.steps), len(p.perms)
        good = (i64(p.step_hoist), i64(p.perm_hoist))
        bad = []
        for k in np.nonzero(good[0] == 0)[0]:  # a step that depends on the assignment, flagged
            flip = good[0].copy()
            flip[k] = 1
            bad.append((flip, good[1]))
        for r in np.nonzero(good[1] == 0)[0]:
            flip = good[1].copy()
            flip[r] = 1
            bad.append((good[0], flip))
        if name == "arena-permute":  # the permute of the kept tensor and the step that writes its source go together
            bad += [(i64([0, 0, 0]), good[1]), (good[0], i64([0]))]
        two = good[0].copy()
        two[0] = 2
        bad.append((two, good[1]))
        h = handle(p)
        try:
            for steps, perms in bad:
                assert L.tnco_hip_contract_set_hoist(h, ptr(steps), ptr(perms)) == _lib.EINVAL, (name, steps, perms)
            assert L.tnco_hip_contract_set_hoist(h, None, ptr(good[1])) == _lib.EINVAL
            zeros = (i64(np.zeros(S)), i64(np.zeros(max(P, 1))))
            assert L.tnco_hip_contract_set_hoist(h, ptr(zeros[0]), ptr(zeros[1])) == _lib.OK
            assert L.tnco_hip_contract_set_hoist(h, ptr(good[0]), ptr(good[1])) == _lib.OK
            assert L.tnco_hip_contract_set_path_kernel(h, 4) == _lib.EINVAL  # (a hoisting handle takes no path kernel)
            assert L.tnco_hip_contract_set_slice_batch(h, 5) == _lib.OK
        finally:
            L.tnco_hip_contract_destroy(h)
    p = hc.case("kept-first-stream-7-9-11").plan(hoist=True)
    over = hc.case("kept-first-stream-7-9-11").plan(hoist=True)
    assert over.kept[0][0] == 0 and over.steps[2, 4] == ctr.ARENA
    over.steps[1, 9] = over.steps[2, 5] = 0  # the result of step 1, which every assignment writes, on top of the kept tensor
    h = handle(over)
    try:
        assert L.tnco_hip_contract_set_hoist(h, ptr(i64(p.step_hoist)), ptr(i64(p.perm_hoist))) == _lib.EINVAL
        assert b"kept tensor is written over" in L.tnco_hip_last_error()
    finally:
        L.tnco_hip_contract_destroy(h)
    h = handle(p)
    try:
        assert L.tnco_hip_contract_set_path_kernel(h, 4) == _lib.OK
        assert L.tnco_hip_contract_set_hoist(h, ptr(i64(p.step_hoist)), ptr(i64(p.perm_hoist))) == _lib.EINVAL
    finally:
        L.tnco_hip_contract_destroy(h)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    h = handle(rows)
    try:
        assert L.tnco_hip_contract_set_hoist(h, ptr(i64([0])), ptr(i64(np.zeros(max(len(rows.perms), 1))))) == _lib.EINVAL
    finally:
        L.tnco_hip_contract_destroy(h)
    assert L.tnco_hip_contract_set_hoist(None, None, None) == _lib.EINVAL
