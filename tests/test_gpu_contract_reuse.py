"""Reuse (`contract(..., reuse=True)`, csrc/contract.hip tnco_hip_contract_set_reuse) and `slice_order=` on the device.

The contract of the feature is bit equality with `reuse=None` under the same order of the sliced indices: every case of
tests/reuse_cases.py is run without and with the keyword and the bytes of the result and the exponents (under scaling)
are compared.  The multiply-adds and every launch count of the reusing run are those that the plan's periods and the
range predict (tests/reuse_cases.py predicted), counted assignment by assignment, and a second call gives the same bytes.

Two equal wrong answers would pass that, so the result is also held, element by element, to numpy's einsum of the
network in double precision under the bound of the mode's own tests (tests/mode_cases.py: plain_bound, split_bound,
storage_bound; inputs uniform in (0.5, 1.5), no cancellation).  Under another order of the sliced indices the assignments
are summed in another order, and that bound is the only comparison with the default order."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mode_cases as mc
from tests import reuse_cases as rc

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64", "complex64", "complex128")
SINGLES = ("float32", "complex64")


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def step_on_u(case):
    """The first step of the path below which u alone is sliced: its result is a kept tensor of period 2."""
    step_dep, _ = rc.deps(case, case.plan())
    return next(k for k, d in enumerate(step_dep) if d == {"u"})


@functools.lru_cache(maxsize=None)
def leaves(name, dtype, storage=None, planted=False):
    case = rc.case(name, dtype)
    arrays = mc.fill(case, storage)
    if planted:  # one element of a leaf below the kept tensor 64 times the others: its largest part is that much larger
        t = sorted(case.path[step_on_u(case)])[0]  # (step 0: the positions of the path are the leaves')
        assert set(case.ts_inds[t]) & set(case.slices) == {"u"} and case.ts_inds[t][0] == "u" and step_on_u(case) == 0
        arrays[t] = arrays[t].copy()
        # at the last value of u: `exponents` are those after the last assignment, which reads the kept tensor as the
        # assignment before left it
        arrays[t][-1].reshape(-1)[0] *= 64  # (exact in either storage type)
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def reference(name, dtype, slice_inds, storage=None, planted=False):
    """(the einsum of the network in double precision, the same of the moduli): once per case and order of the slices
    (the order decides which assignments a slice_range holds)."""
    case = rc.case(name, dtype)
    return mc.reference(case, case.plan(slice_order=slice_inds), leaves(name, dtype, storage, planted))


def check(ctr, name, dtype, mode, bound, order=None, storage=None, planted=False):
    case = rc.case(name, dtype)
    arrays = list(leaves(name, dtype, storage, planted))
    p = case.plan(reuse=True, **rc.order_kw(case, order), **mode)
    same_order = dict(slice_order=p.slice_inds)  # (what "reuse" chose, for the run without the keyword)
    q = case.plan(**same_order, **mode)
    want = rc.predicted(p)
    what = f"{name} {dtype} {mode} {order}"

    def call(**kw):
        return ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices,
                            slice_range=case.slice_range, **mode, **kw)

    base, r = call(**same_order), call(reuse=True, **rc.order_kw(case, order))
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.dtype(dtype), what
    assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the run without reuse"
    assert r.exponents == base.exponents and (r.exponents is not None) == ("scaling" in mode), what
    assert r.reused == p.reused and base.reused is None and r.hoisted is None, what
    assert r.n_slices == base.n_slices == case.n_assignments(), what
    # what ran is what the periods say, slot by slot; the run without the keyword launches everything at every assignment
    assert r.macs == p.macs == want["macs"] and base.macs == q.macs == rc.predicted(q)["macs"], what
    assert r.kernel_launches == want["kernel"] and base.kernel_launches == rc.predicted(q)["kernel"], what
    assert r.indirect_launches == want["indirect"] and r.narrow_launches == want["narrow"], what
    assert r.split_launches == want["split"] and r.matrix_launches == want["matrix"], what
    assert r.launches == want["launches"] == sum(r.kernel_launches) + sum(r.indirect_launches) + r.narrow_launches, what
    assert r.batch_launches == 0 and r.row_kernel_launches == (0, 0, 0) and r.path_launches == (0, 0), what
    # (launches: a permute group with rows of two periods is two gather launches where the plain run has one)
    assert (r.macs < base.macs) == (p.reused[0] > 0), what
    assert r.indirect == p.indirect and base.indirect == q.indirect, what  # (a slower source is not folded: fewer than the plain plan)
    # the library and the plan count the same change of the arena (kept buffers can move its peak)
    assert r.peak_device_bytes - base.peak_device_bytes == p.peak_device_bytes - q.peak_device_bytes, what
    again = call(reuse=True, **rc.order_kw(case, order))
    assert np.array_equal(bits(again.array), bits(r.array)) and again.exponents == r.exponents, f"{what}: a second call differs"
    ref, mag = reference(name, dtype, p.slice_inds, storage, planted)
    err = np.abs(np.asarray(r.array).astype(ref.dtype) - ref)
    limit = bound(case, q, mag)
    print(f"{what}: largest error / bound {float((err / limit).max()):.4f}")
    assert r.array.shape == ref.shape and not np.isnan(r.array).any() and (err <= limit).all(), what
    return r, p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", rc.NAMES)
def test_a_reusing_run_is_the_plain_run_bit_for_bit(ctr, name, dtype):
    _, p = check(ctr, name, dtype, {}, mc.plain_bound)
    assert p.reused == rc.TABLE[name][1]


@pytest.mark.parametrize("dtype", ("float32", "complex128"))
@pytest.mark.parametrize("order", rc.ORDERS[1:], ids=rc.ORDER_IDS[1:])
@pytest.mark.parametrize("name", rc.NAMES)
def test_another_order_of_the_sliced_indices(ctr, name, order, dtype):
    _, p = check(ctr, name, dtype, {}, mc.plain_bound, order=order)
    if order == "reversed":
        assert p.slice_inds == ("w", "u", "p")


HALF_MODES = [dict(storage="bfloat16"), dict(storage="float16", scaling="tensor"), dict(compute="bf16x3"), dict(compute="matrix")]
HALF_IDS = ["bfloat16", "float16-scaled", "bf16x3", "matrix"]


# (matrix mode takes the four dtypes, the others the single-precision ones)
HALF_PARAMS = [pytest.param(m, d, id=f"{i}-{d}") for m, i in zip(HALF_MODES, HALF_IDS) for d in (DTYPES if i == "matrix" else SINGLES)]


@pytest.mark.parametrize("mode,dtype", HALF_PARAMS)
@pytest.mark.parametrize("name", rc.TILED)
def test_a_kept_tensor_feeds_the_matrix_cores(ctr, name, mode, dtype):
    storage, scaled = mode.get("storage"), "scaling" in mode
    if storage is None:
        r, _ = check(ctr, name, dtype, mode, mc.split_bound if mode["compute"] == "bf16x3" else mc.plain_bound)
        assert (r.split_launches if mode["compute"] == "bf16x3" else r.matrix_launches) > 0
        return
    bound = lambda case, p, mag: mc.storage_bound(case, p, mag, storage)  # noqa: E731
    planted = scaled and step_on_u(rc.case(name)) == 0
    r, p = check(ctr, name, dtype, mode, bound, storage=storage, planted=planted)
    if planted:  # the kept tensor is the result of step 0: its exponent is its own, and it stays while the others are rewritten
        case = rc.case(name, dtype)
        slot = len(case.ts_inds)
        assert p.step_period[0] == 2 and r.exponents[slot] != 0
        flat = ctr.contract(list(case.path), case.ts_inds, list(leaves(name, dtype, storage, False)), case.output_inds,
                            slices=case.slices, reuse=True, **mode)
        assert r.exponents[slot] > flat.exponents[slot]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", rc.ORDERS, ids=rc.ORDER_IDS)
@pytest.mark.parametrize("name", rc.INDIRECT)
def test_folded_operands_and_kept_permutes(ctr, name, order, dtype):
    r, p = check(ctr, name, dtype, dict(indirect=True), mc.plain_bound, order=order)
    if order is None:
        # one operand is read in place at its step's period; a slower source stays a permute (but in `nested`) and is kept
        assert p.indirect >= 1 and sum(r.indirect_launches) > 0
        if name != "nested":
            row = p.perms[p.perm_period == 2][0]
            assert p.step_period[int(row[6])] == 1 and (int(row[3]), int(row[5])) in p.kept
        plain = rc.case(name, dtype).plan(reuse=True)
        assert len(p.perms) < len(plain.perms)


def test_nothing_to_reuse_runs_as_without_the_keyword(ctr):
    case = rc.case("kept-first-stream-7-9-11", "complex64").with_(slices=())
    arrays = mc.fill(case)
    call = lambda **kw: ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, **kw)  # noqa: E731
    base, r = call(), call(reuse=True, slice_order="reuse")
    assert np.array_equal(bits(r.array), bits(base.array)) and r.reused == (0, 0) and base.reused is None
    assert r.kernel_launches == base.kernel_launches and r.launches == base.launches and r.macs == base.macs
    a = mc.fill(case)[2]
    one = ctr.contract([], [case.ts_inds[2]], [a], slices=("u",), reuse=True)
    assert one.reused == (0, 0) and np.array_equal(bits(one.array), bits(ctr.contract([], [case.ts_inds[2]], [a], slices=("u",)).array))
    # a path that leaves several tensors: every part unsliced
    parts = ctr.contract([(1, 2)], case.ts_inds[:3], arrays[:3], reuse=True)
    assert parts.reused == (0, 0) and len(parts.array) == 2


def test_the_setter_validates_the_periods(ctr):
    """Through the ABI: every argument the setter refuses, with its status and its text, and the run afterwards
    unchanged: the same counts before the periods are set, the same bytes and counts after."""
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

    def run(h, p, arrays):
        out = np.empty(p.out_numel, p.dtype)
        held = [np.ascontiguousarray(a, p.dtype) for a in arrays]
        ptrs = (C.c_void_p * len(held))(*[a.ctypes.data for a in held])
        _lib.check(L.tnco_hip_contract_run(h, ptrs, ptr(out)))
        stats = np.zeros(4, np.int64)
        _lib.check(L.tnco_hip_contract_stats(h, ptr(stats)))
        return out, int(stats[0]), int(stats[1])

    def refused(h, steps, perms, text):
        assert L.tnco_hip_contract_set_reuse(h, ptr(i64(steps)), ptr(i64(perms))) == _lib.EINVAL, text
        assert L.tnco_hip_last_error() == text.encode(), (L.tnco_hip_last_error(), text)

    not_a_period = "a period must be the place of a sliced index or the number of assignments."
    with_ = lambda v, k, x: np.concatenate([v[:k], [x], v[k + 1:]]).astype(np.int64)  # noqa: E731
    # (case, [(step periods or None for the plan's, permute periods or None, the text)]): one entry per refusal that needs
    # no other tables than the plan's
    by_case = {
        "nested": lambda p: [  # steps [6, 2, 1, 1]; step 0 reads two leaves sliced by p in place
            (with_(p.step_period, 3, 2), None, "the step that writes the output must have period 1."),
            (with_(p.step_period, 0, 12), None, "a step is slower than a sliced leaf it reads allows."),
            (with_(p.step_period, 1, 6), None, "a step is slower than a sliced leaf it reads allows."),
            (None, [2], "a permute is slower than a sliced leaf it reads allows.")],
        "kept-first-stream-7-9-11": lambda p: [  # steps [2, 1, 1, 1]; step 2 reads the results of steps 0 and 1
            (with_(p.step_period, 2, 2), None, "a step is slower than the item that wrote its operand."),
            (with_(p.step_period, 3, 6), None, "the step that writes the output must have period 1.")],
        "arena-permute": lambda p: [  # permutes [2, 1]: row 0 moves the result of step 0, of period 2
            (None, [6, 1], "a permute is slower than the item that wrote its source."),
            (None, [2, 2], "a permute is slower than the item that wrote its source.")],
        "leaf-gather": lambda p: [  # permute [2]: the gather of the leaf (m, u, k)
            (None, [6], "a permute is slower than a sliced leaf it reads allows."),
            (None, [12], "a permute is slower than a sliced leaf it reads allows.")],
        "both-permuted-stream-6-6-5": lambda p: [  # permutes [2, 1, 1] in the groups [2, 2, 3]
            (None, [1, 2, 1], "the rows of a permute group must be ordered by period, the largest first.")],
        "chain": lambda p: [],
        # accepted as planned: the temporary of the slowest phase (step 0) lies where the faster phase on p and u keeps
        # the result of step 2 -- a slower phase may write over a faster phase's kept tensor, which is then written again
        "nested-deep": lambda p: [],
    }
    deep = rc.case("nested-deep").plan(reuse=True)
    assert deep.step_period.tolist() == [6, 6, 2, 1, 1] and deep.steps[0][9] == deep.steps[2][9] == 0
    assert deep.kept == ((64, 30), (0, 35)) and deep.kept_period == (6, 2)
    for name, refusals in by_case.items():
        case = rc.case(name)
        arrays = mc.fill(case)
        p, plain = case.plan(reuse=True), case.plan()
        S, P = len(p.steps), len(p.perms)
        good = (i64(p.step_period), i64(p.perm_period if P else [1]))
        if name == "nested":
            assert p.step_period.tolist() == [6, 2, 1, 1] and p.steps[0][0] == p.steps[0][4] == p.steps[1][0] == ctr.LEAF
        h = handle(p)
        try:
            # the plain plan on a handle of its own: the bytes to get.  The tables of the reusing plan without periods run
            # every item at every assignment in path order, which their arena is not planned for: the counts are
            # compared, not the bytes
            h0 = handle(plain)
            try:
                want_bits = bits(run(h0, plain, arrays)[0])
            finally:
                L.tnco_hip_contract_destroy(h0)
            want = run(h, p, arrays)
            assert want[1] == plain.macs
            for bad in (0, 3, 4, 5, -2, 24):
                refused(h, with_(good[0], 0, bad), good[1], not_a_period)
                if P:
                    refused(h, good[0], with_(good[1], 0, bad), not_a_period)
            for steps, perms, text in refusals(p):
                refused(h, good[0] if steps is None else steps, good[1] if perms is None else perms, text)
            assert L.tnco_hip_contract_set_reuse(h, None, ptr(good[1])) == _lib.EINVAL
            assert run(h, p, arrays)[1:] == want[1:]  # (a refusal leaves the handle as it was)
            # every period 1: as if never called; then the periods of the plan
            assert L.tnco_hip_contract_set_reuse(h, ptr(i64(np.ones(S))), ptr(i64(np.ones(max(P, 1))))) == _lib.OK
            assert run(h, p, arrays)[1:] == want[1:]
            assert L.tnco_hip_contract_set_reuse(h, ptr(good[0]), ptr(good[1])) == _lib.OK
            got = run(h, p, arrays)
            assert np.array_equal(bits(got[0]), want_bits) and got[1] == p.macs <= want[1] and got[2] == rc.predicted(p)["launches"]
            for steps, perms, text in refusals(p):  # (and a refusal leaves the periods as they were)
                refused(h, good[0] if steps is None else steps, good[1] if perms is None else perms, text)
            # a handle with periods takes no slice batch, no path kernel and no hoist flags
            assert L.tnco_hip_contract_set_slice_batch(h, 5) == _lib.EINVAL
            assert L.tnco_hip_last_error() == b"a slice batch is not supported with reuse periods."
            assert L.tnco_hip_contract_set_path_kernel(h, 4) == _lib.EINVAL
            assert L.tnco_hip_last_error() == b"a path kernel is not supported with reuse periods."
            assert L.tnco_hip_contract_set_hoist(h, ptr(i64(np.zeros(S))), ptr(i64(np.zeros(max(P, 1))))) == _lib.EINVAL
            assert L.tnco_hip_last_error() == b"hoisting is not supported with reuse periods: they include it."
            again = run(h, p, arrays)
            assert np.array_equal(bits(again[0]), want_bits) and again[1:] == got[1:]
        finally:
            L.tnco_hip_contract_destroy(h)
    # a kept tensor written over by a faster phase: the result of step 2, which every assignment writes, on top of the
    # kept result of step 0
    p = rc.case("nested").plan(reuse=True)
    assert p.kept == ((0, 30), (64, 35)) and p.kept_period == (6, 2) and p.steps[2][8:10].tolist() == [ctr.ARENA, 256]
    assert p.steps[3][4:6].tolist() == [ctr.ARENA, 256]
    over = rc.case("nested").plan(reuse=True)
    over.steps[2, 9] = over.steps[3, 5] = 0
    h = handle(over)
    try:
        refused(h, p.step_period, p.perm_period, "a kept tensor is written over.")
    finally:
        L.tnco_hip_contract_destroy(h)
    # ... and by a later item of its writer's own phase: steps 0 and 1 of `two-kept` both have period 2 and both results
    # are kept; the second one written where the first one lies
    p = rc.case("two-kept").plan(reuse=True)
    assert p.step_period.tolist() == [2, 2, 1, 1, 1, 1] and p.kept == ((0, 30), (64, 30)) and p.kept_period == (2, 2)
    assert p.steps[1][8:10].tolist() == [ctr.ARENA, 64] and p.steps[4][0:2].tolist() == [ctr.ARENA, 64]
    over = rc.case("two-kept").plan(reuse=True)
    over.steps[1, 9] = over.steps[4, 1] = 0
    h = handle(over)
    try:
        refused(h, p.step_period, p.perm_period, "a kept tensor is written over.")
    finally:
        L.tnco_hip_contract_destroy(h)
    h = handle(p)  # (the same periods on the tables as planned: accepted)
    try:
        assert L.tnco_hip_contract_set_reuse(h, ptr(i64(p.step_period)), ptr(i64(p.perm_period))) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(h)
    # handles that take no periods: a slice batch, a path kernel, hoist flags, row axes
    p = rc.case("nested").plan(reuse=True)
    periods = (ptr(i64(p.step_period)), ptr(i64(p.perm_period)))
    for prepare, text in ((lambda h: L.tnco_hip_contract_set_slice_batch(h, 3), b"a slice batch is not supported with reuse periods."),
                          (lambda h: L.tnco_hip_contract_set_path_kernel(h, 3), b"a path kernel is not supported with reuse periods.")):
        h = handle(p)
        try:
            assert prepare(h) == _lib.OK
            assert L.tnco_hip_contract_set_reuse(h, *periods) == _lib.EINVAL and L.tnco_hip_last_error() == text
        finally:
            L.tnco_hip_contract_destroy(h)
    hp = rc.case("chain").plan(hoist=True)
    assert hp.hoisted == (1, 0) and len(hp.perms) == 0
    h = handle(hp)
    try:
        assert L.tnco_hip_contract_set_hoist(h, ptr(i64(hp.step_hoist)), ptr(i64(np.zeros(1)))) == _lib.OK
        assert L.tnco_hip_contract_set_reuse(h, ptr(i64(np.where(hp.step_hoist == 1, 12, 1))), ptr(i64([1]))) == _lib.EINVAL
        assert L.tnco_hip_last_error() == b"hoisting is not supported with reuse periods: they include it."
    finally:
        L.tnco_hip_contract_destroy(h)
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    h = handle(rows)
    try:
        assert L.tnco_hip_contract_set_reuse(h, ptr(i64([1])), ptr(i64(np.ones(max(len(rows.perms), 1))))) == _lib.EINVAL
        assert L.tnco_hip_last_error() == b"row axes are not supported with reuse periods."
    finally:
        L.tnco_hip_contract_destroy(h)
    assert L.tnco_hip_contract_set_reuse(None, None, None) == _lib.EINVAL
