"""The matrix kernel (csrc/contract_matrix.h, `contract(..., compute="matrix")`) at its edges, element by element, in the
four dtypes.

Every case of tests/matrix_cases.py is a one-step network.  A test asserts which kernel ran, from
`ContractionResult.kernel_launches` and from `matrix_launches`, and compares every element with numpy's einsum of the
inputs in a wider type: float64 / complex128 for float32 / complex64, numpy's longdouble for float64 / complex128 (as
tests/range_cases.py does).  The mode rounds nothing on the way -- a real product is one MFMA, an fma chain of the
element type -- so it is held to the plain kernels' bound of tests/test_gpu_contract_kernels.py, as it stands:

    |got - ref| <= (c kt + 2) u (|A| @ |B|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

which any order of fused multiply-adds in the working precision satisfies.  An element that is not a number fails.
A wrong lane-to-row map of the result tile (the float64 instruction has its own) gives a right number in a wrong place:
the exact-sum test, small integers with all rows of A and all columns of B distinct, must EQUAL the integer einsum.
"""
import numpy as np
import pytest

from tests import contract_cases as cc
from tests import matrix_cases as mc
from tests.test_gpu_contract_kernels import _assert_kernels, _assert_within, _result_inds

pytestmark = pytest.mark.gpu

COMPUTE = "matrix"
DTYPES = [pytest.param(d, id=np.dtype(d).name) for d in cc.ALL]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def is_cplx(dtype) -> bool:
    return np.dtype(dtype).kind == "c"


def wide_of(dtype):
    """The type the reference and the bound are computed in."""
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)):
        return np.complex128 if is_cplx(dtype) else np.float64
    return np.clongdouble if is_cplx(dtype) else np.longdouble


def reference(ts, arrays, inds, dtype):
    """(einsum of the up-cast inputs, the same einsum of their moduli) in wide_of(dtype)."""
    wide = wide_of(dtype)
    sym = {x: k for k, x in enumerate(dict.fromkeys(tuple(ts[0]) + tuple(ts[1])))}
    subs = [[sym[x] for x in xs] for xs in ts]
    up = [np.asarray(a, wide) for a in arrays]
    res = [sym[x] for x in inds]
    ref = np.einsum(up[0], subs[0], up[1], subs[1], res)
    mag = np.einsum(np.abs(up[0]), subs[0], np.abs(up[1]), subs[1], res)
    return ref, mag


def bound(mag, kt, dtype):
    u = np.finfo(dtype).eps / 2  # (finfo of a complex type is that of its parts)
    return ((2 if is_cplx(dtype) else 1) * kt + 2) * mag.dtype.type(u) * mag


def draw(shape, dtype, rng, scale=1.0):
    """Every part's magnitude in scale [2^-3, 2^3], random signs, all bits of the type in play."""
    real = np.float32 if np.dtype(dtype).itemsize // (2 if is_cplx(dtype) else 1) == 4 else np.float64
    part = lambda: (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-3, 3, shape) * scale).astype(real)  # noqa: E731
    return (part() + 1j * part()).astype(dtype) if is_cplx(dtype) else part()


def fill(case, dtype, seed, scales=(1.0, 1.0)):
    rng = np.random.RandomState(seed)
    return [draw(shape, dtype, rng, s) for shape, s in zip(case.shapes(), scales)]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def assert_path(ctr, r, case, what):
    """The path from kernel_launches and from matrix_launches."""
    _assert_kernels(ctr, r, case.kernels, what)
    assert r.matrix_launches == mc.matrix_launches(case), what
    assert r.compute == COMPUTE and r.split_launches == 0, what


def run_case(ctr, case, dtype, seed=71, scales=(1.0, 1.0)):
    """Runs one case, asserts path, type and every element; returns (arrays, result)."""
    arrays = fill(case, dtype, seed, scales)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    what = f"{case.name} {np.dtype(dtype).name}"
    inds = _result_inds(case.ts, case.output)
    assert r.inds == inds and r.n_slices == case.n_slices(), what
    assert_path(ctr, r, case, what)
    op = case.ops
    assert r.macs == case.n_slices() * op["H"] * op["M"] * op["N"] * op["K"]
    assert r.array.dtype == np.dtype(dtype), what
    ref, mag = reference(case.ts, arrays, inds, dtype)
    _assert_within(r.array, ref, bound(mag, case.kt, dtype), f"{what}: kt {case.kt}")
    return arrays, r


_ONE_PASS = mc.EDGES + mc.VEC + [mc.BY_NAME["matrix-64x64x33"]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", _ONE_PASS, ids=[c.name for c in _ONE_PASS])
def test_kernel_path_and_every_element(ctr, case, dtype):
    run_case(ctr, case, dtype)


def planted_integers(case, dtype, seed):
    """Integers in [-8, 8] in every part; the rows of A (its [M, K] view) and the columns of B are all distinct."""
    rng = np.random.RandomState(seed)
    out = []
    for side, shape in enumerate(case.shapes()):
        part = lambda: rng.randint(-8, 9, shape).astype(np.float64)  # noqa: E731
        a = part() + 1j * part() if is_cplx(dtype) else part()
        form = case.ops["form_a"] if side == 0 else 1 - case.ops["form_b"]  # 0: the distinct vectors are the rows
        vectors = a if form == 0 else a.T
        assert len({v.tobytes() for v in vectors}) == len(vectors)
        out.append(a.astype(dtype))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", mc.EXACT, ids=[c.name for c in mc.EXACT])
def test_an_exact_sum_comes_out_exact_in_the_right_place(ctr, case, dtype):
    """|x| <= 8 integers: every product and every partial sum is an integer below 2^24 in magnitude, exact in float32
    and float64 in any order, so every element must EQUAL the integer einsum.  With distinct rows of A and columns of B
    an element stored in another row or column, or a k taken twice or not at all, shows."""
    arrays = planted_integers(case, dtype, seed=72)
    op = case.ops
    assert (op["M"], op["N"], op["K"]) == (65, 129, 97) and 2 * op["K"] * 64 < 2 ** 24
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert_path(ctr, r, case, case.name)
    ref, mag = reference(case.ts, arrays, _result_inds(case.ts, case.output), np.complex64 if is_cplx(dtype) else np.float32)
    assert mag.max() < 2 ** 24  # (float64 holds every integer sum here exactly, whatever numpy's order)
    assert r.array.dtype == np.dtype(dtype)
    wrong = r.array.astype(ref.dtype) != ref
    assert not wrong.any(), f"{case.name} {np.dtype(dtype).name}: {int(wrong.sum())} of {wrong.size} elements differ, " \
                            f"first at {tuple(np.argwhere(wrong)[0])}"
    rows, cols = {v.tobytes() for v in r.array}, {v.tobytes() for v in r.array.T}
    assert len(rows) == op["M"] and len(cols) == op["N"]  # (the test can tell rows and columns apart)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", mc.PLAIN, ids=[c.name for c in mc.PLAIN])
def test_below_the_thresholds_the_plain_kernels_run_and_give_the_bytes_of_the_plain_mode(ctr, case, dtype):
    arrays = fill(case, dtype, seed=73)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    plain = ctr.contract([(0, 1)], case.ts, arrays, case.output)
    assert_path(ctr, r, case, case.name)
    assert r.matrix_launches == 0 and plain.matrix_launches == 0 and plain.compute is None
    assert r.kernel_launches == plain.kernel_launches
    assert np.array_equal(bits(r.array), bits(plain.array))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_plain_mode_of_a_tiled_step_is_untouched_by_the_keyword_at_none(ctr, dtype):
    case = mc.BY_NAME["matrix-64x64x33"]
    arrays = fill(case, dtype, seed=74)
    plain = ctr.contract([(0, 1)], case.ts, arrays, case.output)
    none = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=None)
    matrix = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert np.array_equal(bits(plain.array), bits(none.array)) and none.matrix_launches == 0 and none.compute is None
    assert none.kernel_launches == matrix.kernel_launches and matrix.matrix_launches == 1
    assert matrix.peak_device_bytes == plain.peak_device_bytes


STRIDED_CASE = "matrix_km_kn-1x127x65x33"


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_and_fortran_order_inputs_equal_the_contiguous_copy(ctr, dtype):
    case = mc.BY_NAME[STRIDED_CASE]
    a, b = fill(case, dtype, seed=75)
    plain = ctr.contract([(0, 1)], case.ts, [a, b], case.output, compute=COMPUTE)
    assert_path(ctr, plain, case, case.name)
    view = np.ascontiguousarray(np.moveaxis(a, -1, -2)).swapaxes(-1, -2)  # the same numbers, strides swapped
    fort = np.asfortranarray(b)
    strided = np.repeat(a, 2, axis=-1)[..., ::2]  # every second column of a wider array
    assert not view.flags.c_contiguous and not strided.flags.c_contiguous
    for arrays in ([view, fort], [strided, b]):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
        assert_path(ctr, r, case, case.name)
        assert np.array_equal(bits(r.array), bits(plain.array))


@pytest.mark.parametrize("da,db,dz", [(np.float32, np.complex64, np.complex64),
                                      (np.float64, np.complex64, np.complex128),
                                      (np.float32, np.float64, np.float64)])
def test_mixed_dtypes_compute_in_the_result_type(ctr, da, db, dz):
    case = mc.BY_NAME["matrix_vec_mk_nk-136x72x41"]
    a, _ = fill(case, da, seed=76)
    _, b = fill(case, db, seed=77)
    r = ctr.contract([(0, 1)], case.ts, [a, b], case.output, compute=COMPUTE)
    assert_path(ctr, r, case, case.name)
    assert r.array.dtype == np.dtype(dz)
    same = ctr.contract([(0, 1)], case.ts, [a.astype(dz), b.astype(dz)], case.output, compute=COMPUTE)
    assert np.array_equal(bits(r.array), bits(same.array))
    inds = _result_inds(case.ts, case.output)
    ref, mag = reference(case.ts, [a.astype(dz), b.astype(dz)], inds, dz)
    _assert_within(r.array, ref, bound(mag, case.kt, dz), f"{np.dtype(da).name} x {np.dtype(db).name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_beta_sums_the_assignments_in_the_dtype(ctr, dtype):
    """A sliced index of dimension 2 that is summed: the whole, each half against the einsum of its own assignment, and
    the halves added against the whole (their bounds added: each half rounds on its own)."""
    case = mc.BY_NAME["matrix_beta-summed"]
    run_case(ctr, case, dtype)
    arrays = fill(case, dtype, seed=78)
    inds = _result_inds(case.ts, case.output)
    K = case.ops["K"]
    total, total_bound = 0, 0
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         compute=COMPUTE)
        _assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        assert r.matrix_launches == 1
        part = [np.take(a, [lo], axis=xs.index("s")) for a, xs in zip(arrays, case.ts)]
        ref, mag = reference(case.ts, part, inds, dtype)
        _assert_within(r.array, ref, bound(mag, K, dtype), f"{case.name} [{lo}]")
        total = total + r.array.astype(ref.dtype)
        total_bound = total_bound + bound(mag, K, dtype)
    ref, _ = reference(case.ts, arrays, inds, dtype)
    _assert_within(total, ref, total_bound, f"{case.name}: the halves added")


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_placement_of_a_sliced_index_the_result_holds(ctr, dtype):
    """Each assignment writes its own block once; a half leaves the other block zero, and the halves add up to the
    whole bit for bit."""
    case = mc.BY_NAME["matrix_beta-block"]
    arrays, whole = run_case(ctr, case, dtype, seed=79)
    inds = _result_inds(case.ts, case.output)
    assert inds[0] == "s"
    ref, mag = reference(case.ts, arrays, inds, dtype)
    halves = []
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         compute=COMPUTE)
        _assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        assert r.matrix_launches == 1
        _assert_within(r.array[lo], ref[lo], bound(mag[lo], case.kt, dtype), f"{case.name} block {lo}")
        assert not r.array[1 - lo].any()
        halves.append(r.array)
    assert np.array_equal(bits(halves[0] + halves[1]), bits(whole.array))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["matrix_beta-summed", "matrix_mk_nk-1x127x65x97"])
def test_runs_are_bit_identical(ctr, name, dtype):
    case = mc.BY_NAME[name]
    arrays = fill(case, dtype, seed=80)
    first = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    again = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    assert first.matrix_launches == again.matrix_launches == mc.matrix_launches(case)
    assert np.array_equal(bits(first.array), bits(again.array))


RANGE_CASE = "matrix_mk_kn-1x64x65x33"


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan], ids=["inf", "minus_inf", "nan"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", [0, 1], ids=["A", "B"])
def test_a_part_that_is_not_finite_poisons_the_elements_it_feeds_and_no_others(ctr, side, dtype, value):
    case = mc.BY_NAME[RANGE_CASE]
    arrays = fill(case, dtype, seed=81)
    at = (37, 20) if side == 0 else (20, 41)  # A (i, k) row 37, B (k, j) column 41; k = 20: the second k block
    arrays[side][at] = value + 1j * arrays[side][at].imag if is_cplx(dtype) else value
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert_path(ctr, r, case, "not finite")
    fed = np.zeros(r.array.shape, bool)
    if side == 0:
        fed[37, :] = True
    else:
        fed[:, 41] = True
    got = np.stack([r.array.real, r.array.imag], -1) if is_cplx(dtype) else r.array
    assert not np.isfinite(got[fed]).any()  # (every part: the planted part meets both parts of the other operand)
    arrays[side][at] = 0
    ref, mag = reference(case.ts, arrays, _result_inds(case.ts, case.output), dtype)
    assert np.isfinite(r.array[~fed]).all()
    err = np.abs(r.array.astype(ref.dtype) - ref)
    assert (err[~fed] <= bound(mag, case.kt, dtype)[~fed]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_product_beyond_the_range_of_the_type_gives_an_infinity_of_its_sign(ctr, dtype):
    """Operands finite, every product of A's row 5 with B beyond the largest finite number: +inf where the signs agree,
    -inf where they do not (real); every other row stays finite and inside the bound."""
    case = mc.BY_NAME[RANGE_CASE]
    real = np.finfo(dtype)
    big = 2.0 ** (real.maxexp - 4)
    rng = np.random.RandomState(82)
    arrays = fill(case, dtype, seed=82)
    a, b = arrays
    a[5] = big * (1 + rng.randint(0, 2, a[5].shape))  # all positive, so no inf - inf inside a sum
    b[...] = np.abs(b.real) + (1j * np.abs(b.imag) if is_cplx(dtype) else 0)
    sign = rng.choice([-1.0, 1.0], b.shape[1])
    b *= sign.astype(b.real.dtype) * 2.0 ** 8  # |b| in [2^5, 2^11]: big |b| >= 2^(maxexp + 1)
    if is_cplx(dtype):
        a[5] = a[5].real  # (real times complex: re and im of the row are sums of one sign)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert_path(ctr, r, case, "overflow")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    for got in ([r.array.real[5], r.array.imag[5]] if is_cplx(dtype) else [r.array[5]]):
        assert np.array_equal(got, sign * np.inf)
    others = np.arange(case.ops["M"]) != 5
    ref, mag = reference(case.ts, arrays, _result_inds(case.ts, case.output), dtype)
    assert np.isfinite(r.array[others]).all()
    _assert_within(r.array[others], ref[others], bound(mag, case.kt, dtype)[others], "overflow: the other rows")


def _handle(ctr, L, p):
    import ctypes as C

    from tnco_amd import _lib
    d, keep = ctr._describe(p, 0)
    h = C.c_void_p()
    _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
    del keep
    return h


def test_the_setter_and_the_getter_refuse_with_their_messages_and_leave_the_state(ctr):
    """Through the ABI: 0 and 1 on a handle of a plain dtype without row axes, compute mode 1 or a path kernel; EINVAL
    with the exact tnco_hip_last_error text otherwise, and the handle as it was."""
    import ctypes as C

    from tnco_amd import _lib
    L = _lib.load()
    L.tnco_hip_last_error.restype = C.c_char_p
    err = lambda: L.tnco_hip_last_error().decode()  # noqa: E731
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    mk = lambda **kw: ctr.plan([(0, 1)], ts, shapes, ("a", "b"), **kw)  # noqa: E731

    def refused(call, text):
        assert call() == _lib.EINVAL and err() == text, (err(), text)

    for d in cc.ALL:  # every plain dtype takes it; other values do not
        h = _handle(ctr, L, mk(dtype=d))
        try:
            for on in (1, 0, 1):
                assert L.tnco_hip_contract_set_matrix(h, on) == _lib.OK
            for bad in (2, -1):
                refused(lambda: L.tnco_hip_contract_set_matrix(h, bad), "'on' must be 0 or 1.")
            count = C.c_int64(-1)
            assert L.tnco_hip_contract_matrix_launches(h, C.byref(count)) == _lib.OK and count.value == 0
            refused(lambda: L.tnco_hip_contract_matrix_launches(h, None), "null argument.")
            # matrix mode is on: the other two modes are refused, and it stays on
            if d in (np.float32, np.complex64):
                refused(lambda: L.tnco_hip_contract_set_compute(h, 1), "a compute mode and matrix mode are exclusive.")
                assert L.tnco_hip_contract_set_compute(h, 0) == _lib.OK
            refused(lambda: L.tnco_hip_contract_set_path_kernel(h, 2), "matrix mode is not supported with a path kernel.")
            assert L.tnco_hip_contract_set_matrix(h, 0) == _lib.OK
            assert L.tnco_hip_contract_set_path_kernel(h, 2) == _lib.OK  # (off again: the path kernel is taken ...)
            for on in (0, 1):  # ... and then refuses the mode, whatever the value
                refused(lambda: L.tnco_hip_contract_set_matrix(h, on), "matrix mode is not supported with a path kernel.")
        finally:
            L.tnco_hip_contract_destroy(h)
    refused(lambda: L.tnco_hip_contract_set_matrix(None, 1), "null argument.")
    refused(lambda: L.tnco_hip_contract_matrix_launches(None, C.byref(C.c_int64())), "null argument.")
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float64, sparse_inds=("a", "b"),
                    projs=np.array([[0, 1], [1, 1], [1, 0]]))
    for p, text in ((rows, "row axes are not supported with matrix mode."),
                    (mk(dtype=np.float32, storage="bfloat16"), "matrix mode needs a plain dtype.")):
        h = _handle(ctr, L, p)
        try:
            for on in (0, 1):
                refused(lambda: L.tnco_hip_contract_set_matrix(h, on), text)
        finally:
            L.tnco_hip_contract_destroy(h)
    h = _handle(ctr, L, mk(dtype=np.complex64))
    try:
        assert L.tnco_hip_contract_set_compute(h, 1) == _lib.OK
        for on in (0, 1):
            refused(lambda: L.tnco_hip_contract_set_matrix(h, on), "a compute mode and matrix mode are exclusive.")
        assert L.tnco_hip_contract_set_compute(h, 0) == _lib.OK and L.tnco_hip_contract_set_matrix(h, 1) == _lib.OK
    finally:
        L.tnco_hip_contract_destroy(h)


def test_a_refused_call_leaves_the_run_as_it_was(ctr):
    """State unchanged: a handle that refused set_matrix runs the plain kernel, one that refused the other modes after
    set_matrix runs the matrix kernel."""
    import ctypes as C

    from tnco_amd import _lib
    L = _lib.load()
    case = mc.BY_NAME["matrix-64x64x33"]
    arrays = fill(case, np.float32, seed=83)
    p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, dtype=np.float32)
    want = {0: ctr.contract([(0, 1)], case.ts, arrays, case.output), 1: ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)}
    for on in (0, 1):
        h = _handle(ctr, L, p)
        try:
            if on:
                assert L.tnco_hip_contract_set_matrix(h, 1) == _lib.OK
                assert L.tnco_hip_contract_set_compute(h, 1) == _lib.EINVAL
                assert L.tnco_hip_contract_set_path_kernel(h, 1) == _lib.EINVAL
            else:
                assert L.tnco_hip_contract_set_matrix(h, 2) == _lib.EINVAL
            out = np.empty(p.out_numel, p.dtype)
            ptrs = (C.c_void_p * 2)(*[a.ctypes.data for a in arrays])
            _lib.check(L.tnco_hip_contract_run(h, ptrs, out.ctypes.data_as(C.c_void_p)))
            count = C.c_int64(-1)
            assert L.tnco_hip_contract_matrix_launches(h, C.byref(count)) == _lib.OK and count.value == on
            assert np.array_equal(bits(out), bits(want[on].array))
        finally:
            L.tnco_hip_contract_destroy(h)
