"""The split kernel (csrc/contract_split.h, `contract(..., compute="bf16x3")`) at its edges, element by element.

Every case of tests/split_cases.py is a one-step network.  A test asserts which kernel ran, from
`ContractionResult.kernel_launches` and from `split_launches`, and compares every element with numpy's einsum of the
float32 inputs in float64 / complex128.  Inputs are full-precision float32 with magnitudes 2^uniform(-3, 3) and random
signs (times a power of two where a test says so), inside [2^-100, 2^100], so that every lo of the split is a normal
bfloat16.

bfloat16 has unit roundoff 2^-8: |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-16 |x|, so a product without its lo lo
term is off by at most 3.02 2^-16 |a| |b|.  With kt products per element (complex: c = 2, four real products per term),
each of them three MFMA products summed in float32:

    |got - ref| <= [2^-14 + (2 c 3 kt + 2) 2^-24] (|A| @ |B|)

The second term is the accumulation bound of tests/test_gpu_contract_half.py for three times as many products; 2^-14
leaves a factor 1.3 over the worst case of the first.  A kernel that drops a cross term is off by 2^-8 |a| |b| per
product, which this bound does not hide, and the exactness tests below catch it bit for bit.  tools/split_profile.py
writes the largest err / (2^-16 |A| @ |B|) per type into profiles/contract_split.txt.  An element that is not a number
fails.
"""
import numpy as np
import pytest

from tests import split_cases as sc
from tests.test_gpu_contract_half import assert_kernels, assert_within, reference, result_inds

pytestmark = pytest.mark.gpu

COMPUTE = "bf16x3"
TYPES = [pytest.param(False, id="real"), pytest.param(True, id="complex")]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def draw(shape, cplx, rng, scale=1.0):
    """float32 / complex64 values with all 24 bits in play, every part's magnitude in scale [2^-3, 2^3]."""
    part = lambda: (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-3, 3, shape) * scale).astype(np.float32)  # noqa: E731
    return (part() + 1j * part()).astype(np.complex64) if cplx else part()


def fill(case, cplx, seed, scales=(1.0, 1.0)):
    rng = np.random.RandomState(seed)
    return [draw(shape, cplx, rng, s) for shape, s in zip(case.shapes(), scales)]


def bound(mag, kt, cplx):
    return (2.0 ** -14 + (2 * (2 if cplx else 1) * 3 * kt + 2) * 2.0 ** -24) * mag


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def assert_path(ctr, r, case, what):
    """The path from kernel_launches and from split_launches."""
    assert_kernels(ctr, r, case.kernels, what)
    assert r.split_launches == sc.split_launches(case), what
    assert r.compute == COMPUTE


def run_case(ctr, case, cplx, seed=41, scales=(1.0, 1.0)):
    """Runs one case, asserts path, type and every element; returns max err / (2^-16 |A| @ |B|)."""
    arrays = fill(case, cplx, seed, scales)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    what = f"{case.name} {'complex' if cplx else 'real'}"
    inds = result_inds(case.ts, case.output)
    assert r.inds == inds and r.n_slices == case.n_slices(), what
    assert_path(ctr, r, case, what)
    op = case.ops
    assert r.macs == case.n_slices() * op["H"] * op["M"] * op["N"] * op["K"]
    assert r.array.dtype == (np.complex64 if cplx else np.float32), what
    ref, mag = reference(case.ts, arrays, inds)
    assert_within(r.array, ref, bound(mag, case.kt, cplx), f"{what}: kt {case.kt}")
    return float((np.abs(r.array.astype(ref.dtype) - ref) / (2.0 ** -16 * mag)).max())


_ONE_PASS = [c for c in sc.SPLIT if "beta" not in c.name]


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("case", _ONE_PASS, ids=[c.name for c in _ONE_PASS])
def test_kernel_path_and_every_element(ctr, case, cplx):
    run_case(ctr, case, cplx)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("case", sc.PLAIN, ids=[c.name for c in sc.PLAIN])
def test_below_the_thresholds_the_float32_kernels_run_and_give_the_bytes_of_the_plain_mode(ctr, case, cplx):
    arrays = fill(case, cplx, seed=42)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    plain = ctr.contract([(0, 1)], case.ts, arrays, case.output)
    assert_path(ctr, r, case, case.name)
    assert r.split_launches == 0 and plain.split_launches == 0 and plain.compute is None
    assert r.kernel_launches == plain.kernel_launches
    assert np.array_equal(bits(r.array), bits(plain.array))


@pytest.mark.parametrize("cplx", TYPES)
def test_the_plain_mode_of_a_tiled_step_is_untouched_by_the_keyword_at_none(ctr, cplx):
    case = sc.BY_NAME["split-64x64x33"]
    arrays = fill(case, cplx, seed=43)
    plain = ctr.contract([(0, 1)], case.ts, arrays, case.output)
    none = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=None)
    split = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert np.array_equal(bits(plain.array), bits(none.array)) and none.split_launches == 0 and none.compute is None
    assert none.kernel_launches == split.kernel_launches and split.split_launches == 1
    assert split.peak_device_bytes == plain.peak_device_bytes


@pytest.mark.parametrize("cplx", TYPES)
def test_beta_sums_the_assignments_in_float32(ctr, cplx):
    """A sliced index of dimension 2 that is summed: the whole, each half against the einsum of its own assignment, and
    the halves added against the whole (their bounds added: each half rounds on its own)."""
    case = sc.BY_NAME["split_beta-summed"]
    run_case(ctr, case, cplx)
    arrays = fill(case, cplx, seed=44)
    inds = result_inds(case.ts, case.output)
    K = case.ops["K"]
    total, total_bound = 0, 0
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         compute=COMPUTE)
        assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        assert r.split_launches == 1
        part = [np.take(a, [lo], axis=xs.index("s")) for a, xs in zip(arrays, case.ts)]
        ref, mag = reference(case.ts, part, inds)
        assert_within(r.array, ref, bound(mag, K, cplx), f"{case.name} [{lo}]")
        total = total + r.array.astype(ref.dtype)
        total_bound = total_bound + bound(mag, K, cplx)
    ref, _ = reference(case.ts, arrays, inds)
    assert_within(total, ref, total_bound, f"{case.name}: the halves added")


@pytest.mark.parametrize("cplx", TYPES)
def test_block_placement_of_a_sliced_index_the_result_holds(ctr, cplx):
    """Each assignment writes its own block once; a half leaves the other block zero, and the halves add up to the
    whole bit for bit."""
    case = sc.BY_NAME["split_beta-block"]
    run_case(ctr, case, cplx, seed=45)
    arrays = fill(case, cplx, seed=45)
    whole = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    inds = result_inds(case.ts, case.output)
    assert inds[0] == "s"
    ref, mag = reference(case.ts, arrays, inds)
    halves = []
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         compute=COMPUTE)
        assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        assert r.split_launches == 1
        assert_within(r.array[lo], ref[lo], bound(mag[lo], case.kt, cplx), f"{case.name} block {lo}")
        assert not r.array[1 - lo].any()
        halves.append(r.array)
    assert np.array_equal(halves[0] + halves[1], whole.array)


def planted(shape, cplx, rng, fine):
    """fine: 1 + s 2^-10, s in [0, 1024): 11 significant bits, so hi + lo is the value and lo is not zero for most;
    else: integers in [-4, 4], which hi holds (lo = 0)."""
    part = lambda: (1 + rng.randint(0, 1024, shape) * 2.0 ** -10 if fine else rng.randint(-4, 5, shape)).astype(np.float32)  # noqa: E731
    return (part() + 1j * part()).astype(np.complex64) if cplx else part()


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("fine_side", [0, 1], ids=["A_fine", "B_fine"])
@pytest.mark.parametrize("name", ["split_mk_kn-3x129x64x64", "split_km_nk-1x127x127x64"])
def test_with_both_cross_terms_an_exact_sum_comes_out_exact(ctr, name, fine_side, cplx):
    """One operand 1 + s 2^-10, the other small integers, K = 64: every product of a hi or a lo with an integer, and
    every partial sum (below 2^11, a multiple of 2^-10), is a float32, so whatever the order the result must EQUAL the
    float64 einsum.  Without a_lo b_hi (A fine) or a_hi b_lo (B fine) it does not."""
    case = sc.BY_NAME[name]
    assert case.ops["K"] == 64
    rng = np.random.RandomState(46 + fine_side)
    arrays = [planted(shape, cplx, rng, side == fine_side) for side, shape in enumerate(case.shapes())]
    hi, lo = ctr.split_bf16(arrays[fine_side])
    assert np.array_equal(hi + lo, arrays[fine_side]) and (lo != 0).mean() > 0.5
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert_path(ctr, r, case, name)
    ref, _ = reference(case.ts, arrays, result_inds(case.ts, case.output))
    assert np.array_equal(r.array.astype(ref.dtype), ref)
    # (the test can tell: the same sum from hi alone is not the reference)
    part = list(arrays)
    part[fine_side] = hi
    assert not np.array_equal(reference(case.ts, part, result_inds(case.ts, case.output))[0], ref)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("name", ["split_mk_nk-1x127x65x97", "split_km_kn-1x64x129x63"])
def test_leaf_factors_far_from_one_stay_under_the_bound(ctr, name, cplx):
    """A times 2^40 and B times 2^-70: the split is relative, the bound scales with |A| @ |B|."""
    run_case(ctr, sc.BY_NAME[name], cplx, seed=47, scales=(2.0 ** 40, 2.0 ** -70))
    run_case(ctr, sc.BY_NAME[name], cplx, seed=48, scales=(2.0 ** -70, 2.0 ** 40))


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("side", [0, 1], ids=["A", "B"])
def test_an_inf_part_poisons_the_elements_it_feeds_and_no_others(ctr, side, cplx):
    case = sc.BY_NAME["split_mk_kn-1x127x129x63"]
    arrays = fill(case, cplx, seed=49)
    at = (37, 40) if side == 0 else (40, 101)  # A (i, k) row 37, B (k, j) column 101; k = 40: the second k block
    arrays[side][at] = np.inf
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute=COMPUTE)
    assert_path(ctr, r, case, "inf")
    fed = np.zeros(r.array.shape, bool)
    if side == 0:
        fed[37, :] = True
    else:
        fed[:, 101] = True
    assert not np.isfinite(r.array[fed]).any()
    arrays[side][at] = 0
    ref, mag = reference(case.ts, arrays, result_inds(case.ts, case.output))
    err = np.abs(r.array.astype(ref.dtype) - ref)
    assert (err[~fed] <= bound(mag, case.kt, cplx)[~fed]).all()


@pytest.mark.parametrize("cplx", TYPES)
def test_runs_are_bit_identical(ctr, cplx):
    case = sc.BY_NAME["split_beta-summed"]
    arrays = fill(case, cplx, seed=50)
    first = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    again = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, compute=COMPUTE)
    assert np.array_equal(bits(first.array), bits(again.array))


def test_the_setter_refuses_other_modes_other_dtypes_and_row_axes(ctr):
    """Through the ABI: modes 0 and 1 on a float32 or complex64 handle without row axes, EINVAL otherwise."""
    import ctypes as C

    from tnco_amd import _lib
    L = _lib.load()
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"),
                    projs=np.array([[0, 1], [1, 1], [1, 0]]))
    ok = {0: _lib.OK, 1: _lib.OK, 2: _lib.EINVAL, -1: _lib.EINVAL}
    no = {0: _lib.EINVAL, 1: _lib.EINVAL, 2: _lib.EINVAL}
    plans = [(rows, no)]
    plans += [(ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=d), ok) for d in (np.float32, np.complex64)]
    plans += [(ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=d), no) for d in (np.float64, np.complex128)]
    plans += [(ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, storage="bfloat16"), no)]
    for p, codes in plans:
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        try:
            for mode, code in codes.items():
                assert L.tnco_hip_contract_set_compute(h, mode) == code, (p.dtype, p.storage, mode)
            count = C.c_int64(-1)
            assert L.tnco_hip_contract_split_launches(h, C.byref(count)) == _lib.OK and count.value == 0
            assert L.tnco_hip_contract_split_launches(h, None) == _lib.EINVAL
        finally:
            L.tnco_hip_contract_destroy(h)
        del keep
    assert L.tnco_hip_contract_set_compute(None, 1) == _lib.EINVAL
