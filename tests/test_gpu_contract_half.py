"""The storage-mode kernels (csrc/contract_half.h, `contract(..., storage=...)`) at their edges, element by element.

Every case of tests/half_cases.py is a one-step network.  A test asserts which kernel path ran through
`ContractionResult.kernel_launches` -- under `storage` the four tiled slots count the MFMA kernel -- and compares every
element with numpy's einsum in float64 / complex128.  Inputs are drawn in float32 with magnitudes 2^uniform(-3, 3) and
random signs, then rounded with the engine's own host function (`contraction.round_to_storage`), so device and reference
start from identical values and every product and sum is normal in float16 and in bfloat16.

A step written to the output accumulates in float32 and is not rounded to storage.  The products of two 16-bit values
are exact in float32; with kt products per element (complex: c = 2, four real products per term)

    |got - ref| <= (2 c kt + 2) 2^-24 (|A| @ |B|)

The factor 2 on contract_cases' bound covers any summation order under faithful rather than nearest rounding of each
add: how the MFMA rounds its internal adds has not been measured.  tools/half_profile.py writes the largest
err / (2^-24 kt |A| @ |B|) per type into profiles/contract_half.txt.  An element that is not a number fails.
"""
import numpy as np
import pytest

from tests import half_cases as hc

pytestmark = pytest.mark.gpu

U_STORAGE = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
COMBOS = [pytest.param(s, c, id=f"{s}-{'complex' if c else 'real'}") for s in hc.STORAGES for c in (False, True)]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def draw(ctr, shape, cplx, storage, rng):
    """float32 / complex64 values that `storage` holds exactly, every part's magnitude in [2^-3, 2^3]."""
    part = lambda: (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)  # noqa: E731
    a = (part() + 1j * part()).astype(np.complex64) if cplx else part()
    a = ctr.round_to_storage(a, storage)
    assert np.array_equal(ctr.round_to_storage(a, storage), a)
    return a


def fill(ctr, case, cplx, storage, seed):
    rng = np.random.RandomState(seed)
    return [draw(ctr, shape, cplx, storage, rng) for shape in case.shapes()]


def result_inds(ts, output):
    a, b = ts
    shared = set(a) & set(b)
    keep = shared & set(output) if output is not None else set()
    return tuple(x for x in a if x in keep) + tuple(x for x in a if x not in shared) + \
        tuple(x for x in b if x not in shared)


def reference(ts, arrays, inds):
    """(einsum of the inputs, the same einsum of their moduli), both in double precision."""
    sym = {x: k for k, x in enumerate(dict.fromkeys(tuple(ts[0]) + tuple(ts[1])))}
    subs = [[sym[x] for x in xs] for xs in ts]
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    res = [sym[x] for x in inds]
    ref = np.einsum(wide[0], subs[0], wide[1], subs[1], res, optimize=True)
    mag = np.einsum(np.abs(wide[0]), subs[0], np.abs(wide[1]), subs[1], res, optimize=True)
    return ref, mag


def bound(mag, kt, cplx):
    return (2 * (2 if cplx else 1) * kt + 2) * 2.0 ** -24 * mag


def assert_within(got, ref, bnd, what):
    """|got - ref| <= bnd in every element (not a number: fails); returns the largest error / bound."""
    assert got.shape == ref.shape == bnd.shape, what
    err = np.abs(got.astype(ref.dtype) - ref)
    bad = ~(err <= bnd)
    ratio = np.divide(err, bnd, out=np.zeros_like(bnd), where=bnd > 0)
    ratio[bad & ~(ratio > 1)] = np.inf
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: largest error / bound {worst:.4f}")
    if bad.any():
        at = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound, "
                             f"{int(np.isnan(err).sum())} of them not a number; worst at {at}: got {got[at]}, "
                             f"reference {ref[at]}, error / bound {float(ratio[at]):.3g}")
    return worst


def assert_kernels(ctr, r, kernels, what):
    want = tuple(kernels.get(name, 0) for name in ctr.KERNEL_PATHS)
    assert set(kernels) <= set(ctr.KERNEL_PATHS)
    assert r.kernel_launches == want, f"{what}: launches {dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))}"
    assert sum(r.kernel_launches) == r.launches and r.row_kernel_launches == (0, 0, 0)


def run_case(ctr, case, storage, cplx, seed=21):
    """Runs one case, asserts path, type and every element; returns max err / (2^-24 kt |A| @ |B|)."""
    arrays = fill(ctr, case, cplx, storage, seed)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, storage=storage)
    what = f"{case.name} {storage} {'complex' if cplx else 'real'}"
    inds = result_inds(case.ts, case.output)
    assert r.inds == inds and r.n_slices == case.n_slices(), what
    assert_kernels(ctr, r, case.kernels, what)
    op = case.ops
    assert r.macs == case.n_slices() * op["H"] * op["M"] * op["N"] * op["K"]
    assert r.array.dtype == (np.complex64 if cplx else np.float32), what
    ref, mag = reference(case.ts, arrays, inds)
    assert_within(r.array, ref, bound(mag, case.kt, cplx), f"{what}: kt {case.kt}")
    return float((np.abs(r.array.astype(ref.dtype) - ref) / (2.0 ** -24 * case.kt * mag)).max())


_ONE_PASS = [c for c in hc.CASES if "beta" not in c.name]


@pytest.mark.parametrize("storage,cplx", COMBOS)
@pytest.mark.parametrize("case", _ONE_PASS, ids=[c.name for c in _ONE_PASS])
def test_kernel_path_and_every_element(ctr, case, storage, cplx):
    run_case(ctr, case, storage, cplx)


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_beta_sums_the_assignments_in_float32(ctr, storage, cplx):
    """A sliced index of dimension 2 that is summed: the whole, each half against the einsum of its own assignment, and
    the halves added against the whole (their bounds added: each half rounds on its own)."""
    case = hc.BY_NAME["mfma_beta-summed"]
    run_case(ctr, case, storage, cplx)
    arrays = fill(ctr, case, cplx, storage, seed=22)
    inds = result_inds(case.ts, case.output)
    K = case.ops["K"]
    total, total_bound = 0, 0
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         storage=storage)
        assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        part = [np.take(a, [lo], axis=xs.index("s")) for a, xs in zip(arrays, case.ts)]
        ref, mag = reference(case.ts, part, inds)
        assert_within(r.array, ref, bound(mag, K, cplx), f"{case.name} {storage} [{lo}]")
        total = total + r.array.astype(ref.dtype)
        total_bound = total_bound + bound(mag, K, cplx)
    ref, _ = reference(case.ts, arrays, inds)
    assert_within(total, ref, total_bound, f"{case.name} {storage}: the halves added")


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_block_placement_of_a_sliced_index_the_result_holds(ctr, storage, cplx):
    """Each assignment writes its own block once; a half leaves the other block zero, and the halves add up to the
    whole bit for bit."""
    case = hc.BY_NAME["mfma_beta-block"]
    run_case(ctr, case, storage, cplx, seed=23)
    arrays = fill(ctr, case, cplx, storage, seed=23)
    whole = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, storage=storage)
    inds = result_inds(case.ts, case.output)
    assert inds[0] == "s"
    ref, mag = reference(case.ts, arrays, inds)
    halves = []
    for lo in (0, 1):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, lo + 1),
                         storage=storage)
        assert_kernels(ctr, r, {"tiled_mk_kn": 1}, f"{case.name} [{lo}]")
        assert_within(r.array[lo], ref[lo], bound(mag[lo], case.kt, cplx), f"{case.name} {storage} block {lo}")
        assert not r.array[1 - lo].any()
        halves.append(r.array)
    assert np.array_equal(halves[0] + halves[1], whole.array)


def two_step(ctr, storage, cplx, seed=24):
    """A (i, k) B (k, j) -> Z (i, j) on the MFMA kernel into the arena, rounded to storage there; then Z w over j, a
    stream-class product with a vector, into the output.  Returns (result, reference, bound)."""
    rng = np.random.RandomState(seed)
    I, K, J = 65, 48, 70
    A, B, w = (draw(ctr, s, cplx, storage, rng) for s in ((I, K), (K, J), (J,)))
    r = ctr.contract([(0, 1), (0, 1)], [("i", "k"), ("k", "j"), ("j",)], [A, B, w], storage=storage)
    assert r.inds == ("i",)
    assert_kernels(ctr, r, {"tiled_mk_kn": 1, "stream": 1}, f"two steps {storage}")
    wide = np.complex128 if cplx else np.float64
    A64, B64, w64 = (x.astype(wide) for x in (A, B, w))
    z = A64 @ B64
    z_stored = ctr.round_to_storage(z.astype(np.complex64 if cplx else np.float32), storage).astype(wide)
    ref = z_stored @ w64
    b1 = bound(np.abs(A64) @ np.abs(B64), K, cplx)  # of step 1, before its result is rounded
    zw = np.abs(z) @ np.abs(w64)
    # step 2's own bound, step 1's carried through step 2, and device and reference rounding a value near a boundary
    # to neighbouring storage values
    bnd = bound(np.abs(z_stored) @ np.abs(w64), J, cplx) + b1 @ np.abs(w64) + 2 * U_STORAGE[storage] * zw
    return r, ref, bnd


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_an_intermediate_is_rounded_once_to_storage(ctr, storage, cplx):
    r, ref, bnd = two_step(ctr, storage, cplx)
    assert r.array.dtype == (np.complex64 if cplx else np.float32)
    assert_within(r.array, ref, bnd, f"two steps {storage}")


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_a_single_sliced_leaf_is_widened_into_the_output(ctr, storage, cplx):
    rng = np.random.RandomState(25)
    a = draw(ctr, (5, 3, 7), cplx, storage, rng)
    r = ctr.contract([], [("i", "s", "j")], [a], slices=("s",), storage=storage)
    assert_kernels(ctr, r, {"gather": 3}, "single leaf")
    assert r.array.dtype == a.dtype and r.inds == ("i", "s", "j")
    assert np.array_equal(r.array, a)
    # ... and a leaf that is not in storage yet is rounded by the host function
    raw = (a * np.float32(1.001)).astype(a.dtype)
    r = ctr.contract([], [("i", "s", "j")], [raw], slices=("s",), storage=storage)
    assert np.array_equal(r.array, ctr.round_to_storage(raw, storage))


@pytest.mark.parametrize("storage,cplx", COMBOS)
@pytest.mark.parametrize("name", ["mfma_km_kn-3x65x64x64", "stream-63x64x33"])
def test_views_and_fortran_order_equal_the_contiguous_copy(ctr, name, storage, cplx):
    case = hc.BY_NAME[name]
    a, b = fill(ctr, case, cplx, storage, seed=26)
    view = np.ascontiguousarray(np.moveaxis(a, -1, 0)).transpose(*range(1, a.ndim), 0)  # strides rotated
    fort = np.asfortranarray(b)
    assert not view.flags.c_contiguous and not fort.flags.c_contiguous
    plain = ctr.contract([(0, 1)], case.ts, [a, b], case.output, storage=storage)
    r = ctr.contract([(0, 1)], case.ts, [view, fort], case.output, storage=storage)
    assert_kernels(ctr, r, case.kernels, f"{name} views")
    assert np.array_equal(r.array, plain.array)
    strided = np.repeat(a, 2, axis=-1)[..., ::2]  # every second column of a wider array
    assert not strided.flags.c_contiguous and np.array_equal(strided, a)
    assert np.array_equal(ctr.contract([(0, 1)], case.ts, [strided, b], case.output, storage=storage).array, plain.array)


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_a_real_and_a_complex_input_compute_in_complex64(ctr, storage):
    case = hc.BY_NAME["mfma_mk_nk-3x65x64x65"]
    a, _ = fill(ctr, case, False, storage, seed=27)
    _, b = fill(ctr, case, True, storage, seed=28)
    r = ctr.contract([(0, 1)], case.ts, [a, b], case.output, storage=storage)
    assert_kernels(ctr, r, case.kernels, "mixed")
    assert r.array.dtype == np.complex64
    inds = result_inds(case.ts, case.output)
    ref, mag = reference(case.ts, [a, b], inds)
    assert_within(r.array, ref, bound(mag, case.kt, True), f"float32 x complex64 {storage}")
    same = ctr.contract([(0, 1)], case.ts, [a.astype(np.complex64), b], case.output, storage=storage)
    assert np.array_equal(r.array, same.array)


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_runs_are_bit_identical(ctr, storage, cplx):
    case = hc.BY_NAME["mfma_beta-summed"]
    arrays = fill(ctr, case, cplx, storage, seed=29)
    first = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, storage=storage)
    again = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, storage=storage)
    assert np.array_equal(first.array, again.array)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_a_result_that_re_enters_as_a_leaf_saturates_like_an_intermediate(ctr, cplx):
    """contract_results hands the result of one component to the call that joins the components: marked as an
    intermediate, a value beyond float16 becomes inf on the way in and poisons its own row only."""
    case = hc.BY_NAME["mfma_mk_kn-3x65x127x48"]
    a, b = fill(ctr, case, cplx, "float16", seed=30)
    a[1, 2, 5] = 1e5
    with pytest.raises(ValueError, match="finite values beyond the range of float16"):
        ctr.contract([(0, 1)], case.ts, [a, b], case.output, storage="float16")
    r = ctr.contract([(0, 1)], case.ts, [a, b], case.output, storage="float16", _intermediates=[0])
    assert_kernels(ctr, r, case.kernels, "saturating leaf")
    assert not np.isfinite(r.array[1, 2]).any()
    keep = np.ones(r.array.shape, bool)
    keep[1, 2] = False
    a[1, 2, 5] = 0
    ref, mag = reference(case.ts, [a, b], result_inds(case.ts, case.output))
    err = np.abs(r.array.astype(ref.dtype) - ref)
    assert (err[keep] <= bound(mag, case.kt, cplx)[keep]).all()
