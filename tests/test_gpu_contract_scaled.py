"""Per-tensor scaling of the storage mode (`contract(..., storage=..., scaling="tensor")`, csrc/contract_half.h) on the
device, element by element.

Values are drawn as in tests/test_gpu_contract_half.py -- every part's magnitude 2^uniform(-3, 3), random signs -- times
a factor per tensor far outside float16's range.  The reference of a step is numpy's einsum in float64 / complex128 of
the values `contraction.scale_to_storage` gives for the leaves, so device and reference start from the same numbers, and
power-of-two scaling being exact, the bounds are those of that file, taken from it:

    a step to the output:   |got - ref| <= (2 c kt + 2) 2^-24 (|A| @ |B|)
    a stored intermediate:  the bound of its own step carried through the next one, plus one storage unit of the
                            intermediate where device and reference round to neighbouring values.  The unit is taken at
                            the scaled magnitude: 2 u |z| for a value that is normal after scaling, and the spacing of
                            the storage type's subnormals times 2^e below that (nothing in these tests is that small
                            except where a test says so).

The exponents the device reports (`ContractionResult.exponents`) are held to the host rule.
"""
import numpy as np
import pytest

from tests import scaled_cases as sc
from tests.test_gpu_contract_half import COMBOS, U_STORAGE, assert_within, bound, reference, result_inds

pytestmark = pytest.mark.gpu

SUBNORMAL_STEP = {"float16": 2.0 ** -24, "bfloat16": 2.0 ** -133}  # spacing of the storage type's subnormals


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def draw(shape, cplx, rng, factor=1.0):
    part = lambda: (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)  # noqa: E731
    a = (part() + 1j * part()).astype(np.complex64) if cplx else part()
    return (a * np.float32(factor)).astype(a.dtype)


def wide(a):
    return np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64)


def rule(x) -> int:
    """The scaling rule on float64 values: floor(log2 of the largest finite |part|) - 14, 0 for none."""
    x = np.asarray(x)
    parts = np.concatenate([np.ravel(x.real), np.ravel(x.imag)]) if np.iscomplexobj(x) else np.ravel(x)
    parts = np.abs(parts[np.isfinite(parts)])
    m = float(parts.max()) if parts.size else 0.0
    return 0 if m == 0 else int(np.frexp(m)[1]) - 1 - 14


def kernels_of(ctr, r):
    return {n: v for n, v in zip(ctr.KERNEL_PATHS, r.kernel_launches) if v}


def check_counts(ctr, r, kernels, narrow, what):
    assert kernels_of(ctr, r) == kernels, what
    assert r.narrow_launches == narrow and r.launches == sum(r.kernel_launches) + narrow, what
    assert r.row_kernel_launches == (0, 0, 0) and r.scaling == "tensor"


@pytest.mark.parametrize("storage,cplx", COMBOS)
@pytest.mark.parametrize("case", sc.ONE_STEP, ids=[c.name for c in sc.ONE_STEP])
def test_one_step_to_the_output_in_each_shape_class(ctr, case, storage, cplx):
    rng = np.random.RandomState(41)
    arrays = [draw(shape, cplx, rng, f) for shape, f in zip(case.shapes(), sc.FACTORS)]
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, storage=storage, scaling="tensor")
    what = f"{case.name} {storage} {'complex' if cplx else 'real'}"
    check_counts(ctr, r, case.kernels, 0, what)
    inds = result_inds(case.ts, case.output)
    assert r.inds == inds and r.array.dtype == arrays[0].dtype
    held, exps = zip(*(ctr.scale_to_storage(a, storage) for a in arrays))
    assert r.exponents == exps + (0,), what
    assert exps == (rule(arrays[0]), rule(arrays[1]))
    ref, mag = reference(case.ts, held, inds)
    assert_within(r.array, ref, bound(mag, case.kt, cplx), f"{what}: kt {case.kt}")


def two_step_expected_held(ctr, As, Bs, ws, storage, cplx):
    """A (i, k) B (k, j) -> Z (i, j), stored; Z w over j, for operands as the engine holds them (true scale).
    (reference, bound, exponent of Z, Z before it is rounded)."""
    A64, B64, w64 = wide(As), wide(Bs), wide(ws)
    K, J = As.shape[1], Bs.shape[1]
    z = A64 @ B64
    e = rule(z)
    scaled = np.ldexp(z.real, -e) + (1j * np.ldexp(z.imag, -e) if cplx else 0)
    stored = ctr.round_to_storage(scaled.astype(np.complex64 if cplx else np.float32), storage)
    z_stored = wide(stored) * 2.0 ** e
    ref = z_stored @ w64
    b1 = bound(np.abs(A64) @ np.abs(B64), K, cplx)  # of step 1, before its result is rounded
    unit = np.maximum(2 * U_STORAGE[storage] * np.abs(z), SUBNORMAL_STEP[storage] * 2.0 ** e)
    bnd = bound(np.abs(z_stored) @ np.abs(w64), J, cplx) + b1 @ np.abs(w64) + unit @ np.abs(w64)
    return ref, bnd, e, z


def two_step_expected(ctr, A, B, w, storage, cplx):
    """... from the leaves as given: each enters as `scale_to_storage` holds it."""
    return two_step_expected_held(ctr, *(ctr.scale_to_storage(x, storage)[0] for x in (A, B, w)), storage, cplx)


def two_step_arrays(klass, cplx, seed, factors, plant=True):
    """Leaves of the two-step network with a first step of class `klass`.  plant: Z[0, 0] is made the sum of the moduli
    of its terms (every term positive real), with row 0 of A and column 0 of B raised fourfold: it then stands clear of
    the other, randomly signed, sums also where K is as small as 33."""
    I, K, J = sc.FIRST_STEPS[klass]
    rng = np.random.RandomState(seed)
    A, B, w = (draw(s, cplx, rng, f) for s, f in zip(((I, K), (K, J), (J,)), factors))
    if plant:
        phase = np.conj(B[:, 0]) / np.abs(B[:, 0])
        A[0, :] = (4 * np.abs(A[0, :]) * phase).astype(A.dtype)
        B[:, 0] *= np.float32(4)
    return A, B, w


TWO_STEP_TS = [("i", "k"), ("k", "j"), ("j",)]


def run_two_steps(ctr, arrays, storage, **kw):
    return ctr.contract([(0, 1), (0, 1)], TWO_STEP_TS, arrays, storage=storage, **kw)


@pytest.mark.parametrize("storage,cplx", COMBOS)
@pytest.mark.parametrize("klass", list(sc.FIRST_STEPS))
def test_a_stored_intermediate_gets_the_exponent_of_its_largest_part(ctr, klass, storage, cplx):
    A, B, w = two_step_arrays(klass, cplx, 42, (2.0 ** 40, 2.0 ** -70, 2.0 ** 25))
    # the planted maximum is put at least 2^-3 (relative) away from a power of two, so that float32 sums and the
    # float64 reference cannot disagree about its binade
    for c in (1.0, 1.25, 1.5, 0.75, 0.625):
        trial = A.copy()
        trial[0, :] *= np.float32(c)
        z = wide(ctr.scale_to_storage(trial, storage)[0]) @ wide(ctr.scale_to_storage(B, storage)[0])
        parts = np.abs(np.concatenate([np.ravel(z.real), np.ravel(z.imag)]))
        frac = 2 * np.frexp(parts.max())[0]  # in [1, 2)
        if 1.125 <= frac <= 1.875 and parts.max() == abs(z[0, 0].real) and np.sort(parts)[-2] < 0.5 * parts.max():
            A = trial
            break
    else:
        raise AssertionError("no multiplier puts the planted maximum inside its binade")
    r = run_two_steps(ctr, [A, B, w], storage, scaling="tensor")
    what = f"two steps, first {klass}, {storage} {'complex' if cplx else 'real'}"
    first = dict(stream=2) if klass == "stream" else {klass: 1, "stream": 1}
    check_counts(ctr, r, first, 1, what)
    ref, bnd, e, _ = two_step_expected(ctr, A, B, w, storage, cplx)
    assert r.exponents == tuple(ctr.scale_to_storage(x, storage)[1] for x in (A, B, w)) + (e, 0), what
    assert r.inds == ("i",) and r.array.dtype == A.dtype
    assert_within(r.array, ref, bnd, what)


SLICED_TS = [("s", "i", "k"), ("t", "k", "j"), ("t", "j", "l")]


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_two_sliced_indices_one_placed_one_summed(ctr, storage, cplx):
    """A (s, i, k) B (t, k, j) -> Z (i, j) stored, Z w (t, j, l) -> (s, i, l): s selects a block of the output, t is
    summed with beta = 1.  Every leaf is near 2^-30 at slice value 0 and near 2^10 at slice value 1 of the sliced index
    it holds, so Z's exponent differs from assignment to assignment.  A leaf has one exponent, set by its slice value 1:
    what it holds at slice value 0 is 2^-40 of that, below the storage types' resolution there, and enters the reference
    as `scale_to_storage` gives it."""
    rng = np.random.RandomState(43)
    I, K, J, Lx = 65, 40, 64, 3
    level = np.array([2.0 ** -30, 2.0 ** 10], np.float32)
    A = draw((2, I, K), cplx, rng) * level[:, None, None]
    B = draw((2, K, J), cplx, rng) * level[:, None, None]
    w = draw((2, J, Lx), cplx, rng) * level[:, None, None]
    arrays = [x.astype(np.complex64 if cplx else np.float32) for x in (A, B, w)]
    kw = dict(slices=("s", "t"), storage=storage, scaling="tensor")
    r = ctr.contract([(0, 1), (0, 1)], SLICED_TS, arrays, ("s", "i", "l"), **kw)
    what = f"two sliced indices {storage} {'complex' if cplx else 'real'}"
    order = ("s", "i", "l")
    assert sorted(r.inds) == sorted(order) and r.n_slices == 4 and r.narrow_launches == 4, what
    as_ref = lambda q: q.array.transpose([q.inds.index(x) for x in order])  # noqa: E731
    held, exps = zip(*(ctr.scale_to_storage(x, storage) for x in arrays))
    ref = np.zeros((2, I, Lx), np.complex128 if cplx else np.float64)
    bnd = np.zeros((2, I, Lx))
    e_last = None
    for s in (0, 1):
        for t in (0, 1):
            # (the leaves are scaled whole: the parts are taken from the held values, whose own rule gives them back)
            part_ref, part_bnd, e_last, _ = two_step_expected_held(ctr, held[0][s], held[1][t], held[2][t], storage, cplx)
            ref[s] += part_ref
            bnd[s] += part_bnd
    assert r.exponents[:3] == exps and r.exponents[4] == 0
    # of the last assignment, s = t = 1 (no planted maximum here: float32 sums may see it in the neighbouring binade)
    assert abs(r.exponents[3] - e_last) <= 1
    assert_within(as_ref(r), ref, bnd, what)
    halves = [ctr.contract([(0, 1), (0, 1)], SLICED_TS, arrays, ("s", "i", "l"), slice_range=q, **kw) for q in ((0, 2), (2, 4))]
    assert not as_ref(halves[0])[1].any() and not as_ref(halves[1])[0].any()
    assert_within(as_ref(halves[0]) + as_ref(halves[1]), ref, bnd, what + ": the halves added")


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_a_zero_operand_gives_an_exactly_zero_result(ctr, storage, cplx):
    A, B, w = two_step_arrays("tiled_mk_kn", cplx, 44, (2.0 ** 40, 2.0 ** -70, 1.0), plant=False)
    r = run_two_steps(ctr, [np.zeros_like(A), B, w], storage, scaling="tensor")
    assert r.array.shape == (A.shape[0],) and not r.array.any() and not np.isnan(r.array).any()
    assert r.exponents[0] == 0 and r.exponents[3] == r.exponents[1]  # (a zero sum: s = 0, e_C = e_A + e_B)
    case = sc.BY_NAME["mfma_mk_kn-65x129x64"]
    a, b = (draw(shape, cplx, np.random.RandomState(45), f) for shape, f in zip(case.shapes(), sc.FACTORS))
    r = ctr.contract([(0, 1)], case.ts, [a, np.zeros_like(b)], storage=storage, scaling="tensor")
    assert not r.array.any() and not np.isnan(r.array).any()


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_an_inf_in_a_leaf_poisons_its_own_sums_only(ctr, storage, cplx):
    A, B, w = two_step_arrays("tiled_mk_kn", cplx, 46, (2.0 ** 40, 2.0 ** -70, 2.0 ** 25), plant=False)
    clean = A.copy()
    A[3, 7] = np.inf
    e_clean = ctr.scale_to_storage(np.where(np.isfinite(A), A, 0).astype(A.dtype), storage)[1]
    r = run_two_steps(ctr, [A, B, w], storage, scaling="tensor")
    assert r.exponents[0] == e_clean == ctr.scale_to_storage(A, storage)[1]
    assert not np.isfinite(r.array[3])
    clean[3, :] = 0  # (row 3 of Z is not finite and does not enter Z's maximum: the reference leaves it out)
    ref, bnd, e, _ = two_step_expected(ctr, clean, B, w, storage, cplx)
    assert abs(r.exponents[3] - e) <= 1  # (no planted maximum here)
    keep = np.arange(len(ref)) != 3
    assert np.isfinite(r.array[keep]).all()
    assert_within(r.array[keep], ref[keep], bnd[keep], f"inf in a leaf {storage}")


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_a_single_sliced_leaf_is_widened_and_scaled_into_the_output(ctr, storage, cplx):
    a = draw((5, 3, 7), cplx, np.random.RandomState(47), 2.0 ** -50)
    r = ctr.contract([], [("i", "s", "j")], [a], slices=("s",), storage=storage, scaling="tensor")
    values, e = ctr.scale_to_storage(a, storage)
    assert kernels_of(ctr, r) == {"gather": 3} and r.narrow_launches == 0 and r.exponents == (e,)
    assert r.array.dtype == a.dtype and r.inds == ("i", "s", "j")
    assert np.array_equal(r.array, values)
    assert -70 < e < -55 and np.abs(r.array - a).max() <= 2 * U_STORAGE[storage] * np.abs(a).max()


@pytest.mark.parametrize("storage,cplx", COMBOS)
def test_two_identical_calls_are_bit_equal(ctr, storage, cplx):
    arrays = two_step_arrays("tiled_mk_kn", cplx, 48, (2.0 ** 40, 2.0 ** -70, 2.0 ** 25))
    first = run_two_steps(ctr, arrays, storage, scaling="tensor")
    again = run_two_steps(ctr, arrays, storage, scaling="tensor")
    assert np.array_equal(first.array, again.array) and first.exponents == again.exponents


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_scaling_keeps_what_float16_alone_loses(ctr, cplx):
    """Leaves near 2^-20: in float16 without scaling they are subnormal and their product, near 2^-40, underflows to
    zero when it is stored; nothing is raised.  With scaling the same call meets the bound."""
    arrays = two_step_arrays("tiled_mk_kn", cplx, 49, (2.0 ** -20, 2.0 ** -20, 1.0), plant=False)
    ref, bnd, _, z = two_step_expected(ctr, *arrays, "float16", cplx)
    assert np.abs(z).max() < 2.0 ** -26  # (below half of float16's smallest subnormal)
    plain = run_two_steps(ctr, arrays, "float16")
    assert plain.scaling is None and plain.exponents is None and plain.narrow_launches == 0
    assert not plain.array.any()  # the intermediate underflowed
    assert (np.abs(ref) > bnd).any()  # ... and zero is not within the bound
    r = run_two_steps(ctr, arrays, "float16", scaling="tensor")
    assert_within(r.array, ref, bnd, "leaves near 2^-20, float16 with scaling")
