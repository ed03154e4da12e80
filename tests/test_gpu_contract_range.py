"""The contraction kernels at the edges of their number range, element by element (cases and fills:
tests/range_cases.py; the same bounds held by host emulations, and shown to catch the defects they are for, in
tests/test_contraction_range_plan.py).  Every case is a one-step network, a two-step chain or a network of one tensor;
every test asserts its kernel path from `kernel_launches` (and `split_launches` / `narrow_launches`).

A  `storage=` without scaling, one operand (or both) wholly subnormal in the 16-bit type.  Reference: the float64 einsum
   of the rounded inputs; bound: that of tests/test_gpu_contract_half.py, (2 c kt + 2) 2^-24 (|A| @ |B|).  A matrix unit
   that read subnormal inputs as zero would be beyond it in every element.
B  `compute="bf16x3"`, A in 2^[-120, -118): every hi normal, nearly every lo a bfloat16 subnormal.  Reference: the
   emulation a_lo b_hi + a_hi b_lo + a_hi b_hi in float64 from `split_bf16`, from which the device differs by its
   float32 sums alone: (2 c 3 kt + 2) 2^-24 (|A| @ |B|).  And parts of A just below the admitted limit 2^128 - 2^119:
   finite, and within the mode's bound [2^-14 + (2 c 3 kt + 2) 2^-24] (|A| @ |B|) of the float64 einsum.
C  The plain kernels, every product and nearly every sum subnormal in the type, or A subnormal:
   (c kt + 2) (u mag + eta), eta half the spacing of the type's subnormals (2^-150, 2^-1075); reference and bound in
   float64 for the single types, in numpy's longdouble for the double types.  The single types also with
   `path_kernel=1` and `slice_batch=1`: the bytes of the plain run.
D  A (i, k) B (k, j) -> Z (i, j), stored; then Z times the identity, whose float32 output is the stored Z.  A row of A
   holds one non-zero, so an element of Z is one product, exact in float32, with more bits than storage holds: the
   output must be `round_to_storage` of it bit for bit (a zero: equal to zero, its sign does not survive step 2), on
   ties of both kinds, their neighbours, results in the subnormal range, the underflow tie and the largest finite value.
   Step 1 runs in each class: the MFMA epilogue, the dot's thread 0 and the stream loop narrow on their own.  Overflow
   is a call of its own (inf x 0 in step 2 poisons a row); with `scaling="tensor"` the products spread over 2^-47 ... 1
   of a planted maximum and the result is round_to_storage(product 2^-e) 2^e with e from the host rule.
E  One tensor, no step: every 16-bit pattern that is not a NaN is widened to the float32 the host widens it to.
F  One inf (one NaN) part in A: the row it feeds is not finite in every part, every other element is finite and within
   the case's bound.

An element that is not a number fails a bound.  tools/range_profile.py writes the largest error / bound per group, type
and class into profiles/contract_range.txt."""
import numpy as np
import pytest

from tests import range_cases as rc
from tests.test_gpu_contract_half import assert_kernels, assert_within, bound, reference, result_inds

pytestmark = pytest.mark.gpu

TYPES = [pytest.param(False, id="real"), pytest.param(True, id="complex")]
CASE_IDS = [c.name for c in rc.CASES]
CLASS_CASES = [rc.THRESHOLD, rc.DOT, rc.STREAM]
SINGLES, DOUBLES = (np.float32, np.complex64), (np.float64, np.complex128)


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


MEASURE_ONLY = False  # tools/range_profile.py: return the largest error / bound of a case without asserting on it


def within(got, ref, bnd, what):
    """assert_within; for the profile the figure alone (inf where an element is not a number)."""
    if not MEASURE_ONLY:
        return assert_within(got, ref, bnd, what)
    err = np.abs(got.astype(ref.dtype) - ref)
    ratio = np.divide(err, bnd, out=np.zeros_like(bnd), where=bnd > 0)
    ratio[~(err <= bnd) & ~(ratio > 1)] = np.inf
    return float(ratio.max())


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def check_step(ctr, r, case, what, cplx):
    assert r.inds == result_inds(case.ts, case.output) == ("i", "j") and r.n_slices == 1, what
    assert_kernels(ctr, r, case.kernels, what)
    assert r.macs == case.ops["M"] * case.ops["N"] * case.ops["K"], what
    assert r.narrow_launches == 0 and r.batch_launches == 0 and r.path_launches == (0, 0), what


# --- A ----------------------------------------------------------------------------------------------------------------
A_RUNS = [pytest.param(s, role, id=f"{s}-{role}_subnormal") for s in rc.STORAGES for role in rc.A_ROLES[s]]


def run_a(ctr, case, storage, role, cplx):
    """Returns the largest error / bound."""
    arrays = rc.fill_a(case, storage, cplx, role)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, storage=storage)
    what = f"A {case.name} {storage} {role} subnormal {'complex' if cplx else 'real'}"
    check_step(ctr, r, case, what, cplx)
    assert r.array.dtype == (np.complex64 if cplx else np.float32) and r.split_launches == 0, what
    ref, mag = reference(case.ts, arrays, r.inds)
    return within(r.array, ref, bound(mag, case.kt, cplx), what)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,role", A_RUNS)
@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_subnormal_16_bit_operands_are_summed_not_flushed(ctr, case, storage, role, cplx):
    run_a(ctr, case, storage, role, cplx)


# --- B ----------------------------------------------------------------------------------------------------------------
def split_sum_bound(mag, kt, cplx):
    return (2 * (2 if cplx else 1) * 3 * kt + 2) * 2.0 ** -24 * mag


def run_b(ctr, case, cplx):
    arrays = rc.fill_b(case, cplx)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute="bf16x3")
    what = f"B {case.name} {'complex' if cplx else 'real'}"
    check_step(ctr, r, case, what, cplx)
    assert r.split_launches == 1 and r.compute == "bf16x3", what
    A, B = rc.mats(case, arrays)
    emul = rc.split_emulation(A, B)
    mag = np.abs(A.astype(emul.dtype)) @ np.abs(B.astype(emul.dtype))
    return within(r.array, emul, split_sum_bound(mag, case.kt, cplx), what)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("case", rc.TILED, ids=[c.name for c in rc.TILED])
def test_a_subnormal_lo_of_the_split_is_summed_not_flushed(ctr, case, cplx):
    run_b(ctr, case, cplx)


def run_b_top(ctr, cplx):
    from tests.test_gpu_contract_split import bound as split_bound
    case = rc.THRESHOLD
    arrays = rc.fill_b_top(case, cplx)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute="bf16x3")
    what = f"B top of the range {'complex' if cplx else 'real'}"
    check_step(ctr, r, case, what, cplx)
    assert r.split_launches == 1, what
    assert MEASURE_ONLY or np.isfinite(r.array).all(), what
    ref, mag = reference(case.ts, arrays, r.inds)
    return within(r.array, ref, split_bound(mag, case.kt, cplx), what)


@pytest.mark.parametrize("cplx", TYPES)
def test_parts_just_below_the_limit_of_the_split_give_finite_sums_inside_its_bound(ctr, cplx):
    run_b_top(ctr, cplx)


# --- C ----------------------------------------------------------------------------------------------------------------
def run_c(ctr, case, dtype, kind):
    arrays = rc.fill_c(case, dtype, kind)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output)
    what = f"C {case.name} {np.dtype(dtype).name} subnormal {kind}"
    check_step(ctr, r, case, what, np.dtype(dtype).kind == "c")
    assert r.array.dtype == np.dtype(dtype), what
    ref, mag = rc.reference_c(case, arrays)
    worst = within(r.array, ref, rc.bound_c(mag, case.kt, dtype), what)
    return worst, arrays, r


@pytest.mark.parametrize("kind", rc.C_KINDS)
@pytest.mark.parametrize("dtype", SINGLES + DOUBLES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", CLASS_CASES, ids=["tiled", "dot", "stream"])
def test_the_plain_kernels_keep_subnormal_operands_products_and_sums(ctr, case, dtype, kind):
    if rc.real_size(dtype) == 8 and np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy's longdouble has no more precision than float64 here: no reference for the double types")
    _, arrays, r = run_c(ctr, case, dtype, kind)
    if np.dtype(dtype) in [np.dtype(d) for d in SINGLES]:
        fused = ctr.contract([(0, 1)], case.ts, arrays, case.output, path_kernel=1)
        assert fused.path_launches == (1, 1) and not any(fused.kernel_launches) and fused.launches == 2
        assert np.array_equal(bits(fused.array), bits(r.array))
        batched = ctr.contract([(0, 1)], case.ts, arrays, case.output, slice_batch=1)
        assert batched.kernel_launches == r.kernel_launches and batched.batch_launches == 1
        assert np.array_equal(bits(batched.array), bits(r.array))


# --- D ----------------------------------------------------------------------------------------------------------------
D_RUNS = [pytest.param(s, cls, id=f"{s}-{cls}") for s in rc.STORAGES for cls in rc.D_SHAPES]
D_KERNELS = {"tiled": {"tiled_mk_kn": 1, "tiled_km_nk": 1}, "dot": {"dot": 1, "stream": 1}, "stream": {"stream": 2}}


def chain(ctr, A, B, storage, cls, what, **kw):
    """The two-step chain; returns (the result, its array as [i, l]: the stored Z widened)."""
    r = ctr.contract(rc.CHAIN_PATH, rc.CHAIN_TS, [A, B, rc.IDENTITY], storage=storage, **kw)
    assert r.inds == ("l", "i") and r.array.dtype == A.dtype, what
    want = tuple(D_KERNELS[cls].get(name, 0) for name in ctr.KERNEL_PATHS)
    assert r.kernel_launches == want, f"{what}: launches {dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))}"
    assert r.narrow_launches == (1 if kw else 0) and r.launches == sum(r.kernel_launches) + r.narrow_launches, what
    return r, np.ascontiguousarray(r.array.T)


def same_stored(got, want):
    """Per part: the float32 bit pattern of `want` where that is not zero, equal to zero where it is."""
    g, w = (np.ascontiguousarray(rc.parts(x), np.float32) for x in (got, want))
    return np.where(w != 0, g.view(np.uint32) == w.view(np.uint32), g == 0)


def assert_stored(got, want, what, rows=None):
    ok = same_stored(got, want)
    if rows is not None:
        ok = ok[rows]
        got, want = got[rows], want[rows]
    if not ok.all():
        at = tuple(int(v) for v in np.argwhere(~ok)[0])
        g, w = rc.parts(got)[at], rc.parts(want)[at]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} parts differ from the host's rounding; first at {at}: "
                             f"got {float(g)!r} ({np.float32(g).view(np.uint32):#010x}), host {float(w)!r} "
                             f"({np.float32(w).view(np.uint32):#010x})")
    return int(ok.size)


def run_d(ctr, storage, cls, cplx):
    """Returns per category (parts compared, parts that differ): the assert is on all of them."""
    t = rc.narrow_table(storage, cls, cplx)
    what = f"D {storage} {cls} {'complex' if cplx else 'real'}"
    r, got = chain(ctr, t["A"], t["B"], storage, cls, what)
    want = ctr.round_to_storage(t["Z"].astype(t["A"].dtype), storage)
    ok = same_stored(got, want)
    flags = rc.round_model(t["P"], t["E"], storage)[2]
    counts = {name: (int(flags[name].sum()), int((flags[name] & ~ok).sum())) for name in rc.CATEGORIES}
    print(f"{what}: parts that differ per category: " + ", ".join(f"{k} {bad}/{n}" for k, (n, bad) in counts.items()))
    if not MEASURE_ONLY:
        assert_stored(got, want, what)
    return counts


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_a_stored_product_is_the_hosts_rounding_bit_for_bit(ctr, storage, cls, cplx):
    run_d(ctr, storage, cls, cplx)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_a_product_at_or_beyond_the_overflow_tie_is_stored_as_inf(ctr, storage, cls, cplx):
    A, B, planted = rc.overflow_table(storage, cls, cplx)
    what = f"D overflow {storage} {cls} {'complex' if cplx else 'real'}"
    r, got = chain(ctr, A, B, storage, cls, what)
    K = A.shape[1]
    i = np.arange(len(A))
    z = A[i, i % K].astype(np.complex128)[:, None] * B[i % K].astype(np.complex128)
    want = rc.stored(z.astype(np.complex64) if cplx else z.real.astype(np.float32), storage)
    g = rc.parts(got)
    clean = np.ones(len(A), bool)
    for row, col, part, sign in planted:
        assert (g[row, col, part] if cplx else g[row, col]) == sign * np.inf, (what, row, col)
        assert not np.isfinite(g[row]).any(), (what, row)
        clean[row] = False
    assert np.isfinite(g[clean]).all(), what
    assert_stored(got, want, what, rows=clean)


def run_d_scaled(ctr, storage, cls, cplx):
    A, B, Z = rc.scaled_table(storage, cls, cplx)
    what = f"D scaled {storage} {cls} {'complex' if cplx else 'real'}"
    r, got = chain(ctr, A, B, storage, cls, what, scaling="tensor")
    want, e = rc.expected_scaled(Z, storage)
    if MEASURE_ONLY:
        return int((~same_stored(got, want)).sum()), r.exponents[3] - e
    assert r.exponents == (ctr.scale_exponent(A), ctr.scale_exponent(B), -ctr.SCALE_BITS, e, 0), (what, r.exponents, e)
    return assert_stored(got, want, what)


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_a_scaled_stored_product_is_the_hosts_rounding_at_the_hosts_exponent(ctr, storage, cls, cplx):
    run_d_scaled(ctr, storage, cls, cplx)


# --- E ----------------------------------------------------------------------------------------------------------------
def run_e(ctr, storage, cplx):
    leaf = rc.widen(rc.all_patterns(storage), storage)
    leaf = leaf.view(np.complex64) if cplx else leaf
    r = ctr.contract([], [("n",)], [leaf], storage=storage)
    assert_kernels(ctr, r, {"gather": 1}, f"E {storage}")
    assert r.inds == ("n",) and r.array.dtype == leaf.dtype and r.array.shape == leaf.shape
    differ = int((r.array.view(np.uint32) != leaf.view(np.uint32)).sum())
    assert differ == 0, f"E {storage}: {differ} of {leaf.view(np.uint32).size} patterns are widened to another float32"
    return leaf


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage", rc.STORAGES)
def test_every_16_bit_pattern_is_widened_as_the_host_widens_it(ctr, storage, cplx):
    leaf = run_e(ctr, storage, cplx).copy()
    leaf.view(np.float32)[5] = np.nan
    r = ctr.contract([], [("n",)], [leaf], storage=storage)
    got, want = r.array.view(np.float32), leaf.view(np.float32)
    assert np.isnan(got[5]) and np.isnan(got).sum() == 1
    keep = np.arange(got.size) != 5
    assert np.array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])


# --- F ----------------------------------------------------------------------------------------------------------------
F_RUNS = [pytest.param(c, None, id=rc.class_of(c)) for c in CLASS_CASES] + \
    [pytest.param(rc.THRESHOLD, s, id=f"mfma-{s}") for s in rc.STORAGES]


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan], ids=["inf", "minus_inf", "nan"])
@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("case,storage", F_RUNS)
def test_a_part_that_is_not_finite_poisons_the_row_it_feeds_and_no_other(ctr, case, storage, cplx, value):
    from tests.test_gpu_contract_kernels import _bound as plain_bound
    arrays = rc.fill_f(case, cplx, storage=storage)
    assert all((rc.parts(a) != 0).all() for a in arrays)
    row, k = rc.F_AT[rc.class_of(case)]
    assert case.ops["form_a"] == 0 and row < case.ops["M"] and k < case.ops["K"]
    arrays[0][row, k] = value + 1j * arrays[0][row, k].imag if cplx else value
    kw = dict(storage=storage) if storage else {}
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, **kw)
    what = f"F {case.name} {storage} {'complex' if cplx else 'real'} {value}"
    check_step(ctr, r, case, what, cplx)
    assert not np.isfinite(rc.parts(r.array)[row]).any(), what
    arrays[0][row, k] = 0
    ref, mag = reference(case.ts, arrays, r.inds)
    dtype = np.complex64 if cplx else np.float32
    bnd = bound(mag, case.kt, cplx) if storage else plain_bound(mag, case.kt, dtype)
    others = np.arange(case.ops["M"]) != row
    assert np.isfinite(r.array[others]).all(), what
    assert_within(r.array[others], ref[others], bnd[others], what)
