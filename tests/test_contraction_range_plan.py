"""The number-range cases (tests/range_cases.py) without a GPU.  For every group of tests/test_gpu_contract_range.py:
plan() routes each case to the kernel slot the device test asserts; a numpy emulation of a correct kernel -- a chain of
float32 (or float64) products and sums, two roundings per term -- stays inside the group's bound; and the same emulation
with the defect the group is there to catch leaves it: subnormal inputs of the matrix unit flushed (A), the subnormal lo
of the split flushed (B), subnormal products and sums flushed (C), truncation instead of nearest-even (D).  "Leaves"
means every element for A and C and more than half of them for B, where an element can have its flushed terms cancel.
The D table is shown to hold its categories, and the host's round_to_storage to agree with an integer model on it."""
import numpy as np
import pytest

from tests import range_cases as rc
from tests.test_gpu_contract_half import bound as storage_bound
from tnco_amd import contraction as ctr

TYPES = [pytest.param(False, id="real"), pytest.param(True, id="complex")]
CASE_IDS = [c.name for c in rc.CASES]
SINGLES, DOUBLES = (np.float32, np.complex64), (np.float64, np.complex128)


def slot_of(op):
    """The kernel path the dispatcher of csrc/contract.hip takes for a step (its thresholds restated)."""
    if op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32:
        return "tiled_" + ("mk" if op["form_a"] == 0 else "km") + "_" + ("kn" if op["form_b"] == 0 else "nk")
    return "dot" if op["K"] >= 512 and op["H"] * op["M"] * op["N"] <= 8192 else "stream"


@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_plan_routes_a_case_to_its_kernel_slot(case):
    for kw in (dict(dtype=np.float32), dict(dtype=np.complex128), dict(dtype=np.complex64, storage="float16"),
               dict(dtype=np.float32, storage="bfloat16"), dict(dtype=np.float32, compute="bf16x3"),
               dict(dtype=np.complex64, path_kernel=1), dict(dtype=np.float32, slice_batch=1)):
        p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, **kw)
        op, = p.ops
        assert {k: op[k] for k in ("H", "M", "N", "K", "form_a", "form_b")} == {k: v for k, v in case.ops.items() if k != "perms"}
        assert len(p.perms) == 0 and p.inds == ("i", "j") and case.kernels == {slot_of(op): 1}
    assert {rc.class_of(c) for c in rc.CASES} == {"tiled", "dot", "stream"}
    assert {(c.ops["form_a"], c.ops["form_b"]) for c in rc.TILED} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("cls", rc.D_SHAPES)
def test_plan_routes_the_chain_of_group_d(cls):
    M, K = rc.D_SHAPES[cls]
    for kw in (dict(), dict(scaling="tensor")):
        p = ctr.plan(rc.CHAIN_PATH, rc.CHAIN_TS, [(M, K), (K, rc.D_N), (rc.D_N, rc.D_N)], dtype=np.float32,
                     storage="float16", **kw)
        first, second = p.ops
        assert slot_of(first).split("_")[0] == cls and slot_of(second).split("_")[0] == rc.step2_class(cls)
        assert len(p.perms) == 0 and p.steps[0, 8] == ctr.ARENA and p.steps[1, 8] == ctr.OUT and p.inds == ("l", "i")


def test_plan_gathers_the_single_leaf_of_group_e():
    p = ctr.plan([], [("n",)], [(len(rc.all_patterns("float16")),)], dtype=np.float32, storage="float16")
    assert len(p.steps) == 0 and len(p.perms) == 1 and p.perms[0, 2] == ctr.OUT


# --- A ----------------------------------------------------------------------------------------------------------------
A_RUNS = [pytest.param(s, role, id=f"{s}-{role}_subnormal") for s in rc.STORAGES for role in rc.A_ROLES[s]]


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,role", A_RUNS)
@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_a_float32_chain_meets_the_bound_of_group_a_and_flushed_inputs_leave_it(case, storage, role, cplx):
    arrays = rc.fill_a(case, storage, cplx, role)
    A, B = rc.mats(case, arrays)
    wide = np.complex128 if cplx else np.float64
    ref, mag = A.astype(wide) @ B.astype(wide), np.abs(A.astype(wide)) @ np.abs(B.astype(wide))
    bnd = storage_bound(mag, case.kt, cplx)
    good = np.abs(rc.chain(A, B, np.float32) - ref) / bnd
    flushed = np.abs(rc.chain(rc.flush_storage(A, storage), rc.flush_storage(B, storage), np.float32) - ref) / bnd
    print(f"{case.name} {storage} {role}: chain {good.max():.4f}, flushed inputs at least {flushed.min():.1f} of the bound")
    assert good.max() < 0.25 and flushed.min() > 1


# --- B ----------------------------------------------------------------------------------------------------------------
def split_bound(mag, kt, cplx):
    return (2 * (2 if cplx else 1) * 3 * kt + 2) * 2.0 ** -24 * mag


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("case", rc.TILED, ids=[c.name for c in rc.TILED])
def test_the_three_products_in_float32_meet_the_bound_of_group_b_and_a_flushed_lo_leaves_it(case, cplx):
    A, B = rc.mats(case, rc.fill_b(case, cplx))
    (a_hi, a_lo), (b_hi, b_lo) = ctr.split_bf16(A), ctr.split_bf16(B)
    assert np.isfinite(rc.parts(a_hi)).all() and (np.abs(rc.parts(a_hi)) >= 2.0 ** -126).all()  # every hi is normal
    lo = np.abs(rc.parts(a_lo))
    assert ((lo > 0) & (lo < 2.0 ** -126)).mean() > 0.95
    emul = rc.split_emulation(A, B)
    bnd = split_bound(np.abs(A.astype(emul.dtype)) @ np.abs(B.astype(emul.dtype)), case.kt, cplx)
    good = np.abs(rc.chain(None, None, np.float32, terms=[(a_lo, b_hi), (a_hi, b_lo), (a_hi, b_hi)]) - emul) / bnd
    flushed = np.abs(rc.split_emulation(A, B, flush_lo=True) - emul) / bnd
    print(f"{case.name}: chain {good.max():.4f}, flushed lo: median {np.median(flushed):.1f}, "
          f"{(flushed > 1).mean():.3f} of the elements beyond the bound")
    assert good.max() < 0.25 and (flushed > 1).mean() > 0.5


@pytest.mark.parametrize("cplx", TYPES)
def test_the_top_of_the_split_range_is_admitted_and_its_sums_are_finite(cplx):
    A, B = rc.fill_b_top(rc.THRESHOLD, cplx)
    ctr._check_split_range(A)
    hi, lo = ctr.split_bf16(A)
    assert (np.abs(rc.parts(hi)) == np.float32(2.0 ** 128 - 2.0 ** 120)).all() and (rc.parts(lo) != 0).mean() > 0.9
    up = np.nextafter(np.abs(rc.parts(A)).max(), np.float32(np.inf))
    assert up == np.float32(2.0 ** 128 - 2.0 ** 119)
    with pytest.raises(ValueError, match="beyond the range of the bfloat16 split"):
        ctr._check_split_range(np.array([up], np.float32))
    with np.errstate(over="raise"):
        assert np.isfinite(rc.chain(A, B, np.float32)).all()


# --- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.C_KINDS)
@pytest.mark.parametrize("dtype", SINGLES + DOUBLES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", [rc.THRESHOLD, rc.DOT, rc.STREAM], ids=["tiled", "dot", "stream"])
def test_a_two_rounding_chain_meets_the_bound_of_group_c_and_a_flushed_one_leaves_it(case, dtype, kind):
    if rc.real_size(dtype) == 8 and np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy's longdouble has no more precision than float64 here: no reference for the double types")
    arrays = rc.fill_c(case, dtype, kind)
    A, B = rc.mats(case, arrays)
    real = np.float32 if rc.real_size(dtype) == 4 else np.float64
    tiny = float(np.finfo(real).tiny)
    if kind == "operands":
        assert (np.abs(rc.parts(A)) < tiny).all() and (rc.parts(A) != 0).all()
    ref, mag = rc.reference_c(case, arrays)
    if kind == "sums":
        assert (np.abs(rc.parts(ref)) < tiny).mean() > 0.5  # (the products all are: |a b| < 2^-130, 2^-1054)
    bnd = rc.bound_c(mag, case.kt, dtype)
    good = np.abs(rc.chain(A, B, real) - ref) / bnd
    if kind == "sums":
        flushed = np.abs(rc.chain(A, B, real, flush=True) - ref) / bnd
    else:  # a kernel that reads its subnormal operand as zero
        flushed = np.abs(rc.chain(np.zeros_like(A), B, real) - ref) / bnd
    print(f"{case.name} {np.dtype(dtype).name} {kind}: chain {float(good.max()):.4f}, flushed at least "
          f"{float(flushed.min()):.1f} of the bound")
    assert good.max() < 0.5 and flushed.min() > 1


# --- D ----------------------------------------------------------------------------------------------------------------
D_RUNS = [pytest.param(s, cls, id=f"{s}-{cls}") for s in rc.STORAGES for cls in rc.D_SHAPES]


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_the_narrowing_table_holds_its_categories_and_truncation_would_show(storage, cls, cplx):
    t = rc.narrow_table(storage, cls, cplx)
    nearest, cut, flags = rc.round_model(t["P"], t["E"], storage)
    for name in rc.CATEGORIES:
        per_part = flags[name].reshape(-1, 2 if cplx else 1).sum(0)
        print(f"{storage} {cls} {name}: {per_part.tolist()}")
        assert (per_part >= 8).all(), (name, per_part)
    # the host's rounding is the integer model's, on every entry
    single = np.complex64 if cplx else np.float32
    want = rc.parts(ctr.round_to_storage(t["Z"].astype(single), storage)).astype(np.float64)
    assert np.array_equal(np.abs(want), nearest) and np.isfinite(nearest).all()
    assert (nearest[flags["underflow_tie"]] == 0).all() and (nearest[flags["tie_down"]] == cut[flags["tie_down"]]).all()
    tiny = 2.0 ** (rc.E_MIN[storage] - rc.P_BITS[storage] + 1)
    assert (nearest[flags["above_underflow_tie"]] == tiny).all()
    # a narrowing that truncates differs on every tie that rounds up and on every neighbour above a tie
    for name in ("tie_up", "above_tie", "above_underflow_tie"):
        assert (cut[flags[name]] != nearest[flags[name]]).all()
    assert (cut != nearest).mean() > 0.25


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_the_overflow_call_poisons_its_planted_rows_only(storage, cls, cplx):
    A, B, planted = rc.overflow_table(storage, cls, cplx)
    assert [row for row, *_ in planted] == list(rc.OVER_ROWS)
    for x in (A, B):
        assert np.array_equal(ctr.round_to_storage(x, storage), x)
    K = A.shape[1]
    i = np.arange(len(A))
    z = (A[i, i % K].astype(np.complex128)[:, None] * B[i % K].astype(np.complex128))
    z = z.astype(np.complex64) if cplx else z.real.astype(np.float32)
    assert np.isfinite(z).all()  # (float32 holds the products; storage does not)
    zs = rc.parts(rc.stored(z, storage))
    assert (~np.isfinite(zs)).sum() == len(planted)  # (the planted parts and nothing else)
    assert sorted(set(np.argwhere(~np.isfinite(zs))[:, 0].tolist())) == sorted(rc.OVER_ROWS)
    for row, col, part, sign in planted:
        assert (zs[row, col, part] if cplx else zs[row, col]) == sign * np.inf
    top = (2.0 - 2.0 ** (1 - rc.P_BITS[storage])) * 2.0 ** rc.E_MAX[storage]
    first = rc.parts(z)[planted[0][0], planted[0][1]]
    assert abs(first[planted[0][2]] if cplx else first) == top + 2.0 ** (rc.E_MAX[storage] - rc.P_BITS[storage])  # the tie


@pytest.mark.parametrize("cplx", TYPES)
@pytest.mark.parametrize("storage,cls", D_RUNS)
def test_the_scaled_table_spreads_over_45_binades(storage, cls, cplx):
    A, B, Z = rc.scaled_table(storage, cls, cplx)
    x = np.abs(rc.parts(Z))
    x = x[x > 0]
    assert x.max() / x.min() >= 2.0 ** 40 and x.max() / x.min() < 2.0 ** 48
    want, e = rc.expected_scaled(Z, storage)
    assert e == int(np.floor(np.log2(x.max()))) - 14
    w = np.abs(rc.parts(want)).astype(np.float64)
    exact = np.abs(rc.parts(Z))
    assert (w[exact > 0] == 0).sum() >= (8 if storage == "float16" else 0)  # below 2^-39 of the largest float16 has nothing
    if storage == "float16":  # below 2^-28 of the largest: float16 subnormals, fewer than 11 bits
        low = (exact > 0) & (exact < 2.0 ** -30 * x.max()) & (w > 0)
        assert low.sum() >= 8 and (np.abs(w[low] - exact[low]) > 2.0 ** -12 * exact[low]).any()
    assert (w != exact).mean() > 0.5  # (ties and neighbours: most entries are rounded)


# --- E ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", rc.STORAGES)
def test_the_patterns_of_group_e_pass_the_host_unchanged(storage):
    bits = rc.all_patterns(storage)
    assert len(bits) == (1 << 16) - (2046 if storage == "float16" else 254) and len(bits) % 2 == 0
    wide = rc.widen(bits, storage)
    assert not np.isnan(wide).any() and np.isinf(wide).sum() == 2 and len(np.unique(wide.view(np.uint32))) == len(bits)
    assert np.array_equal(ctr._storage_bits(wide, storage), bits)  # what the device is handed: every pattern once
    pairs = wide.view(np.complex64)
    assert np.array_equal(ctr._storage_bits(pairs, storage).reshape(-1), bits)
