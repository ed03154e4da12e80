"""Slice batches (`contract(..., slice_batch=B)`, csrc/contract.hip MemberArgs and ct_batch_reduce_kernel) on the device.

The contract of the feature is bit equality with `slice_batch=None`: every case of tests/batch_cases.py is run once
unbatched and once per B in (1, 2, 5, 12, 64), and the bytes of the result, the multiply-adds, the exponents (under
scaling) and the launch counts are compared.  With n assignments a batched run makes ceil(n / B) launches where the
unbatched one makes n, path by path, and ceil(n / B) launches of the reduce kernel on top.

Two equal wrong answers would pass that, so per dtype the unbatched-equal result is also held to numpy's einsum of the
whole sliced sum in float64 / complex128, under the bound of tests/test_gpu_contract_kernels.py,

    |got - ref| <= (c kt + 2) u (|A| |B| |C|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

with kt the roundings an element of the result goes through: K of the stored step, K of the output step, and the
assignments added into the element (first order: the error of the stored step enters the second step's terms once).
Inputs are uniform(0.5, 1.5) in both parts, no cancellation, as in that file.
"""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as bc

pytestmark = pytest.mark.gpu

N = bc.N_ASSIGNMENTS
STORAGE_COMBOS = [pytest.param(s, c, id=f"{s}-{'complex' if c else 'real'}") for s in ("float16", "bfloat16")
                  for c in (False, True)]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def fill(chain, dtype, seed):
    rng = np.random.RandomState(seed)
    out = []
    for shape in chain.shapes():
        a = rng.uniform(0.5, 1.5, shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.uniform(0.5, 1.5, shape)
        out.append(a.astype(dtype))
    return out


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def tiled(ctr, r):
    return sum(v for name, v in zip(ctr.KERNEL_PATHS, r.kernel_launches) if name.startswith("tiled"))


def by_class(ctr, r):
    k = dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))
    return dict(tiled=tiled(ctr, r), dot=k["dot"], stream=k["stream"])


def assert_batched_equals(ctr, base, r, B, n, what):
    """`r`, run with slice_batch=B over n assignments, against `base`, the same call with slice_batch=None."""
    groups = -(-n // B)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype and r.array.shape == base.array.shape, what
    assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the unbatched run"
    assert r.macs == base.macs and r.n_slices == base.n_slices == n, what
    assert r.exponents == base.exponents, what
    assert all(v % n == 0 for v in base.kernel_launches) and base.narrow_launches % n == 0
    assert r.kernel_launches == tuple(v // n * groups for v in base.kernel_launches), what
    assert r.narrow_launches == base.narrow_launches // n * groups, what
    assert r.row_kernel_launches == (0, 0, 0)
    assert r.batch_launches == groups and base.batch_launches == 0, what
    assert r.launches == sum(r.kernel_launches) + r.narrow_launches + r.batch_launches, what
    assert r.slice_batch == min(B, n) and base.slice_batch is None


def run_all_batches(ctr, chain, arrays, what, batches=bc.BATCHES, **kw):
    call = lambda **more: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, **kw, **more)  # noqa: E731
    base = call()
    for B in batches:
        assert_batched_equals(ctr, base, call(slice_batch=B), B, N, f"{what} B = {B}")
    return base


def assert_classes(ctr, chain, base):
    """The unbatched run took the kernel paths the case is named after, once per assignment each."""
    want = dict(tiled=0, dot=0, stream=0)
    for k in chain.classes:
        want[k] += N
    assert by_class(ctr, base) == want, f"{chain.name}: launches {dict(zip(ctr.KERNEL_PATHS, base.kernel_launches))}"
    assert base.kernel_launches[0] == N  # (B is gathered once per assignment; A and C are read in place)


def einsum_reference(chain, arrays):
    """(the whole sliced sum, the same of the moduli) in double precision, axes in chain.output order."""
    sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in chain.ts for x in xs))}
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    args = lambda ws: [q for w, xs in zip(ws, chain.ts) for q in (w, [sym[x] for x in xs])]  # noqa: E731
    res = [sym[x] for x in chain.output]
    return np.einsum(*args(wide), res, optimize=True), np.einsum(*args([np.abs(w) for w in wide]), res, optimize=True)


def assert_einsum(chain, arrays, r, dtype, what):
    ref, mag = einsum_reference(chain, arrays)
    got = r.array.transpose([r.inds.index(x) for x in chain.output])
    (_, _, k1), (_, _, k2) = chain.steps()
    kt = k1 + k2 + chain.summed
    u = float(np.finfo(dtype).eps) / 2
    bound = ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * u * mag
    err = np.abs(got.astype(ref.dtype) - ref)
    print(f"{what}: largest error / bound {float((err / bound).max()):.4f} (kt {kt})")
    assert got.shape == ref.shape and (err <= bound).all(), what


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=[np.dtype(d).name for d in bc.DTYPES])
@pytest.mark.parametrize("chain", bc.PLAIN, ids=[c.name for c in bc.PLAIN])
def test_every_shape_class_as_stored_and_as_output_step(ctr, chain, dtype):
    arrays = fill(chain, dtype, seed=61)
    what = f"{chain.name} {np.dtype(dtype).name}"
    base = run_all_batches(ctr, chain, arrays, what)
    assert_classes(ctr, chain, base)
    assert base.array.dtype == np.dtype(dtype)
    assert_einsum(chain, arrays, base, dtype, what)


@pytest.mark.parametrize("storage,cplx", STORAGE_COMBOS)
@pytest.mark.parametrize("chain", bc.HALF, ids=[c.name for c in bc.HALF])
def test_storage_mode_runs_the_mfma_kernel_with_a_member_axis(ctr, chain, storage, cplx):
    arrays = fill(chain, np.complex64 if cplx else np.float32, seed=62)
    arrays = [(a / np.float32(8)).astype(a.dtype) for a in arrays]  # (sums of 65 x 65 products stay inside float16)
    base = run_all_batches(ctr, chain, arrays, f"{chain.name} {storage}", storage=storage)
    assert_classes(ctr, chain, base)
    assert tiled(ctr, base) == 2 * N
    one = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, storage=storage, slice_batch=5)
    assert tiled(ctr, one) == 2 * 3  # both steps of each of the three batches on the MFMA kernel
    assert np.isfinite(base.array).all() and base.array.any()


def scaled_leaves(chain, cplx, seed):
    """Leaves whose level depends on the slice value of u (A), of t (B) and of both (C): the stored intermediate's
    exponent then differs from one assignment to the next by 6 or 12.  (Milder than the 2^-40 of
    tests/test_gpu_contract_scaled.py, so that the low level keeps bits in float16 under the leaf's one exponent.)"""
    A, B, Cc = fill(chain, np.complex64 if cplx else np.float32, seed)
    level = np.array([2.0 ** -6, 1.0], np.float32)
    A = A * level[None, :, None, None]  # (p, u, i, k)
    B = B * level[None, :, None]  # (k, t, j)
    Cc = Cc * level[:, None, None, None] * level[None, :, None, None]  # (t, u, j, l)
    return [x.astype(np.complex64 if cplx else np.float32) * np.float32(2.0 ** 20) for x in (A, B, Cc)]


@pytest.mark.parametrize("storage,cplx", STORAGE_COMBOS)
@pytest.mark.parametrize("chain", bc.SCALED, ids=[c.name for c in bc.SCALED])
def test_scaling_keeps_exponent_slots_and_max_words_per_member(ctr, chain, storage, cplx):
    arrays = scaled_leaves(chain, cplx, seed=63)
    kw = dict(storage=storage, scaling="tensor")
    base = run_all_batches(ctr, chain, arrays, f"{chain.name} {storage} scaled", **kw)
    assert_classes(ctr, chain, base)
    assert base.narrow_launches == N and base.exponents is not None
    assert np.isfinite(base.array).all() and base.array.any()
    # the intermediate's exponent does differ between assignments: runs of one assignment each report it
    seen = {ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, slice_range=(s, s + 1), slice_batch=1,
                         **kw).exponents[3] for s in range(4)}
    assert len(seen) >= 3, seen


@pytest.mark.parametrize("kw", [dict(), dict(storage="float16", scaling="tensor")], ids=["plain", "scaled"])
def test_a_range_that_starts_off_a_multiple_of_the_batch(ctr, kw):
    chain = bc.SMALL
    arrays = scaled_leaves(chain, True, 64) if kw else fill(chain, np.complex64, 64)
    call = lambda **more: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, slice_range=(1, 11),  # noqa: E731
                                       **kw, **more)
    base = call()
    r = call(slice_batch=4)  # batches 1..4, 5..8, 9..10
    assert_batched_equals(ctr, base, r, 4, 10, f"slice_range (1, 11) {kw}")
    assert r.batch_launches == 3
    whole = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, **kw)
    assert not np.array_equal(bits(whole.array), bits(base.array))  # (assignments 0 and 11 are missing from the range)


@pytest.mark.parametrize("chain", [bc.SUMMED, bc.PLACED], ids=["one_block", "a_block_per_assignment"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_members_that_all_share_a_block_and_members_that_never_do(ctr, chain, dtype):
    arrays = fill(chain, dtype, seed=65)
    what = f"{chain.name} {np.dtype(dtype).name}"
    base = run_all_batches(ctr, chain, arrays, what)
    p = ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=dtype)
    assert len(p.block_inds) == (0 if chain.variant == "summed" else 3)
    assert_einsum(chain, arrays, base, dtype, what)


@pytest.mark.parametrize("kw", [dict(), dict(storage="bfloat16"), dict(storage="float16", scaling="tensor")],
                         ids=["plain", "bfloat16", "float16-scaled"])
def test_a_single_leaf_plan_takes_the_keyword_and_runs_as_before(ctr, kw):
    rng = np.random.RandomState(66)
    a = (rng.uniform(0.5, 1.5, (5, 3, 7)) + 1j * rng.uniform(0.5, 1.5, (5, 3, 7))).astype(np.complex64)
    base = ctr.contract([], [("i", "s", "j")], [a], slices=("s",), **kw)
    r = ctr.contract([], [("i", "s", "j")], [a], slices=("s",), slice_batch=2, **kw)
    assert np.array_equal(bits(r.array), bits(base.array)) and r.inds == base.inds
    assert r.kernel_launches == base.kernel_launches and r.launches == base.launches == 3
    assert r.batch_launches == 0 and r.slice_batch == 1 and r.exponents == base.exponents
    assert r.peak_device_bytes == base.peak_device_bytes


def test_peak_device_bytes_counts_what_the_batch_reserves(ctr):
    chain = bc.SMALL
    arrays = scaled_leaves(chain, False, 67)
    for kw in (dict(), dict(storage="float16", scaling="tensor")):
        call = lambda **more: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, **kw, **more)  # noqa: E731
        base, r = call(), call(slice_batch=5)
        p0 = ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=np.float32, **kw)
        p5 = ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=np.float32, slice_batch=5, **kw)
        # the library and the plan count the same growth (their totals differ by the padding of leaves and tables)
        assert r.peak_device_bytes - base.peak_device_bytes == p5.peak_device_bytes - p0.peak_device_bytes > 0


def test_the_setter_refuses_row_axes_and_batches_out_of_range(ctr):
    """Through the ABI: a handle from a plan with projections (row axes) takes no slice batch; a plain one takes 1..64."""
    from tnco_amd import _lib
    L = _lib.load()
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"),
                    projs=np.array([[0, 1], [1, 1], [1, 0]]))
    assert rows.row_steps is not None and len(rows.row_steps) == 1
    plain = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32)
    for p, codes in ((rows, {4: _lib.EINVAL, 1: _lib.EINVAL}),
                     (plain, {0: _lib.EINVAL, 65: _lib.EINVAL, -1: _lib.EINVAL, 1: _lib.OK, 64: _lib.OK, 7: _lib.OK})):
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        try:
            for batch, code in codes.items():
                assert L.tnco_hip_contract_set_slice_batch(h, batch) == code, (p is rows, batch)
            count = C.c_int64(-1)
            assert L.tnco_hip_contract_batch_launches(h, C.byref(count)) == _lib.OK and count.value == 0
            assert L.tnco_hip_contract_batch_launches(h, None) == _lib.EINVAL
        finally:
            L.tnco_hip_contract_destroy(h)
        del keep
    assert L.tnco_hip_contract_set_slice_batch(None, 4) == _lib.EINVAL
