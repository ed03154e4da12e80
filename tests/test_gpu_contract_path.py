"""The path kernel (`contract(..., path_kernel=G)`, csrc/contract_path.h ct_path_kernel and ct_path_reduce_kernel) on the
device.

The contract of the feature is bit equality with `path_kernel=None`: every case of tests/path_cases.py is run once unfused
and once per G in (1, 2, 5, 12, 1024), and the bytes of the result, the multiply-adds and the launch counts are compared.
With n assignments a fused run makes ceil(n / G) launches of the path kernel and as many of the reduce kernel, and none
of any other kernel.

Two equal wrong answers would pass that, so per dtype the result is also held to numpy's einsum of the whole sliced sum
in float64 / complex128, under the bound of tests/test_gpu_contract_kernels.py,

    |got - ref| <= (c kt + 2) u (|A| |B| |C|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

with kt the roundings an element of the result goes through: K of the stored step, K of the output step, and the
assignments added into the element.  Inputs are uniform(0.5, 1.5) in both parts: no exact zeros, no cancellation.
"""
import ctypes as C

import numpy as np
import pytest

from tests import path_cases as pc

pytestmark = pytest.mark.gpu

N = pc.N_ASSIGNMENTS
DTYPE_IDS = [np.dtype(d).name for d in pc.DTYPES]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def assert_fused_equals(ctr, base, r, G, n, what):
    """`r`, run with path_kernel=G over n assignments, against `base`, the same call with path_kernel=None."""
    groups = -(-n // G)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype and r.array.shape == base.array.shape, what
    assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the unfused run"
    assert r.macs == base.macs and r.n_slices == base.n_slices == n, what
    assert r.path_launches == (groups, groups) and base.path_launches == (0, 0), what
    assert r.launches == 2 * groups, what
    assert r.kernel_launches == (0,) * len(ctr.KERNEL_PATHS) and r.row_kernel_launches == (0, 0, 0), what
    assert r.batch_launches == 0 and r.narrow_launches == 0 and r.split_launches == 0, what
    assert r.path_kernel == min(G, n) and base.path_kernel is None, what
    assert sum(base.kernel_launches) == base.launches > r.launches, what


def run_all_groups(ctr, chain, arrays, what, groups=pc.GROUPS, **kw):
    call = lambda **more: ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, **kw, **more)  # noqa: E731
    base = call()
    for G in groups:
        assert_fused_equals(ctr, base, call(path_kernel=G), G, N, f"{what} G = {G}")
    return base


def assert_classes(ctr, chain, base):
    """The unfused run took the kernel paths the case is named after, once per assignment each."""
    k = dict(zip(ctr.KERNEL_PATHS, base.kernel_launches))
    got = dict(tiled=sum(v for name, v in k.items() if name.startswith("tiled")), dot=k["dot"], stream=k["stream"])
    want = dict(tiled=0, dot=0, stream=0)
    for name in chain.classes:
        want[name] += N
    assert got == want, f"{chain.name}: launches {k}"


def assert_einsum(chain, arrays, r, dtype, what):
    ref, mag = pc.einsum_reference(chain, arrays)
    got = r.array.transpose([r.inds.index(x) for x in chain.output])
    (_, _, k1), (_, _, k2) = chain.steps()
    kt = k1 + k2 + chain.summed
    u = float(np.finfo(dtype).eps) / 2
    bound = ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * u * mag
    err = np.abs(got.astype(ref.dtype) - ref)
    print(f"{what}: largest error / bound {float((err / bound).max()):.4f} (kt {kt})")
    assert got.shape == ref.shape and (err <= bound).all(), what


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("chain", pc.CASES, ids=[c.name for c in pc.CASES])
def test_every_shape_class_as_stored_and_as_output_step(ctr, chain, dtype):
    arrays = pc.fill(chain, dtype, seed=71)
    what = f"{chain.name} {np.dtype(dtype).name}"
    base = run_all_groups(ctr, chain, arrays, what)
    assert_classes(ctr, chain, base)
    assert base.array.dtype == np.dtype(dtype)
    assert_einsum(chain, arrays, base, dtype, what)


def test_the_permuted_case_moves_an_intermediate_inside_the_arena(ctr):
    chain = next(c for c in pc.CASES if c.name == "permuted-intermediate")
    p = ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES, dtype=np.float32, path_kernel=5)
    moved = [(int(r[0]), int(r[2]), int(r[6])) for r in p.perms]
    assert (ctr.ARENA, ctr.ARENA, 1) in moved and (ctr.LEAF, ctr.ARENA, -1) in moved, moved
    batch = next(c for c in pc.CASES if c.name == "batch-h3")
    q = ctr.plan(pc.PATH, batch.ts, batch.shapes(), batch.output, slices=pc.SLICES, dtype=np.float32)
    assert [op["H"] for op in q.ops] == [3, 3]


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_a_range_that_starts_off_a_multiple_of_the_group(ctr, dtype):
    chain = pc.SMALL
    arrays = pc.fill(chain, dtype, 72)
    call = lambda **more: ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, slice_range=(1, 11),  # noqa: E731
                                       **more)
    base = call()
    for G in (4, 3, 1024):  # groups 1..4, 5..8, 9..10; 1..3, 4..6, 7..9, 10; 1..10
        r = call(path_kernel=G)
        assert_fused_equals(ctr, base, r, G, 10, f"slice_range (1, 11) G = {G}")
    assert call(path_kernel=4).path_launches == (3, 3)
    whole = ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES)
    assert not np.array_equal(bits(whole.array), bits(base.array))  # (assignments 0 and 11 are missing from the range)


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_three_assignments_in_groups_of_two_and_four(ctr, dtype):
    """A last group of one member, and a group larger than the range; the range (3, 6) holds the last assignment of block
    p = 0 and the first two of p = 1."""
    chain = pc.SMALL
    arrays = pc.fill(chain, dtype, 78)
    call = lambda **more: ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, slice_range=(3, 6),  # noqa: E731
                                       **more)
    base = call()
    for G in (2, 4):
        assert_fused_equals(ctr, base, call(path_kernel=G), G, 3, f"slice_range (3, 6) G = {G}")


@pytest.mark.parametrize("chain", [pc.SUMMED, pc.PLACED], ids=["one_block", "a_block_per_assignment"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_members_that_all_share_a_block_and_members_that_never_do(ctr, chain, dtype):
    arrays = pc.fill(chain, dtype, seed=73)
    what = f"{chain.name} {np.dtype(dtype).name}"
    base = run_all_groups(ctr, chain, arrays, what)
    p = ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES, dtype=dtype)
    assert len(p.block_inds) == (0 if chain.variant == "summed" else 3)
    assert_einsum(chain, arrays, base, dtype, what)


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=DTYPE_IDS)
def test_two_calls_are_byte_equal(ctr, dtype):
    chain = pc.CASES[5]  # (a dot step, whose tree runs in LDS, and a stream step)
    arrays = pc.fill(chain, dtype, seed=74)
    a, b = (ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, path_kernel=5) for _ in range(2))
    assert np.array_equal(bits(a.array), bits(b.array)) and a.array.any() and np.isfinite(a.array).all()
    assert a.path_launches == b.path_launches == (3, 3)


def test_a_single_leaf_plan_takes_the_keyword_and_runs_as_before(ctr):
    rng = np.random.RandomState(75)
    a = (rng.uniform(0.5, 1.5, (5, 3, 7)) + 1j * rng.uniform(0.5, 1.5, (5, 3, 7))).astype(np.complex64)
    base = ctr.contract([], [("i", "s", "j")], [a], slices=("s",))
    r = ctr.contract([], [("i", "s", "j")], [a], slices=("s",), path_kernel=2)
    assert np.array_equal(bits(r.array), bits(base.array)) and r.inds == base.inds
    assert r.kernel_launches == base.kernel_launches and r.launches == base.launches == 3
    assert r.path_launches == (0, 0) and r.path_kernel == 1
    assert r.peak_device_bytes == base.peak_device_bytes


def test_peak_device_bytes_counts_what_the_path_kernel_reserves(ctr):
    chain = pc.SMALL
    arrays = pc.fill(chain, np.float32, 76)
    call = lambda **more: ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, **more)  # noqa: E731
    base, r = call(), call(path_kernel=5)
    p0 = ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES, dtype=np.float32)
    p5 = ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES, dtype=np.float32, path_kernel=5)
    # the library and the plan count the same growth (their totals differ by the padding of leaves and tables)
    assert r.peak_device_bytes - base.peak_device_bytes == p5.peak_device_bytes - p0.peak_device_bytes > 0


def test_contract_refuses_before_the_device_is_touched(ctr):
    chain = pc.SMALL
    arrays = pc.fill(chain, np.float32, 77)
    call = lambda **kw: ctr.contract(pc.PATH, chain.ts, arrays, chain.output, slices=pc.SLICES, **kw)  # noqa: E731
    for bad in (0, 1025, -1, 2.0, "8", True):
        with pytest.raises(ValueError, match=r"'path_kernel' must be None or an integer from 1 to 1024\."):
            call(path_kernel=bad)
    with pytest.raises(ValueError, match="'path_kernel' and 'slice_batch' are exclusive"):
        call(path_kernel=4, slice_batch=4)
    with pytest.raises(NotImplementedError, match="'storage' is not supported with 'path_kernel'"):
        call(path_kernel=4, storage="bfloat16")
    with pytest.raises(NotImplementedError, match="'compute' is not supported with 'path_kernel'"):
        call(path_kernel=4, compute="bf16x3")
    big = [np.ones((257, 256), np.float32), np.ones((256, 256), np.float32)]
    with pytest.raises(ValueError, match=r"step 0 .*more than 2\^24 multiply-adds"):
        ctr.contract([(0, 1)], [("i", "k"), ("k", "j")], big, path_kernel=1)


def test_the_setter_refuses_what_the_kernel_does_not_take(ctr):
    """Through the ABI: row axes, a storage dtype, a slice batch, a compute mode, a step beyond the cap and a group out of
    range are EINVAL; a handle that took the call refuses a slice batch and a compute mode."""
    from tnco_amd import _lib
    L = _lib.load()
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    rows = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, sparse_inds=("a", "b"),
                    projs=np.array([[0, 1], [1, 1], [1, 0]]))
    plain = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32)
    half = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, storage="bfloat16")
    over = ctr.plan([(0, 1)], [("i", "k"), ("k", "j")], [(257, 256), (256, 256)], dtype=np.float32)
    edge = ctr.plan([(0, 1)], [("i", "k"), ("k", "j")], [(256, 256), (256, 256)], dtype=np.float32)

    def with_handle(p, body):
        d, keep = ctr._describe(p, 0)
        h = C.c_void_p()
        _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
        try:
            body(h)
        finally:
            L.tnco_hip_contract_destroy(h)
        del keep

    def set_path(h, group):
        return L.tnco_hip_contract_set_path_kernel(h, group)

    def refuses(h):
        assert set_path(h, 1) == _lib.EINVAL and set_path(h, 4) == _lib.EINVAL
    with_handle(rows, refuses)
    with_handle(half, refuses)

    def over_cap(h):
        assert set_path(h, 1) == _lib.EINVAL and b"step 0" in L.tnco_hip_last_error()
    with_handle(over, over_cap)

    def takes(h):  # (a step of exactly 2^24 multiply-adds)
        assert set_path(h, 1) == _lib.OK
    with_handle(edge, takes)

    def values(h):
        for group in (0, 1025, -1):
            assert set_path(h, group) == _lib.EINVAL, group
        counts = np.full(2, -1, np.int64)
        assert L.tnco_hip_contract_path_launches(h, counts.ctypes.data_as(C.c_void_p)) == _lib.OK and not counts.any()
        assert L.tnco_hip_contract_path_launches(h, None) == _lib.EINVAL
        assert set_path(h, 1024) == _lib.OK
        assert L.tnco_hip_contract_set_slice_batch(h, 4) == _lib.EINVAL
        assert L.tnco_hip_contract_set_compute(h, 1) == _lib.EINVAL
    with_handle(plain, values)

    def after_batch(h):
        assert L.tnco_hip_contract_set_slice_batch(h, 4) == _lib.OK and set_path(h, 4) == _lib.EINVAL
    with_handle(plain, after_batch)

    def after_compute(h):
        assert L.tnco_hip_contract_set_compute(h, 1) == _lib.OK and set_path(h, 4) == _lib.EINVAL
    with_handle(plain, after_compute)
    assert set_path(None, 4) == _lib.EINVAL
