"""The host side of the storage mode of tnco_amd.contraction (`storage="float16" | "bfloat16"`), no GPU: the plan is the
plan of the compute dtype with another memory count, the refusals come before any device use, and the bfloat16 rounding
helper is held to an exact integer restatement of round-to-nearest-even."""
import dataclasses

import numpy as np
import pytest

from tests import half_cases as hc
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn

STORAGES = ("float16", "bfloat16")


def _network(seed, n=14):
    ts, d, o = syn.random_regular_tn(n, seed=seed)
    dims = {x: (d[x] if isinstance(d, dict) else d) for xs in ts for x in xs}
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    path = [(0, 1)] * (len(ts) - 1)
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    return path, ts, shapes, o, every


def _same_tables(p, q):
    assert np.array_equal(p.steps, q.steps) and np.array_equal(p.perms, q.perms)
    assert np.array_equal(p.leaf_sl, q.leaf_sl) and np.array_equal(p.leaf_numel, q.leaf_numel)
    assert repr(p.ops) == repr(q.ops)
    for f in ("dtype", "inds", "shape", "slice_inds", "slice_dims", "block_inds", "arena_elems", "out_numel",
              "macs_per_slice", "slice_range"):
        assert getattr(p, f) == getattr(q, f), f


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("seed", range(3))
def test_a_storage_plan_has_the_steps_of_the_plain_plan_and_counts_memory_at_the_storage_size(seed, storage, dtype):
    path, ts, shapes, o, every = _network(seed)
    cut = every[:seed]
    plain = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype)
    p = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, storage=storage)
    assert p.storage == storage and plain.storage is None
    _same_tables(p, plain)
    item = np.dtype(dtype).itemsize
    tables = 8 * (p.leaf_sl.size + p.perms.size + 2 * p.leaf_numel.size)
    assert p.peak_device_bytes == (item // 2) * (int(p.leaf_numel.sum()) + p.arena_elems) + item * p.out_numel + tables
    assert plain.peak_device_bytes == item * (int(p.leaf_numel.sum()) + p.arena_elems + p.out_numel) + tables
    assert p.peak_device_bytes < plain.peak_device_bytes
    ctr.check_memory(p, p.peak_device_bytes)
    with pytest.raises(RuntimeError, match="bytes of device memory"):
        ctr.check_memory(p, p.peak_device_bytes - 1)
    ctr.check_memory(p, plain.peak_device_bytes - 1)


@pytest.mark.parametrize("seed", range(3))
def test_storage_none_is_the_plan_built_without_the_keyword(seed):
    path, ts, shapes, o, every = _network(seed)
    for dtype in (np.float32, np.float64, np.complex64, np.complex128):
        a = ctr.plan(path, ts, shapes, o, slices=every[:2], dtype=dtype)
        b = ctr.plan(path, ts, shapes, o, slices=every[:2], dtype=dtype, storage=None)
        assert [f.name for f in dataclasses.fields(a)] == [f.name for f in dataclasses.fields(b)]
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and np.array_equal(x, y), f.name
            else:
                assert repr(x) == repr(y), f.name
        assert a.peak_device_bytes == b.peak_device_bytes and b.storage is None


def test_the_cases_of_the_gpu_test_plan_as_their_table_says():
    for case in hc.CASES:
        for dtype in (np.float32, np.complex64):
            p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, slices=case.slices, dtype=dtype,
                         storage="bfloat16")
            (op,) = p.ops
            assert {k: op[k] for k in ("H", "M", "N", "K", "form_a", "form_b")} == \
                {k: case.ops[k] for k in ("H", "M", "N", "K", "form_a", "form_b")}, case.name
            assert len(p.perms) == case.ops["perms"], case.name
            tiled = op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32  # the dispatch rule of csrc/contract.hip
            assert tiled == any(k.startswith("tiled") for k in case.kernels), case.name


def test_refusals_before_any_device_use(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts = [("a", "b"), ("b", "c")]
    f32 = [np.ones((2, 3), np.float32), np.ones((3, 4), np.float32)]
    for storage in STORAGES:
        for wide in (np.float64, np.complex128):
            with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
                ctr.contract([(0, 1)], ts, [f32[0], f32[1].astype(wide)], storage=storage)
            with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
                ctr.plan([(0, 1)], ts, [(2, 3), (3, 4)], dtype=wide, storage=storage)
        with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
            ctr.plan([(0, 1)], ts, [(2, 3), (3, 4)], storage=storage)  # (plan's default dtype is float64)
        # float16 input arrays stay refused, with the keyword as without
        with pytest.raises(TypeError, match="dtype float16 is not supported"):
            ctr.contract([(0, 1)], ts, [f32[0].astype(np.float16), f32[1]], storage=storage)
        with pytest.raises(NotImplementedError, match="projections are not supported with 'storage'."):
            ctr.contract([(0, 1)], ts, f32, ("a", "c"), sparse_inds=("a",), projs=np.array([[0], [1]]), storage=storage)
        with pytest.raises(NotImplementedError, match="projections are not supported with 'storage'."):
            ctr.plan([(0, 1)], ts, [(2, 3), (3, 4)], ("a", "c"), dtype=np.float32, sparse_inds=("a",),
                     projs=np.array([[0]]), storage=storage)
    with pytest.raises(TypeError, match="dtype float16 is not supported"):
        ctr.contract([(0, 1)], ts, [f32[0].astype(np.float16), f32[1]])
    for name in ("float32", "fp16", "half", np.float16, 16):
        with pytest.raises(ValueError, match="'storage' must be None, 'float16' or 'bfloat16'."):
            ctr.contract([(0, 1)], ts, f32, storage=name)
        with pytest.raises(ValueError, match="'storage' must be None, 'float16' or 'bfloat16'."):
            ctr.plan([(0, 1)], ts, [(2, 3), (3, 4)], dtype=np.float32, storage=name)
    # a finite float32 that float16 does not hold: refused on the host (65520 is the first value that rounds to inf)
    for bad in (np.float32(65520.0), np.float32(-1e5), np.float32(3e38)):
        a = f32[0].copy()
        a[1, 2] = bad
        with pytest.raises(ValueError, match="finite values beyond the range of float16"):
            ctr.contract([(0, 1)], ts, [a, f32[1]], storage="float16")
        c = a.astype(np.complex64) * 1j
        with pytest.raises(ValueError, match="finite values beyond the range of float16"):
            ctr.contract([(0, 1)], ts, [c, f32[1]], storage="float16")
    # ... and the one float32 binade top that bfloat16 rounds to inf
    a = f32[0].copy()
    a[0, 0] = np.finfo(np.float32).max
    with pytest.raises(ValueError, match="finite values beyond the range of bfloat16"):
        ctr.contract([(0, 1)], ts, [a, f32[1]], storage="bfloat16")
    # what is in range reaches the device (here: the stand-in for it); inf and NaN are values, not overflows
    a[0, 0], a[0, 1] = np.inf, np.nan
    a[1, 0] = 65519.0
    for storage in STORAGES:
        with pytest.raises(AssertionError, match="the device was reached"):
            ctr.contract([(0, 1)], ts, [a, f32[1]], storage=storage)


def _bf16_exact(u: int) -> int:
    """Round-to-nearest-even of the float32 with bits u to bfloat16, in integers: the candidates are the 16 upper bits
    and their successor; the remainder against half a unit decides, a tie goes to the even candidate."""
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return -1  # NaN: any NaN
    down, rem = u >> 16, u & 0xFFFF
    if rem > 0x8000 or (rem == 0x8000 and down & 1):
        return down + 1  # (a carry out of the mantissa raises the exponent; out of the largest exponent it gives inf)
    return down


@pytest.mark.parametrize("upper", [0x3F80, 0x3F81, 0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x3FFF, 0xBFFF, 0x7F7F, 0xFF7F,
                                   0x7EFF, 0x4049])
def test_bfloat16_rounding_is_nearest_even_on_every_lower_half(upper):
    u = (np.uint32(upper) << np.uint32(16)) | np.arange(1 << 16, dtype=np.uint32)
    got = ctr._bf16_bits(u.view(np.float32))
    assert got.dtype == np.uint16 and got.shape == u.shape
    want = np.array([_bf16_exact(int(v)) for v in u], np.int64)
    assert np.array_equal(got.astype(np.int64), want)
    assert (got[u & 0xFFFF == 0] == upper).all()  # (what bfloat16 holds is left alone)


def test_bfloat16_rounding_special_values():
    f = lambda *bits: ctr._bf16_bits(np.array(bits, np.uint32).view(np.float32)).tolist()  # noqa: E731
    assert f(0x00000000, 0x80000000) == [0x0000, 0x8000]  # +-0
    assert f(0x7F800000, 0xFF800000) == [0x7F80, 0xFF80]  # +-inf
    # ties: to the even neighbour, up and down; one bit off a tie: to the nearer
    assert f(0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF) == [0x3F80, 0x3F82, 0x3F81, 0x3F81]
    # a carry into the exponent, and out of the largest one
    assert f(0x3FFF8000, 0x3FFFFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF) == [0x4000, 0x4000, 0x7F80, 0x7F7F, 0xFF80]
    # the smallest subnormals: 2^-149 rounds to zero, half of bfloat16's smallest is a tie to zero, above it rounds up
    assert f(0x00000001, 0x00008000, 0x00008001, 0x00018000) == [0x0000, 0x0000, 0x0001, 0x0002]
    # NaN stays NaN, whatever its payload (also one whose upper half alone would read as inf)
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF80FFFF, 0x7FFFFFFF, 0xFFFFFFFF):
        (r,) = f(bits)
        assert r & 0x7F80 == 0x7F80 and r & 0x007F != 0 and r >> 15 == bits >> 31, hex(bits)


def test_round_to_storage_is_numpys_float16_and_the_bfloat16_helper():
    rng = np.random.RandomState(5)
    x = (rng.standard_normal(4000) * 2.0 ** rng.uniform(-12, 12, 4000)).astype(np.float32)
    assert np.array_equal(ctr.round_to_storage(x, "float16"), x.astype(np.float16).astype(np.float32))
    b = ctr.round_to_storage(x, "bfloat16")
    assert np.array_equal(b.view(np.uint32), ctr._bf16_bits(x).astype(np.uint32) << 16)
    assert (np.abs(b - x) <= 2.0 ** -8 * np.abs(x)).all()
    z = (x[:2000] + 1j * x[2000:]).astype(np.complex64).reshape(40, 50)
    for storage in STORAGES:
        r = ctr.round_to_storage(z, storage)
        assert r.dtype == np.complex64 and r.shape == z.shape
        assert np.array_equal(r.real, ctr.round_to_storage(z.real.copy(), storage).reshape(z.shape))
        assert np.array_equal(r.imag, ctr.round_to_storage(z.imag.copy(), storage).reshape(z.shape))
        # the device layout: interleaved (re, im) pairs of storage values
        bits = ctr._storage_bits(z, storage)
        assert bits.dtype == np.uint16 and bits.shape == z.shape + (2,) and bits.flags.c_contiguous
        assert np.array_equal(bits[..., 0], ctr._storage_bits(z.real.copy(), storage))
        assert np.array_equal(bits[..., 1], ctr._storage_bits(z.imag.copy(), storage))
    assert ctr.round_to_storage(np.float32(1.0009765625), "float16") == np.float32(1.0009765625)
    assert ctr.round_to_storage(np.complex64(3 + 1j), "bfloat16").shape == ()


def test_tensors_the_path_leaves_alone_are_rounded_and_intermediates_saturate(monkeypatch):
    """A path that leaves several tensors returns an untouched one as the single-leaf plan would: rounded to storage
    (no device involved); its overflow is refused like any leaf's.  An array marked as the result of an earlier
    storage-mode call (contract_results: a component's result entering the call that joins the components) is an
    intermediate: beyond the range it becomes inf and goes on to the device."""
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    rng = np.random.RandomState(9)
    ts = [("a", "b"), ("c",)]
    x = rng.standard_normal((3, 4)).astype(np.float32)
    y = (rng.standard_normal(5) + 1j * rng.standard_normal(5)).astype(np.complex64)
    for storage in STORAGES:
        r = ctr.contract([], ts, [x, y], storage=storage)
        assert [tuple(i) for i in r.inds] == ts and r.macs == 0
        assert np.array_equal(r.array[0], ctr.round_to_storage(x.astype(np.complex64), storage))
        assert np.array_equal(r.array[1], ctr.round_to_storage(y, storage))
        assert not np.array_equal(r.array[1], y)
    plain = ctr.contract([], ts, [x, y])
    assert np.array_equal(plain.array[1], y)
    big = x.copy()
    big[0, 0] = 1e5
    with pytest.raises(ValueError, match="finite values beyond the range of float16"):
        ctr.contract([], ts, [big, y], storage="float16")
    r = ctr.contract([], ts, [big, y], storage="float16", _intermediates=[0])
    assert np.isinf(r.array[0][0, 0]) and np.isfinite(r.array[0].ravel()[1:]).all()
    # ... and on the way to the device
    pair = [("a", "b"), ("b",)]
    v = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="finite values beyond the range of float16"):
        ctr.contract([(0, 1)], pair, [big, v], storage="float16")
    with pytest.raises(AssertionError, match="the device was reached"):
        ctr.contract([(0, 1)], pair, [big, v], storage="float16", _intermediates=[0])
    assert np.isinf(ctr._storage_bits(big, "float16", check=False).view(np.float16)[0, 0])
    assert ctr._storage_bits(np.float32(3.4e38), "bfloat16", check=False) == 0x7F80
