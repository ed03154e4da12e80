"""The host side of per-tensor scaling (`scaling="tensor"`, tnco_amd.contraction), no GPU: the keyword's refusals, the
plan's exponent slots and staging buffers, and `scale_to_storage` held to an integer restatement of the rule."""
import dataclasses
from fractions import Fraction

import numpy as np
import pytest

from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn

STORAGES = ("float16", "bfloat16")


def _network(seed, n=14):
    ts, d, o = syn.random_regular_tn(n, seed=seed)
    dims = {x: (d[x] if isinstance(d, dict) else d) for xs in ts for x in xs}
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    return [(0, 1)] * (len(ts) - 1), ts, shapes, o, every


def test_refusals_and_their_precedence(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts = [("a", "b"), ("b", "c")]
    shapes = [(2, 3), (3, 4)]
    f32 = [np.ones(s, np.float32) for s in shapes]
    with pytest.raises(ValueError, match="'scaling' needs 'storage'."):
        ctr.contract([(0, 1)], ts, f32, scaling="tensor")
    with pytest.raises(ValueError, match="'scaling' needs 'storage'."):
        ctr.plan([(0, 1)], ts, shapes, dtype=np.float32, scaling="tensor")
    with pytest.raises(ValueError, match="'scaling' needs 'storage'."):
        ctr.contract_results(None, f32, None, None, scaling="tensor")
    for bad in ("row", "block", "Tensor", True, 1, ("tensor",)):
        for storage in (None,) + STORAGES:
            with pytest.raises(ValueError, match="'scaling' must be None or 'tensor'."):
                ctr.contract([(0, 1)], ts, f32, storage=storage, scaling=bad)
            with pytest.raises(ValueError, match="'scaling' must be None or 'tensor'."):
                ctr.plan([(0, 1)], ts, shapes, dtype=np.float32, storage=storage, scaling=bad)
        with pytest.raises(ValueError, match="'scaling' must be None or 'tensor'."):
            ctr.contract_results(None, f32, None, None, storage="float16", scaling=bad)
    # every refusal of storage mode keeps its text and comes first
    for storage in STORAGES:
        for wide in (np.float64, np.complex128):
            with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
                ctr.contract([(0, 1)], ts, [f32[0], f32[1].astype(wide)], storage=storage, scaling="tensor")
            with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
                ctr.plan([(0, 1)], ts, shapes, dtype=wide, storage=storage, scaling="tensor")
            with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
                ctr.plan([(0, 1)], ts, shapes, dtype=wide, storage=storage, scaling="nonsense")
        with pytest.raises(TypeError, match="dtype float16 is not supported"):
            ctr.contract([(0, 1)], ts, [f32[0].astype(np.float16), f32[1]], storage=storage, scaling="tensor")
        with pytest.raises(NotImplementedError, match="projections are not supported with 'storage'."):
            ctr.contract([(0, 1)], ts, f32, ("a", "c"), sparse_inds=("a",), projs=np.array([[0], [1]]), storage=storage,
                         scaling="tensor")
        with pytest.raises(NotImplementedError, match="projections are not supported with 'storage'."):
            ctr.plan([(0, 1)], ts, shapes, ("a", "c"), dtype=np.float32, sparse_inds=("a",), projs=np.array([[0]]),
                     storage=storage, scaling="tensor")
    with pytest.raises(ValueError, match="'storage' must be None, 'float16' or 'bfloat16'."):
        ctr.contract([(0, 1)], ts, f32, storage="half", scaling="tensor")
    with pytest.raises(TypeError, match="dtype float16 is not supported"):
        ctr.contract([(0, 1)], ts, [f32[0].astype(np.float16), f32[1]], scaling="tensor")
    # with scaling a finite leaf is never beyond the range: what storage mode alone refuses goes on to the device
    a = f32[0].copy()
    a[1, 2] = 3e38
    with pytest.raises(ValueError, match="finite values beyond the range of float16"):
        ctr.contract([(0, 1)], ts, [a, f32[1]], storage="float16")
    for storage in STORAGES:
        with pytest.raises(AssertionError, match="the device was reached"):
            ctr.contract([(0, 1)], ts, [a, f32[1]], storage=storage, scaling="tensor")


@pytest.mark.parametrize("seed", range(3))
def test_scaling_none_is_the_plan_built_without_the_keyword(seed):
    path, ts, shapes, o, every = _network(seed)
    for dtype, storage in ((np.float32, None), (np.complex128, None), (np.float32, "float16"), (np.complex64, "bfloat16")):
        a = ctr.plan(path, ts, shapes, o, slices=every[:2], dtype=dtype, storage=storage)
        b = ctr.plan(path, ts, shapes, o, slices=every[:2], dtype=dtype, storage=storage, scaling=None)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes() and x.shape == y.shape, f.name
            else:
                assert repr(x) == repr(y), f.name
        assert b.scaling is None and b.stage_refs is None and not b.steps[:, 14:].any()
        assert a.peak_device_bytes == b.peak_device_bytes


def test_exponent_slots_on_a_path_with_a_permuted_intermediate():
    """A (i, k) B (k, j) -> Z (i, j); Z C (i, l) -> Y (j, l): Z is read along i, which it holds outermost with j between
    -- no operand form of the step, so Z is permuted and keeps its slot; Y D (l, j) -> the output."""
    ts = [("i", "k"), ("k", "j"), ("i", "l", "m"), ("m", "l", "j")]
    shapes = [(8, 4), (4, 6), (8, 5, 3), (3, 5, 6)]
    path = [(0, 1), (0, 2), (0, 1)]
    plain = ctr.plan(path, ts, shapes, dtype=np.float32, storage="float16")
    p = ctr.plan(path, ts, shapes, dtype=np.float32, storage="float16", scaling="tensor")
    assert p.scaling == "tensor" and len(p.steps) == 3
    L = len(ts)
    # live tensors: [2, 3, Z] -> step 1 takes (leaf 2, Z) -> [3, Y] -> step 2 takes (leaf 3, Y)
    assert p.steps[:, 14:].tolist() == [[0, 1], [2, L + 0], [3, L + 1]]
    assert len(p.perms) > 0 and (p.perms[:, 0] == ctr.ARENA).any(), "the path was meant to permute an intermediate"
    # everything but the slots and the staging is the plan without scaling
    assert np.array_equal(p.steps[:, :14], plain.steps[:, :14]) and np.array_equal(p.perms, plain.perms)
    assert p.stage_refs.shape == (3,) and p.stage_refs[2] == -1 and (p.stage_refs[:2] >= 0).all()
    for k in range(2):  # staging: 2 numel storage elements, apart from the operands, the result and live buffers
        nc = int(np.prod(p.steps[k, 10:13]))
        lo, hi = p.stage_refs[k], p.stage_refs[k] + 2 * nc
        assert hi <= p.arena_elems and lo % ctr.ALIGN == 0
        spans = [(p.steps[k, 9], nc)]
        spans += [(p.steps[k, 4 * side + 1], int(p.steps[k, 10] * p.steps[k, 13] * p.steps[k, 12 - side]))
                  for side in (0, 1) if p.steps[k, 4 * side] == ctr.ARENA]
        for at, n in spans:
            assert hi <= at or at + n <= lo


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
@pytest.mark.parametrize("seed", range(3))
def test_staging_costs_memory_only_where_it_raises_the_peak(seed, dtype):
    path, ts, shapes, o, every = _network(seed, n=20)
    cut = every[:seed]
    plain = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, storage="float16")
    full = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype)
    p = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, storage="float16", scaling="tensor")
    stored = [int(np.prod(r[10:13])) for r in p.steps if r[8] == ctr.ARENA]
    assert stored
    align = lambda n: max(ctr.ALIGN, -(-n // ctr.ALIGN) * ctr.ALIGN)  # noqa: E731  (the arena's granule)
    assert plain.arena_elems <= p.arena_elems <= plain.arena_elems + align(2 * max(stored))
    if max(stored) % (ctr.ALIGN // 2) == 0:
        assert p.arena_elems <= plain.arena_elems + 2 * max(stored)
    n_slots = len(ts) + len(p.steps)
    item = np.dtype(dtype).itemsize
    assert p.peak_device_bytes == plain.peak_device_bytes + (item // 2) * (p.arena_elems - plain.arena_elems) + \
        4 * (n_slots + len(p.steps))
    # by arithmetic: leaves, arena and staging at half the size against everything at the full size --
    # below the plain plan's as soon as the staging and the exponent words are less than half of leaves + arena
    extra = (item // 2) * (p.arena_elems - plain.arena_elems) + 4 * (n_slots + len(p.steps))
    saved = (item // 2) * (int(p.leaf_numel.sum()) + plain.arena_elems)
    assert (p.peak_device_bytes < full.peak_device_bytes) == (extra < saved)
    ctr.check_memory(p, p.peak_device_bytes)
    with pytest.raises(RuntimeError, match="bytes of device memory"):
        ctr.check_memory(p, p.peak_device_bytes - 1)


def test_peak_stays_below_the_plain_plan_where_arithmetic_says_so():
    """Two large leaves, one small stored result: A (i, k) B (k, j) -> Z (i, j) with k long, then Z w (j).  Leaves
    2 x 64 x 4096 elements, Z 64 x 64: storage mode saves 2 bytes on each of 524288 leaf elements; staging adds
    2 x 4096 storage elements of 2 bytes and the exponents a few words."""
    ts, shapes = [("i", "k"), ("k", "j"), ("j",)], [(64, 4096), (4096, 64), (64,)]
    full = ctr.plan([(0, 1), (0, 1)], ts, shapes, dtype=np.float32)
    p = ctr.plan([(0, 1), (0, 1)], ts, shapes, dtype=np.float32, storage="float16", scaling="tensor")
    assert p.arena_elems == 4096 + 2 * 4096 and p.stage_refs.tolist() == [4096, -1]
    assert p.peak_device_bytes < full.peak_device_bytes
    assert full.peak_device_bytes - p.peak_device_bytes == 2 * (2 * 64 * 4096 + 64) + 4 * 4096 - 2 * (3 * 4096) - 4 * (5 + 2)


def _rule_exact(parts) -> int:
    """The rule in exact rational arithmetic on the values themselves."""
    finite = [abs(Fraction(float(v))) for v in parts if np.isfinite(v)]
    m = max(finite, default=Fraction(0))
    if m == 0:
        return 0
    lg = 0
    while Fraction(2) ** (lg + 1) <= m:
        lg += 1
    while Fraction(2) ** lg > m:
        lg -= 1
    return lg - 14


def _margins():
    out = []
    for b in (-149, -127, -126, -40, -1, 0, 14, 15, 16, 100, 127):
        for name, f in (("", Fraction(1)), ("+", 1 + Fraction(1, 2 ** 23)), ("-", 1 - Fraction(1, 2 ** 24)),
                        ("--", 1 - Fraction(1, 2 ** 23)), ("top", 2 - Fraction(1, 2 ** 23))):
            out.append(pytest.param(b, f, id=f"2^{b}{name}"))
    return out


@pytest.mark.parametrize("b,f", _margins())
@pytest.mark.parametrize("storage", STORAGES)
def test_scale_to_storage_at_the_margins_of_the_binades(storage, b, f):
    """m = 2^b, 2^b (1 +- 2^-23) and 2^b (2 - 2^-23), as float32 holds them (rounded to nearest where b is in the
    subnormal range; (1 - 2^-23) is two float32 steps below 2^b, (1 - 2^-24) the one step)."""
    with np.errstate(over="ignore", under="ignore"):
        m = np.float32(float(Fraction(2) ** b * f))
    if not np.isfinite(m) or m == 0:
        pytest.skip("not a float32")
    a = np.array([m * np.float32(0.25), -m, m * np.float32(0.5), 0.0], np.float32)
    values, e = ctr.scale_to_storage(a, storage)
    assert isinstance(e, int) and e == _rule_exact(a) == ctr.scale_exponent(a)
    _check_values(a, values, e, storage)
    z = np.array([complex(a[0], a[2]), complex(a[3], a[1])], np.complex64)  # the largest part is an imaginary one
    zv, ze = ctr.scale_to_storage(z, storage)
    assert ze == e and zv.dtype == np.complex64
    assert np.array_equal(zv.view(np.float32), values[[0, 2, 3, 1]], equal_nan=True)


def _check_values(a, values, e, storage):
    """values == ldexp(round(ldexp(a, -e)), e) exactly, and the largest stored magnitude is in [2^14, 2^15], finite."""
    assert values.dtype == a.dtype and values.shape == a.shape
    parts = a.reshape(-1).view(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        scaled = np.ldexp(parts, np.int32(-e)).astype(np.float32)
        stored = ctr.round_to_storage(scaled, storage)
        want = np.ldexp(stored, np.int32(e)).astype(np.float32)
    assert np.array_equal(values.reshape(-1).view(np.float32), want, equal_nan=True)
    finite = np.isfinite(parts)
    if finite.any() and np.abs(parts[finite]).max() > 0:
        top = np.abs(stored[finite]).max()
        assert 2.0 ** 14 <= top <= 2.0 ** 15 and np.isfinite(stored[finite]).all()
        assert np.isfinite(np.float16(top)) and top == np.float32(np.float16(top)) if storage == "float16" else True


@pytest.mark.parametrize("storage", STORAGES)
def test_scale_to_storage_zero_inf_and_complex(storage):
    values, e = ctr.scale_to_storage(np.zeros((3, 2), np.float32), storage)
    assert e == 0 and not values.any() and values.shape == (3, 2)
    values, e = ctr.scale_to_storage(np.array([np.inf, np.nan, -np.inf], np.float32), storage)
    assert e == 0 and np.isinf(values[[0, 2]]).all() and np.isnan(values[1])
    rng = np.random.RandomState(3)
    a = (rng.standard_normal(500) * 2.0 ** rng.uniform(-4, 4, 500) * 2.0 ** 60).astype(np.float32)
    e_finite = ctr.scale_to_storage(a, storage)[1]
    b = a.copy()
    b[17], b[18] = np.inf, np.nan
    values, e = ctr.scale_to_storage(b, storage)
    assert e == e_finite == _rule_exact(a) and np.isinf(values[17]) and np.isnan(values[18])
    _check_values(b, values, e, storage)
    keep = np.ones(500, bool)
    keep[17:19] = False
    assert np.array_equal(values[keep], ctr.scale_to_storage(a, storage)[0][keep])
    # complex parts are treated jointly: one exponent, from the larger part wherever it is
    z = (a[:250] * np.float32(2.0 ** -30) + 1j * a[250:]).astype(np.complex64).reshape(10, 25)
    zv, ze = ctr.scale_to_storage(z, storage)
    assert ze == _rule_exact(np.concatenate([z.real.ravel(), z.imag.ravel()])) == ctr.scale_to_storage(z.imag.copy(), storage)[1]
    assert zv.shape == z.shape and zv.dtype == np.complex64
    _check_values(z, zv, ze, storage)
    assert np.array_equal(zv.imag, ctr.scale_to_storage(z.imag.copy(), storage)[0])
    u = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[storage]
    assert (np.abs(zv.imag - z.imag) <= u * np.abs(z.imag)).all()
    # round_to_storage stays as it is: it refuses what scaling takes
    with pytest.raises(ValueError, match="finite values beyond the range of float16"):
        ctr.round_to_storage(a, "float16")
    for bad in (None, "half"):
        with pytest.raises(ValueError, match="'storage' must be"):
            ctr.scale_to_storage(a, bad)
    with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
        ctr.scale_to_storage(a.astype(np.float64), storage)
