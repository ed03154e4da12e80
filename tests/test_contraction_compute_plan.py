"""The host side of the compute mode of tnco_amd.contraction (`compute="bf16x3"`), no GPU: the plan is the plan of
`compute=None` table for table and byte for byte of memory, the refusals come before any device use and in a fixed
precedence, a leaf beyond the range of the split is refused, and the numpy split helper (`contraction.split_bf16`) is held
to an integer restatement of round-to-nearest-even on every lower half of chosen upper halves."""
import numpy as np
import pytest

from tests import split_cases as sc
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn


def _network(seed, n=14):
    ts, d, o = syn.random_regular_tn(n, seed=seed)
    dims = {x: (d[x] if isinstance(d, dict) else d) for xs in ts for x in xs}
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    path = [(0, 1)] * (len(ts) - 1)
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    return path, ts, shapes, o, every


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
@pytest.mark.parametrize("batch", [None, 3])
@pytest.mark.parametrize("seed", range(3))
def test_the_plan_is_the_plain_plan_byte_for_byte(seed, batch, dtype):
    path, ts, shapes, o, every = _network(seed)
    cut = every[:seed]
    plain = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, slice_batch=batch)
    p = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, slice_batch=batch, compute="bf16x3")
    assert p.compute == "bf16x3" and plain.compute is None and p.storage is None
    for f in ("steps", "perms", "leaf_sl", "leaf_numel"):
        x, y = getattr(p, f), getattr(plain, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert repr(p.ops) == repr(plain.ops)
    for f in ("dtype", "inds", "shape", "slice_inds", "slice_dims", "block_inds", "arena_elems", "out_numel",
              "macs_per_slice", "slice_range", "slice_batch", "scaling", "stage_refs", "row_steps"):
        assert getattr(p, f) == getattr(plain, f), f
    assert p.peak_device_bytes == plain.peak_device_bytes


def test_the_cases_of_the_gpu_test_plan_as_their_table_says():
    for case in sc.CASES:
        for dtype in (np.float32, np.complex64):
            p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, slices=case.slices, dtype=dtype, compute="bf16x3")
            (op,) = p.ops
            assert {k: op[k] for k in ("H", "M", "N", "K", "form_a", "form_b")} == \
                {k: case.ops[k] for k in ("H", "M", "N", "K", "form_a", "form_b")}, case.name
            assert len(p.perms) == case.ops["perms"], case.name
            tiled = op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32  # the dispatch rule of csrc/contract.hip
            assert tiled == any(k.startswith("tiled") for k in case.kernels), case.name
            assert tiled == (sc.split_launches(case) > 0), case.name


def test_a_plan_without_steps_takes_the_keyword():
    p = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), dtype=np.complex64, compute="bf16x3")
    q = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), dtype=np.complex64)
    assert p.compute == "bf16x3" and len(p.steps) == 0 and p.perms.tobytes() == q.perms.tobytes()
    assert p.peak_device_bytes == q.peak_device_bytes


def test_refusals_before_any_device_use_and_their_precedence(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts, shapes = [("a", "b"), ("b", "c")], [(2, 3), (3, 4)]
    f32 = [np.ones(s, np.float32) for s in shapes]
    f64 = [a.astype(np.float64) for a in f32]
    projs = dict(output_inds=("a", "c"), sparse_inds=("a",), projs=np.array([[0], [1]]))
    unknown = "'compute' must be None or 'bf16x3'."
    exclusive = "'compute' and 'storage' are exclusive."
    wide = "with 'compute' the compute dtype must be float32 or complex64"
    no_projs = "projections are not supported with 'compute'."
    # 1. an unknown value, whatever else is wrong with the call
    for name in ("bf16", "bf16x6", "tf32", "BF16X3", 3, np.float32, True):
        for kw in (dict(), dict(storage="bfloat16"), projs):
            for arrays in (f32, f64):
                with pytest.raises(ValueError, match=unknown):
                    ctr.contract([(0, 1)], ts, arrays, compute=name, **kw)
        with pytest.raises(ValueError, match=unknown):
            ctr.plan([(0, 1)], ts, shapes, compute=name, storage="float16")
    # 2. with storage, before the dtype and the projections are looked at
    for storage in ("float16", "bfloat16"):
        for arrays in (f32, f64):
            for kw in (dict(), projs):
                with pytest.raises(ValueError, match=exclusive):
                    ctr.contract([(0, 1)], ts, arrays, compute="bf16x3", storage=storage, **kw)
        with pytest.raises(ValueError, match=exclusive):
            ctr.plan([(0, 1)], ts, shapes, compute="bf16x3", storage=storage, scaling="tensor")
    # 3. double precision, before the projections
    for dtype in (np.float64, np.complex128):
        for kw in (dict(), projs):
            with pytest.raises(TypeError, match=wide):
                ctr.contract([(0, 1)], ts, [f32[0], f32[1].astype(dtype)], compute="bf16x3", **kw)
        with pytest.raises(TypeError, match=wide):
            ctr.plan([(0, 1)], ts, shapes, dtype=dtype, compute="bf16x3")
    with pytest.raises(TypeError, match=wide):
        ctr.plan([(0, 1)], ts, shapes, compute="bf16x3")  # (plan's default dtype is float64)
    # 4. projections
    with pytest.raises(NotImplementedError, match=no_projs):
        ctr.contract([(0, 1)], ts, f32, compute="bf16x3", **projs)
    with pytest.raises(NotImplementedError, match=no_projs):
        ctr.plan([(0, 1)], ts, shapes, dtype=np.complex64, compute="bf16x3", **projs)
    # the keyword at None changes nothing about the other refusals
    with pytest.raises(TypeError, match="with 'storage' the compute dtype must be float32 or complex64"):
        ctr.contract([(0, 1)], ts, f64, storage="float16", compute=None)


def test_a_leaf_beyond_the_range_of_the_split_is_refused_on_the_host(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts = [("a", "b"), ("b", "c")]
    f32 = [np.ones((2, 3), np.float32), np.ones((3, 4), np.float32)]
    first = np.array(0x7F7F8000, np.uint32).view(np.float32)  # 2^128 - 2^119: the first value whose hi is inf (a tie, to even)
    assert float(first) == 2.0 ** 128 - 2.0 ** 119
    for bad in (first, -first, np.float32(np.finfo(np.float32).max)):
        for cplx in (False, True):
            a = f32[0].astype(np.complex64) if cplx else f32[0].copy()
            a[1, 2] = 1j * bad if cplx else bad
            with pytest.raises(ValueError, match="finite values beyond the range of the bfloat16 split"):
                ctr.contract([(0, 1)], ts, [a, f32[1]], compute="bf16x3")
            with pytest.raises(ValueError, match="finite values beyond the range of the bfloat16 split"):
                ctr.contract([], [("a", "b")], [a], compute="bf16x3")
    # the value just below it, inf and NaN pass the host (and reach for the device)
    below = np.array(0x7F7F7FFF, np.uint32).view(np.float32)
    for fine in (below, np.float32(np.inf), np.float32(np.nan)):
        a = f32[0].copy()
        a[0, 0] = fine
        with pytest.raises(AssertionError, match="the device was reached"):
            ctr.contract([(0, 1)], ts, [a, f32[1]], compute="bf16x3")


def _split_by_integers(u):
    """(bits of hi, bits of lo, x - hi exact?) of the float32 patterns u (uint32), in Python-width integers and exact
    float64 arithmetic: round to nearest even on the pattern, the rest taken in float64 (where float32 - float32 of
    these magnitudes is exact) and required to be a float32."""
    u = u.astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    low, up = u & 0xFFFF, u >> 16
    round_up = (low > 0x8000) | ((low == 0x8000) & ((up & 1) == 1))
    hi = np.where(nan, up | 0x40, up + round_up).astype(np.uint32)
    x = u.astype(np.uint32).view(np.float32).astype(np.float64)
    hf = (hi << np.uint32(16)).view(np.float32).astype(np.float64)
    finite = (hi & 0x7F80) != 0x7F80
    with np.errstate(invalid="ignore"):
        rest = np.where(finite, x - hf, 0.0)
    exact = rest.astype(np.float32).astype(np.float64) == rest
    v = rest.astype(np.float32).view(np.uint32).astype(np.uint64)
    low, up = v & 0xFFFF, v >> 16
    lo = (up + ((low > 0x8000) | ((low == 0x8000) & ((up & 1) == 1)))).astype(np.uint32)
    return hi, lo, exact


# upper halves: 1.0, an odd and an even last kept bit, negative, a large and a small exponent, the smallest normal, a
# subnormal, zero, the last finite upper half (its upper lower-halves round to inf), inf, a NaN
UPPER = (0x3F80, 0x3F81, 0x3F82, 0xBF81, 0x7149, 0x0DB0, 0x0080, 0x0001, 0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x7F80, 0x7FC1)


@pytest.mark.parametrize("upper", UPPER, ids=[f"{u:04x}" for u in UPPER])
def test_split_bf16_is_round_to_nearest_even_twice_with_an_exact_rest(upper):
    u = (np.uint32(upper) << np.uint32(16)) | np.arange(1 << 16, dtype=np.uint32)
    x = u.view(np.float32)
    hi, lo = ctr.split_bf16(x)
    assert hi.dtype == lo.dtype == np.float32 and hi.shape == lo.shape == x.shape
    want_hi, want_lo, exact = _split_by_integers(u)
    assert exact.all()  # x - hi is a float32
    hb, lb = hi.view(np.uint32), lo.view(np.uint32)
    assert not (hb & 0xFFFF).any() and not (lb & 0xFFFF).any()  # both are bfloat16 values
    nan = np.isnan(x)
    assert np.array_equal(hb[~nan] >> 16, want_hi[~nan]) and np.isnan(hi[nan]).all()
    assert np.array_equal(lb >> 16, want_lo)
    finite = np.isfinite(hi)
    assert not lo[~finite].any()  # lo is 0 where hi is not finite
    # what the split keeps: |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-16 |x| wherever lo is normal
    normal = finite & (np.abs(x) >= 2.0 ** -100)
    x64, h64, l64 = (q[normal].astype(np.float64) for q in (x, hi, lo))
    assert (np.abs(x64 - h64) <= 2.0 ** -8 * np.abs(x64)).all()
    assert (np.abs(x64 - h64 - l64) <= 2.0 ** -16 * np.abs(x64)).all()


def test_split_bf16_of_a_complex_array_splits_both_parts():
    rng = np.random.RandomState(3)
    z = (rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))).astype(np.complex64)
    hi, lo = ctr.split_bf16(z)
    assert hi.dtype == lo.dtype == np.complex64 and hi.shape == lo.shape == z.shape
    for part in ("real", "imag"):
        h, l = ctr.split_bf16(np.ascontiguousarray(getattr(z, part)))
        assert np.array_equal(getattr(hi, part), h) and np.array_equal(getattr(lo, part), l)
