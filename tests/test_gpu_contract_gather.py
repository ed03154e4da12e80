"""The kernels that only move numbers, past the first trip of their loops, on the device: every case of
tests/gather_cases.py through `contraction.contract()`, byte for byte.

ct_gather_body (ct_gather_kernel, ct_half_gather_kernel, ct_half_gather_scaled_kernel), ct_batch_reduce_kernel,
ct_path_reduce_kernel and the permute loop of the path kernel run at most 2048 blocks of 256 lanes and carry on in a
grid-stride loop above TRIP = 524 288 elements; ct_scale_narrow_kernel does the same above 4 TRIP float32 parts, in quads
with a tail of n % 4 parts.  The cases cross those sizes (tests/test_contraction_gather_plan.py asserts that from the
plans, and that the comparison below fails when the loop's second trip, a stride or the tail is wrong).

These kernels copy, add in a fixed order or round once, so nothing here has a tolerance.  Per case and dtype:
  - the launch counts say which kernels ran (gather launches, the steps by shape class, narrowing passes, the reduce of
    a slice batch, the two kernels of the path kernel);
  - the result equals the numpy expectation of gather_cases.expected in every byte (an element that is not a number
    fails), and under scaling the exponents are those of the documented rule;
  - the same call with slice_batch= / path_kernel= returns the bytes of the call without;
  - a second call returns the bytes of the first.

Out of reach here, as in tests/test_gpu_contract_kernels.py: the tiled kernels' own loop (more than 2^20 tiles) and
anything beyond 2^31 elements.
"""
import numpy as np
import pytest

from tests import gather_cases as gc

pytestmark = pytest.mark.gpu

_FILLED, _BASE = {}, {}


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def filled(case, dtype):
    """(leaves, expected result, expected exponents) of a run, computed once and never written to."""
    key = (case.name, np.dtype(dtype))
    if key not in _FILLED:
        arrays = gc.fill(case, dtype)
        want, exps = gc.expected(case, dtype, arrays)
        for a in arrays + [want]:
            a.setflags(write=False)
        _FILLED[key] = (arrays, want, exps)
    return _FILLED[key]


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def call(ctr, case, dtype, **more):
    arrays, _, _ = filled(case, dtype)
    return ctr.contract(list(case.path), case.ts, arrays, case.out_inds, **case.keywords(), **more)


def counts(ctr, r) -> dict:
    k = dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))
    return dict(gather=k["gather"], tiled=sum(v for name, v in k.items() if name.startswith("tiled")), dot=k["dot"],
                stream=k["stream"], narrow=r.narrow_launches, batch=r.batch_launches, path=tuple(r.path_launches))


def assert_expected(ctr, case, dtype, r, what, keyword=None, value=None):
    """The launch counts, the bytes and the exponents of one run."""
    _, want, exps = filled(case, dtype)
    p = case.plan(dtype)
    assert counts(ctr, r) == gc.launches(case, p, keyword, value), what
    assert r.launches == sum(r.kernel_launches) + r.narrow_launches + r.batch_launches + sum(r.path_launches), what
    assert r.row_kernel_launches == (0, 0, 0) and r.indirect_launches == (0, 0, 0) and r.n_slices == len(case.assignments())
    got = r.array.transpose([r.inds.index(x) for x in case.out_inds])
    assert got.dtype == want.dtype == np.dtype(dtype) and got.shape == want.shape, what
    assert np.isfinite(got).all(), f"{what}: an element is not a number"
    same = bits(got) == bits(want)
    if not same.all():
        item = want.dtype.itemsize
        bad = np.unique(np.flatnonzero(~same) // item)
        at = np.unravel_index(int(bad[0]), want.shape) if want.shape else ()
        raise AssertionError(f"{what}: {bad.size} of {want.size} elements differ from the expectation, the first at {at} "
                             f"(flat {int(bad[0])}): got {got[at]!r}, expected {want[at]!r}")
    if case.scaling is not None:
        arrays = filled(case, dtype)[0]
        n = len(arrays)
        assert r.exponents[:n] == tuple(gc.narrow_exponent(a) for a in arrays), what
        if case.path:  # the stored tensor's exponent as the last assignment left it; the step for the output has none
            assert r.exponents[n:] == (exps[-1], 0), (what, r.exponents, exps)
    else:
        assert r.exponents is None


@pytest.mark.parametrize("case,dtype", gc.RUNS, ids=gc.RUN_IDS)
def test_the_plain_run_gives_the_expected_bytes_twice(ctr, case, dtype):
    what = f"{case.name} {dtype.name}"
    r = call(ctr, case, dtype)
    assert_expected(ctr, case, dtype, r, what)
    again = call(ctr, case, dtype)
    assert np.array_equal(bits(again.array), bits(r.array)) and again.exponents == r.exponents, f"{what}: a second call differs"
    assert again.kernel_launches == r.kernel_launches and again.launches == r.launches


BATCHED = [(c, d, k, v) for c, d in gc.RUNS for k, v in c.batching]


@pytest.mark.parametrize("case,dtype,keyword,value", BATCHED, ids=[f"{c.name}-{d.name}-{k}-{v}" for c, d, k, v in BATCHED])
def test_a_batched_run_gives_the_bytes_of_the_plain_run_twice(ctr, case, dtype, keyword, value):
    what = f"{case.name} {dtype.name} {keyword}={value}"
    key = (case.name, dtype)
    if key not in _BASE:  # the run without the keyword, once per case and dtype; only its bytes are kept
        base = call(ctr, case, dtype)
        _BASE[key] = (bits(base.array).copy(), base.inds, base.exponents, base.macs)
    base_bits, inds, exponents, macs = _BASE[key]
    r = call(ctr, case, dtype, **{keyword: value})
    assert getattr(r, keyword) == min(value, len(case.assignments())), what
    assert_expected(ctr, case, dtype, r, what, keyword, value)
    assert r.inds == inds and np.array_equal(bits(r.array), base_bits), f"{what}: the result differs from the run without"
    assert r.exponents == exponents and r.macs == macs, what
    again = call(ctr, case, dtype, **{keyword: value})
    assert np.array_equal(bits(again.array), base_bits) and again.exponents == exponents, f"{what}: a second call differs"
