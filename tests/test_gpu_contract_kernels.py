"""The contraction kernels of csrc/contract.hip at their edges, element by element.

Every case of tests/contract_cases.py is a one-step network handed to `contraction.contract()`.  A test asserts which
kernel path ran, through the launch counts of `ContractionResult.kernel_launches`
(tnco_hip_contract_kernel_launches): a case that lands on another kernel fails instead of testing something else.
Then it compares every element with numpy's einsum of the up-cast inputs in float64 / complex128 -- nothing of
tnco_amd.contraction is part of the reference.  A result element is a sum of kt products (K of the step times the
slice assignments accumulated into it), and any order of fused multiply-adds in the working precision satisfies

    |got - ref| <= (c kt + 2) u (|A| @ |B|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

(|A| @ |B| in float64 with the same index pattern; the + 2 covers rounding to the output type).  That bound is used as
it stands, no factor on top.  Inputs are uniform(0.5, 1.5) in both parts: no cancellation, so one dropped or doubled
product moves an element by about 0.11 / kt relative, well over the bound while kt <= 600 in single precision
(contract_cases.KT_SINGLE) and always in double.  Longer sums run in the double types; where a single type is listed
for them it checks beta and offsets, not single terms.  A standard_normal fill on some cases keeps signs and the
complex cross terms honest.

Not reached here: the tiled kernel's own grid-stride loop (more than 2^20 tiles) and anything beyond 2^31 elements --
too large for a shared card.
"""
import numpy as np
import pytest

from tests import contract_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def _fill(case, dtype, seed, normal=False):
    rng = np.random.RandomState(seed)
    draw = (lambda s: rng.standard_normal(s)) if normal else (lambda s: rng.uniform(0.5, 1.5, s))
    out = []
    for shape in case.shapes():
        a = draw(shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * draw(shape)
        out.append(np.asarray(a).astype(dtype))
    return out


def _result_inds(ts, output):
    """Axes of the one step: [shared indices the output keeps][rest of the first][rest of the second]."""
    a, b = ts
    shared = set(a) & set(b)
    keep = shared & set(output) if output is not None else set()
    return tuple(x for x in a if x in keep) + tuple(x for x in a if x not in shared) + \
        tuple(x for x in b if x not in shared)


def _reference(ts, arrays, inds):
    """(einsum of the up-cast inputs, the same einsum of their moduli), both in double precision."""
    sym = {x: k for k, x in enumerate(dict.fromkeys(tuple(ts[0]) + tuple(ts[1])))}
    subs = [[sym[x] for x in xs] for xs in ts]
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    res = [sym[x] for x in inds]
    ref = np.einsum(wide[0], subs[0], wide[1], subs[1], res, optimize=True)
    mag = np.einsum(np.abs(wide[0]), subs[0], np.abs(wide[1]), subs[1], res, optimize=True)
    return ref, mag


def _bound(mag, kt, dtype):
    u = float(np.finfo(dtype).eps) / 2  # (finfo of a complex type is that of its parts)
    return ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * u * mag


def _assert_within(got, ref, bound, what):
    """|got - ref| <= bound in every element; an element that is not a number does not satisfy it."""
    assert got.shape == ref.shape == bound.shape, what
    err = np.abs(got.astype(ref.dtype) - ref)
    bad = ~(err <= bound)
    ratio = np.divide(err, bound, out=np.zeros_like(bound), where=bound > 0)
    ratio[bad & ~(ratio > 1)] = np.inf  # NaN, or an error over a zero bound: reported as the worst
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    print(f"{what}: largest error / bound {float(ratio[at]):.4f} at {at}")
    if bad.any():
        where = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound, "
                             f"{int(np.isnan(err).sum())} of them not a number; first at "
                             f"{tuple(where[0].tolist())}, last at {tuple(where[-1].tolist())}, worst at {at}: got "
                             f"{got[at]}, reference {ref[at]}, error / bound {float(ratio[at]):.3g}")


def _assert_elements(got, ref, mag, kt, dtype, what):
    assert got.dtype == np.dtype(dtype), what
    _assert_within(got, ref, _bound(mag, kt, dtype), f"{what}: kt {kt}")


def _assert_kernels(ctr, r, kernels, what):
    want = tuple(kernels.get(name, 0) for name in ctr.KERNEL_PATHS)
    assert set(kernels) <= set(ctr.KERNEL_PATHS)
    assert r.kernel_launches == want, f"{what}: launches {dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))}"
    assert sum(r.kernel_launches) == r.launches


def _run_case(ctr, case, dtype, seed, normal=False):
    arrays = _fill(case, dtype, seed, normal)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices)
    what = f"{case.name} {np.dtype(dtype).name}"
    inds = _result_inds(case.ts, case.output)
    assert r.inds == inds and r.n_slices == case.n_slices(), what
    _assert_kernels(ctr, r, case.kernels, what)
    op = case.ops
    assert r.macs == case.n_slices() * op["H"] * op["M"] * op["N"] * op["K"]
    ref, mag = _reference(case.ts, arrays, inds)
    _assert_elements(r.array, ref, mag, case.kt, dtype, what)
    return arrays, r


_RUNS = [pytest.param(c, d, id=f"{c.name}-{np.dtype(d).name}") for c in cc.CASES for d in c.run_dtypes()]
_NORMAL = [pytest.param(cc.BY_NAME[n], d, id=f"{n}-{np.dtype(d).name}")
           for n in cc.NORMAL_FILL for d in cc.BY_NAME[n].run_dtypes()]


@pytest.mark.parametrize("case,dtype", _RUNS)
def test_kernel_path_and_every_element(ctr, case, dtype):
    _run_case(ctr, case, dtype, seed=11)


@pytest.mark.parametrize("case,dtype", _NORMAL)
def test_kernel_path_and_every_element_with_signs(ctr, case, dtype):
    _run_case(ctr, case, dtype, seed=12, normal=True)


@pytest.mark.parametrize("name,cut", [("tiled_beta-in_place", 2), ("dot_batched_beta-K777", 1),
                                      ("stream_batched_outer_beta", 2)])
@pytest.mark.parametrize("dtype", cc.DOUBLES + (cc.F32,))
def test_slice_range_halves_add_up_to_the_whole(ctr, name, cut, dtype):
    """Each half against the einsum of its own assignments, and their sum against the whole (the halves' bounds
    added: each half rounds on its own)."""
    case = cc.BY_NAME[name]
    (s,) = case.slices
    n, K = case.dims[s], case.ops["K"]
    (path,) = case.kernels
    arrays = _fill(case, dtype, seed=13)
    inds = _result_inds(case.ts, case.output)
    total, total_bound = 0, 0
    for lo, hi in ((0, cut), (cut, n)):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, hi))
        assert r.n_slices == hi - lo
        _assert_kernels(ctr, r, {path: hi - lo}, f"{name} [{lo}, {hi})")
        part = [np.take(a, range(lo, hi), axis=xs.index(s)) for a, xs in zip(arrays, case.ts)]
        ref, mag = _reference(case.ts, part, inds)
        _assert_elements(r.array, ref, mag, K * (hi - lo), dtype, f"{name} [{lo}, {hi})")
        total = total + r.array.astype(ref.dtype)
        total_bound = total_bound + _bound(mag, K * (hi - lo), dtype)
    ref, _ = _reference(case.ts, arrays, inds)
    _assert_within(total, ref, total_bound, f"{name}: the halves added")


def _pair(ctr, ts, arrays, kernels, kt, what):
    r = ctr.contract([(0, 1)], ts, arrays)
    _assert_kernels(ctr, r, kernels, what)
    inds = _result_inds(ts, None)
    assert r.inds == inds
    wide = np.result_type(*arrays)
    ref, mag = _reference(ts, [np.asarray(a, wide) for a in arrays], inds)
    _assert_elements(r.array, ref, mag, kt, wide, what)
    return r


@pytest.mark.parametrize("da,db,dz", [(np.float32, np.complex64, np.complex64),
                                      (np.float64, np.complex64, np.complex128),
                                      (np.complex64, np.float32, np.complex64)])
def test_mixed_dtypes_compute_in_the_result_type(ctr, da, db, dz):
    case = cc.BY_NAME["tiled_mk_nk-65x127x48"]
    a, _ = _fill(case, da, seed=14)
    _, b = _fill(case, db, seed=15)
    r = _pair(ctr, case.ts, [a, b], case.kernels, case.kt, f"{np.dtype(da).name} x {np.dtype(db).name}")
    assert r.array.dtype == np.dtype(dz)
    same = ctr.contract([(0, 1)], case.ts, [a.astype(dz), b.astype(dz)])
    assert np.array_equal(r.array, same.array)


@pytest.mark.parametrize("dtype", cc.ALL)
@pytest.mark.parametrize("name", ["tiled_km_kn-128x64x49", "stream-just_misses_tiled"])
def test_views_and_fortran_order_equal_the_contiguous_copy(ctr, name, dtype):
    case = cc.BY_NAME[name]
    a, b = _fill(case, dtype, seed=16)
    view = np.ascontiguousarray(a.T).T  # the same numbers, strides swapped
    fort = np.asfortranarray(b)
    assert not view.flags.c_contiguous and not fort.flags.c_contiguous
    assert np.array_equal(view, a) and np.array_equal(fort, b)
    r = _pair(ctr, case.ts, [view, fort], case.kernels, case.kt, f"{name} views")
    plain = ctr.contract([(0, 1)], case.ts, [a, b])
    assert np.array_equal(r.array, plain.array)
    strided = np.repeat(a, 2, axis=1)[:, ::2]  # every second column of a wider array
    assert not strided.flags.c_contiguous and np.array_equal(strided, a)
    assert np.array_equal(ctr.contract([(0, 1)], case.ts, [strided, b]).array, plain.array)


@pytest.mark.parametrize("name,dtype", [("tiled_beta-in_place", np.float32), ("tiled_beta-gathered", np.complex64),
                                        ("dot_batched_beta-K777", np.float64), ("dot_batched_beta-K777", np.complex128),
                                        ("stream_batched_outer_beta", np.float32)])
def test_runs_are_bit_identical_per_kernel_path(ctr, name, dtype):
    case = cc.BY_NAME[name]
    arrays, first = _run_case(ctr, case, dtype, seed=17)
    again = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices)
    assert again.kernel_launches == first.kernel_launches
    assert np.array_equal(again.array, first.array)
