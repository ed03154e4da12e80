"""Projected contractions (`sparse_inds=` / `projs=`) on multi-step networks, on the device, element by element: the
cases of tests/projs_cases.py, in which the row-mapped kernels read operands that lie in the arena -- written by a row
step, a folded step or a permute -- through maps, in place, or as one row for every r.

Per case (`check_case`, also what `tools/fuzz_contract.py --projs` runs over seeds beyond the table):

    values      every element against numpy's einsum of the whole network in float64 / complex128 at the projections
                (`projs_cases.reference`; nothing of tnco_amd.contraction takes part),
                    |got - ref| <= (c kt + 2) u mag
                mag the same einsum of the moduli, kt = mode_cases.kt(plan), c = 1 real / 2 complex, u = eps / 2; an
                element that is not a number fails;
    counts      `row_kernel_launches` and `kernel_launches` per slot are what `projs_cases.launches_per_assignment`
                predicts from the tables, times the assignments; `launches` their sum; `macs` and `inds` the plan's;
                the dtype is kept;
    invariants  byte for byte: a second call; `projs` with its columns reversed and `sparse_inds` reversed; `projs`
                doubled as [projs, projs[::-1]] gives the slabs of the single run in that order, with equal macs;
                two parts of `slice_range`, each within its own bound against the reference of its part, add up to the
                whole within the sum of their bounds;
    dense       where `projs` lists every assignment of the sparse indices: `contract()` without `projs`, indexed at
                `projs`, lies within the same bound of the same reference, with equal macs.

A non-finite part stays in its rows: one +inf (one NaN) in one row of a leaf of the branch that goes to the arena makes
exactly the elements non-finite that an einsum of the non-finite mask says, and leaves every other one within the bound.

tests/test_contraction_projs_cases_plan.py shows without a device that a correct contraction meets the bound on these
inputs and that four planted defects do not.
"""
import numpy as np
import pytest

from tests import projs_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _within(got, ref, bound, what, out, skip=None):
    """|got - ref| <= bound in every element (but those of `skip`); one that is not a number does not satisfy it.
    Returns the largest error / bound."""
    got = np.asarray(got)
    assert got.shape == ref.shape == bound.shape, what
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(ref.dtype) - ref)
    bad = ~(err <= bound)
    ratio = np.divide(err, bound, out=np.zeros_like(bound), where=bound > 0)
    ratio[bad & ~(ratio > 1)] = np.inf
    if skip is not None:
        bad, ratio = bad & ~skip, np.where(skip, 0.0, ratio)
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    out(f"{what}: largest error / bound {float(ratio[at]):.4f} at {at}")
    if bad.any():
        where = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound, "
                             f"{int(np.isnan(err[bad]).sum())} of them not a number; first at {tuple(where[0].tolist())}, "
                             f"last at {tuple(where[-1].tolist())}, worst at {at}: got {got[at]}, reference {ref[at]}, "
                             f"error / bound {float(ratio[at]):.3g}")
    return float(ratio[at])


def _call(ctr, case, arrays, projs, sparse=None, slice_range=None, dense=False):
    kw = {} if dense else dict(sparse_inds=case.sparse if sparse is None else sparse, projs=projs)
    return ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices,
                        slice_range=slice_range or case.slice_range, **kw)


def check_case(ctr, case, out=print):
    """Run `case` and assert the module docstring; returns the largest error / bound of the whole run and the launches
    per row slot."""
    what = f"{case.name} {case.dtype}"
    dtype = np.dtype(case.dtype)
    arrays, projs, p = pc.fill(case), case.projs(), case.plan()
    n = case.n_assignments()
    ref, mag = pc.reference(case, p, arrays)
    bound = pc.bound(case, p, mag)

    base = _call(ctr, case, arrays, projs)
    assert base.inds == p.inds and base.array.dtype == dtype and base.array.shape == p.shape, what
    assert base.n_slices == n and base.macs == p.macs, (what, base.macs, p.macs)
    plain, rows = pc.launches_per_assignment(p)
    assert base.row_kernel_launches == tuple(v * n for v in rows), (what, base.row_kernel_launches, rows)
    assert base.kernel_launches == tuple(v * n for v in plain), (what, base.kernel_launches, plain)
    assert base.launches == sum(base.kernel_launches) + sum(base.row_kernel_launches), what
    ratio = _within(base.array, ref, bound, f"{what} (kt {pc.kt(p)}, {n} assignments, {len(projs)} projections)", out)

    again = _call(ctr, case, arrays, projs)
    assert np.array_equal(bits(again.array), bits(base.array)), f"{what}: a second call differs"
    flipped = _call(ctr, case, arrays, projs[:, ::-1], sparse=case.sparse[::-1])
    assert flipped.inds == base.inds and flipped.macs == base.macs, what
    assert np.array_equal(bits(flipped.array), bits(base.array)), f"{what}: the columns reversed differ"
    twice = _call(ctr, case, arrays, np.concatenate([projs, projs[::-1]]))
    assert twice.macs == base.macs and twice.row_kernel_launches == base.row_kernel_launches, what
    assert np.array_equal(bits(twice.array), bits(np.concatenate([base.array, base.array[::-1]]))), \
        f"{what}: the doubled projections are not the slabs of the single run"

    if n >= 2:
        lo, hi = p.slice_range
        mid = lo + max(1, n // 3)
        total, total_bound = 0, 0
        for part in ((lo, mid), (mid, hi)):
            q = case.plan(slice_range=part)
            r = _call(ctr, case, arrays, projs, slice_range=part)
            assert r.n_slices == part[1] - part[0] and r.macs == q.macs, (what, part)
            ref_q, mag_q = pc.reference(case, q, arrays)
            _within(r.array, ref_q, pc.bound(case, q, mag_q), f"{what} [{part[0]}, {part[1]})", out)
            total, total_bound = total + r.array.astype(ref.dtype), total_bound + pc.bound(case, q, mag_q)
        _within(total, ref, total_bound, f"{what}: the parts added", out)

    if case.projs_spec == "all":
        dense = _call(ctr, case, arrays, None, dense=True)
        assert dense.macs == base.macs and dense.row_kernel_launches == (0, 0, 0), (what, dense.macs, base.macs)
        front = [dense.inds.index(x) for x in case.sparse]
        assert tuple(x for x in dense.inds if x not in case.sparse) == base.inds[1:], what
        at_projs = np.moveaxis(dense.array, front, range(len(front)))[tuple(projs.T)]
        _within(at_projs, ref, bound, f"{what}: the dense result at the projections", out)
    return ratio, base.row_kernel_launches


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_projections_on_a_multi_step_network(ctr, case):
    check_case(ctr, case)


@pytest.mark.parametrize("name,value", [("hand-tiled-both-00", np.inf), ("hand-dot-both", np.inf),
                                        ("hand-stream-both", np.inf), ("hand-stream-both", np.nan)])
def test_a_part_that_is_not_finite_stays_in_its_rows(ctr, name, value):
    """One +inf (NaN) in T0, the leaf with the rows of s of the branch Z1 that goes to the arena, at the s of the first
    projection: with the uniform fill every product is positive, so nothing but that part makes an element non-finite."""
    case = pc.BY_NAME[name].with_(fill="uniform")
    assert np.dtype(case.dtype).kind == "f" and case.ts_inds[0][0] == "s"
    arrays, projs, p = pc.fill(case), case.projs(), case.plan()
    j = int(projs[0, case.sparse.index("s")])
    at = (j,) + tuple(d - 1 for d in arrays[0].shape[1:])
    clean = [a.copy() for a in arrays]
    clean[0][at] = 0  # (the elements that part does not feed do not depend on it)
    arrays[0][at] = value
    mask = [np.zeros(a.shape) if t == 0 else np.ones(a.shape) for t, a in enumerate(arrays)]
    mask[0][at] = 1
    fed = pc.reference(case, p, mask)[0] > 0
    assert 0 < fed.sum() < fed.size and fed[0].any()
    r = _call(ctr, case, arrays, projs)
    assert r.row_kernel_launches == tuple(v * case.n_assignments() for v in pc.launches_per_assignment(p)[1])
    got = r.array
    assert not np.isfinite(got[fed]).any(), f"{name}: {int(np.isfinite(got[fed]).sum())} fed elements are finite"
    assert np.isfinite(got[~fed]).all(), f"{name}: {int((~np.isfinite(got[~fed])).sum())} other elements are not finite"
    if np.isnan(value):
        assert np.isnan(got[fed]).all()
    else:
        assert (got[fed] == np.inf).all()
    ref, mag = pc.reference(case, p, clean)
    _within(got, ref, pc.bound(case, p, mag), f"{name} with one {value}", print, skip=fed)
