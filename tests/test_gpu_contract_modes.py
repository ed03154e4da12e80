"""Every way of running a plan, on the device, over the random networks of tests/mode_cases.py: plain, `slice_batch=`,
`path_kernel=`, `compute="bf16x3"`, `storage="bfloat16"` and `storage="float16", scaling="tensor"`.

Per case, in this order:

    plain       element by element against numpy's einsum of the whole network in float64 / complex128,
                    |got - ref| <= (c kt + 2) u mag
                mag the same einsum of the moduli, kt the sum of K over the steps plus the assignments added into an
                element, c = 1 real / 2 complex, u = eps / 2; the launch counts per kernel path are those the plan's
                signature predicts, times the assignments;
    slice_batch (3, 64), path_kernel (3, 1024): the bytes of the plain result, equal multiply-adds, the launch counts of
                the mode;
    float32 / complex64 cases only:
    bf16x3      alone and with slice_batch=3, byte-equal to each other; without a tiled-class step byte-equal to plain and
                no split launch; else a split launch per tiled step and assignment, and
                    [s_t 2^-14 + (2 c 3 kt + 2) 2^-24] mag,   s_t tiled steps on the longest chain feeding the output;
    storage     each of the two modes alone and with slice_batch=3, byte-equal to each other (exponents included), and
                    [d u_s + (2 c kt + 2) 2^-24] mag,   d = steps - 1 stored intermediates, u_s = 2^-8 / 2^-11
                against the einsum of the leaves as rounded to the storage type; a narrowing launch per stored step.

tests/test_contraction_modes_plan.py shows without a device that a correct contraction meets these bounds on these
inputs.  `check_case` is also what tools/fuzz_contract.py runs over seeds beyond the table.
"""
import numpy as np
import pytest

from tests import mode_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _ratio(r, ref, bound, what, out):
    got = np.asarray(r.array)
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    err = np.abs(got.astype(ref.dtype) - ref)
    ratio = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())
    out(f"{what}: largest error / bound {ratio:.4f}")
    assert (err <= bound).all(), what
    return ratio


def check_case(ctr, case, out=print):
    """Run `case` in every mode and assert the module docstring; returns the largest error / bound per mode."""
    what = f"{case.name} {case.dtype}"
    dtype = np.dtype(case.dtype)
    arrays = mc.fill(case)
    p = case.plan()
    n = case.n_assignments()
    zeros = (0,) * len(ctr.KERNEL_PATHS)

    def call(leaves=arrays, **mode):
        return ctr.contract(list(case.path), case.ts_inds, leaves, case.output_inds, slices=case.slices,
                            slice_range=case.slice_range, **mode)

    ratios = {}
    base = call()
    ref, mag = mc.reference(case, p, arrays)
    assert base.inds == p.inds and base.array.dtype == dtype and base.n_slices == n and base.macs == p.macs, what
    ratios["plain"] = _ratio(base, ref, mc.plain_bound(case, p, mag), f"{what} plain (kt {mc.kt(p)})", out)
    per = mc.launches_per_assignment(p)
    assert base.kernel_launches == tuple(v * n for v in per), (what, base.kernel_launches, per)
    assert base.launches == sum(per) * n and base.row_kernel_launches == (0, 0, 0), what
    assert base.batch_launches == 0 and base.path_launches == (0, 0) and base.split_launches == 0, what

    for B in mc.BATCHES:
        r, groups = call(slice_batch=B), -(-n // B)
        tag = f"{what} slice_batch={B}"
        assert r.inds == base.inds and np.array_equal(bits(r.array), bits(base.array)), f"{tag}: differs from the plain run"
        assert r.macs == base.macs and r.n_slices == n and r.slice_batch == min(B, n), tag
        assert r.kernel_launches == tuple(v * groups for v in per) and r.batch_launches == groups, tag
        assert r.launches == sum(per) * groups + groups and r.path_launches == (0, 0), tag
    for G in mc.GROUPS:
        r, groups = call(path_kernel=G), -(-n // G)
        tag = f"{what} path_kernel={G}"
        assert r.inds == base.inds and np.array_equal(bits(r.array), bits(base.array)), f"{tag}: differs from the plain run"
        assert r.macs == base.macs and r.n_slices == n and r.path_kernel == min(G, n), tag
        assert r.path_launches == (groups, groups) and r.launches == 2 * groups, tag
        assert r.kernel_launches == zeros and r.row_kernel_launches == (0, 0, 0), tag
        assert r.batch_launches == 0 and r.narrow_launches == 0 and r.split_launches == 0, tag
    if dtype not in mc.SINGLES:
        return ratios

    tiled = sum(sig[0] == "tiled" for sig in mc.signature(p))
    groups = -(-n // mc.HALF_BATCH)
    split, split_b = call(compute="bf16x3"), call(compute="bf16x3", slice_batch=mc.HALF_BATCH)
    assert np.array_equal(bits(split.array), bits(split_b.array)), f"{what} bf16x3: the batched run differs"
    assert split.macs == split_b.macs == base.macs and split.kernel_launches == base.kernel_launches, what
    assert split.split_launches == tiled * n and split_b.split_launches == tiled * groups, what
    if not tiled:
        assert np.array_equal(bits(split.array), bits(base.array)), f"{what} bf16x3: no tiled step, yet not the plain bytes"
    else:
        ratios["bf16x3"] = _ratio(split, ref, mc.split_bound(case, p, mag),
                                  f"{what} bf16x3 ({tiled} tiled, depth {mc.tiled_depth(case, p)})", out)

    for mode in mc.STORAGE_MODES:
        storage, scaled = mode["storage"], "scaling" in mode
        tag = f"{what} {storage}" + (" scaled" if scaled else "")
        leaves = mc.fill(case, storage)
        ref_s, mag_s = mc.reference(case, p, leaves)
        r, rb = call(leaves, **mode), call(leaves, slice_batch=mc.HALF_BATCH, **mode)
        assert r.inds == base.inds and r.array.dtype == dtype, tag
        assert np.array_equal(bits(r.array), bits(rb.array)), f"{tag}: the batched run differs"
        assert r.exponents == rb.exponents and (r.exponents is not None) == scaled, tag
        assert r.macs == rb.macs == base.macs and r.kernel_launches == base.kernel_launches, tag
        stored = int((case.plan(**mode).stage_refs >= 0).sum()) if scaled else 0
        assert stored == (len(p.steps) - 1 if scaled else 0), tag
        assert r.narrow_launches == stored * n and rb.narrow_launches == stored * groups, tag
        assert rb.batch_launches == groups and rb.kernel_launches == tuple(v * groups for v in per), tag
        ratios[tag.split(" ", 2)[2]] = _ratio(r, ref_s, mc.storage_bound(case, p, mag_s, storage), tag, out)
    return ratios


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_every_mode_on_a_random_network(ctr, case):
    check_case(ctr, case)
