"""A whole network through optimize(max_width=...) -> contract_results(..., accumulate="float64"), alone and with
slice_batch=8 and hoist=True: the two runs byte-equal, both the float64 fold of the assignments' blocks
(tests/accumulate_cases.py `model`; the network has at most 16 assignments, each run singly without the keyword), and no
further from the complex128 host contraction than the default call plus one float32 ulp of the result's norm.  The
network, its arrays and its optimization are those of tests/test_gpu_contract_batch_network.py and
tests/test_gpu_contract_hoist_network.py (tests/test_gpu_contract_half_network.py, shared with them)."""
import numpy as np
import pytest

from tests import accumulate_cases as ac
from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def test_a_sliced_network_is_the_float64_fold_of_its_assignments(ctr):
    tn0, arrays, tn, res, ref = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert 4 <= n <= 16
    plain = ctr.contract_results(tn0, arrays, tn, res)
    alone = ctr.contract_results(tn0, arrays, tn, res, accumulate="float64")
    both = ctr.contract_results(tn0, arrays, tn, res, accumulate="float64", slice_batch=8, hoist=True)
    assert alone.inds == both.inds == plain.inds and alone.array.dtype == both.array.dtype == np.complex64
    assert np.array_equal(ac.bits(alone.array), ac.bits(both.array))
    assert np.isfinite(alone.array).all() and alone.array.any()
    # the model: the network is one component and was not pre-fused, so contract_results is one call of contract
    assert not tn.tags.get("fuse_path") and len([q for q in getattr(res, "disconnected_paths", ()) if q]) <= 1
    call = lambda **kw: ctr.contract(res.path, tn.ts_inds, arrays, tn.output_inds, slices=res.slices, **kw)  # noqa: E731
    p = ctr.plan(res.path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, slices=res.slices, dtype=np.complex64)
    assert p.n_slices == n and p.inds == plain.inds
    parts = [(ac.where_of(p, a), call(slice_range=(a, a + 1)).array[ac.where_of(p, a)].copy()) for a in range(n)]
    assert ac.same_bytes(plain.array, ac.running_float32(parts, p.shape, np.complex64))  # (existing behaviour)
    assert ac.same_bytes(alone.array, ac.model(parts, p.shape, np.complex64))
    # the counts: a fold per assignment (per group), one launch that rounds the accumulator, the multiply-adds of the plan
    assert alone.macs == plain.macs and alone.n_slices == both.n_slices == n
    assert alone.kernel_launches == plain.kernel_launches
    assert (alone.batch_launches, alone.narrow_launches) == (n, 1) and alone.launches == plain.launches + n + 1
    assert (both.batch_launches, both.narrow_launches) == (-(-n // 8), 1) and both.hoisted[0] > 0
    assert both.launches == sum(both.kernel_launches) + both.batch_launches + 1
    # accuracy: no worse than the float32 sum, up to one float32 ulp of the result's norm
    ref = ref.transpose([hn._ref_inds(tn, res).index(x) for x in plain.inds]) if plain.inds else ref
    norm = float(np.linalg.norm(np.ravel(ref)))
    e_wide = float(np.linalg.norm(np.ravel(alone.array - ref)))
    e_none = float(np.linalg.norm(np.ravel(plain.array - ref)))
    print(f"open network, {n} assignments: |wide - ref| / |ref| {e_wide / norm:.3e}, |float32 - ref| / |ref| {e_none / norm:.3e}")
    assert e_wide <= e_none + float(np.finfo(np.float32).eps) * norm
