"""A whole network through optimize(max_width=...) -> contract_results(..., hoist=True): bit for bit the result of the
default call, with fewer launches, alone and with slice_batch=8.  The network, its arrays and its optimization are those
of tests/test_gpu_contract_batch_network.py (tests/test_gpu_contract_half_network.py, shared with it)."""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("kw", [dict(), dict(slice_batch=8)], ids=["unbatched", "slice_batch-8"])
def test_a_sliced_network_hoisted_equals_the_default_call(ctr, kw):
    tn0, arrays, tn, res, _ = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    base = ctr.contract_results(tn0, arrays, tn, res, **kw)
    r = ctr.contract_results(tn0, arrays, tn, res, hoist=True, **kw)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.complex64
    as_bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(as_bits(r.array), as_bits(base.array))
    assert np.isfinite(r.array).all() and r.array.any()
    assert base.hoisted is None and r.hoisted[0] > 0, r.hoisted
    assert r.macs < base.macs and r.n_slices == base.n_slices == n
    # launches: every group of assignments after the first saves the hoisted share.  A single group (8 or fewer
    # assignments in batches of 8) runs everything once either way, and a permute group with rows of both kinds is
    # then two launches where the default call has one
    groups = n if not kw else -(-n // 8)
    if groups > 1:
        assert r.launches < base.launches
    else:
        assert base.launches <= r.launches <= base.launches + r.hoisted[1]
    assert r.launches == sum(r.kernel_launches) + r.batch_launches and r.batch_launches == base.batch_launches
    assert r.slice_batch == base.slice_batch
