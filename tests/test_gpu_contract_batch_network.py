"""A whole network through optimize(max_width=...) -> contract_results(..., slice_batch=8): bit for bit the result of
`slice_batch=None`, plain, in storage mode and with per-tensor scaling.  The network, its arrays and its optimization are
those of tests/test_gpu_contract_half_network.py (shared with it); what the modes cost in accuracy is tested there."""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn
from tnco_amd.app.app import cost_to_decimal

pytestmark = pytest.mark.gpu

MODES = [dict(), dict(storage="bfloat16"), dict(storage="float16", scaling="tensor")]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("mode", MODES, ids=["plain", "bfloat16", "float16-scaled"])
def test_a_sliced_network_in_batches_of_eight_equals_the_unbatched_run(ctr, mode):
    tn0, arrays, tn, res, _ = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    base = ctr.contract_results(tn0, arrays, tn, res, **mode)
    r = ctr.contract_results(tn0, arrays, tn, res, slice_batch=8, **mode)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.complex64
    as_bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(as_bits(r.array), as_bits(base.array))
    assert np.isfinite(r.array).all() and r.array.any()
    assert r.macs == base.macs and cost_to_decimal(r.macs) == res.cost
    assert r.n_slices == base.n_slices == n and r.exponents == base.exponents
    groups = -(-n // 8)
    assert r.slice_batch == min(8, n) and r.batch_launches == groups and base.batch_launches == 0
    assert r.kernel_launches == tuple(v // n * groups for v in base.kernel_launches)
    assert r.narrow_launches == base.narrow_launches // n * groups
    assert r.launches == sum(r.kernel_launches) + r.narrow_launches + r.batch_launches
    assert r.launches < base.launches and r.peak_device_bytes > base.peak_device_bytes
