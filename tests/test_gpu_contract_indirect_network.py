"""A whole network through optimize(max_width=...) -> contract_results(..., indirect=True): bit for bit the result of
the same call without the keyword, with fewer launches, alone, with slice_batch=8 and with slice_batch=8, hoist=True, and
inside the norm bound of the plain run (tests/test_gpu_contract_path_network.py).  The network, its arrays and its
optimization are those of tests/test_gpu_contract_hoist_network.py (tests/test_gpu_contract_half_network.py)."""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("kw", [dict(), dict(slice_batch=8), dict(slice_batch=8, hoist=True)],
                         ids=["unbatched", "slice_batch-8", "slice_batch-8-hoist"])
def test_a_sliced_network_read_in_place_equals_the_same_call_without_the_keyword(ctr, kw):
    tn0, arrays, tn, res, ref = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    base = ctr.contract_results(tn0, arrays, tn, res, **kw)
    r = ctr.contract_results(tn0, arrays, tn, res, indirect=True, **kw)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.complex64
    as_bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(as_bits(r.array), as_bits(base.array))
    assert np.isfinite(r.array).all() and r.array.any()
    assert base.indirect is None and base.indirect_launches == (0, 0, 0) and r.indirect > 0
    assert r.macs == base.macs and r.n_slices == base.n_slices == n and r.hoisted == base.hoisted
    # every folded operand was a permute of every assignment; the steps that read one run the indirect kernels
    assert r.launches < base.launches and r.kernel_launches[0] < base.kernel_launches[0]
    assert sum(r.indirect_launches) > 0
    assert sum(r.kernel_launches[1:]) + sum(r.indirect_launches) == sum(base.kernel_launches[1:])
    assert r.launches == sum(r.kernel_launches) + sum(r.indirect_launches) + r.batch_launches
    assert r.batch_launches == base.batch_launches and r.slice_batch == base.slice_batch and r.fuse_macs == base.fuse_macs
    # against the host: the complex128 contraction along the same path, and the same of the moduli
    p = ctr.plan(res.path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, slices=res.slices, dtype=np.complex64)
    kt = sum(op["K"] for op in p.ops) + n
    _, mag = hn.host_contract(res.path, tn.ts_inds, [np.abs(a) for a in arrays], tn.output_inds)
    order = [hn._ref_inds(tn, res).index(x) for x in r.inds]
    err = np.linalg.norm(np.ravel(r.array - ref.transpose(order)))
    bound = (2 * kt + 2) * 2.0 ** -24 * np.linalg.norm(np.ravel(mag))
    print(f"|| got - ref || = {err:.3e}, bound {bound:.3e} (kt {kt})")
    assert err <= bound
