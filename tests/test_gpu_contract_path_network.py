"""A whole network through optimize(max_width=...) -> contract_results(..., path_kernel=64): bit for bit the result of the
default call.  The network, its arrays, its optimization and its complex128 host reference are those of
tests/test_gpu_contract_half_network.py (shared with it).

Two equal wrong answers would pass that, so the result is also held to the host einsum along the same path, by norm:

    || got - ref || <= (2 kt + 2) u || mag ||       u = 2^-24

with mag the same contraction of the moduli of the arrays (every term of every sum with its sign and phase removed) and
kt = the sum of K over the steps of the path + the assignments added into an element: no term goes through more
roundings than that, whichever tensors it comes from (first order, as in tests/test_gpu_contract_kernels.py; 2 for the
four real products of a complex one).
"""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn
from tnco_amd.app.app import cost_to_decimal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def test_a_sliced_network_in_one_group_of_the_path_kernel_equals_the_default_call(ctr):
    tn0, arrays, tn, res, ref = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    base = ctr.contract_results(tn0, arrays, tn, res)
    r = ctr.contract_results(tn0, arrays, tn, res, path_kernel=64)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.complex64
    as_bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(as_bits(r.array), as_bits(base.array))
    assert np.isfinite(r.array).all() and r.array.any()
    assert r.macs == base.macs and cost_to_decimal(r.macs) == res.cost
    assert r.n_slices == base.n_slices == n
    groups = -(-n // 64)
    assert r.path_kernel == min(64, n) and base.path_kernel is None
    assert r.path_launches == (groups, groups) and base.path_launches == (0, 0)
    assert r.launches == 2 * groups < base.launches
    assert r.kernel_launches == (0,) * len(ctr.KERNEL_PATHS) and r.row_kernel_launches == (0, 0, 0)
    assert r.batch_launches == 0 and r.fuse_macs == base.fuse_macs
    assert r.peak_device_bytes > base.peak_device_bytes
    # against the host: the complex128 contraction along the same path, and the same of the moduli
    p = ctr.plan(res.path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, slices=res.slices, dtype=np.complex64)
    kt = sum(op["K"] for op in p.ops) + n
    _, mag = hn.host_contract(res.path, tn.ts_inds, [np.abs(a) for a in arrays], tn.output_inds)
    order = [hn._ref_inds(tn, res).index(x) for x in r.inds]
    err = np.linalg.norm(np.ravel(r.array - ref.transpose(order)))
    bound = (2 * kt + 2) * 2.0 ** -24 * np.linalg.norm(np.ravel(mag))
    print(f"|| got - ref || = {err:.3e}, bound {bound:.3e} (kt {kt}); relative to || ref ||: {hn._rel(r.array, ref.transpose(order)):.3e}")
    assert err <= bound
