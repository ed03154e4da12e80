"""A whole network through optimize(max_width=...) -> contract_results(..., reuse=True), with the sliced indices in
the default order and in the order slice_order="reuse" picks: bit for bit the result of the same call without `reuse` under
the same order, with no more multiply-adds than `hoist=True`, and inside the norm bound of the plain run
(tests/test_gpu_contract_path_network.py).  The network, its arrays and its optimization are those of
tests/test_gpu_contract_hoist_network.py (tests/test_gpu_contract_half_network.py)."""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("kw", [dict(), dict(slice_order="reuse"), dict(slice_order="reuse", indirect=True)],
                         ids=["default-order", "reuse-order", "reuse-order-indirect"])
def test_a_sliced_network_reused_equals_the_same_call_without_the_keyword(ctr, kw):
    tn0, arrays, tn, res, ref = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    mode = {k: v for k, v in kw.items() if k != "slice_order"}
    shapes = [a.shape for a in arrays]
    p = ctr.plan(res.path, tn.ts_inds, shapes, tn.output_inds, slices=res.slices, dtype=np.complex64, reuse=True, **kw)
    r = ctr.contract_results(tn0, arrays, tn, res, reuse=True, **kw)
    base = ctr.contract_results(tn0, arrays, tn, res, slice_order=p.slice_inds, **mode)  # (the order that was used)
    hoisted = ctr.contract_results(tn0, arrays, tn, res, hoist=True, **mode)
    assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.complex64
    as_bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(as_bits(r.array), as_bits(base.array))
    assert np.isfinite(r.array).all() and r.array.any()
    assert base.reused is None and r.reused == p.reused and r.hoisted is None
    assert r.macs == p.macs <= hoisted.macs <= base.macs and r.n_slices == base.n_slices == n
    assert (r.macs < base.macs) == (p.reused[0] > 0)
    assert r.launches == sum(r.kernel_launches) + sum(r.indirect_launches) and r.fuse_macs == base.fuse_macs
    assert r.indirect == p.indirect
    print(f"{kw}: order {p.slice_inds}, periods {p.step_period.tolist()}, macs reuse {r.macs} hoist {hoisted.macs} plain {base.macs}, "
          f"launches {r.launches} / {base.launches}, kept {len(p.kept)}")
    again = ctr.contract_results(tn0, arrays, tn, res, reuse=True, **kw)
    assert np.array_equal(as_bits(again.array), as_bits(r.array))
    # against the host: the complex128 contraction along the same path, and the same of the moduli
    kt = sum(op["K"] for op in p.ops) + n
    _, mag = hn.host_contract(res.path, tn.ts_inds, [np.abs(a) for a in arrays], tn.output_inds)
    order = [hn._ref_inds(tn, res).index(x) for x in r.inds]
    err = np.linalg.norm(np.ravel(r.array - ref.transpose(order)))
    bound = (2 * kt + 2) * 2.0 ** -24 * np.linalg.norm(np.ravel(mag))
    print(f"|| got - ref || = {err:.3e}, bound {bound:.3e} (kt {kt})")
    assert err <= bound
