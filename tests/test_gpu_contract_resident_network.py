"""A whole network through optimize(max_width=...) -> Contractor(result.path, slices=result.slices, path_kernel=64) with
every leaf bound from a torch tensor and the result left on the device: bit for bit the result of `contract()` with the
same keywords.  The network, its arrays, its optimization (loaded with fuse=None) and its complex128 host reference are
those of tests/test_gpu_contract_half_network.py (shared with it).

Two equal wrong answers would pass that, so the result is also held to the host einsum along the same path by the norm
bound of the plain run (tests/test_gpu_contract_path_network.py):

    || got - ref || <= (2 kt + 2) u || mag ||       u = 2^-24

with mag the same contraction of the moduli of the arrays and kt = the sum of K over the steps of the path + the
assignments added into an element.  A second run with one leaf bound again must equal `contract()` on the changed arrays.
"""
import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def as_bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def counters(r):
    return {k: v for k, v in vars(r).items() if k not in ("array", "device_s")}


def test_a_sliced_network_bound_from_torch_equals_contract(ctr):
    import torch
    tn0, arrays, tn, res, ref = hn.optimized("open")
    n = 2 ** len(res.slices)
    assert n >= 4
    arrays = [np.asarray(a) for a in arrays]
    assert {a.dtype for a in arrays} == {np.dtype(np.complex64)}
    kw = dict(slices=res.slices, path_kernel=64)
    base = ctr.contract(res.path, tn.ts_inds, arrays, tn.output_inds, **kw)
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    with ctr.Contractor(res.path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, dtype=np.complex64, **kw) as c:
        c.bind(dict(enumerate(tensors)))
        r = c.run()
        assert isinstance(r.array, np.ndarray)  # (no arrays and no out: numpy)
        assert np.array_equal(as_bits(r.array), as_bits(base.array))
        out = torch.empty(c.plan.shape, dtype=torch.complex64, device="cuda")
        r = c.run(out=out)
        assert r.array is out and counters(r) == counters(base)
        got = out.cpu().numpy()
        assert got.dtype == base.array.dtype and got.shape == base.array.shape
        assert np.array_equal(as_bits(got), as_bits(base.array))
        assert np.isfinite(got).all() and got.any()
        assert r.path_launches == (-(-n // 64),) * 2 and r.n_slices == n
        assert c.io_launches == (len(arrays), 1)
        # against the host: the complex128 contraction along the same path, and the same of the moduli
        kt = sum(op["K"] for op in c.plan.ops) + n
        _, mag = hn.host_contract(res.path, tn.ts_inds, [np.abs(a) for a in arrays], tn.output_inds)
        order = [hn._ref_inds(tn, res).index(x) for x in r.inds]
        err = np.linalg.norm(np.ravel(got - ref.transpose(order)))
        bound = (2 * kt + 2) * 2.0 ** -24 * np.linalg.norm(np.ravel(mag))
        print(f"|| got - ref || = {err:.3e}, bound {bound:.3e} (kt {kt})")
        assert err <= bound
        # one leaf bound again, the others stay
        t = max(range(len(arrays)), key=lambda q: arrays[q].size)
        changed = list(arrays)
        changed[t] = (arrays[t] * np.complex64(0.5 - 0.25j)).astype(np.complex64)
        c.bind({t: torch.from_numpy(changed[t]).cuda()})
        again = c.run(out=out)
        want = ctr.contract(res.path, tn.ts_inds, changed, tn.output_inds, **kw)
        assert np.array_equal(as_bits(out.cpu().numpy()), as_bits(want.array)) and counters(again) == counters(want)
        assert not np.array_equal(as_bits(want.array), as_bits(base.array))
        assert c.io_launches == (len(arrays) + 1, 2)
