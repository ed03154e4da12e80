"""Whole networks through optimize(max_width=...) -> contract_results(storage=...): what the storage mode costs in
accuracy, measured against a numpy emulation of the same rounding.

Three distances to a complex128 host contraction of the original arrays, relative, by norm:
    e_dev   the storage-mode call;
    e_emul  a numpy interpreter of the same path and slices in complex128 that rounds the leaves and every
            intermediate to storage with the engine's host function (`contraction.round_to_storage`);
    e_f32   the engine with storage=None.
Required: e_dev <= 2 e_emul + e_f32.  The emulation is the measure of what the mode costs; device and emulation differ
by one-storage-ulp flips at each stored step (the device rounds a float32 sum, the emulation a complex128 one), which
are of the size of the roundings themselves: hence the 2.  tools/half_profile.py writes the three numbers per network
and storage type into profiles/contract_half.txt.

The arrays are standard normal times 2^-3/4: in a 3-regular network of dimension 2 a sub-network's values then neither
grow nor shrink by more than about 2^-t/4 over t tensors, and stay in float16's normal range.
"""
import itertools
import math

import numpy as np
import pytest

from tnco_amd import synthetic as syn
from tnco_amd.app import tn as tnmod
from tnco_amd.app.app import Optimizer

pytestmark = pytest.mark.gpu

NETWORKS = ("closed", "open")
STORAGES = ("float16", "bfloat16")


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def _sym(inds):
    table = {i: k for k, i in enumerate(dict.fromkeys(inds))}
    return table.__getitem__


def host_contract(path, ts_inds, arrays, output_inds, store=lambda a: a):
    """Pairwise einsum along the path in complex128, axes in the index-only contract's order; `store` is applied to
    every intermediate (not to the last result)."""
    ts, arrs = [tuple(x) for x in ts_inds], [np.asarray(a, np.complex128) for a in arrays]
    left, out = tnmod.get_hyper_count(ts), frozenset(output_inds)
    for n, (a, b) in enumerate(path):
        a, b = sorted((a, b))
        yb, y = ts.pop(b), arrs.pop(b)
        xa, x = ts.pop(a), arrs.pop(a)
        shared = set(xa) & set(yb)
        stay = {i for i in shared if left[i] > 1 or i in out}
        for i in shared:
            left[i] -= 1
        z = tuple(i for i in xa if i in stay) + tuple(i for i in xa if i not in shared) + \
            tuple(i for i in yb if i not in shared)
        s = _sym(xa + yb)
        r = np.einsum(x, [*map(s, xa)], y, [*map(s, yb)], [*map(s, z)])
        arrs.append(r if n == len(path) - 1 else store(r))
        ts.append(z)
    (inds,), (array,) = ts, arrs
    return inds, array


def emulate(ctr, path, ts_inds, arrays, output_inds, slices, dims, inds, storage):
    """The sliced run as the engine does it, in complex128: leaves and intermediates rounded to storage, every
    assignment's result added (or placed, for a sliced index the result holds) unrounded."""
    store = lambda a: ctr.round_to_storage(a.astype(np.complex64), storage).astype(np.complex128)  # noqa: E731
    leaves = [store(np.asarray(a)) for a in arrays]
    cut = [x for x in dict.fromkeys(x for xs in ts_inds for x in xs) if x in set(slices)]
    total = np.zeros([dims[x] for x in inds], np.complex128)
    for values in itertools.product(*(range(dims[x]) for x in cut)):
        at = dict(zip(cut, values))
        part = [a[tuple(at.get(x, slice(None)) for x in xs)] for xs, a in zip(ts_inds, leaves)]
        part_inds = [tuple(x for x in xs if x not in at) for xs in ts_inds]
        z, r = host_contract(path, part_inds, part, [x for x in output_inds if x not in at], store)
        rest = [x for x in inds if x not in at]
        total[tuple(at.get(x, slice(None)) for x in inds)] += r.transpose([z.index(x) for x in rest])
    return total


def _network(kind):
    if kind == "closed":
        ts, d, _ = syn.random_regular_tn(40, seed=3)
        ts = [tuple(xs) for xs in ts]
    else:  # three tensors get an open leg each
        ts, d, _ = syn.random_regular_tn(36, seed=4)
        top = max(x for xs in ts for x in xs)
        ts = [tuple(xs) + ((top + 1 + (3, 17, 30).index(k),) if k in (3, 17, 30) else ()) for k, xs in enumerate(ts)]
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs), tags=dict(name=f"t{k}")) for k, xs in enumerate(ts)])
    rng = np.random.RandomState(31 + len(ts))
    arrays = [((rng.standard_normal((d,) * len(xs)) + 1j * rng.standard_normal((d,) * len(xs))) * 2.0 ** -1.25
               ).astype(np.complex64) for xs in ts]  # (each part 2^-1.25 sigma: modulus 2^-3/4 rms)
    return tn0, arrays


_CACHE = {}


def optimized(kind):
    """(tn0, arrays, tn, result, reference): one optimization and one complex128 reference per network, shared."""
    if kind not in _CACHE:
        tn0, arrays = _network(kind)
        tn, res = Optimizer(method="sa", max_width=MAX_WIDTH[kind], seed=0).optimize(tn0, betas=(0, 50), n_steps=100,
                                                                                    n_runs=128, fuse=None)
        _, ref = host_contract(res[0].path, tn.ts_inds, arrays, tn.output_inds)
        _CACHE[kind] = (tn0, arrays, tn, res[0], ref)
    return _CACHE[kind]


MAX_WIDTH = dict(closed=5, open=5)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def measure(ctr, kind, storage):
    """(e_dev, e_emul, e_f32, the storage-mode result, the storage=None result)."""
    tn0, arrays, tn, res, ref = optimized(kind)
    plain = ctr.contract_results(tn0, arrays, tn, res)
    half = ctr.contract_results(tn0, arrays, tn, res, storage=storage)
    assert half.inds == plain.inds and half.array.dtype == np.complex64
    final, _ = tnmod.contract(res.path, tn.ts_inds, tn.output_inds, tn0.dims)
    assert tuple(final[0]) == tuple(half.inds)
    emul = emulate(ctr, res.path, tn.ts_inds, arrays, tn.output_inds, res.slices, tn0.dims, half.inds, storage)
    ref = ref.transpose([_ref_inds(tn, res).index(x) for x in half.inds]) if half.inds else ref
    return _rel(half.array, ref), _rel(emul, ref), _rel(plain.array, ref), half, plain


def _ref_inds(tn, res):
    return tuple(tnmod.contract(res.path, tn.ts_inds, tn.output_inds)[0][0])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", NETWORKS)
def test_storage_mode_costs_what_its_rounding_costs(ctr, kind, storage):
    _, _, tn, res, _ = optimized(kind)
    assert 2 <= len(res.slices) <= 4, res.slices
    assert (len(tn.output_inds) > 0) == (kind == "open")
    e_dev, e_emul, e_f32, half, plain = measure(ctr, kind, storage)
    print(f"{kind} {storage}: e_dev {e_dev:.3e}  e_emul {e_emul:.3e}  e_f32 {e_f32:.3e}  slices {len(res.slices)}")
    assert e_dev <= 2 * e_emul + e_f32
    assert half.macs == plain.macs and half.n_slices == plain.n_slices == math.prod(2 for _ in res.slices)
    assert half.peak_device_bytes < plain.peak_device_bytes
    again = ctr.contract_results(*optimized(kind)[:4], storage=storage)
    assert np.array_equal(again.array, half.array)
