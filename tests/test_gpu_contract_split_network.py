"""A whole network through optimize(max_width=...) -> contract_results(compute="bf16x3"): what the compute mode costs in
accuracy, measured against a numpy emulation of the same split.

The network is a chain of four matrices of 256 x 256 whose row and column are four indices of dimension 4 each, the two
ends open: every step of any sensible path is of the tiled shape class (M, N >= 64 and K > 32), and stays so when
max_width = 14 slices an index away (the tensors have width 16).

Three distances to a complex128 host contraction of the original arrays, relative, by norm:
    e_dev   the compute-mode call;
    e_emul  a numpy interpreter of the same path and slices in complex128 that, at the steps `Plan.ops` shows to be of
            the tiled class, takes both operands as complex64, splits them with `contraction.split_bf16` and sums
            lo hi + hi lo + hi hi;
    e_f32   the engine with compute=None.
Required: e_dev <= 2 e_emul + e_f32 -- the emulation is the measure of what the split costs, the device adds its
float32 sums to it, and device and emulation split intermediates that differ by those sums (hence the 2) -- and e_dev
below the error of storage="bfloat16" on the same network.  tools/split_profile.py writes the numbers into
profiles/contract_split.txt.
"""
import itertools

import numpy as np
import pytest

from tnco_amd.app import tn as tnmod
from tnco_amd.app.app import Optimizer

pytestmark = pytest.mark.gpu

MAX_WIDTH = 14
COMPUTE = "bf16x3"


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def _network():
    groups = [tuple(range(4 * g, 4 * g + 4)) for g in range(5)]  # g0 | g1 | g2 | g3 | g4: g0 and g4 stay open
    ts = [groups[t] + groups[t + 1] for t in range(4)]
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [4] * len(xs), tags=dict(name=f"t{k}")) for k, xs in enumerate(ts)])
    rng = np.random.RandomState(81)
    arrays = [((rng.standard_normal((4,) * 8) + 1j * rng.standard_normal((4,) * 8)) * 2.0 ** -3).astype(np.complex64)
              for _ in ts]
    return tn0, arrays


def _sym(inds):
    table = {i: k for k, i in enumerate(dict.fromkeys(inds))}
    return table.__getitem__


def host_contract(ctr, path, ts_inds, arrays, output_inds, split_steps=()):
    """Pairwise einsum along the path in complex128, axes in the index-only contract's order; at the steps of
    `split_steps` the product is that of the split kernel."""
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
        mul = lambda p, q: np.einsum(p, [*map(s, xa)], q, [*map(s, yb)], [*map(s, z)], optimize=True)  # noqa: E731
        if n in split_steps:
            (xh, xl), (yh, yl) = (tuple(q.astype(np.complex128) for q in ctr.split_bf16(v.astype(np.complex64))) for v in (x, y))
            r = mul(xl, yh) + mul(xh, yl) + mul(xh, yh)
        else:
            r = mul(x, y)
        arrs.append(r)
        ts.append(z)
    (inds,), (array,) = ts, arrs
    return inds, array


def emulate(ctr, path, ts_inds, arrays, output_inds, slices, dims, inds, split_steps):
    """The sliced run as the engine does it, in complex128: every assignment's result added (or placed, for a sliced
    index the result holds)."""
    cut = [x for x in dict.fromkeys(x for xs in ts_inds for x in xs) if x in set(slices)]
    total = np.zeros([dims[x] for x in inds], np.complex128)
    for values in itertools.product(*(range(dims[x]) for x in cut)):
        at = dict(zip(cut, values))
        part = [np.asarray(a)[tuple(at.get(x, slice(None)) for x in xs)] for xs, a in zip(ts_inds, arrays)]
        part_inds = [tuple(x for x in xs if x not in at) for xs in ts_inds]
        z, r = host_contract(ctr, path, part_inds, part, [x for x in output_inds if x not in at], split_steps)
        rest = [x for x in inds if x not in at]
        total[tuple(at.get(x, slice(None)) for x in inds)] += r.transpose([z.index(x) for x in rest])
    return total


_CACHE = {}


def optimized(ctr):
    """(tn0, arrays, tn, result, reference in the result's axis order, the steps of the tiled class): shared."""
    if not _CACHE:
        tn0, arrays = _network()
        tn, res = Optimizer(method="sa", max_width=MAX_WIDTH, seed=0).optimize(tn0, betas=(0, 50), n_steps=100, n_runs=128,
                                                                             fuse=None)
        res = res[0]
        p = ctr.plan(res.path, tn.ts_inds, [a.shape for a in arrays], tn.output_inds, slices=res.slices,
                     dtype=np.complex64, compute=COMPUTE)
        tiled = frozenset(k for k, op in enumerate(p.ops) if op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32)
        z, ref = host_contract(ctr, res.path, tn.ts_inds, arrays, tn.output_inds)
        _CACHE["v"] = (tn0, arrays, tn, res, ref.transpose([z.index(x) for x in p.inds]), tiled, p)
    return _CACHE["v"]


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def measure(ctr):
    """(e_dev, e_emul, e_f32, e_bf16, the compute-mode result, the compute=None result)."""
    tn0, arrays, tn, res, ref, tiled, p = optimized(ctr)
    plain = ctr.contract_results(tn0, arrays, tn, res)
    split = ctr.contract_results(tn0, arrays, tn, res, compute=COMPUTE)
    stored = ctr.contract_results(tn0, arrays, tn, res, storage="bfloat16")
    assert split.inds == plain.inds == p.inds and split.array.dtype == np.complex64
    emul = emulate(ctr, res.path, tn.ts_inds, arrays, tn.output_inds, res.slices, tn0.dims, split.inds, tiled)
    return _rel(split.array, ref), _rel(emul, ref), _rel(plain.array, ref), _rel(stored.array, ref), split, plain


def test_the_compute_mode_costs_what_its_split_costs(ctr):
    _, _, tn, res, _, tiled, p = optimized(ctr)
    assert len(res.slices) >= 1 and len(tiled) >= 1, (res.slices, p.ops)
    e_dev, e_emul, e_f32, e_bf16, split, plain = measure(ctr)
    print(f"chain: e_dev {e_dev:.3e}  e_emul {e_emul:.3e}  e_f32 {e_f32:.3e}  storage bfloat16 {e_bf16:.3e}  "
          f"slices {len(res.slices)}  split steps {len(tiled)} of {len(p.ops)}")
    assert split.split_launches == len(tiled) * split.n_slices > 0 and plain.split_launches == 0
    assert split.compute == COMPUTE and plain.compute is None
    assert split.kernel_launches == plain.kernel_launches and split.launches == plain.launches
    assert split.macs == plain.macs and split.n_slices == plain.n_slices
    assert split.peak_device_bytes == plain.peak_device_bytes
    assert e_dev <= 2 * e_emul + e_f32
    assert e_dev < e_bf16
    again = ctr.contract_results(*optimized(ctr)[:4], compute=COMPUTE)
    assert np.array_equal(again.array, split.array)
    batched = ctr.contract_results(*optimized(ctr)[:4], compute=COMPUTE, slice_batch=4)
    assert np.array_equal(batched.array, split.array) and batched.split_launches == len(tiled) * -(-split.n_slices // 4)
