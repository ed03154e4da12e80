"""The contraction engine on the GPU (tnco_amd/contraction.py, csrc/contract.hip) against an independent host
contraction: numpy einsum pairwise along the same path, unsliced, and np.einsum of the whole network where it has few
enough indices.  Every dtype, the tiled / streaming / split-K GEMM shapes, sliced runs (summed, block and hyper
indices), reproducibility, slice_range partitions, and optimize() -> contract_results() end to end."""
import math

import numpy as np
import pytest

from tnco_amd import synthetic as syn
from tnco_amd.app import tn as tnmod
from tnco_amd.app.app import Optimizer, cost_to_decimal

pytestmark = pytest.mark.gpu

TOL = {np.float32: 1e-5, np.complex64: 1e-5, np.float64: 1e-11, np.complex128: 1e-11}


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def _host(path, ts_inds, arrays, output_inds):
    """Pairwise einsum along the path, axes in the index-only contract's order (tn.contract)."""
    ts, arrs = [tuple(x) for x in ts_inds], [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64)
                                             for a in arrays]
    left, out = tnmod.get_hyper_count(ts), frozenset(output_inds)
    for a, b in path:
        a, b = sorted((a, b))
        yb, y = ts.pop(b), arrs.pop(b)
        xa, x = ts.pop(a), arrs.pop(a)
        shared = set(xa) & set(yb)
        stay = {i for i in shared if left[i] > 1 or i in out}
        for i in shared:
            left[i] -= 1
        z = tuple(i for i in xa if i in stay) + tuple(i for i in xa if i not in shared) + \
            tuple(i for i in yb if i not in shared)
        arrs.append(np.einsum(x, [*map(_sym(xa + yb), xa)], y, [*map(_sym(xa + yb), yb)], [*map(_sym(xa + yb), z)]))
        ts.append(z)
    return ts, arrs


def _sym(inds):
    table = {i: k for k, i in enumerate(dict.fromkeys(inds))}
    return table.__getitem__


def _einsum_all(ts_inds, arrays, final):
    every = list(dict.fromkeys(x for xs in ts_inds for x in xs))
    if len(every) > 52:
        return None
    sym = {x: k for k, x in enumerate(every)}
    ops = []
    for xs, a in zip(ts_inds, arrays):
        ops += [a, [sym[x] for x in xs]]
    return np.einsum(*ops, [sym[x] for x in final], optimize="greedy")


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _arrays(ts_inds, dims, dtype, seed, positive=False):
    rng = np.random.RandomState(seed)
    out = []
    for xs in ts_inds:
        shape = tuple(dims[x] for x in xs)
        a = rng.uniform(0.5, 1.5, shape) if positive else rng.standard_normal(shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * (rng.uniform(0.5, 1.5, shape) if positive else rng.standard_normal(shape))
        scale = math.sqrt(max(1, math.prod(shape)))
        out.append((a / scale).astype(dtype))
    return out


def _greedy_path(ts_inds):
    ts = [set(x) for x in ts_inds]
    path = []
    while len(ts) > 1:
        a, b = next(((a, b) for a in range(len(ts)) for b in range(a + 1, len(ts)) if ts[a] & ts[b]), (0, 1))
        tb, ta = ts.pop(b), ts.pop(a)
        ts.append(ta | tb)
        path.append((a, b))
    return path


def _hyper(seed=5):
    ts, d, o = syn.random_hyper_tn(12, 20, k=3, n_output=3, seed=seed, dims_choices=(2, 3, 4))
    return ts, {i: int(x) for i, x in enumerate(d)}, o


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_dtypes_on_a_hyper_network(ctr, dtype):
    ts, dims, o = _hyper()
    path = _greedy_path(ts)
    arrays = _arrays(ts, dims, dtype, 1)
    r = ctr.contract(path, ts, arrays, o)
    final, (ref,) = _host(path, ts, arrays, o)
    assert r.inds == final[0] and r.array.shape == ref.shape and r.array.dtype == np.dtype(dtype)
    assert _rel(r.array, ref) <= TOL[dtype]
    whole = _einsum_all(ts, arrays, final[0])
    assert _rel(r.array, whole) <= max(TOL[dtype], 1e-10)
    assert r.macs == ctr.plan(path, ts, [a.shape for a in arrays], o).macs


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("layout", [(("i", "k"), ("k", "j")), (("k", "i"), ("k", "j")), (("i", "k"), ("j", "k")),
                                    (("k", "i"), ("j", "k"))])
def test_large_square_step_takes_the_tiled_gemm(ctr, dtype, layout):
    dims = dict(i=530, k=515, j=512)
    arrays = _arrays(layout, dims, dtype, 2)
    r = ctr.contract([(0, 1)], layout, arrays)
    letter = dict(i="m", j="n", k="k")  # (the kernel path is named by the memory order of A, then of B)
    tiled = "tiled_" + "".join(letter[c] for c in layout[0]) + "_" + "".join(letter[c] for c in layout[1])
    assert dict(zip(ctr.KERNEL_PATHS, r.kernel_launches)) == {name: int(name == tiled) for name in ctr.KERNEL_PATHS}
    assert r.launches == 1
    ref = np.einsum(arrays[0].astype(np.complex128), [ord(c) - 97 for c in layout[0]],
                    arrays[1].astype(np.complex128), [ord(c) - 97 for c in layout[1]], [8, 9])
    assert r.inds == ("i", "j") and r.macs == 530 * 515 * 512
    assert _rel(r.array, ref) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.complex128])
def test_skinny_outer_and_long_sum_steps(ctr, dtype):
    cases = [
        ([("h", "i"), ("h", "j")], dict(h=64, i=300, j=200), ("h", "i", "j")),  # batched outer product, K = 1
        ([("i", "k"), ("k", "j")], dict(i=20000, k=8, j=4), None),  # skinny: K, N small
        ([("i", "k"), ("k",)], dict(i=4, k=70000), None),  # few outputs, long K: split over a block
        ([("k", "i"), ("k", "j")], dict(i=3, k=5000, j=2), None),
    ]
    for ts, dims, out in cases:
        arrays = _arrays(ts, dims, dtype, 3)
        r = ctr.contract([(0, 1)], ts, arrays, out)
        final, (ref,) = _host([(0, 1)], ts, arrays, out if out else tnmod.contract([], ts)[1])
        assert r.inds == final[0]
        assert _rel(r.array, ref) <= TOL[dtype], ts


def _sliced_case():
    ts, dims, o = _hyper(seed=11)
    path = _greedy_path(ts)
    final = tnmod.contract(path, ts, o, dims)[0][0]
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    summed = [x for x in every if x not in final]
    held = [x for x in every if x in final]
    cut, n = [held[0]], dims[held[0]]
    for x in summed:
        if n >= 96:
            break
        cut.append(x)
        n *= dims[x]
    return ts, dims, o, path, cut, n


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_sliced_runs_match_the_unsliced_host_contraction(ctr, dtype):
    ts, dims, o, path, cut, n = _sliced_case()
    assert n >= 64
    assert any(c > 1 for c in tnmod.get_hyper_count(ts).values())  # (a hyper-index network)
    arrays = _arrays(ts, dims, dtype, 4)
    r = ctr.contract(path, ts, arrays, o, slices=cut)
    final, (ref,) = _host(path, ts, arrays, o)
    assert r.n_slices == n and r.inds == final[0]
    assert _rel(r.array, ref) <= TOL[dtype]
    p = ctr.plan(path, ts, [a.shape for a in arrays], o, slices=cut)
    assert r.macs == p.macs and p.block_inds
    again = ctr.contract(path, ts, arrays, o, slices=cut)
    assert np.array_equal(again.array, r.array)  # bit-identical
    cuts = [0, n // 5, n // 2, n - 1, n]
    parts = [ctr.contract(path, ts, arrays, o, slices=cut, slice_range=(a, b)) for a, b in zip(cuts, cuts[1:])]
    assert sum(q.n_slices for q in parts) == n
    assert _rel(sum(q.array for q in parts), r.array) <= TOL[dtype]


def _network_tn(n, seed):
    ts, d, _ = syn.random_regular_tn(n, seed=seed)
    return tnmod.TensorNetwork([tnmod.Tensor(xs, [d] * len(xs), tags=dict(name=f"t{k}")) for k, xs in enumerate(ts)])


def _order_one(tn0, arrays):
    """The leaves scaled by one common factor so that the amplitude is 1 (positive entries: no cancellation)."""
    _, (ref,) = _host(_greedy_path(tn0.ts_inds), tn0.ts_inds, arrays, ())
    return [a * abs(float(ref)) ** (-1.0 / len(arrays)) for a in arrays]


@pytest.mark.parametrize("fuse", [None, 4])
def test_optimize_then_contract_results(ctr, fuse):
    """The loop closed: the finite-width optimizer's path and slices run on arrays; the numbers are those of the
    unsliced host contraction and the multiply-adds launched are the cost the optimizer reported."""
    tn0 = _network_tn(48, seed=6)
    tn, res = Optimizer(method="sa", max_width=6, seed=0).optimize(tn0, betas=(0, 50), n_steps=100, n_runs=128,
                                                                 fuse=fuse)
    assert res[0].slices and (fuse is None) == ("fuse_path" not in tn.tags)
    dims = tn0.dims
    arrays = _order_one(tn0, _arrays(tn0.ts_inds, dims, np.float64, 7, positive=True))
    r = ctr.contract_results(tn0, {t.tags["name"]: a for t, a in zip(tn0.tensors, arrays)}, tn, res[0])
    assert cost_to_decimal(r.macs) == res[0].cost
    assert r.n_slices == math.prod(dims[x] for x in res[0].slices)
    assert (r.fuse_macs > 0) == (fuse is not None)
    _, (ref,) = _host(_greedy_path(tn0.ts_inds), tn0.ts_inds, arrays, ())
    assert r.inds == () and 1e-3 < abs(float(ref)) < 1e3
    assert _rel(r.array, ref) <= 1e-11


def test_contract_results_of_a_disconnected_network(ctr):
    """Each component sliced by its own set, then the components joined."""
    a, b = _network_tn(20, seed=1), _network_tn(24, seed=2)
    tensors = list(a.tensors) + [tnmod.Tensor(tuple(("b", x) for x in t.inds), t.dims, tags=dict(name="b" + t.tags["name"]))
                                 for t in b.tensors]
    tn0 = tnmod.TensorNetwork(tensors)
    tn, res = Optimizer(method="sa", max_width=4, seed=1).optimize(tn0, betas=(0, 50), n_steps=60, n_runs=64, fuse=None)
    assert len([p for p in res[0].disconnected_paths if p]) == 2
    arrays = _order_one(tn0, _arrays(tn0.ts_inds, tn0.dims, np.float64, 8, positive=True))
    r = ctr.contract_results(tn0, arrays, tn, res[0])
    _, (ref,) = _host(_greedy_path(tn0.ts_inds), tn0.ts_inds, arrays, ())
    assert _rel(r.array, ref) <= 1e-11
    assert r.n_slices == sum(math.prod(2 for _ in s) for p, s in zip(res[0].disconnected_paths,
                                                                     res[0].disconnected_slices) if p)
