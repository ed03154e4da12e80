"""Whole networks contracted at projections of their sparse indices on the GPU (`contract(..., sparse_inds=, projs=)`,
`contract_results(..., projs=)`), against the pairwise host einsum of the dense output indexed at `projs`; tolerance
TOL[dtype] of tests/test_gpu_contraction.py by relative norm.  Sliced runs, reproducibility, slice_range partitions,
`projs` = every assignment against the dense contraction and the sparse cost model, and optimize(n_projs=) ->
contract_results(projs=) end to end."""
import itertools
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


def _sym(inds):
    table = {i: k for k, i in enumerate(dict.fromkeys(inds))}
    return table.__getitem__


def _host(path, ts_inds, arrays, output_inds):
    """Pairwise einsum along the path in double precision, axes in the index-only contract's order (tn.contract)."""
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


def _at_projs(inds, dense, sparse, projs):
    """(("proj",) + the other axes in their order, dense[..., sparse = projs[p], ...] for every p)."""
    rest = tuple(x for x in inds if x not in sparse)
    z = dense.transpose([inds.index(x) for x in tuple(sparse) + rest])
    return ("proj",) + rest, z[tuple(np.asarray(projs).T)]


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _arrays(ts_inds, dims, dtype, seed):
    rng = np.random.RandomState(seed)
    out = []
    for xs in ts_inds:
        shape = tuple(dims[x] for x in xs)
        a = rng.standard_normal(shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.standard_normal(shape)
        out.append((a / math.sqrt(max(1, math.prod(shape)))).astype(dtype))
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
    """A hyper-index network with five output indices, three of them sparse (hyper-indices among them)."""
    ts, d, o = syn.random_hyper_tn(12, 20, k=3, n_output=5, seed=seed, dims_choices=(2, 3, 4))
    dims = {i: int(x) for i, x in enumerate(d)}
    o = tuple(o)
    assert len(o) == 5
    return ts, dims, o, (o[3], o[0], o[2])


def _projs(dims, sparse, P, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, dims[x], P) for x in sparse], axis=1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_dtypes_on_a_hyper_network(ctr, dtype):
    ts, dims, o, sparse = _hyper()
    assert any(c > 1 for c in tnmod.get_hyper_count(ts).values())
    path = _greedy_path(ts)
    arrays = _arrays(ts, dims, dtype, 1)
    projs = _projs(dims, sparse, 23, 2)
    projs[5] = projs[20]
    r = ctr.contract(path, ts, arrays, o, sparse_inds=sparse, projs=projs)
    final, (dense,) = _host(path, ts, arrays, o)
    inds, ref = _at_projs(final[0], dense, sparse, projs)
    assert r.inds == inds and r.array.shape == ref.shape and r.array.dtype == np.dtype(dtype)
    assert _rel(r.array, ref) <= TOL[dtype]
    assert np.array_equal(r.array[5], r.array[20])
    p = ctr.plan(path, ts, [a.shape for a in arrays], o, sparse_inds=sparse, projs=projs)
    assert r.macs == p.macs and sum(r.row_kernel_launches) > 0
    assert r.launches == sum(r.kernel_launches) + sum(r.row_kernel_launches)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_sliced_runs_repeat_bit_for_bit_and_partition(ctr, dtype):
    ts, dims, o, sparse = _hyper(seed=11)
    path = _greedy_path(ts)
    final = tnmod.contract(path, ts, o, dims)[0][0]
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    cut = [x for x in every if x in final and x not in sparse][:1] + [x for x in every if x not in final][:4]
    n = math.prod(dims[x] for x in cut)
    assert n >= 16 and cut[0] in final
    arrays = _arrays(ts, dims, dtype, 4)
    projs = _projs(dims, sparse, 17, 3)
    kw = dict(slices=cut, sparse_inds=sparse, projs=projs)
    r = ctr.contract(path, ts, arrays, o, **kw)
    _, (dense,) = _host(path, ts, arrays, o)
    inds, ref = _at_projs(final, dense, sparse, projs)
    assert r.n_slices == n and r.inds == inds
    assert _rel(r.array, ref) <= TOL[dtype]
    p = ctr.plan(path, ts, [a.shape for a in arrays], o, **kw)
    assert r.macs == p.macs and p.block_inds == (cut[0],)
    again = ctr.contract(path, ts, arrays, o, **kw)
    assert np.array_equal(again.array, r.array)  # bit-identical
    cuts = [0, n // 5, n // 2, n - 1, n]
    parts = [ctr.contract(path, ts, arrays, o, slice_range=(a, b), **kw) for a, b in zip(cuts, cuts[1:])]
    assert sum(q.n_slices for q in parts) == n
    assert _rel(sum(q.array for q in parts), r.array) <= TOL[dtype]


def _every(dims, sparse):
    return np.array(list(itertools.product(*(range(dims[x]) for x in sparse))), np.int64)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_every_assignment_is_the_dense_contraction(ctr, dtype):
    ts, dims, o, sparse = _hyper(seed=7)
    path = _greedy_path(ts)
    arrays = _arrays(ts, dims, dtype, 5)
    projs = _every(dims, sparse)
    r = ctr.contract(path, ts, arrays, o, sparse_inds=sparse, projs=projs)
    dense = ctr.contract(path, ts, arrays, o)
    inds, ref = _at_projs(tuple(dense.inds), dense.array, sparse, projs)
    assert r.inds == inds and _rel(r.array, ref) <= TOL[dtype]
    assert r.macs == dense.macs


def _sparse_network(n, seed, n_sparse):
    """A connected random regular network with an open index on some tensors: those are its output indices, the
    first n_sparse of them sparse."""
    ts, d, _ = syn.random_regular_tn(n, seed=seed)
    tensors, out = [], []
    for k, xs in enumerate(ts):
        xs = tuple(xs) + ((f"o{k}",) if k % 3 == 0 else ())
        out += [x for x in xs if isinstance(x, str)]
        tensors.append(tnmod.Tensor(xs, [d] * len(xs), tags=dict(name=f"t{k}")))
    return tnmod.TensorNetwork(tensors, output_inds=out, sparse_inds=out[:n_sparse])


@pytest.mark.parametrize("subset", [False, True])
def test_optimize_with_n_projs_then_contract_results(ctr, subset):
    """The loop closed for the sparse cost model: an infinite-memory path optimized for P projections runs on arrays;
    with every assignment the multiply-adds launched are the cost the optimizer reported, with fewer they are at
    most that."""
    tn0 = _sparse_network(24, seed=6, n_sparse=5)
    dims = tn0.dims
    sparse = sorted(tn0.sparse_inds, key=str)
    projs = _every(dims, sparse)
    if subset:
        projs = projs[np.random.RandomState(0).choice(len(projs), 11, replace=False)]
    P = len(projs)
    tn, res = Optimizer(method="sa", seed=0).optimize(tn0, betas=(0, 50), n_steps=100, n_runs=64, n_projs=P,
                                                      fuse=None, decompose_hyper_inds=False)
    assert "fuse_path" not in tn.tags and set(tn.sparse_inds) == set(sparse)
    arrays = _arrays(tn0.ts_inds, dims, np.float64, 7)
    r = ctr.contract_results(tn0, {t.tags["name"]: a for t, a in zip(tn0.tensors, arrays)}, tn, res[0], projs=projs)
    if subset:
        assert cost_to_decimal(r.macs) <= res[0].cost
    else:
        assert cost_to_decimal(r.macs) == res[0].cost
    final, (dense,) = _host(res[0].path, tn0.ts_inds, arrays, tn0.output_inds)
    inds, ref = _at_projs(final[0], dense, tuple(sparse), projs)
    assert r.inds == inds and r.array.shape[0] == P
    assert _rel(r.array, ref) <= TOL[np.float64]
    with pytest.raises(NotImplementedError, match="projs="):
        ctr.contract_results(tn0, arrays, tn, res[0])


def test_contract_results_from_the_string_form(ctr):
    """The index-list form load_tn reads: a line per index, its dimension and the tensors that hold it; `*` among
    them marks an output index, `/` a sparse one."""
    text = "\n".join(["2 A B", "3 B C", "2 C D", "2 D A", "3 A C * /", "2 B * /", "2 D * /", "2 D *", "2 A B C *"])
    tn0 = tnmod.load_tn(text, fuse=None, decompose_hyper_inds=False)
    assert tn0.sparse_inds == {4, 5, 6} and tn0.output_inds == {4, 5, 6, 7, 8}
    sparse = sorted(tn0.sparse_inds, key=str)
    dims = tn0.dims
    projs = _projs(dims, sparse, 6, 1)
    tn, res = Optimizer(method="sa", seed=0).optimize(tn0, betas=(0, 10), n_steps=20, n_runs=8, n_projs=6, fuse=None,
                                                      decompose_hyper_inds=False)
    arrays = _arrays(tn0.ts_inds, dims, np.complex128, 9)
    r = ctr.contract_results(tn0, arrays, tn, res[0], projs=projs)
    final, (dense,) = _host(res[0].path, tn0.ts_inds, arrays, tn0.output_inds)
    inds, ref = _at_projs(final[0], dense, tuple(sparse), projs)
    assert r.inds == inds and _rel(r.array, ref) <= TOL[np.complex128]
    back = ctr.contract_results(tn0, arrays, tn, res[0], projs=projs[:, ::-1], sparse_inds=sparse[::-1])
    assert np.array_equal(back.array, r.array)
