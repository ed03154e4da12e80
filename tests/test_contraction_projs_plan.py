"""The plan of a contraction at projections of sparse indices (tnco_amd/contraction.py, `sparse_inds=` / `projs=`),
without a GPU: the row tables and row maps against numpy.unique, the tables replayed by a numpy interpreter of the
device's semantics (rows included) against an einsum of the whole network indexed at the projections, the
multiply-adds against the dense plan and the sparse cost model, folding, every refusal, and the code objects of the
row-mapped kernels."""
import itertools
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn
from tnco_amd.app import tn as tnmod

ROOT = Path(__file__).resolve().parent.parent


def _greedy_path(ts_inds):
    ts = [set(x) for x in ts_inds]
    path = []
    while len(ts) > 1:
        a, b = next(((a, b) for a in range(len(ts)) for b in range(a + 1, len(ts)) if ts[a] & ts[b]), (0, 1))
        tb, ta = ts.pop(b), ts.pop(a)
        ts.append(ta | tb)
        path.append((a, b))
    return path


def _random_path(n, seed):
    rng = np.random.RandomState(seed)
    path = []
    while n > 1:
        a, b = rng.choice(n, 2, replace=False)
        path.append((int(a), int(b)))
        n -= 1
    return path


def _arrays(ts_inds, dims, seed):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal(tuple(dims[x] for x in xs)) / math.sqrt(max(1, math.prod(dims[x] for x in xs)))
            for xs in ts_inds]


def _network(seed, n_sparse=3):
    """A hyper-index network with an open index on some tensors; (ts, dims, output, sparse): the sparse indices are
    output indices, some of them hyper-indices held by several tensors."""
    ts, d, o = syn.random_hyper_tn(8, 12, k=3, n_output=3, seed=seed, dims_choices=(2, 3))
    ts = [tuple(x) + ((100 + t,) if t % 2 else ()) for t, x in enumerate(ts)]
    dims = {**{i: int(x) for i, x in enumerate(d)}, **{100 + t: 2 for t in range(8)}}
    output = tuple(o) + tuple(100 + t for t in range(8) if t % 2)
    rng = np.random.RandomState(seed)
    sparse = tuple(rng.permutation(np.array(output, object))[:n_sparse].tolist())
    return ts, dims, output, sparse


def _projs(dims, sparse, P, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, dims[x], P) for x in sparse], axis=1).reshape(P, len(sparse))


def _dense(ts, arrays, inds):
    sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in ts for x in xs))}
    ops = []
    for xs, a in zip(ts, arrays):
        ops += [a, [sym[x] for x in xs]]
    return np.einsum(*ops, [sym[x] for x in inds], optimize="greedy")


def _expected(path, ts, arrays, output, sparse, projs):
    """einsum(whole network)[..., sparse = projs[p], ...] for every p: (axes, array [P][rest])."""
    final = tuple(tnmod.contract(path, ts, output)[0][0])
    z = _dense(ts, arrays, final)
    rest = tuple(x for x in final if x not in sparse)
    z = z.transpose([final.index(x) for x in tuple(sparse) + rest])
    return ("proj",) + rest, z[tuple(np.asarray(projs).T)] if len(sparse) else np.broadcast_to(z, (len(projs),) + z.shape)


def _interpret(p, arrays):
    """The device semantics of the tables in numpy, rows included: leaves restricted to their rows, the gathers, and
    Z[r][h][m][n] = sum_k X[a_map[r]][h][m][k] Y[b_map[r]][h][k][n] per step; then the host's expansion to P rows."""
    W = ctr.MAX_AXES
    leaves = []
    for a, rows in zip(arrays, p.leaf_rows or (None,) * len(arrays)):
        a = np.asarray(a, p.dtype)
        if rows is not None:
            axes, values = rows
            a = np.stack([a[tuple(values[r, axes.index(k)] if k in axes else slice(None) for k in range(a.ndim))]
                          for r in range(len(values))])
        leaves.append(np.ascontiguousarray(a).ravel())
    assert [a.size for a in leaves] == p.leaf_numel.tolist()
    arena = np.zeros(max(p.arena_elems, 1), p.dtype)
    out = np.zeros(p.out_numel, p.dtype)
    n_blocks = math.prod(p.slice_dims[p.slice_inds.index(x)] for x in p.block_inds)
    block_numel = p.out_numel // n_blocks
    place = [math.prod(p.slice_dims[k + 1:]) for k in range(len(p.slice_dims))]
    digit = lambda sid, s: (sid // place[s]) % p.slice_dims[s]  # noqa: E731

    def leaf_off(t, sid):
        row = p.leaf_sl[t]
        return sum(digit(sid, int(row[1 + j])) * int(row[1 + W + j]) for j in range(int(row[0])))

    visited = set()
    for sid in range(*p.slice_range):
        blk = 0
        for x in p.block_inds:
            s = p.slice_inds.index(x)
            blk = blk * p.slice_dims[s] + digit(sid, s)
        beta = blk in visited
        visited.add(blk)
        for k in [-1] + list(range(len(p.steps))):
            writes = []
            for row in p.perms[p.perms[:, 6] == k]:
                nd = int(row[4])
                shape, strides = row[8:8 + nd], row[8 + W:8 + W + nd]
                src, base = (leaves[row[1]], leaf_off(int(row[1]), sid)) if row[0] == ctr.LEAF else (arena, int(row[1]))
                idx = np.full(tuple(shape), base, np.int64)
                for ax in range(nd):
                    sh = [1] * nd
                    sh[ax] = int(shape[ax])
                    idx = idx + (np.arange(shape[ax]) * strides[ax]).reshape(sh)
                writes.append((row, src[idx.ravel()].copy()))
            for row, vals in writes:
                if row[2] == ctr.ARENA:
                    arena[row[3]:row[3] + int(row[5])] = vals
                else:
                    out[blk * block_numel:(blk + 1) * block_numel] = vals
            if k < 0:
                continue
            st = p.steps[k]
            H, M, N, K = (int(v) for v in st[10:14])
            R, ra, am, rb, bm = (int(v) for v in p.row_steps[k])
            ops = []
            for side, (n_in, s2, rows, at) in enumerate(((M, st[3], ra, am), (N, st[7], rb, bm))):
                kind, ref = int(st[4 * side]), int(st[4 * side + 1])
                buf, off = (leaves[ref], leaf_off(ref, sid)) if kind == ctr.LEAF else (arena, ref)
                flat = buf[off:off + rows * H * n_in * K].reshape(rows, H, -1)
                assert flat.size == rows * H * n_in * K
                if at >= 0:
                    flat = flat[p.row_maps[at:at + R]]
                else:
                    assert rows in (1, R)
                    flat = np.broadcast_to(flat, (R, H, n_in * K))
                if side == 0:
                    ops.append(flat.reshape(R, H, M, K) if s2 == 1 else flat.reshape(R, H, K, M).transpose(0, 1, 3, 2))
                else:
                    ops.append(flat.reshape(R, H, K, N) if s2 == 1 else flat.reshape(R, H, N, K).transpose(0, 1, 3, 2))
            z = np.matmul(ops[0], ops[1]).ravel()
            if st[8] == ctr.OUT:
                sl = slice(blk * block_numel, (blk + 1) * block_numel)
                out[sl] = out[sl] + z if beta else z
            else:
                arena[st[9]:st[9] + z.size] = z
    # the host's side: [block axes][rows of the final tensor][the others] -> ("proj",) + the others, a row per projection
    n_rows, row_of_proj = p.out_rows
    named = p.inds[1:]
    rest = tuple(x for x in named if x not in set(p.slice_inds))
    held = p.block_inds + ("proj",) + rest
    extent = dict(zip(named, p.shape[1:]), proj=n_rows)
    arr = out.reshape(tuple(extent[x] for x in held)).transpose([held.index(x) for x in p.inds])
    return arr[row_of_proj]


def _plan(path, ts, dims, output, **kw):
    return ctr.plan(path, ts, [tuple(dims[x] for x in xs) for xs in ts], output, **kw)


@pytest.mark.parametrize("seed", range(6))
def test_row_tables_and_maps(seed):
    ts, dims, output, sparse = _network(seed)
    path = _random_path(len(ts), seed) if seed % 2 else _greedy_path(ts)
    P = (1, 5, 40)[seed % 3]
    projs = _projs(dims, sparse, P, seed)
    p = _plan(path, ts, dims, output, sparse_inds=sparse, projs=projs)
    col = {x: j for j, x in enumerate(sparse)}

    def table(inds):
        cols = sorted(col[x] for x in inds if x in col)
        return np.unique(projs[:, cols], axis=0) if cols else np.zeros((1, 0), np.int64), cols

    # leaves: the rows they are restricted to
    for xs, rows in zip(ts, p.leaf_rows):
        u, cols = table(xs)
        if not cols:
            assert rows is None
            continue
        axes, values = rows
        assert [xs[a] for a in axes] == [sparse[c] for c in cols]
        assert np.array_equal(values, u) and len(u) <= min(math.prod(dims[sparse[c]] for c in cols), P)
    # steps: row counts and maps, against the index-only contraction along the same path
    for k, (a, b) in enumerate(sorted(q) for q in path):
        live, nxt = (tnmod.contract(path[:n], ts, output, dims)[0] for n in (k, k + 1))
        ux, cx = table(live[a])
        uy, cy = table(live[b])
        uz, cz = table(nxt[-1])
        assert set(cz) == set(cx) | set(cy)
        op, (R, ra, am, rb, bm) = p.ops[k], p.row_steps[k]
        if op["folded"]:
            assert (R, ra, am, rb, bm) == (1, 1, -1, 1, -1) and not cy and cx == cz
            assert op["M"] == len(uz) * math.prod(dims[x] for x in op["x"])
        else:
            assert (R, ra, rb) == (len(uz), len(ux), len(uy))
            assert R <= min(math.prod(dims[sparse[c]] for c in cz), P)
            for u, cols, at in ((ux, cx, am), (uy, cy, bm)):
                if at < 0:
                    assert cols == cz or not cols
                    continue
                m = p.row_maps[at:at + R]
                assert m.dtype == np.int32
                assert np.array_equal(u[m], uz[:, [cz.index(c) for c in cols]])
    assert p.macs_per_slice == sum(int(w[0]) * int(r[10]) * int(r[11]) * int(r[12]) * int(r[13])
                                   for w, r in zip(p.row_steps, p.steps))
    q = _plan(path, ts, dims, output)
    assert p.peak_device_bytes >= 4 * p.row_maps.size and q.row_maps is None


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("P", [1, 6, 30])
def test_tables_reproduce_the_dense_result_at_the_projections(seed, P):
    ts, dims, output, sparse = _network(seed, n_sparse=2 + seed % 3)
    path = _greedy_path(ts) if seed % 2 else _random_path(len(ts), seed + 10)
    arrays = _arrays(ts, dims, seed)
    projs = _projs(dims, sparse, P, seed + 1)
    if P > 2:
        projs[-1] = projs[0]  # a duplicate row
    inds, ref = _expected(path, ts, arrays, output, sparse, projs)
    p = _plan(path, ts, dims, output, sparse_inds=sparse, projs=projs)
    assert p.inds == inds and p.shape == ref.shape
    np.testing.assert_allclose(_interpret(p, arrays), ref, rtol=1e-10, atol=1e-13)
    # non-sparse slices: summed ones and one the result holds, whole and in two pieces of slice_range
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    final = tnmod.contract(path, ts, output)[0][0]
    cut = [x for x in every if x not in final][:2] + [x for x in every if x in final and x not in sparse][:1]
    ps = _plan(path, ts, dims, output, sparse_inds=sparse, projs=projs, slices=cut)
    assert ps.inds == inds and ps.n_slices == math.prod(dims[x] for x in cut) and ps.macs == ps.n_slices * ps.macs_per_slice
    np.testing.assert_allclose(_interpret(ps, arrays), ref, rtol=1e-10, atol=1e-13)
    n = ps.n_slices
    parts = [_plan(path, ts, dims, output, sparse_inds=sparse, projs=projs, slices=cut, slice_range=r)
             for r in ((0, n // 3), (n // 3, n))]
    np.testing.assert_allclose(sum(_interpret(q, arrays) for q in parts), ref, rtol=1e-10, atol=1e-13)


def test_a_sparse_index_in_three_tensors_and_a_sliced_axis_between_two_sparse_ones():
    ts = [("s", "x", "t", "a"), ("s", "a", "b"), ("s", "b", "x", "c"), ("c", "t")]
    dims = dict(s=3, t=2, x=4, a=2, b=3, c=2)
    output = ("s", "t", "c")
    arrays = _arrays(ts, dims, 3)
    projs = np.array([[2, 1], [0, 0], [2, 1], [1, 1], [2, 0]])
    for path in ([(0, 1), (0, 1), (0, 1)], [(2, 3), (0, 2), (0, 1)], [(1, 2), (0, 2), (0, 1)]):
        for cut in ((), ("x",), ("x", "c")):
            for sparse, pr in ((("s", "t"), projs), (("t", "s"), projs[:, ::-1])):
                inds, ref = _expected(path, ts, arrays, output, sparse, pr)
                p = _plan(path, ts, dims, output, sparse_inds=sparse, projs=pr, slices=cut)
                assert p.leaf_rows[0][0] == tuple(ts[0].index(x) for x in sparse)
                assert p.inds == inds == ("proj", "c")
                np.testing.assert_allclose(_interpret(p, arrays), ref, rtol=1e-10, atol=1e-13)
    one = ctr.plan([], [("s", "x", "t")], [(3, 4, 2)], ("s", "x", "t"), sparse_inds=("s", "t"), projs=projs, slices=["x"])
    a = _arrays([("s", "x", "t")], dims, 4)[0]
    assert one.inds == ("proj", "x")
    np.testing.assert_array_equal(_interpret(one, [a]), a[projs[:, 0], :, projs[:, 1]])


def _sparse_cost(path, ts, dims, output, sparse, n_projs):
    """The sparse cost model restated: per step, prod of the dense dims of both operands' indices times
    min(prod of their sparse dims, n_projs)."""
    tot = 0
    for k, (a, b) in enumerate(path):
        live = tnmod.contract(path[:k], ts, output, dims)[0]
        both = set(live[a]) | set(live[b])
        tot += math.prod(dims[x] for x in both if x not in sparse) * \
            min(math.prod(dims[x] for x in both if x in sparse), n_projs)
    return tot


@pytest.mark.parametrize("seed", range(6))
def test_every_assignment_costs_the_dense_output_and_the_sparse_model(seed):
    ts, dims, output, sparse = _network(seed)
    path = _random_path(len(ts), seed + 3)
    projs = np.array(list(itertools.product(*(range(dims[x]) for x in sparse))))
    P = len(projs)
    p = _plan(path, ts, dims, output, sparse_inds=sparse, projs=projs)
    dense = _plan(path, ts, dims, output)
    assert p.macs == dense.macs == _sparse_cost(path, ts, dims, output, sparse, P)
    # ... and any subset of projections launches no more than the model prices
    some = projs[np.random.RandomState(seed).choice(P, max(1, P // 3), replace=False)]
    q = _plan(path, ts, dims, output, sparse_inds=sparse, projs=some)
    assert q.macs <= _sparse_cost(path, ts, dims, output, sparse, len(some)) <= p.macs


def test_folding_into_a_plain_gemm():
    dims = dict(s=5, t=3, i=4, k=6, j=7, h=2)
    projs = _projs(dims, ("s", "t"), 9, 0)
    R = len(np.unique(projs[:, :1], axis=0))
    # only the first operand has rows, stored [r][m][k], H = 1: one ordinary step with R M rows
    p = _plan([(0, 1)], [("s", "i", "k"), ("k", "j")], dims, ("s", "i", "j"), sparse_inds=("s",), projs=projs[:, :1])
    (op,) = p.ops
    assert op["folded"] and (op["H"], op["M"], op["N"], op["K"]) == (1, R * 4, 7, 6) and not len(p.perms)
    assert p.row_steps.tolist() == [[1, 1, -1, 1, -1]] and p.row_maps.size == 0
    assert p.steps[0, 2:4].tolist() == [6, 1] and p.macs == R * 4 * 7 * 6
    # H > 1: the rows stay, the first operand read in place, the second one row for every r
    p = _plan([(0, 1)], [("s", "h", "i", "k"), ("h", "k", "j")], dims, ("s", "h", "i", "j"), sparse_inds=("s",),
              projs=projs[:, :1])
    assert not p.ops[0]["folded"] and p.row_steps.tolist() == [[R, R, -1, 1, -1]] and p.ops[0]["H"] == 2
    # both operands sparse: maps
    p = _plan([(0, 1)], [("s", "i", "k"), ("t", "k", "j")], dims, ("s", "t", "i", "j"), sparse_inds=("s", "t"),
              projs=projs)
    Rz, Rt = len(np.unique(projs, axis=0)), len(np.unique(projs[:, 1:], axis=0))
    assert not p.ops[0]["folded"] and p.row_steps.tolist() == [[Rz, R, 0, Rt, Rz]] and p.row_maps.size == 2 * Rz
    # only the second operand has rows: its rows in place, no fold (the result is [r][m][n])
    p = _plan([(0, 1)], [("i", "k"), ("s", "k", "j")], dims, ("s", "i", "j"), sparse_inds=("s",), projs=projs[:, :1])
    assert not p.ops[0]["folded"] and p.row_steps.tolist() == [[R, 1, -1, R, -1]]
    # the first operand stored [r][k][m]: no fold either
    p = _plan([(0, 1)], [("s", "k", "i"), ("k", "j")], dims, ("s", "i", "j"), sparse_inds=("s",), projs=projs[:, :1])
    assert not p.ops[0]["folded"] and p.ops[0]["form_a"] == 1 and not len(p.perms)


def test_refusals_before_any_device_use(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts = [("a", "b", "s"), ("b", "c", "t")]
    arrays = [np.ones((2, 3, 2)), np.ones((3, 4, 3))]
    out = ("a", "s", "t")
    ok = np.array([[0, 1], [1, 2]])
    run = lambda **kw: ctr.contract([(0, 1)], ts, arrays, kw.pop("out", out), **kw)  # noqa: E731
    with pytest.raises(ValueError, match="output indices"):
        run(sparse_inds=("s", "b"), projs=ok, out=("a", "s", "t", "c"))  # b is summed
    with pytest.raises(ValueError, match="not in 'ts_inds'"):
        run(sparse_inds=("s", "z"), projs=ok)
    with pytest.raises(ValueError, match="not in 'ts_inds'"):
        run(sparse_inds=("s", "s"), projs=ok)
    with pytest.raises(NotImplementedError, match="sliced index that is also sparse"):
        run(sparse_inds=("s", "t"), projs=ok, slices=("s",))
    with pytest.raises(NotImplementedError, match="leaves one tensor"):
        ctr.contract([], ts, arrays, out, sparse_inds=("s", "t"), projs=ok)
    with pytest.raises(ValueError, match="beyond the dimensions"):
        run(sparse_inds=("s", "t"), projs=np.array([[2, 0]]))
    with pytest.raises(ValueError, match="beyond the dimensions"):
        run(sparse_inds=("s", "t"), projs=np.array([[0, -1]]))
    with pytest.raises(TypeError, match="integers"):
        run(sparse_inds=("s", "t"), projs=np.array([[0.0, 1.0]]))
    with pytest.raises(ValueError, match="shape"):
        run(sparse_inds=("s", "t"), projs=np.array([[0, 1, 0]]))
    with pytest.raises(ValueError, match="shape"):
        run(sparse_inds=("s", "t"), projs=np.array([0, 1]))
    with pytest.raises(ValueError, match="shape"):
        run(sparse_inds=("s", "t"), projs=np.zeros((0, 2), np.int64))
    with pytest.raises(ValueError, match="need 'projs'"):
        run(sparse_inds=("s", "t"))
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, a.shape) for xs, a in zip(ts, arrays)], output_inds=out,
                              sparse_inds=["s", "t"])

    class Res:
        path = [(0, 1)]

    with pytest.raises(NotImplementedError, match="projs="):
        ctr.contract_results(tn0, arrays, tn0, Res())
    with pytest.raises(ValueError, match="sparse indices of the network"):
        ctr.contract_results(tn0, arrays, tn0, Res(), projs=ok, sparse_inds=("s",))
    with pytest.raises(ValueError, match="beyond the dimensions"):  # (columns in sorted order: s, t)
        ctr.contract_results(tn0, arrays, tn0, Res(), projs=np.array([[2, 0]]))


def test_without_projs_the_tables_are_those_of_a_call_without_the_keywords():
    for seed in range(3):
        ts, dims, output, _ = _network(seed)
        path = _random_path(len(ts), seed)
        every = list(dict.fromkeys(x for xs in ts for x in xs))
        for cut in ((), every[1:4]):
            a = _plan(path, ts, dims, output, slices=cut)
            b = _plan(path, ts, dims, output, slices=cut, sparse_inds=(), projs=None)
            for name in ("leaf_numel", "leaf_sl", "perms", "steps"):
                x, y = getattr(a, name), getattr(b, name)
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
            assert (a.inds, a.shape, a.arena_elems, a.out_numel, a.macs, a.peak_device_bytes, a.ops) == \
                (b.inds, b.shape, b.arena_elems, b.out_numel, b.macs, b.peak_device_bytes, b.ops)
            assert b.row_steps is None and b.row_maps is None and b.out_rows is None and b.leaf_rows == ()


def test_row_kernels_use_no_scratch():
    """4 dtypes x (4 tiled layouts + dot + stream) row-mapped kernels, none with scratch or spills; the kernels that
    were there are still 4 x 7."""
    sys.path.insert(0, str(ROOT / "tools"))
    import code_objects
    if not code_objects.LIB.exists() or not (code_objects.LLVM / "llvm-objdump").exists():
        pytest.skip("no built library / LLVM tools")
    rows = old = 0
    for elf in code_objects.code_objects():
        for name, meta in code_objects.kernel_table(elf).items():
            if "ct_rows_" in name:
                rows += 1
                assert meta["private_segment_fixed_size"] == 0, name
                assert meta.get("vgpr_spill_count", 0) == 0, name
            if "ct_gather_kernel" in name or "ct_gemm_" in name:
                old += 1
    assert rows == 4 * 6
    assert old == 4 * 7
