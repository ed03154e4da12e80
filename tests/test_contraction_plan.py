"""The contraction engine's plan (tnco_amd/contraction.py), without a GPU: axes against the index-only contract, MACs
against the cost models, every refusal before any device use, the tables replayed by a numpy interpreter of the
device's semantics, the code objects of the new kernels, and the plan side of the kernels' edge cases
(tests/contract_cases.py)."""
import math
import sys
from decimal import Decimal
from pathlib import Path

import numpy as np
import pytest

from tests import contract_cases as cc
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn
from tnco_amd.app import tn as tnmod
from tnco_amd.app.app import cost_to_decimal

ROOT = Path(__file__).resolve().parent.parent


def _dims(ts_inds, dims):
    if isinstance(dims, int):
        return {x: dims for xs in ts_inds for x in xs}
    if isinstance(dims, dict):
        return dims
    return {i: int(d) for i, d in enumerate(dims)}


def _random_path(n, seed):
    rng = np.random.RandomState(seed)
    path = []
    while n > 1:
        a, b = rng.choice(n, 2, replace=False)
        path.append((int(a), int(b)))
        n -= 1
    return path


def _greedy_path(ts_inds):
    """Joins tensors that share an index first (keeps the intermediates small), then the rest."""
    ts = [set(x) for x in ts_inds]
    path = []
    while len(ts) > 1:
        pair = next(((a, b) for a in range(len(ts)) for b in range(a + 1, len(ts)) if ts[a] & ts[b]), (0, 1))
        a, b = pair
        tb, ta = ts.pop(b), ts.pop(a)
        ts.append(ta | tb)
        path.append(pair)
    return path


def _networks():
    """(name, ts_inds, dims dict, output_inds) of the networks the plan is checked on."""
    out = []
    ts, d, o = syn.random_regular_tn(12, seed=3)
    out.append(("regular", ts, _dims(ts, d), o))
    ts, d, o = syn.random_hyper_tn(10, 16, k=3, n_output=3, seed=5, dims_choices=(2, 3, 4))
    out.append(("hyper", ts, _dims(ts, d), o))
    ts, d, o = syn.random_hyper_tn(8, 12, k=3, n_output=2, seed=9, dims_choices=(2, 3))
    ts = [list(x) + [100 + t] for t, x in enumerate(ts)]  # an open index on every tensor
    dd = {**{i: int(x) for i, x in enumerate(d)}, **{100 + t: 2 for t in range(8)}}
    out.append(("hyper_open", ts, dd, tuple(o) + tuple(100 + t for t in range(8))))
    return out


def _gather(row, src, base):
    """The elements a row of `perms` moves, in the order of its destination: src[base + sum of digit x stride]."""
    P = ctr.MAX_AXES
    nd = int(row[4])
    shape, strides = row[8:8 + nd], row[8 + P:8 + P + nd]
    idx = np.full(tuple(shape), base, np.int64)
    for ax in range(nd):
        sh = [1] * nd
        sh[ax] = int(shape[ax])
        idx = idx + (np.arange(shape[ax]) * strides[ax]).reshape(sh)
    return src[idx.ravel()].copy()


def _interpret(p, arrays, gather=_gather, store=None):
    """The device semantics of the tables, in numpy: what csrc/contract.hip does, element by element.  `gather`: what a
    row of `perms` moves (tests/test_contraction_gather_plan.py plants its defects there); `store`: what a step leaves
    in the arena of its flat result z, as store(k, z) (storage modes round there; None: z itself)."""
    P = ctr.MAX_AXES
    leaves = [np.ascontiguousarray(a, p.dtype).ravel() for a in arrays]
    arena = np.zeros(max(p.arena_elems, 1), p.dtype)
    out = np.zeros(p.out_numel, p.dtype)
    n_blocks = math.prod(p.slice_dims[p.slice_inds.index(x)] for x in p.block_inds)
    block_numel = p.out_numel // n_blocks
    place = [math.prod(p.slice_dims[k + 1:]) for k in range(len(p.slice_dims))]
    digit = lambda sid, s: (sid // place[s]) % p.slice_dims[s]  # noqa: E731

    def leaf_off(t, sid):
        row = p.leaf_sl[t]
        return sum(digit(sid, int(row[1 + j])) * int(row[1 + P + j]) for j in range(int(row[0])))

    visited = set()
    for sid in range(*p.slice_range):
        blk = 0
        for x in p.block_inds:
            s = p.slice_inds.index(x)
            blk = blk * p.slice_dims[s] + digit(sid, s)
        beta = blk in visited
        visited.add(blk)
        for k in [-1] + list(range(len(p.steps))):
            writes = []  # (the rows of a group are one launch: every row reads before any row writes)
            for row in p.perms[p.perms[:, 6] == k]:
                src, base = (leaves[row[1]], leaf_off(int(row[1]), sid)) if row[0] == ctr.LEAF else (arena, int(row[1]))
                writes.append((row, gather(row, src, base)))
            for row, vals in writes:
                if row[2] == ctr.ARENA:
                    arena[row[3]:row[3] + int(row[5])] = vals
                else:
                    out[blk * block_numel:(blk + 1) * block_numel] = vals
            if k < 0:
                continue
            st = p.steps[k]
            H, M, N, K = (int(v) for v in st[10:14])
            ops = []
            for side, (n_in, s1, s2) in enumerate(((M, st[2], st[3]), (N, st[6], st[7]))):
                kind, ref = int(st[4 * side]), int(st[4 * side + 1])
                buf, off = (leaves[ref], leaf_off(ref, sid)) if kind == ctr.LEAF else (arena, ref)
                flat = buf[off:off + H * n_in * K].reshape(H, -1)
                if side == 0:
                    ops.append(flat.reshape(H, M, K) if s2 == 1 else flat.reshape(H, K, M).transpose(0, 2, 1))
                else:
                    ops.append(flat.reshape(H, K, N) if s2 == 1 else flat.reshape(H, N, K).transpose(0, 2, 1))
            z = np.matmul(ops[0], ops[1]).ravel()
            if st[8] == ctr.OUT:
                sl = slice(blk * block_numel, (blk + 1) * block_numel)
                out[sl] = out[sl] + z if beta else z
            else:
                arena[st[9]:st[9] + z.size] = z if store is None else store(k, z)
    rest = tuple(x for x in p.inds if x not in set(p.slice_inds))
    held = p.block_inds + rest
    arr = out.reshape(tuple(p.shape[p.inds.index(x)] for x in held))
    return arr.transpose([held.index(x) for x in p.inds])


def _host(path, ts_inds, arrays, output_inds):
    """Independent host contraction: numpy tensordot step by step, axes as the index-only contract orders them."""
    ts = [tuple(x) for x in ts_inds]
    arrs = list(arrays)
    left = tnmod.get_hyper_count(ts)
    out = frozenset(output_inds)
    for a, b in path:
        a, b = sorted((a, b))
        yb, y = ts.pop(b), arrs.pop(b)
        xa, x = ts.pop(a), arrs.pop(a)
        shared = set(xa) & set(yb)
        stay = {i for i in shared if left[i] > 1 or i in out}
        for i in shared:
            left[i] -= 1
        letters = {i: chr(65 + k) if k < 26 else chr(71 + k) for k, i in enumerate(dict.fromkeys(xa + yb))}
        z = tuple(i for i in xa if i in stay) + tuple(i for i in xa if i not in shared) + \
            tuple(i for i in yb if i not in shared)
        spec = "".join(letters[i] for i in xa) + "," + "".join(letters[i] for i in yb) + "->" + \
            "".join(letters[i] for i in z)
        arrs.append(np.einsum(spec, x, y))
        ts.append(z)
    return ts, arrs


def _arrays(ts_inds, dims, dtype, seed):
    rng = np.random.RandomState(seed)
    out = []
    for xs in ts_inds:
        shape = tuple(dims[x] for x in xs)
        a = rng.standard_normal(shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.standard_normal(shape)
        out.append((a / math.sqrt(max(1, np.prod(shape)))).astype(dtype))
    return out


@pytest.mark.parametrize("name,ts,dims,output", _networks(), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("pathkind", ["random", "greedy"])
def test_plan_axes_equal_index_contract(name, ts, dims, output, pathkind):
    path = _random_path(len(ts), 1) if pathkind == "random" else _greedy_path(ts)
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    expect = tnmod.contract(path, ts, output, dims)[0]
    p = ctr.plan(path, ts, shapes, output)
    assert [p.inds] == [tuple(x) for x in expect]
    assert p.shape == tuple(dims[x] for x in p.inds)
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    for cut in (set(every[:3]), set([x for x in every if x in expect[0]][:2] + every[3:4])):
        ps = ctr.plan(path, ts, shapes, output, slices=cut)
        assert ps.inds == p.inds  # with or without slices
        assert ps.n_slices == math.prod(dims[x] for x in cut)


@pytest.mark.parametrize("name,ts,dims,output", _networks(), ids=lambda v: v if isinstance(v, str) else "")
def test_plan_tables_reproduce_the_host_contraction(name, ts, dims, output):
    """The tables, replayed with the device's semantics in numpy, give the numbers of a tensordot contraction --
    unsliced, and sliced (summed and block indices) in pieces of `slice_range`."""
    path = _greedy_path(ts)
    arrays = _arrays(ts, dims, np.float64, 0)
    shapes = [a.shape for a in arrays]
    _, (ref,) = _host(path, ts, arrays, output)
    p = ctr.plan(path, ts, shapes, output)
    np.testing.assert_allclose(_interpret(p, arrays), ref, rtol=1e-10, atol=1e-12)
    final = set(p.inds)
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    cut = [x for x in every if x not in final][:3] + [x for x in every if x in final][:1]
    ps = ctr.plan(path, ts, shapes, output, slices=cut)
    n = ps.n_slices
    np.testing.assert_allclose(_interpret(ps, arrays), ref, rtol=1e-10, atol=1e-12)
    parts = [ctr.plan(path, ts, shapes, output, slices=cut, slice_range=r) for r in ((0, n // 3), (n // 3, n))]
    np.testing.assert_allclose(sum(_interpret(q, arrays) for q in parts), ref, rtol=1e-10, atol=1e-12)


def test_plan_of_two_components_and_a_single_leaf():
    ts = [("a", "b"), ("b", "c"), ("d", "e"), ("e", "f")]
    dims = dict(a=2, b=3, c=4, d=2, e=3, f=2)
    arrays = _arrays(ts, dims, np.float64, 1)
    path = [(0, 1), (0, 1), (0, 1)]  # each component, then their outer product
    p = ctr.plan(path, ts, [a.shape for a in arrays])
    _, (ref,) = _host(path, ts, arrays, ("a", "c", "d", "f"))
    assert p.inds == tnmod.contract(path, ts)[0][0]
    np.testing.assert_allclose(_interpret(p, arrays), ref, rtol=1e-12)
    one = ctr.plan([], [("a", "b")], [(2, 3)], slices=["a"])
    a = arrays[0]
    np.testing.assert_array_equal(_interpret(one, [a]), a)


def _cost(path, ts, dims, output, slices=()):
    """The cost models restated: sum over the steps of prod dims(in1 | in2 | slices)."""
    tot = 0
    for k, (a, b) in enumerate(path):
        live = tnmod.contract(path[:k], ts, output, dims)[0]
        tot += math.prod(dims[x] for x in set(live[a]) | set(live[b]) | set(slices))
    return tot


@pytest.mark.parametrize("name,ts,dims,output", _networks(), ids=lambda v: v if isinstance(v, str) else "")
def test_plan_macs_equal_the_cost_by_hand(name, ts, dims, output):
    path = _random_path(len(ts), 4)
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    p = ctr.plan(path, ts, shapes, output)
    assert cost_to_decimal(p.macs) == cost_to_decimal(_cost(path, ts, dims, output))
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    cut = every[1:5]
    ps = ctr.plan(path, ts, shapes, output, slices=cut)
    assert cost_to_decimal(ps.macs) == cost_to_decimal(_cost(path, ts, dims, output, cut))
    assert ps.macs == ps.n_slices * ps.macs_per_slice


def test_plan_macs_are_exact_integers_of_the_cost():
    """Unrounded too: the MACs of a path are the cost model's sum exactly (the GPU test closes the loop with
    optimize(): tests/test_gpu_contraction.py)."""
    ts, d, o = syn.random_regular_tn(16, seed=2)
    dims = _dims(ts, d)
    path = _greedy_path(ts)
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    p = ctr.plan(path, ts, shapes, o)
    assert Decimal(p.macs) == Decimal(_cost(path, ts, dims, o))


def test_refusals_before_any_device_use(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    ts = [("a", "b"), ("b", "c")]
    ok = [np.ones((2, 3)), np.ones((3, 4))]
    with pytest.raises(ValueError, match="'ts_inds' is not consistent with 'arrays'."):
        ctr.contract([(0, 1)], ts, [np.ones((2, 3)), np.ones((2, 4))])
    with pytest.raises(ValueError, match="'ts_inds' is not consistent with 'arrays'."):
        ctr.contract([(0, 1)], ts, [np.ones((2, 3))])
    with pytest.raises(ValueError, match="'path' is not valid."):
        ctr.contract([(0, 0)], ts, ok)
    with pytest.raises(ValueError, match="'path' is not valid."):
        ctr.contract([(0, 2)], ts, ok)
    with pytest.raises(ValueError, match="'path' is not valid."):
        ctr.contract([(0, 1), (0, 1)], ts, ok)
    with pytest.raises(TypeError):
        ctr.contract([(0, 1)], ts, [np.ones((2, 3), np.int32), np.ones((3, 4))])
    with pytest.raises(TypeError):
        ctr.contract([(0, 1)], ts, [np.ones((2, 3), np.float16), np.ones((3, 4))])
    wide = [tuple(range(ctr.MAX_AXES + 1)), (0,)]
    with pytest.raises(NotImplementedError):
        ctr.contract([(0, 1)], wide, [np.ones((1,) * (ctr.MAX_AXES + 1)), np.ones(1)])
    tn0 = tnmod.TensorNetwork([tnmod.Tensor(("a", "b"), (2, 3)), tnmod.Tensor(("b", "c"), (3, 4))],
                              sparse_inds=["b"])

    class R:
        path = [(0, 1)]

    with pytest.raises(NotImplementedError):
        ctr.contract_results(tn0, ok, tn0, R())
    p = ctr.plan([(0, 1)], ts, [(2, 3), (3, 4)])
    with pytest.raises(RuntimeError):
        ctr.check_memory(p, p.peak_device_bytes - 1)
    ctr.check_memory(p, p.peak_device_bytes)


def test_sliced_axes_are_dropped_and_blocks_counted():
    ts = [("a", "b", "c"), ("c", "d"), ("d", "a")]
    dims = dict(a=2, b=3, c=4, d=5)
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    p = ctr.plan([(0, 1), (0, 1)], ts, shapes, ("b", "a"), slices=["c", "a"])
    assert p.slice_inds == ("a", "c") and p.n_slices == 8
    assert p.block_inds == ("a",)
    assert p.inds == tuple(tnmod.contract([(0, 1), (0, 1)], ts, ("b", "a"), dims)[0][0])
    for op in p.ops:
        assert not ({"a", "c"} & set(op["h"] + op["x"] + op["y"] + op["s"]))


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, str(ROOT / "tools"))
    import code_objects
    if not code_objects.LIB.exists() or not (code_objects.LLVM / "llvm-objdump").exists():
        pytest.skip("no built library / LLVM tools")
    seen = 0
    for elf in code_objects.code_objects():
        for name, meta in code_objects.kernel_table(elf).items():
            if "ct_gather_kernel" in name or "ct_gemm_" in name:
                seen += 1
                assert meta["private_segment_fixed_size"] == 0, name
                assert meta.get("vgpr_spill_count", 0) == 0, name
    assert seen == 4 * 7


@pytest.mark.parametrize("seed", range(6))
def test_permutes_of_one_launch_do_not_overlap(seed):
    """The rows of a group run in one launch: no row writes where another row of it reads."""
    ts, d, o = syn.random_regular_tn(24, seed=seed)
    dims = _dims(ts, d)
    p = ctr.plan(_random_path(len(ts), seed), ts, [tuple(dims[x] for x in xs) for xs in ts], o,
                 slices=list(range(seed % 3)))
    P = ctr.MAX_AXES
    for g in set(p.perms[:, 6].tolist()):
        rows = p.perms[p.perms[:, 6] == g]
        dst = [(int(r[3]), int(r[3] + r[5])) for r in rows if r[2] == ctr.ARENA]
        src = [(int(r[1]), int(r[1] + sum((r[8 + k] - 1) * r[8 + P + k] for k in range(int(r[4]))) + 1))
               for r in rows if r[0] == ctr.ARENA]
        for a0, a1 in dst:
            assert all(a1 <= b0 or b1 <= a0 for b0, b1 in src), (g, dst, src)
        assert all(a1 <= b0 or b1 <= a0 for i, (a0, a1) in enumerate(dst) for b0, b1 in dst[i + 1:])


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_kernel_edge_cases_plan_as_designed(case):
    """Every case of the kernels' GPU tests gives the one step it was designed for -- sizes, operand forms, permutes --
    so that a planner change that reroutes a case shows where there is no GPU; and the interpreter of the tables agrees
    with a plain einsum on it."""
    p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, slices=case.slices)
    (op,) = p.ops
    got = {k: op[k] for k in ("H", "M", "N", "K", "form_a", "form_b")}
    assert dict(got, perms=len(p.perms)) == case.ops
    assert p.n_slices == case.n_slices() and p.slice_inds == case.slices
    assert p.macs == case.n_slices() * op["H"] * op["M"] * op["N"] * op["K"]
    held = [x for x in case.slices if x in p.inds]
    assert p.block_inds == tuple(held)
    assert case.kt == op["K"] * math.prod(case.dims[x] for x in case.slices if x not in p.inds)
    # the dtype rule: without a list of its own a case runs every type up to KT_SINGLE products per element and
    # the double types beyond; a list of its own may add single types to a long sum, never drop one from a short one
    # except where memory says so (the 4100 x 4100 outer product runs in the two real types)
    if not case.dtypes:
        assert case.run_dtypes() == (cc.ALL if case.kt <= cc.KT_SINGLE else cc.DOUBLES)
    else:
        assert case.run_dtypes() == case.dtypes
        assert set(cc.DOUBLES) <= set(case.dtypes) or p.out_numel > 1 << 24
    assert sum(case.kernels.values()) == case.n_slices() * (1 + (case.ops["perms"] > 0))
    if p.out_numel <= 1 << 20:
        arrays = _arrays(case.ts, case.dims, np.float64, 2)
        sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in case.ts for x in xs))}
        ref = np.einsum(arrays[0], [sym[x] for x in case.ts[0]], arrays[1], [sym[x] for x in case.ts[1]],
                        [sym[x] for x in p.inds], optimize=True)
        np.testing.assert_allclose(_interpret(p, arrays), ref, rtol=1e-10, atol=1e-13)


def test_kernel_edge_cases_reach_every_kernel_path_in_every_dtype():
    """The seven launch-count slots -- the gather, the four tiled layouts, dot, stream -- are each expected non-zero
    by at least one case per dtype; the GPU tests assert those expectations against the device's counts."""
    assert len(ctr.KERNEL_PATHS) == 7 and len(set(ctr.KERNEL_PATHS)) == 7
    for dtype in cc.ALL:
        reached = {name for c in cc.CASES if dtype in c.run_dtypes() for name, n in c.kernels.items() if n > 0}
        assert reached == set(ctr.KERNEL_PATHS), (np.dtype(dtype).name, set(ctr.KERNEL_PATHS) - reached)
    assert set(cc.NORMAL_FILL) <= set(cc.BY_NAME)
    pairs = {(c.ops["form_a"], c.ops["form_b"], c.ops["M"], c.ops["N"], c.ops["K"]) for c in cc.CASES
             if next(iter(c.kernels)).startswith("tiled") and c.ops["H"] == 1 and not c.slices}
    assert len(pairs) >= 12
