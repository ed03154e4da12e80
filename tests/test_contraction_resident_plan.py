"""`contraction.Contractor` without a GPU: what it refuses, in which order and with which words, before the device is
touched (`_lib.load` is made to raise); that its plan is `plan()`'s; the axis-merging helper and the extent check the
wrapper applies before a tensor's pointer goes down; and the numpy models of the two kernels (tests/resident_cases.py)
against an emulation of what the kernels do with the merged dims and strides."""
import dataclasses

import numpy as np
import pytest

from tests import batch_cases as bc
from tests import resident_cases as rc


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.fixture
def no_gpu(monkeypatch):
    from tnco_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", refuse)


def outcome(call):
    try:
        return call()
    except Exception as e:  # noqa: BLE001 (every type is compared)
        return type(e), str(e)


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    return a == b


CHAIN = bc.SMALL
KEYWORDS = [dict(), dict(slice_range=(1, 11)), dict(slice_batch=5), dict(slice_batch=64), dict(path_kernel=5),
            dict(path_kernel=1024), dict(hoist=True), dict(reuse=True), dict(reuse=True, slice_order="reuse"),
            dict(reuse=True, slice_order=("t", "u", "p")), dict(indirect=True), dict(compute="matrix"),
            dict(compute="bf16x3"), dict(accumulate="float64"), dict(storage="float16"), dict(storage="bfloat16", scaling="tensor"),
            dict(hoist=True, slice_batch=5, indirect=True)]


@pytest.mark.parametrize("kw", KEYWORDS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "plain" for kw in KEYWORDS])
def test_the_plan_is_the_plan_of_plan(ctr, no_gpu, kw):
    args = (bc.PATH, CHAIN.ts, CHAIN.shapes(), CHAIN.output)
    want = ctr.plan(*args, slices=bc.SLICES, dtype=np.complex64, **kw)
    with ctr.Contractor(*args, slices=bc.SLICES, dtype=np.complex64, **kw) as c:
        assert type(c.plan) is ctr.Plan
        for f in dataclasses.fields(ctr.Plan):
            assert same(getattr(c.plan, f.name), getattr(want, f.name)), f.name
        assert c.plan.peak_device_bytes == want.peak_device_bytes and c.plan.macs == want.macs
        assert c.io_launches == (0, 0)


def test_the_plan_of_a_projected_network(ctr, no_gpu):
    ts, shapes = [("a", "k"), ("k", "b")], [(3, 4), (4, 5)]
    kw = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [2, 4], [0, 1]]))
    want = ctr.plan([(0, 1)], ts, shapes, ("a", "b"), **kw)
    with ctr.Contractor([(0, 1)], ts, shapes, ("a", "b"), **kw) as c:
        for f in dataclasses.fields(ctr.Plan):
            assert same(getattr(c.plan, f.name), getattr(want, f.name)), f.name


REFUSED_BY_PLAN = [
    dict(path=[(0, 0)]), dict(path=[(0, 1)]), dict(shapes=[(3, 2, 5, 7), (7, 2, 6), (2, 2, 6)]), dict(storage="float8"),
    dict(storage="float16", dtype=np.float64), dict(scaling="tensor"), dict(slice_batch=0), dict(slice_batch=65),
    dict(slice_batch=2, path_kernel=2), dict(path_kernel=1025), dict(compute="bf16x3", dtype=np.float64),
    dict(compute="matrix", storage="float16"), dict(hoist=True, path_kernel=2), dict(reuse=True, hoist=True),
    dict(slice_order="reuse"), dict(slice_order=("p",)), dict(accumulate="float64", dtype=np.complex128),
    dict(slice_range=(3, 2)), dict(slices=("nope",)), dict(sparse_inds=("i",)),
    dict(slice_batch=2, sparse_inds=("i",), projs=np.array([[0]])),
]


@pytest.mark.parametrize("bad", REFUSED_BY_PLAN, ids=[",".join(bad) for bad in REFUSED_BY_PLAN])
def test_the_constructor_refuses_what_plan_refuses(ctr, no_gpu, bad):
    given = dict(path=bc.PATH, shapes=CHAIN.shapes(), slices=bc.SLICES, dtype=np.float32)
    given.update(bad)
    path, shapes = given.pop("path"), given.pop("shapes")
    want = outcome(lambda: ctr.plan(path, CHAIN.ts, shapes, CHAIN.output, **given))
    assert isinstance(want, tuple) and issubclass(want[0], Exception), want
    assert outcome(lambda: ctr.Contractor(path, CHAIN.ts, shapes, CHAIN.output, **given)) == want


# ---- what bind and run refuse, before the device ------------------------------------------------------------------------

TS, SHAPES = [("i", "k"), ("k", "j"), ("j", "l")], [(3, 4), (4, 5), (5, 2)]
PATH3 = [(0, 1), (0, 1)]


def contractor(ctr, **kw):
    kw.setdefault("dtype", np.float32)
    return ctr.Contractor(PATH3, TS, SHAPES, ("i", "l"), **kw)


def arrays(dtype=np.float32):
    return [rc.fill(s, dtype, seed=k) for k, s in enumerate(SHAPES)]


def refusal(call, error, text):
    with pytest.raises(error) as e:
        call()
    assert type(e.value) is error and text in str(e.value), (type(e.value), str(e.value))


def test_use_after_close_is_refused_and_closing_twice_is_fine(ctr, no_gpu):
    c = contractor(ctr)
    c.close()
    c.close()
    for call in (lambda: c.run(arrays()), lambda: c.bind({0: arrays()[0]}), lambda: c.io_launches):
        refusal(call, ValueError, "the Contractor is closed.")
    with contractor(ctr) as c:
        pass
    refusal(lambda: c.run(), ValueError, "the Contractor is closed.")


def test_what_a_call_refuses_of_its_arrays(ctr, no_gpu):
    import torch
    a = arrays()
    t = [torch.from_numpy(x) for x in a]  # (on the host: never on the Contractor's device)
    with contractor(ctr) as c:
        refusal(lambda: c.run(a[:2]), ValueError, "'ts_inds' is not consistent with 'arrays'.")
        refusal(lambda: c.run({3: a[0]}), ValueError, "3 is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.bind({-1: a[0]}), ValueError, "-1 is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.bind({"0": a[0]}), ValueError, "'0' is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.run([a[0], t[1], a[2]]), TypeError, "the arrays of one run must be all numpy arrays or all torch tensors.")
        refusal(lambda: c.bind({0: a[0], 1: t[1]}), ValueError, "a tensor is on cpu, not on cuda:0.")  # (bind takes both kinds)
        refusal(lambda: c.run([a[0], a[1].T, a[2]]), ValueError, "'ts_inds' is not consistent with 'arrays'.")
        refusal(lambda: c.run([a[0], a[1].astype(np.float64), a[2]]), TypeError,
                "an array of dtype float64 does not cast safely to float32.")
        refusal(lambda: c.run([a[0], a[1].astype(np.complex64), a[2]]), TypeError, "does not cast safely to float32.")
        refusal(lambda: c.bind({1: t[1].T}), ValueError, "'ts_inds' is not consistent with 'arrays'.")
        refusal(lambda: c.bind({1: t[1].double()}), TypeError, "a tensor of dtype torch.float64 does not widen exactly to float32.")
        refusal(lambda: c.bind({1: t[1].to(torch.float16)}), TypeError, "a tensor of dtype torch.float16 does not widen exactly")
        refusal(lambda: c.bind({1: t[1].to(torch.int32)}), TypeError, "does not widen exactly")
        refusal(lambda: c.bind({1: t[1]}), ValueError, "a tensor is on cpu, not on cuda:0.")
        refusal(lambda: c.run(t), ValueError, "a tensor is on cpu, not on cuda:0.")
        # a leaf that is neither bound nor given: after the arrays that were given passed their checks
        refusal(lambda: c.run({0: a[0], 2: a[2]}), ValueError, "leaf 1 is neither bound nor given.")
        refusal(lambda: c.run(), ValueError, "leaf 0 is neither bound nor given.")
        refusal(lambda: c.run({0: a[0].T}), ValueError, "'ts_inds' is not consistent with 'arrays'.")
    # the dtype is judged before the device of a tensor, the shape before the dtype
    with contractor(ctr, dtype=np.complex128) as c:
        refusal(lambda: c.bind({1: t[1]}), ValueError, "a tensor is on cpu")  # (float32 widens to complex128)
        refusal(lambda: c.bind({1: t[1].T.double()}), ValueError, "'ts_inds' is not consistent")
    with contractor(ctr, dtype=np.float64) as c:
        refusal(lambda: c.bind({1: t[1].to(torch.complex64)}), TypeError, "torch.complex64 does not widen exactly to float64.")
    with contractor(ctr, device=1) as c:
        assert c.device == 1
        refusal(lambda: c.bind({1: t[1]}), ValueError, "a tensor is on cpu, not on cuda:1.")


@pytest.mark.parametrize("kw, name", [(dict(storage="float16"), "storage"), (dict(storage="bfloat16", scaling="tensor"), "storage"),
                                      (dict(sparse_inds=("i",), projs=np.array([[0], [2]])), "projs")],
                         ids=["storage", "scaling", "projs"])
def test_torch_tensors_are_refused_with_the_host_side_keywords(ctr, no_gpu, kw, name):
    import torch
    a = arrays()
    t = [torch.from_numpy(x) for x in a]
    with contractor(ctr, **kw) as c:
        refusal(lambda: c.run(t), NotImplementedError, f"torch tensors are not supported with '{name}'.")
        refusal(lambda: c.bind({0: t[0].T}), NotImplementedError, f"torch tensors are not supported with '{name}'.")
        refusal(lambda: c.bind({0: a[0], 1: t[1]}), NotImplementedError, f"torch tensors are not supported with '{name}'.")
        refusal(lambda: c.run(a, out=torch.empty(2, 3)), NotImplementedError, f"a torch tensor as 'out' is not supported with '{name}'.")
        # (a mix is a mix whatever the keywords)
        refusal(lambda: c.run([a[0], t[1], a[2]]), TypeError, "the arrays of one run must be all numpy arrays or all torch tensors.")


def test_a_leaf_beyond_the_range_of_a_mode_is_refused_on_the_host(ctr, no_gpu):
    a = arrays()
    a[1][0, 0] = 3.4e38
    with contractor(ctr, compute="bf16x3") as c:
        refusal(lambda: c.run(a), ValueError, "beyond the range of the bfloat16 split (|x| >= 2^128 - 2^119).")
    a[1][0, 0] = 70000.0
    with contractor(ctr, storage="float16") as c:
        refusal(lambda: c.bind({1: a[1]}), ValueError, "an array has finite values beyond the range of float16.")


def test_tensors_whose_numbers_are_not_those_in_their_memory_are_refused(ctr, no_gpu):
    """`t.conj()` shares data_ptr and strides with t and differs in a bit that no kernel sees; its `.imag` is a real tensor with
    the negative bit.  Both, and layouts without strides, are refused before the device of the tensor is looked at (every
    tensor here is on the host), after its shape and dtype."""
    import torch
    z = [torch.from_numpy(x) for x in arrays(np.complex64)]
    conj, neg = z[1].conj(), z[1].conj().imag
    assert conj.is_conj() and conj.data_ptr() == z[1].data_ptr() and conj.stride() == z[1].stride()
    assert neg.is_neg() and not neg.is_conj() and neg.dtype == torch.float32
    with contractor(ctr, dtype=np.complex64) as c:
        good = tuple(c.plan.shape)
        refusal(lambda: c.bind({1: conj}), ValueError, "a tensor is lazily conjugated (is_conj()): pass tensor.resolve_conj().")
        refusal(lambda: c.run([z[0].conj(), z[1], z[2]]), ValueError, "a tensor is lazily conjugated (is_conj()): pass tensor.resolve_conj().")
        refusal(lambda: c.bind({1: neg}), ValueError, "a tensor is lazily negated (is_neg()): pass tensor.resolve_neg().")
        refusal(lambda: c.bind({1: z[1].real.to_sparse()}), ValueError, "a tensor has the layout torch.sparse_coo: only strided tensors")
        refusal(lambda: c.bind({1: conj.T}), ValueError, "'ts_inds' is not consistent with 'arrays'.")  # (the shape first)
        refusal(lambda: c.bind({1: conj.to(torch.complex128)}), TypeError, "does not widen exactly")  # (then the dtype)
        refusal(lambda: c.bind({1: conj.resolve_conj()}), ValueError, "a tensor is on cpu, not on cuda:0.")  # (resolved: the device)
        refusal(lambda: c.bind({1: neg.resolve_neg()}), ValueError, "a tensor is on cpu, not on cuda:0.")
        a = arrays(np.complex64)
        out = torch.empty(good, dtype=torch.complex64)
        refusal(lambda: c.run(a, out=out.conj()), ValueError, "'out' is lazily conjugated (is_conj()): pass tensor.resolve_conj().")
        refusal(lambda: c.run(a, out=out.to_sparse()), ValueError, "'out' has the layout torch.sparse_coo: only strided tensors")
        refusal(lambda: c.run(a, out=out.conj().to(torch.complex128)), TypeError, "'out' must be of dtype complex64")
        refusal(lambda: c.run(a, out=out), ValueError, "'out' is on cpu, not on cuda:0.")
    with contractor(ctr, dtype=np.float32) as c:
        out = torch.empty(tuple(c.plan.shape), dtype=torch.complex64).conj().imag
        assert out.is_neg()
        refusal(lambda: c.run(arrays(), out=out), ValueError, "'out' is lazily negated (is_neg()): pass tensor.resolve_neg().")


def test_a_run_that_fails_leaves_no_leaf_bound_that_it_was_given(ctr, monkeypatch):
    """A bound leaf that a run is given another array for is dropped from the bound leaves before anything is loaded: when
    the run then fails, a later run() must ask for the leaf again and not use what the failed run left in its buffer."""
    a = arrays()
    c = contractor(ctr)
    c._bound = {0, 1, 2}  # (as after bind; no handle is needed for what follows)

    def fail(*args, **kw):
        raise RuntimeError("the load failed")

    monkeypatch.setattr(c, "_handle", lambda: (None, None))
    monkeypatch.setattr(c, "_load", fail)
    with pytest.raises(RuntimeError, match="the load failed"):
        c.run({1: a[1]})
    assert c._bound == {0, 2}
    refusal(lambda: c.run(), ValueError, "leaf 1 is neither bound nor given.")
    with pytest.raises(RuntimeError, match="the load failed"):
        c.bind({2: a[2]})
    assert c._bound == {0}


def test_what_a_run_refuses_of_out(ctr, no_gpu):
    import torch
    a = arrays()
    with contractor(ctr) as c:
        good = tuple(c.plan.shape)
        bad = good[::-1]
        assert sorted(good) == [2, 3] and c.plan.dtype == np.float32
        refusal(lambda: c.run(a, out=[[0.0] * 2] * 3), TypeError, "'out' must be a numpy array or a torch tensor.")
        refusal(lambda: c.run(a, out=np.empty(good, np.float64)), TypeError, "'out' must be of dtype float32, not float64.")
        refusal(lambda: c.run(a, out=np.empty(bad, np.float32)), ValueError, f"'out' must be C-contiguous and of shape {good}.")
        refusal(lambda: c.run(a, out=np.empty(bad, np.float32).T), ValueError, f"'out' must be C-contiguous and of shape {good}.")
        refusal(lambda: c.run(a, out=torch.empty(good, dtype=torch.float64)), TypeError, "'out' must be of dtype float32, not torch.float64.")
        refusal(lambda: c.run(a, out=torch.empty(good)), ValueError, "'out' is on cpu, not on cuda:0.")
        # the arrays are judged before out
        refusal(lambda: c.run(a[:2], out=np.empty(bad, np.float32)), ValueError, "'ts_inds' is not consistent with 'arrays'.")


# ---- the helpers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", rc.VIEWS, ids=[v.name for v in rc.VIEWS])
def test_merge_axes_on_the_views_of_the_table(ctr, view):
    import torch
    a = rc.apply(view, np.zeros(view.base, np.float32))
    assert ctr.merge_axes(a.shape, rc.numpy_strides(a)) == view.merged
    t = rc.apply(view, torch.zeros(view.base))  # torch states the same dims, strides and offset
    assert tuple(t.shape) == a.shape and t.storage_offset() == view.offset
    assert ctr.merge_axes(t.shape, t.stride()) == view.merged
    assert len(view.merged[0]) <= ctr.MAX_AXES and all(d > 1 for d in view.merged[0])


@pytest.mark.parametrize("name, shape, strides, want", rc.MANY_AXES, ids=[c[0] for c in rc.MANY_AXES])
def test_merge_axes_at_the_axis_limit(ctr, name, shape, strides, want):
    if isinstance(want, type):
        with pytest.raises(want):
            ctr.merge_axes(shape, strides)
    else:
        assert ctr.merge_axes(shape, strides) == want
        assert len(want[0]) <= ctr.MAX_AXES


def test_merge_axes_of_nothing(ctr):
    assert ctr.merge_axes((), ()) == ((), ())
    assert ctr.merge_axes((1, 1, 1), (7, 0, 1)) == ((), ())
    assert ctr.merge_axes((2, 3, 4), (12, 4, 1)) == ((24,), (1,))
    assert ctr.merge_axes((2, 3, 4), (0, 0, 0)) == ((24,), (0,))  # (expanded neighbours merge)
    assert ctr.merge_axes((2, 3, 4), (0, 4, 1)) == ((2, 12), (0, 1))


def test_the_extent_check_from_both_sides_of_the_end(ctr):
    # the last element reached: offset + sum (d - 1) s
    for offset, dims, strides in ((0, (), ()), (5, (), ()), (0, (7,), (1,)), (3, (4, 4), (7, 1)), (0, (6, 6), (11, 2)),
                                  (2, (4, 3, 5), (5, 0, 1)), (0, (2,) * 16, tuple(2 ** k for k in range(16)))):
        last = offset + sum((d - 1) * s for d, s in zip(dims, strides))
        ctr.check_extent(offset, dims, strides, last + 1)
        with pytest.raises(ValueError, match=f"reaches element {last} of a storage of {last} elements"):
            ctr.check_extent(offset, dims, strides, last)
    with pytest.raises(ValueError):
        ctr.check_extent(-1, (2,), (1,), 10)
    for view in rc.VIEWS:  # the views of the table end where their base ends, or before
        n = int(np.prod(view.base, dtype=np.int64))
        ctr.check_extent(view.offset, *view.merged, n)


# ---- the models ----------------------------------------------------------------------------------------------------

def kernel_offsets(dims, strides):
    """The offset on the strided side of every element of the contiguous side, as io_offset (csrc/contract_io.h) computes it."""
    off = np.zeros(1, np.int64)
    for d, s in zip(dims, strides):
        off = (off.reshape(-1, 1) + np.arange(d, dtype=np.int64) * s).reshape(-1)
    return off


@pytest.mark.parametrize("view", rc.VIEWS, ids=[v.name for v in rc.VIEWS])
def test_the_ingest_model_is_a_gather_through_the_merged_axes(ctr, view):
    for src, dst in ((np.float32, np.float32), (np.complex64, np.complex64)) + rc.WIDENINGS:
        base = rc.fill(view.base, src, seed=3)
        want = rc.ingest_model(view, base, dst)
        assert want.dtype == dst and want.flags.c_contiguous and want.shape == view.shape
        got = base.reshape(-1)[view.offset + kernel_offsets(*view.merged)]
        assert np.array_equal(got.astype(dst), want.reshape(-1))
        if np.dtype(dst).kind == "c" and np.dtype(src).kind != "c":  # a real source: +0.0, not -0.0
            assert not np.signbit(want.imag).any()


def emit_plans(ctr):
    for name, ts, dims, path, output, slices in (rc.EMIT_SCALAR, rc.EMIT_PERMUTE):
        yield name, ctr.plan(path, ts, [tuple(dims[x] for x in xs) for xs in ts], output, slices=slices, dtype=np.float32)
    for chain in (bc.SMALL, bc.SUMMED, bc.PLACED):
        yield chain.name, ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=np.float32)


def test_the_emit_model_is_a_scatter_through_the_merged_axes(ctr):
    seen = set()
    for name, p in emit_plans(ctr):
        staging = np.arange(p.out_numel, dtype=np.float32)
        want = rc.emit_model(p, staging)
        from tnco_amd.contraction import _c_strides, _host_layout
        assert np.array_equal(want, _host_layout(p, staging)) and want.shape == tuple(p.shape), name
        rest = tuple(x for x in p.inds if x not in set(p.slice_inds))
        held = p.block_inds + rest
        at = [p.inds.index(x) for x in held]
        dims, strides = ctr.merge_axes([p.shape[q] for q in at], [_c_strides(p.shape)[q] for q in at])
        got = np.empty(p.out_numel, np.float32)
        got[kernel_offsets(dims, strides)] = staging
        assert np.array_equal(got.reshape(p.shape), want), name
        seen.add(held == tuple(p.inds))
    assert seen == {True, False}  # (identity and a real permutation both occur)
    name, p = list(emit_plans(ctr))[1]
    assert p.block_inds == ("p",) and p.inds.index("p") != 0
