"""`contraction.Contractor` on the device: leaves from torch tensors through ct_ingest_kernel, results into torch tensors
through ct_emit_kernel (csrc/contract_io.h), one handle over many runs.

The oracle is `contract()` on the same numpy arrays (for a tensor: on the numpy model of the ingest, the view made
contiguous and widened on the host): `array` must be byte for byte equal, every other field of the result but
`device_s` equal, a second run byte-equal again.  The values are small integers in both parts (tests/resident_cases.py),
exact in every dtype, so every result is finite; an element that is not a number fails.  The cases are those of
tests/resident_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as bc
from tests import gather_cases as gc
from tests import resident_cases as rc

pytestmark = pytest.mark.gpu

DTYPE_IDS = [np.dtype(d).name for d in rc.DTYPES]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def fields(r):
    return {k: v for k, v in vars(r).items() if k not in ("array", "device_s")}


def assert_same(r, want, what):
    got = host(r.array)
    assert got.dtype == want.array.dtype and got.shape == want.array.shape, what
    assert np.isfinite(got).all(), what
    assert np.array_equal(bits(got), bits(want.array)), f"{what}: the bytes differ from contract()"
    assert fields(r) == fields(want), what


def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(np.shape(a))).cuda()  # (ascontiguousarray gives a 0-d array an axis)


def run_view(ctr, torch, view, src, dst, seed):
    """The view, a tensor of dtype `src`, into a plan of dtype `dst`: alone and as the first operand of a step."""
    base = rc.fill(view.base, src, seed)
    leaf = rc.ingest_model(view, base, dst)
    tensor = rc.apply(view, on_device(torch, base))
    assert tensor.storage_offset() == view.offset and ctr.merge_axes(tensor.shape, tensor.stride()) == view.merged
    for name, ts, shapes, path, output in rc.networks(view):
        what = f"{view.name} {np.dtype(src).name} -> {np.dtype(dst).name} {name}"
        arrays, tensors = [leaf], [tensor]
        if len(ts) == 2:
            arrays.append(rc.fill(shapes[1], dst, seed + 1))
            tensors.append(on_device(torch, arrays[1]))
        want = ctr.contract(path, ts, arrays, output)
        with ctr.Contractor(path, ts, shapes, output, dtype=dst) as c:
            r = c.run(tensors)
            assert isinstance(r.array, torch.Tensor) and r.array.device.index == c.device and r.array.is_contiguous(), what
            assert_same(r, want, what)
            assert_same(c.run(tensors), want, what + " (second run)")
            assert c.io_launches == (2 * len(ts), 2), what


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DTYPE_IDS)
def test_contiguous_leaves_at_every_remainder_of_the_16_byte_path(ctr, torch, dtype):
    for k, view in enumerate(rc.CONTIGUOUS + rc.UNALIGNED):
        run_view(ctr, torch, view, dtype, dtype, seed=10 + k)


@pytest.mark.parametrize("view", [rc.BIG, rc.BIG_UNALIGNED, rc.BIG_STRIDED], ids=lambda v: v.name)
@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DTYPE_IDS)
def test_a_leaf_past_one_trip_of_the_grid(ctr, torch, view, dtype):
    assert view.numel > rc.TRIP and view.numel % 2 == 1
    run_view(ctr, torch, view, dtype, dtype, seed=30)


@pytest.mark.parametrize("view", rc.STRIDED, ids=lambda v: v.name)
def test_strided_leaves(ctr, torch, view):
    for k, dtype in enumerate(rc.DTYPES):
        run_view(ctr, torch, view, dtype, dtype, seed=40 + k)


@pytest.mark.parametrize("src, dst", rc.WIDENINGS, ids=[f"{np.dtype(s).name}-{np.dtype(d).name}" for s, d in rc.WIDENINGS])
def test_the_five_widenings_contiguous_and_strided(ctr, torch, src, dst):
    by_name = {v.name: v for v in rc.VIEWS}
    for k, name in enumerate(("plain-4x5", "unaligned-5", "contiguous-7", "permuted", "expanded", "offset", "past-one-trip")):
        run_view(ctr, torch, by_name[name], src, dst, seed=50 + k)


# ---- emit ----------------------------------------------------------------------------------------------------------

def emit_case(ctr, torch, ts, shapes, path, output, slices, dtype, seed, what):
    arrays = [rc.fill(s, dtype, seed + k) for k, s in enumerate(shapes)]
    want = ctr.contract(path, ts, arrays, output, slices=slices)
    tensors = [on_device(torch, a) for a in arrays]
    with ctr.Contractor(path, ts, shapes, output, dtype=dtype, slices=slices) as c:
        r = c.run(tensors)
        assert_same(r, want, what)
        assert tuple(r.array.shape) == tuple(c.plan.shape)
        out = torch.full(tuple(c.plan.shape), 7, dtype=r.array.dtype, device="cuda")
        c.bind(dict(enumerate(tensors)))
        r2 = c.run(out=out)
        assert r2.array is out
        assert_same(r2, want, what + " (out=)")
        out.zero_()
        assert_same(c.run(tensors, out=out), want, what + " (a second run into the same out)")
        assert c.io_launches == (3 * len(ts), 3), what
        # numpy leaves, a torch result; torch leaves, a numpy result
        assert_same(c.run(arrays, out=out), want, what + " (numpy in, torch out)")
        into = np.full(tuple(c.plan.shape), 7, dtype)
        r3 = c.run(tensors, out=into)
        assert r3.array is into
        assert_same(r3, want, what + " (torch in, numpy out)")
        assert c.io_launches == (4 * len(ts), 4), what
        return c.plan


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=DTYPE_IDS)
def test_a_scalar_result_and_a_result_that_emit_must_permute(ctr, torch, dtype):
    for name, ts, dims, path, output, slices in (rc.EMIT_SCALAR, rc.EMIT_PERMUTE):
        p = emit_case(ctr, torch, ts, [tuple(dims[x] for x in xs) for xs in ts], path, output, slices, dtype, 60, name)
    assert p.block_inds == ("p",) and p.inds.index("p") != 0


@pytest.mark.parametrize("variant", ["base", "summed", "placed"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_the_chain_with_three_one_and_twelve_blocks(ctr, torch, variant, dtype):
    chain = bc.Chain(f"small-{variant}", bc.SMALL.sizes, bc.SMALL.classes, variant)
    p = emit_case(ctr, torch, chain.ts, chain.shapes(), bc.PATH, chain.output, bc.SLICES, dtype, 70, chain.name)
    assert p.out_numel // (p.out_numel // chain.n_blocks) == chain.n_blocks


@pytest.mark.parametrize("variant, dtype", [("base", np.float32), ("summed", np.float32), ("placed", np.float32),
                                            ("base", np.complex128), ("summed", np.complex128)],
                         ids=["base-float32", "summed-float32", "placed-float32", "base-complex128", "summed-complex128"])
def test_the_chain_with_a_block_past_one_trip(ctr, torch, variant, dtype):
    """The block of 1030 x 513 = 528 390 elements of tests/gather_cases.py (twelve blocks of it in complex128 are 101 MB:
    that variant stays out, as it does there)."""
    assert gc.RD_BLOCK > rc.TRIP
    chain = bc.Chain(f"reduce-{variant}", gc.RD_SIZES, ("stream", "stream"), variant)
    arrays = [rc.fill(s, dtype, 80 + k) for k, s in enumerate(chain.shapes())]
    want = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES)
    with ctr.Contractor(bc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, slices=bc.SLICES) as c:
        c.bind({t: on_device(torch, a) for t, a in enumerate(arrays)})
        r = c.run(out=torch.empty(tuple(c.plan.shape), dtype=torch.from_numpy(arrays[0]).dtype, device="cuda"))
        assert_same(r, want, chain.name)
        assert_same(c.run(out=r.array), want, chain.name + " (a second run into the same out)")


# ---- resident behaviour ----------------------------------------------------------------------------------------------

def test_bound_leaves_stay_and_given_leaves_change(ctr, torch):
    chain, dtype = bc.SMALL, np.complex64
    a = [rc.fill(s, dtype, 90 + k) for k, s in enumerate(chain.shapes())]
    third = [rc.fill(chain.shapes()[2], dtype, 95), rc.fill(chain.shapes()[2], dtype, 96)]
    first = rc.fill(chain.shapes()[0], dtype, 97)
    call = lambda arrays: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES)  # noqa: E731
    with ctr.Contractor(bc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, slices=bc.SLICES) as c:
        c.bind({0: a[0], 1: on_device(torch, a[1])})  # (one from numpy, one from torch)
        assert c.io_launches == (1, 0)
        for t in third:
            r = c.run({2: on_device(torch, t)})
            assert isinstance(r.array, torch.Tensor)
            assert_same(r, call([a[0], a[1], t]), "two bound, the third given")
        with pytest.raises(ValueError, match="leaf 2 is neither bound nor given."):
            c.run()  # (a leaf given to a run is not bound by it)
        c.bind({0: on_device(torch, first)})  # bound again: replaced
        r = c.run({2: third[0]})  # bound from torch, run from numpy
        assert isinstance(r.array, np.ndarray)
        assert_same(r, call([first, a[1], third[0]]), "a leaf bound again")
        c.bind({2: third[1]})
        r = c.run()
        assert isinstance(r.array, np.ndarray)
        assert_same(r, call([first, a[1], third[1]]), "every leaf bound")
        r = c.run(a)  # every leaf given, numpy: the one-call path
        assert_same(r, call(a), "every leaf given")
        with pytest.raises(ValueError, match="leaf 0 is neither bound nor given."):
            c.run()  # (a bound leaf that a run was given another array for is bound no longer)
        assert c.io_launches == (4, 2)
    with pytest.raises(ValueError, match="the Contractor is closed."):
        c.run()


# ---- keywords --------------------------------------------------------------------------------------------------------

KEYWORDS = [dict(slice_batch=1), dict(slice_batch=5), dict(slice_batch=64), dict(path_kernel=1), dict(path_kernel=5),
            dict(path_kernel=1024), dict(hoist=True), dict(reuse=True), dict(reuse=True, slice_order=("t", "u", "p")),
            dict(indirect=True), dict(compute="matrix"), dict(compute="bf16x3"), dict(accumulate="float64"),
            dict(slice_range=(1, 11))]


@pytest.mark.parametrize("kw", KEYWORDS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in KEYWORDS])
def test_the_chain_under_every_keyword_with_tensors_in_and_out(ctr, torch, kw):
    chain = bc.PLAIN[0] if "compute" in kw else bc.SMALL  # (a compute mode changes the tiled class only)
    dtype = np.float32
    arrays = [rc.fill(s, dtype, 100 + k) for k, s in enumerate(chain.shapes())]
    want = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, **kw)
    if "compute" in kw:
        assert (want.matrix_launches or want.split_launches) > 0
    with ctr.Contractor(bc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, slices=bc.SLICES, **kw) as c:
        tensors = [on_device(torch, a) for a in arrays]
        r = c.run(tensors)
        assert isinstance(r.array, torch.Tensor)
        assert_same(r, want, str(kw))
        assert r.launches == want.launches and r.kernel_launches == want.kernel_launches
        assert_same(c.run(tensors, out=r.array), want, f"{kw} (second run)")
        assert r.peak_device_bytes == want.peak_device_bytes  # (ingest and emit reserve nothing)


def test_a_tensor_beyond_the_range_of_the_split_is_refused(ctr, torch):
    chain = bc.SMALL
    arrays = [rc.fill(s, np.float32, 110 + k) for k, s in enumerate(chain.shapes())]
    arrays[1].reshape(-1)[3] = 3.4e38
    text = r"an array has finite values beyond the range of the bfloat16 split \(\|x\| >= 2\^128 - 2\^119\)\."
    with ctr.Contractor(bc.PATH, chain.ts, chain.shapes(), chain.output, dtype=np.float32, slices=bc.SLICES, compute="bf16x3") as c:
        with pytest.raises(ValueError, match=text):
            c.run([on_device(torch, a) for a in arrays])
        arrays[1].reshape(-1)[3] = 3.3e38  # (inside the range)
        want = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, compute="bf16x3")
        r = c.run([on_device(torch, a) for a in arrays])
        assert np.array_equal(bits(host(r.array)), bits(want.array))


HOST_SIDE = [dict(storage="float16"), dict(storage="bfloat16"), dict(storage="float16", scaling="tensor"),
             dict(storage="bfloat16", scaling="tensor", slice_batch=5)]


@pytest.mark.parametrize("kw", HOST_SIDE, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in HOST_SIDE])
def test_the_numpy_path_with_storage_and_scaling(ctr, kw):
    chain, dtype = bc.SMALL, np.complex64
    arrays = [rc.fill(s, dtype, 120 + k) for k, s in enumerate(chain.shapes())]
    other = rc.fill(chain.shapes()[2], dtype, 125) * np.float32(64)  # (another exponent under scaling)
    call = lambda a: ctr.contract(bc.PATH, chain.ts, a, chain.output, slices=bc.SLICES, **kw)  # noqa: E731
    with ctr.Contractor(bc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, slices=bc.SLICES, **kw) as c:
        assert_same(c.run(arrays), call(arrays), str(kw))
        c.bind({0: arrays[0], 1: arrays[1]})
        assert_same(c.run({2: other}), call(arrays[:2] + [other]), f"{kw} (two bound)")
        assert_same(c.run({2: arrays[2]}), call(arrays), f"{kw} (the third given again)")
        assert c.io_launches == (0, 0)


def test_the_numpy_path_with_projections(ctr):
    ts, shapes = [("a", "k", "p"), ("k", "b", "p")], [(3, 4, 2), (4, 5, 2)]
    kw = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [2, 4], [0, 1], [1, 0]]), slices=("p",))
    arrays = [rc.fill(s, np.float64, 130 + k) for k, s in enumerate(shapes)]
    want = ctr.contract([(0, 1)], ts, arrays, ("a", "b"), **kw)
    with ctr.Contractor([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float64, **kw) as c:
        assert_same(c.run(arrays), want, "projs")
        c.bind({1: arrays[1]})
        out = np.empty(want.array.shape, np.float64)
        r = c.run({0: arrays[0]}, out=out)
        assert r.array is out
        assert_same(r, want, "projs (one bound, out=)")


# ---- the C ABI -------------------------------------------------------------------------------------------------------

def test_what_the_entry_points_refuse_and_that_the_handle_stays_as_it_was(ctr, torch):
    from tnco_amd import _lib
    L = _lib.load()
    ts, shapes = [("i", "k"), ("k", "j")], [(4, 5), (5, 6)]
    arrays = [rc.fill(s, np.float32, 140 + k) for k, s in enumerate(shapes)]
    want = ctr.contract([(0, 1)], ts, arrays, ("i", "j"))
    tensors = [on_device(torch, a) for a in arrays]
    wide = on_device(torch, arrays[0].astype(np.float64))
    i64 = lambda *v: np.array(v, np.int64).ctypes.data_as(C.c_void_p)  # noqa: E731
    dev = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hostp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def refused(rc_, text):
        assert rc_ == _lib.EINVAL and L.tnco_hip_last_error().decode() == text, (rc_, L.tnco_hip_last_error())

    out_t = torch.zeros(4, 6, dtype=torch.float32, device="cuda")
    out_n = np.zeros(24, np.float32)
    torch.cuda.synchronize()
    with ctr.Contractor([(0, 1)], ts, shapes, ("i", "j"), dtype=np.float32) as c:
        _, h = c._handle()
        counts = np.zeros(2, np.int64)
        refused(L.tnco_hip_contract_io_launches(None, hostp(counts)), "null argument.")
        refused(L.tnco_hip_contract_io_launches(h, None), "null argument.")
        # nothing is loaded yet
        refused(L.tnco_hip_contract_run_loaded(h, hostp(out_n), 0, 0, None, None), "leaf 0 was never loaded.")
        assert L.tnco_hip_contract_load_leaf(h, 0, dev(tensors[0]), 1, 0, 2, i64(4, 5), None) == _lib.OK
        refused(L.tnco_hip_contract_run_loaded(h, hostp(out_n), 0, 0, None, None), "leaf 1 was never loaded.")
        assert L.tnco_hip_contract_load_leaf(h, 1, hostp(arrays[1]), 0, 0, 1, i64(30), None) == _lib.OK
        load = L.tnco_hip_contract_load_leaf
        refused(load(None, 0, dev(tensors[0]), 1, 0, 2, i64(4, 5), None), "null argument.")
        refused(load(h, 0, None, 1, 0, 2, i64(4, 5), None), "null argument.")
        refused(load(h, -1, dev(tensors[0]), 1, 0, 2, i64(4, 5), None), "'leaf' is not a leaf of the plan.")
        refused(load(h, 2, dev(tensors[0]), 1, 0, 2, i64(4, 5), None), "'leaf' is not a leaf of the plan.")
        refused(load(h, 0, dev(tensors[0]), 2, 0, 2, i64(4, 5), None), "'where' must be 0 (host) or 1 (device).")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 33, i64(*([1] * 32), 20), None), "'ndim' must be from 0 to 32.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, -1, i64(20), None), "'ndim' must be from 0 to 32.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 2, None, None), "null argument.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 2, i64(0, 5), None), "dims must be positive.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 2, i64(4, 5), i64(5, -1)), "a stride is negative.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 2, i64(4, 6), None), "dims do not multiply to the leaf's elements.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 2, i64(2, 5), None), "dims do not multiply to the leaf's elements.")
        refused(load(h, 0, dev(tensors[0]), 1, 0, 0, None, None), "dims do not multiply to the leaf's elements.")
        refused(load(h, 0, hostp(arrays[0]), 0, 1, 1, i64(20), None), "a host leaf must have the plan's dtype.")
        refused(load(h, 0, hostp(arrays[0]), 0, 0, 1, i64(20), i64(1)), "a host leaf must be C-contiguous: 'strides' must be NULL.")
        for code in (1, 2, 3, 4, 7, -1, 8):  # (a narrowing, a storage code, no code at all)
            refused(load(h, 0, dev(wide), 1, code, 2, i64(4, 5), None), "'src_dtype' does not widen to the plan's dtype.")
        run = L.tnco_hip_contract_run_loaded
        refused(run(None, dev(out_t), 1, 2, i64(4, 6), i64(6, 1)), "null argument.")
        refused(run(h, None, 1, 2, i64(4, 6), i64(6, 1)), "null argument.")
        refused(run(h, dev(out_t), 2, 2, i64(4, 6), i64(6, 1)), "'where' must be 0 (host) or 1 (device).")
        refused(run(h, dev(out_t), 1, 2, i64(4, 6), None), "null argument.")
        refused(run(h, dev(out_t), 1, 33, i64(*([1] * 32), 24), i64(*([1] * 33))), "'ndim' must be from 0 to 32.")
        refused(run(h, dev(out_t), 1, 2, i64(4, 0), i64(6, 1)), "dims must be positive.")
        refused(run(h, dev(out_t), 1, 2, i64(4, 5), i64(5, 1)), "dims do not multiply to the output's elements.")
        refused(run(h, dev(out_t), 1, 2, i64(4, 6), i64(6, -1)), "a stride is negative.")
        refused(run(h, dev(out_t), 1, 2, i64(4, 6), i64(0, 1)), "a destination stride is 0.")
        assert not out_t.any() and not out_n.any()  # (nothing ran)
        assert L.tnco_hip_contract_io_launches(h, hostp(counts)) == _lib.OK and tuple(counts) == (1, 0)
        # the handle is as it was: the two leaves loaded above, a valid run
        assert run(h, dev(out_t), 1, 2, i64(4, 6), i64(6, 1)) == _lib.OK
        assert np.array_equal(bits(host(out_t)), bits(want.array))
        assert run(h, hostp(out_n), 0, 0, None, None) == _lib.OK
        assert np.array_equal(bits(out_n), bits(want.array))
        assert_same(c.run(tensors), want, "after the refusals")
        assert L.tnco_hip_contract_io_launches(h, hostp(counts)) == _lib.OK and tuple(counts) == (3, 2)
    # a handle with a storage dtype, and one with scaling: no device leaves
    half = on_device(torch, arrays[0])
    for kw in (dict(storage="float16"), dict(storage="bfloat16", scaling="tensor")):
        with ctr.Contractor([(0, 1)], ts, shapes, ("i", "j"), dtype=np.float32, **kw) as c:
            _, h = c._handle()
            refused(L.tnco_hip_contract_load_leaf(h, 0, dev(half), 1, 0, 2, i64(4, 5), None),
                    "a device leaf is not supported with a storage dtype or scaling.")
            assert_same(c.run(arrays), ctr.contract([(0, 1)], ts, arrays, ("i", "j"), **kw), str(kw))
    # a handle with row axes: no device result
    ts, shapes = [("a", "k"), ("k", "b")], [(3, 4), (4, 5)]
    kw = dict(sparse_inds=("a", "b"), projs=np.array([[0, 1], [2, 4]]))
    arrays = [rc.fill(s, np.float32, 150 + k) for k, s in enumerate(shapes)]
    with ctr.Contractor([(0, 1)], ts, shapes, ("a", "b"), dtype=np.float32, **kw) as c:
        want = ctr.contract([(0, 1)], ts, arrays, ("a", "b"), **kw)
        assert_same(c.run(arrays), want, "projs")
        _, h = c._handle()
        n = c.plan.out_numel
        spare = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        refused(L.tnco_hip_contract_run_loaded(h, dev(spare), 1, 1, i64(n), i64(1)), "a device result is not supported with row axes.")
        assert_same(c.run(arrays), want, "projs, after the refusal")


def test_a_conjugated_tensor_is_refused_and_its_resolved_form_is_the_conjugate(ctr, torch):
    """`t.conj()` is t's memory with a bit set that the kernels do not see: refused, as an operand and as `out=`.
    `t.conj().resolve_conj()` holds the conjugated numbers and runs as `contract()` does on np.conj(a)."""
    ts, shapes = [("i", "k"), ("k", "j")], [(4, 5), (5, 6)]
    arrays = [rc.fill(s, np.complex64, 160 + k) for k, s in enumerate(shapes)]
    want = ctr.contract([(0, 1)], ts, [np.conj(arrays[0]), arrays[1]], ("i", "j"))
    plain = ctr.contract([(0, 1)], ts, arrays, ("i", "j"))
    assert not np.array_equal(bits(want.array), bits(plain.array))
    t = [on_device(torch, a) for a in arrays]
    lazy = t[0].conj()
    assert lazy.is_conj() and lazy.data_ptr() == t[0].data_ptr()
    with ctr.Contractor([(0, 1)], ts, shapes, ("i", "j"), dtype=np.complex64) as c:
        with pytest.raises(ValueError, match=r"a tensor is lazily conjugated \(is_conj\(\)\): pass tensor.resolve_conj\(\)\."):
            c.run([lazy, t[1]])
        with pytest.raises(ValueError, match=r"a tensor is lazily negated \(is_neg\(\)\): pass tensor.resolve_neg\(\)\."):
            c.bind({0: torch._neg_view(t[0])})
        assert c.io_launches == (0, 0)
        assert_same(c.run([lazy.resolve_conj(), t[1]]), want, "resolve_conj()")
        out = torch.empty(tuple(c.plan.shape), dtype=torch.complex64, device="cuda")
        with pytest.raises(ValueError, match=r"'out' is lazily conjugated \(is_conj\(\)\): pass tensor.resolve_conj\(\)\."):
            c.run(t, out=out.conj())
        assert_same(c.run(t, out=out), plain, "the tensors as they are")
