"""The host side of the matrix mode of tnco_amd.contraction (`compute="matrix"`), no GPU: in the four dtypes the plan is
the plan of `compute=None` table for table and byte for byte of memory, the refusals come before any device use and in a
fixed precedence, and the refusals of `compute="bf16x3"` are what they were."""
import numpy as np
import pytest

from tests import matrix_cases as mc
from tests import split_cases as sc
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn

ALL = (np.float32, np.float64, np.complex64, np.complex128)
TABLES = ("steps", "perms", "leaf_sl", "leaf_numel")
FIELDS = ("dtype", "inds", "shape", "slice_inds", "slice_dims", "block_inds", "arena_elems", "out_numel",
          "macs_per_slice", "slice_range", "slice_batch", "scaling", "stage_refs", "row_steps", "hoisted", "kept")


def assert_same_plan(p, plain, what):
    assert p.compute == "matrix" and plain.compute is None and p.storage is None, what
    for f in TABLES:
        x, y = getattr(p, f), getattr(plain, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, f)
    assert repr(p.ops) == repr(plain.ops), what
    for f in FIELDS:
        assert getattr(p, f) == getattr(plain, f), (what, f)
    for f in ("step_hoist", "perm_hoist"):
        x, y = getattr(p, f), getattr(plain, f)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), (what, f)
    assert p.peak_device_bytes == plain.peak_device_bytes, what


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: np.dtype(d).name)
def test_the_plan_of_every_split_case_is_the_plain_plan_byte_for_byte(dtype):
    for case in sc.CASES + mc.CASES:
        for kw in (dict(), dict(slice_batch=3), dict(hoist=True)):
            args = ([(0, 1)], case.ts, case.shapes(), case.output)
            plain = ctr.plan(*args, slices=case.slices, dtype=dtype, **kw)
            p = ctr.plan(*args, slices=case.slices, dtype=dtype, compute="matrix", **kw)
            assert_same_plan(p, plain, (case.name, kw))


def _network(seed, n=14):
    ts, d, o = syn.random_regular_tn(n, seed=seed)
    dims = {x: (d[x] if isinstance(d, dict) else d) for xs in ts for x in xs}
    shapes = [tuple(dims[x] for x in xs) for xs in ts]
    path = [(0, 1)] * (len(ts) - 1)
    every = list(dict.fromkeys(x for xs in ts for x in xs))
    return path, ts, shapes, o, every


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("seed", range(3))
def test_the_plan_of_a_sliced_network_is_the_plain_plan_byte_for_byte(seed, dtype):
    path, ts, shapes, o, every = _network(seed)
    cut = every[:seed]
    for kw in (dict(), dict(slice_batch=3), dict(hoist=True), dict(slice_batch=2, hoist=True)):
        plain = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, **kw)
        p = ctr.plan(path, ts, shapes, o, slices=cut, dtype=dtype, compute="matrix", **kw)
        assert_same_plan(p, plain, (seed, kw))


def test_the_default_dtype_of_plan_is_accepted():
    p = ctr.plan([(0, 1)], [("a", "b"), ("b", "c")], [(2, 3), (3, 4)], compute="matrix")
    assert p.compute == "matrix" and p.dtype == np.dtype(np.float64)


def test_the_cases_of_the_gpu_test_plan_as_their_table_says():
    for case in mc.CASES:
        for dtype in ALL:
            p = ctr.plan([(0, 1)], case.ts, case.shapes(), case.output, slices=case.slices, dtype=dtype, compute="matrix")
            (op,) = p.ops
            assert {k: op[k] for k in ("H", "M", "N", "K", "form_a", "form_b")} == \
                {k: case.ops[k] for k in ("H", "M", "N", "K", "form_a", "form_b")}, case.name
            assert len(p.perms) == case.ops["perms"], case.name
            tiled = op["M"] >= 64 and op["N"] >= 64 and op["K"] > 32  # the dispatch rule of csrc/contract.hip
            assert tiled == any(k.startswith("tiled") for k in case.kernels), case.name
            assert tiled == (mc.matrix_launches(case) > 0), case.name


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: np.dtype(d).name)
def test_a_plan_without_steps_takes_the_keyword(dtype):
    p = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), dtype=dtype, compute="matrix")
    q = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slices=("s",), dtype=dtype)
    assert p.compute == "matrix" and len(p.steps) == 0 and p.perms.tobytes() == q.perms.tobytes()
    assert p.peak_device_bytes == q.peak_device_bytes


def test_the_result_counts_the_launches_in_a_last_field_with_a_default():
    import dataclasses
    fields = [f.name for f in dataclasses.fields(ctr.ContractionResult)]
    assert fields[-1] == "matrix_launches" and "matrix" in ctr.COMPUTES and list(ctr.COMPUTES)[0] == "bf16x3"
    assert ctr.ContractionResult((), None, 0, 1, 0).matrix_launches == 0


def _no_gpu(monkeypatch):
    from tnco_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)


def test_refusals_before_any_device_use_and_their_precedence(monkeypatch):
    _no_gpu(monkeypatch)
    ts, shapes = [("a", "b"), ("b", "c")], [(2, 3), (3, 4)]
    f32 = [np.ones(s, np.float32) for s in shapes]
    f64 = [a.astype(np.float64) for a in f32]
    projs = dict(output_inds=("a", "c"), sparse_inds=("a",), projs=np.array([[0], [1]]))
    unknown = "'compute' must be None or 'bf16x3' or 'matrix'."
    exclusive = "'compute' and 'storage' are exclusive."
    no_projs = "projections are not supported with 'compute'."
    no_path = "'compute' is not supported with 'path_kernel'."
    # 1. an unknown value, whatever else is wrong with the call
    for name in ("Matrix", "MATRIX", "mfma", "matrix ", "f64", 1, True):
        for kw in (dict(), dict(storage="bfloat16"), projs, dict(path_kernel=2)):
            for arrays in (f32, f64):
                with pytest.raises(ValueError, match=unknown):
                    ctr.contract([(0, 1)], ts, arrays, compute=name, **kw)
        with pytest.raises(ValueError, match=unknown):
            ctr.plan([(0, 1)], ts, shapes, compute=name, storage="float16")
    # 2. with storage, before the projections and the path kernel are looked at
    for storage in ("float16", "bfloat16"):
        for arrays in (f32, f64):
            for kw in (dict(), projs, dict(path_kernel=2)):
                with pytest.raises(ValueError, match=exclusive):
                    ctr.contract([(0, 1)], ts, arrays, compute="matrix", storage=storage, **kw)
        with pytest.raises(ValueError, match=exclusive):
            ctr.plan([(0, 1)], ts, shapes, compute="matrix", storage=storage, scaling="tensor")
    # 3. projections, in every dtype, before the path kernel
    for arrays in (f32, f64, [f32[0], f32[1].astype(np.complex128)]):
        for kw in (dict(), dict(path_kernel=2)):
            with pytest.raises(NotImplementedError, match=no_projs):
                ctr.contract([(0, 1)], ts, arrays, compute="matrix", **projs, **kw)
    with pytest.raises(NotImplementedError, match=no_projs):
        ctr.plan([(0, 1)], ts, shapes, dtype=np.complex64, compute="matrix", **projs)
    # 4. a path kernel, as for any compute mode
    for arrays in (f32, f64):
        with pytest.raises(NotImplementedError, match=no_path):
            ctr.contract([(0, 1)], ts, arrays, compute="matrix", path_kernel=2)
    with pytest.raises(NotImplementedError, match=no_path):
        ctr.plan([(0, 1)], ts, shapes, compute="matrix", path_kernel=2)
    # no refusal: every dtype reaches for the device, with a slice batch and with hoisting too
    for arrays in (f32, f64, [a.astype(np.complex64) for a in f32], [a.astype(np.complex128) for a in f32]):
        for kw in (dict(), dict(slice_batch=4), dict(hoist=True)):
            with pytest.raises(AssertionError, match="the device was reached"):
                ctr.contract([(0, 1)], ts, arrays, compute="matrix", **kw)
    # a leaf beyond the range of the bfloat16 split is no concern of this mode
    big = [f32[0] * np.finfo(np.float32).max, f32[1]]
    with pytest.raises(AssertionError, match="the device was reached"):
        ctr.contract([(0, 1)], ts, big, compute="matrix")
    with pytest.raises(ValueError, match="finite values beyond the range of the bfloat16 split"):
        ctr.contract([(0, 1)], ts, big, compute="bf16x3")


def test_the_refusals_of_bf16x3_are_unchanged(monkeypatch):
    _no_gpu(monkeypatch)
    ts, shapes = [("a", "b"), ("b", "c")], [(2, 3), (3, 4)]
    f32 = [np.ones(s, np.float32) for s in shapes]
    wide = "with 'compute' the compute dtype must be float32 or complex64"
    for dtype in (np.float64, np.complex128):
        with pytest.raises(TypeError, match=wide):
            ctr.contract([(0, 1)], ts, [f32[0], f32[1].astype(dtype)], compute="bf16x3")
        with pytest.raises(TypeError, match=wide):
            ctr.plan([(0, 1)], ts, shapes, dtype=dtype, compute="bf16x3")
    with pytest.raises(TypeError, match=wide):
        ctr.plan([(0, 1)], ts, shapes, compute="bf16x3")  # (plan's default dtype is float64)
    for name in ("bf16", "bf16x6", "tf32", "BF16X3"):
        with pytest.raises(ValueError, match="'compute' must be None or 'bf16x3'."):
            ctr.plan([(0, 1)], ts, shapes, dtype=np.float32, compute=name)
    with pytest.raises(ValueError, match="'compute' and 'storage' are exclusive."):
        ctr.plan([(0, 1)], ts, shapes, dtype=np.float32, compute="bf16x3", storage="bfloat16")
    assert ctr.COMPUTES["bf16x3"] == 1


def test_contract_results_refuses_before_the_network_is_looked_at(monkeypatch):
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match="'compute' and 'storage' are exclusive."):
        ctr.contract_results(None, [], None, None, compute="matrix", storage="float16")
    with pytest.raises(NotImplementedError, match="projections are not supported with 'compute'."):
        ctr.contract_results(None, [], None, None, compute="matrix", projs=np.zeros((1, 1), int))
    with pytest.raises(NotImplementedError, match="'compute' is not supported with 'path_kernel'."):
        ctr.contract_results(None, [], None, None, compute="matrix", path_kernel=4)
