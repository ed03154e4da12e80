"""`slice_batch=` on the host side of the contraction engine (tnco_amd/contraction.py): the plan is that of the unbatched
run, the memory a batch reserves is counted, and the keyword is validated before anything else happens.  No GPU."""
import numpy as np
import pytest

from tests import batch_cases as bc
from tnco_amd import contraction as ctr

CHAIN = bc.PLAIN[0]
MODES = [dict(), dict(storage="bfloat16"), dict(storage="float16", scaling="tensor")]
MESSAGE = r"'slice_batch' must be None or an integer from 1 to 64\."


def make(chain=CHAIN, dtype=np.float32, **kw):
    return ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=dtype, **kw)


def tables(p):
    out = [p.perms, p.steps, p.leaf_sl, p.leaf_numel]
    return [np.asarray(a).tobytes() for a in out] + [None if p.stage_refs is None else p.stage_refs.tobytes()]


@pytest.mark.parametrize("mode", MODES, ids=["plain", "storage", "scaled"])
def test_none_is_the_default_and_a_batch_leaves_the_tables_alone(mode):
    a, b = make(**mode), make(slice_batch=None, **mode)
    assert tables(a) == tables(b) and a.peak_device_bytes == b.peak_device_bytes
    assert a.slice_batch is None and b.slice_batch is None
    c = make(slice_batch=5, **mode)
    assert tables(c) == tables(a) and c.arena_elems == a.arena_elems and c.ops == a.ops
    assert c.peak_device_bytes > a.peak_device_bytes


@pytest.mark.parametrize("mode", [MODES[0], MODES[2]], ids=["plain", "scaled"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_peak_device_bytes_counts_the_members(mode, B):
    for dtype in (np.float32, np.complex64):
        base, p = make(dtype=dtype, **mode), make(dtype=dtype, slice_batch=B, **mode)
        eff = min(B, bc.N_ASSIGNMENTS)
        assert p.slice_batch == eff
        item = np.dtype(dtype).itemsize
        held = item // 2 if mode else item
        n_blocks = 3  # (p, of dimension 3, is the one sliced index the result holds)
        words = 4 * (len(p.leaf_numel) + 2 * len(p.steps)) if mode else 0
        assert base.peak_device_bytes == held * (int(p.leaf_numel.sum()) + p.arena_elems) + item * p.out_numel + \
            8 * (p.leaf_sl.size + p.perms.size + 2 * p.leaf_numel.size) + words
        assert p.peak_device_bytes - base.peak_device_bytes == \
            held * p.arena_elems * (eff - 1) + item * eff * p.out_numel // n_blocks + words * (eff - 1)


def test_the_effective_batch_is_bounded_by_the_range():
    assert make(slice_batch=64).slice_batch == 12
    assert make(slice_batch=64, slice_range=(1, 11)).slice_batch == 10
    assert make(slice_batch=4, slice_range=(1, 11)).slice_batch == 4
    assert make(slice_batch=4, slice_range=(3, 5)).slice_batch == 2
    assert make(slice_batch=64, slice_range=(1, 11)).peak_device_bytes == make(slice_batch=10).peak_device_bytes


def test_a_plan_without_steps_has_a_batch_of_one_and_reserves_nothing_more():
    kw = dict(slices=("s",), dtype=np.float32)
    a = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], **kw)
    b = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], slice_batch=2, **kw)
    assert b.slice_batch == 1 and a.slice_batch is None
    assert a.peak_device_bytes == b.peak_device_bytes and tables(a) == tables(b)


def test_check_memory_sees_the_batch():
    a, b = make(), make(slice_batch=8)
    budget = (a.peak_device_bytes + b.peak_device_bytes) // 2
    assert a.peak_device_bytes < budget < b.peak_device_bytes
    ctr.check_memory(a, budget)
    with pytest.raises(RuntimeError, match="bytes of device memory"):
        ctr.check_memory(b, budget)
    ctr.check_memory(b, b.peak_device_bytes)


@pytest.mark.parametrize("bad", [0, 65, -1, 2.0, "8", True], ids=repr)
def test_values_that_are_refused(bad):
    with pytest.raises(ValueError, match=MESSAGE):
        make(slice_batch=bad)
    arrays = [np.ones(s, np.float32) for s in CHAIN.shapes()]
    with pytest.raises(ValueError, match=MESSAGE):  # (before any device use: the arrays never leave the host)
        ctr.contract(bc.PATH, CHAIN.ts, arrays, CHAIN.output, slices=bc.SLICES, slice_batch=bad)


@pytest.mark.parametrize("good", [1, 8, 64], ids=repr)
def test_values_that_are_taken(good):
    assert make(slice_batch=good).slice_batch == min(int(good), 12)


def test_projections_are_refused_by_plan():
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    kw = dict(dtype=np.float32, sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    assert ctr.plan([(0, 1)], ts, shapes, ("a", "b"), **kw).row_steps is not None
    with pytest.raises(NotImplementedError, match=r"projections are not supported with 'slice_batch'\."):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), slice_batch=4, **kw)
    with pytest.raises(ValueError, match=MESSAGE):  # (the value is checked first)
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), slice_batch=0, **kw)


def test_storage_and_scaling_are_reported_first():
    with pytest.raises(ValueError, match="'storage' must be"):
        make(storage="float8", slice_batch=0)
    with pytest.raises(ValueError, match="'scaling' must be"):
        make(storage="float16", scaling="block", slice_batch=0)
    with pytest.raises(ValueError, match="'scaling' needs 'storage'"):
        make(scaling="tensor", slice_batch=65)
    with pytest.raises(TypeError, match="with 'storage' the compute dtype"):
        make(dtype=np.float64, storage="float16", slice_batch=True)


def test_the_result_type_carries_the_new_fields():
    r = ctr.ContractionResult((), np.zeros(()), 0, 1, 0)
    assert r.slice_batch is None and r.batch_launches == 0
    assert ctr.MAX_SLICE_BATCH == 64 and "MAX_SLICE_BATCH" in ctr.__all__
