"""`path_kernel=` on the host side of the contraction engine (tnco_amd/contraction.py): the plan is that of the unfused
run, the memory the path kernel reserves is counted term by term, and the keyword is validated, in a fixed order, before
anything else happens.  No GPU."""
import numpy as np
import pytest

from tests import path_cases as pc
from tnco_amd import contraction as ctr

CHAIN = pc.CASES[0]
MESSAGE = r"'path_kernel' must be None or an integer from 1 to 1024\."
EXCLUSIVE = r"'path_kernel' and 'slice_batch' are exclusive\."
SQUARE = [("i", "k"), ("k", "j")]


def make(chain=CHAIN, dtype=np.float32, **kw):
    return ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES, dtype=dtype, **kw)


def tables(p):
    return [np.asarray(a).tobytes() for a in (p.perms, p.steps, p.leaf_sl, p.leaf_numel)]


@pytest.mark.parametrize("chain", pc.CASES, ids=[c.name for c in pc.CASES])
def test_none_is_the_default_and_a_group_leaves_the_tables_alone(chain):
    a, b = make(chain), make(chain, path_kernel=None)
    assert tables(a) == tables(b) and a.peak_device_bytes == b.peak_device_bytes
    assert a.path_kernel is None and b.path_kernel is None
    c = make(chain, path_kernel=5)
    assert tables(c) == tables(a) and c.arena_elems == a.arena_elems and c.ops == a.ops
    assert c.macs == a.macs and c.inds == a.inds and c.shape == a.shape and c.slice_batch is None
    assert c.peak_device_bytes > a.peak_device_bytes


@pytest.mark.parametrize("G", [1, 5, 64, 1024])
def test_peak_device_bytes_counts_the_members_and_the_new_tables(G):
    for dtype in pc.DTYPES:
        base, p = make(dtype=dtype), make(dtype=dtype, path_kernel=G)
        eff = min(G, pc.N_ASSIGNMENTS)
        assert p.path_kernel == eff
        item = np.dtype(dtype).itemsize
        n_blocks = 3  # (p, of dimension 3, is the one sliced index the result holds)
        n_steps = len(p.steps)
        assert n_steps == 2 and p.steps.size == 2 * ctr.STEP_W
        assert base.peak_device_bytes == item * (int(p.leaf_numel.sum()) + p.arena_elems) + item * p.out_numel + \
            8 * (p.leaf_sl.size + p.perms.size + 2 * p.leaf_numel.size)
        arenas = item * p.arena_elems * (eff - 1)
        staging = item * eff * p.out_numel // n_blocks
        steps_table = 8 * n_steps * ctr.STEP_W
        permute_groups = 8 * 2 * (n_steps + 1)  # (first row and count of group -1 and of the group of every step)
        placement = 8 * pc.N_ASSIGNMENTS  # (a word per assignment of the range: block offset and beta bit)
        assert p.peak_device_bytes - base.peak_device_bytes == arenas + staging + steps_table + permute_groups + placement


def test_the_placement_table_follows_the_range():
    a, b = make(path_kernel=4, slice_range=(1, 11)), make(path_kernel=4)
    assert b.peak_device_bytes - a.peak_device_bytes == 8 * 2


def test_the_effective_group_is_bounded_by_the_range():
    assert make(path_kernel=1024).path_kernel == 12
    assert make(path_kernel=1024, slice_range=(1, 11)).path_kernel == 10
    assert make(path_kernel=4, slice_range=(1, 11)).path_kernel == 4
    assert make(path_kernel=4, slice_range=(3, 5)).path_kernel == 2
    assert make(path_kernel=1024, slice_range=(1, 11)).peak_device_bytes == make(path_kernel=10, slice_range=(1, 11)).peak_device_bytes


def test_a_plan_without_steps_has_a_group_of_one_and_reserves_nothing_more():
    kw = dict(slices=("s",), dtype=np.float32)
    a = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], **kw)
    b = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], path_kernel=2, **kw)
    assert b.path_kernel == 1 and a.path_kernel is None
    assert a.peak_device_bytes == b.peak_device_bytes and tables(a) == tables(b)


def test_check_memory_sees_the_group():
    a, b = make(), make(path_kernel=8)
    budget = (a.peak_device_bytes + b.peak_device_bytes) // 2
    assert a.peak_device_bytes < budget < b.peak_device_bytes
    ctr.check_memory(a, budget)
    with pytest.raises(RuntimeError, match="bytes of device memory"):
        ctr.check_memory(b, budget)
    ctr.check_memory(b, b.peak_device_bytes)


@pytest.mark.parametrize("bad", [0, 1025, -1, 2.0, "8", True, False], ids=repr)
def test_values_that_are_refused(bad):
    with pytest.raises(ValueError, match=MESSAGE):
        make(path_kernel=bad)
    arrays = [np.ones(s, np.float32) for s in CHAIN.shapes()]
    with pytest.raises(ValueError, match=MESSAGE):  # (before any device use: the arrays never leave the host)
        ctr.contract(pc.PATH, CHAIN.ts, arrays, CHAIN.output, slices=pc.SLICES, path_kernel=bad)


@pytest.mark.parametrize("good", [1, 8, 1024], ids=repr)
def test_values_that_are_taken(good):
    assert make(path_kernel=good).path_kernel == min(int(good), 12)


def test_slice_batch_is_exclusive_and_comes_after_the_value():
    with pytest.raises(ValueError, match=EXCLUSIVE):
        make(path_kernel=4, slice_batch=4)
    with pytest.raises(ValueError, match=MESSAGE):  # (1: the value)
        make(path_kernel=0, slice_batch=4)
    with pytest.raises(ValueError, match=EXCLUSIVE):  # (2 before 3)
        make(path_kernel=4, slice_batch=4, compute="bf16x3")
    with pytest.raises(ValueError, match=EXCLUSIVE):
        make(path_kernel=4, slice_batch=4, storage="bfloat16")


@pytest.mark.parametrize("kw,name", [(dict(storage="bfloat16"), "storage"), (dict(storage="float16", scaling="tensor"), "storage"),
                                     (dict(compute="bf16x3"), "compute")], ids=["storage", "scaled", "compute"])
def test_storage_and_compute_are_not_implemented(kw, name):
    with pytest.raises(NotImplementedError, match=f"'{name}' is not supported with 'path_kernel'"):
        make(path_kernel=4, **kw)
    with pytest.raises(ValueError, match=MESSAGE):  # (1 before 3)
        make(path_kernel=1025, **kw)
    arrays = [np.ones(s, np.float32) for s in CHAIN.shapes()]
    with pytest.raises(NotImplementedError, match=f"'{name}' is not supported with 'path_kernel'"):
        ctr.contract(pc.PATH, CHAIN.ts, arrays, CHAIN.output, slices=pc.SLICES, path_kernel=4, **kw)


def test_projections_are_not_implemented():
    ts, shapes = [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)]
    kw = dict(dtype=np.float32, sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1]]))
    assert ctr.plan([(0, 1)], ts, shapes, ("a", "b"), **kw).row_steps is not None
    with pytest.raises(NotImplementedError, match=r"projections are not supported with 'path_kernel'\."):
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), path_kernel=4, **kw)
    with pytest.raises(ValueError, match=MESSAGE):  # (1 before 3)
        ctr.plan([(0, 1)], ts, shapes, ("a", "b"), path_kernel=0, **kw)


def test_the_existing_refusals_come_first_with_their_messages():
    with pytest.raises(ValueError, match="'storage' must be"):
        make(storage="float8", path_kernel=0)
    with pytest.raises(ValueError, match="'scaling' needs 'storage'"):
        make(scaling="tensor", path_kernel=0)
    with pytest.raises(ValueError, match=r"'slice_batch' must be None or an integer from 1 to 64\."):
        make(slice_batch=65, path_kernel=4)
    with pytest.raises(ValueError, match="'compute' and 'storage' are exclusive"):
        make(compute="bf16x3", storage="bfloat16", path_kernel=4)


def test_a_step_of_exactly_two_to_the_24_is_taken_and_one_more_row_is_refused():
    assert ctr.MAX_PATH_STEP_MACS == 1 << 24
    edge = ctr.plan([(0, 1)], SQUARE, [(256, 256), (256, 256)], dtype=np.float32, path_kernel=1)
    assert edge.macs == 1 << 24 and edge.path_kernel == 1
    assert (edge.ops[0]["M"], edge.ops[0]["N"], edge.ops[0]["K"]) == (256, 256, 256)
    with pytest.raises(ValueError, match=r"step 0 \(H M N K = 1 x 257 x 256 x 256\) has more than 2\^24 multiply-adds"):
        ctr.plan([(0, 1)], SQUARE, [(257, 256), (256, 256)], dtype=np.float32, path_kernel=1)
    assert ctr.plan([(0, 1)], SQUARE, [(257, 256), (256, 256)], dtype=np.float32).macs == 257 << 16  # (fine without the keyword)


def test_the_message_names_the_step_and_the_cap_comes_last():
    ts, shapes = [("i", "k"), ("k", "j"), ("j", "l")], [(4, 4), (4, 4096), (4096, 4097)]
    with pytest.raises(ValueError, match=r"step 1 \(H M N K = 1 x 4097 x 4 x 4096\)"):  # (the later tensor is the first operand)
        ctr.plan([(0, 1), (0, 1)], ts, shapes, dtype=np.float64, path_kernel=8)
    with pytest.raises(ValueError, match=EXCLUSIVE):  # (2 before 4)
        ctr.plan([(0, 1), (0, 1)], ts, shapes, dtype=np.float64, path_kernel=8, slice_batch=2)
    with pytest.raises(NotImplementedError, match="'compute' is not supported"):  # (3 before 4)
        ctr.plan([(0, 1), (0, 1)], ts, shapes, dtype=np.float32, path_kernel=8, compute="bf16x3")


def test_the_result_type_carries_the_new_fields():
    r = ctr.ContractionResult((), np.zeros(()), 0, 1, 0)
    assert r.path_kernel is None and r.path_launches == (0, 0)
    assert ctr.MAX_PATH_KERNEL == 1024 and "MAX_PATH_KERNEL" in ctr.__all__ and "MAX_PATH_STEP_MACS" in ctr.__all__
