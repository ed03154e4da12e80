"""`Contractor.run_many` without a GPU: what it refuses, with which type and words and in which order, before the device is
touched (`_lib.load` is made to raise); `many_bytes` term by term; the launch schedule of tests/many_cases.py against
brute-force enumeration; the fields of `ManyResult`, and that `ContractionResult` and `Plan` kept theirs."""
import dataclasses

import numpy as np
import pytest

from tests import many_cases as mc
from tests import path_cases as pc

CHAIN = pc.SMALL
ARGS = (mc.PATH, CHAIN.ts, CHAIN.shapes(), CHAIN.output)


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


def contractor(ctr, **kw):
    kw.setdefault("dtype", np.float32)
    kw.setdefault("slices", mc.SLICES)
    kw.setdefault("path_kernel", 5)
    return ctr.Contractor(*ARGS, **kw)


def refusal(call, error, text):
    with pytest.raises(error) as e:
        call()
    assert type(e.value) is error and str(e.value) == text, (type(e.value), str(e.value))


def stacks(R=2, dtype=np.float32, leaves=(0, 1, 2)):
    sets = mc.fill_sets(CHAIN, dtype, R, seed=5)
    return {t: mc.stack(sets, t) for t in leaves}


# the texts, in the order of the refusals
CLOSED = "the Contractor is closed."
NO_PATH = "'run_many' needs a Contractor with 'path_kernel'."
WIDE = "'accumulate' is not supported with 'run_many'."
NO_STEPS = "'run_many' needs a plan with steps."
GROUP = "'group' must be None or an integer from 1 to 1024."
STACKS = "'stacks' must be a dict {leaf number: array} with at least one leaf."
KINDS = "the arrays of one run must be all numpy arrays or all torch tensors."
MISSING = "leaf 0 is neither bound nor given."


def test_every_refusal_with_its_type_and_text(ctr, no_gpu):
    import torch
    s = stacks()
    c = contractor(ctr)
    c.close()
    refusal(lambda: c.run_many(s), ValueError, CLOSED)
    refusal(lambda: c.many_bytes(2), ValueError, CLOSED)
    for kw in (dict(path_kernel=None), dict(path_kernel=None, slice_batch=5), dict(path_kernel=None, hoist=True),
               dict(path_kernel=None, reuse=True), dict(path_kernel=None, indirect=True), dict(path_kernel=None, storage="float16"),
               dict(path_kernel=None, compute="matrix")):
        with contractor(ctr, **kw) as c:
            refusal(lambda: c.run_many(s), NotImplementedError, NO_PATH)
            refusal(lambda: c.many_bytes(2), NotImplementedError, NO_PATH)
    with contractor(ctr, accumulate="float64") as c:
        refusal(lambda: c.run_many(s), NotImplementedError, WIDE)
    with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), path_kernel=2) as c:
        refusal(lambda: c.run_many({0: np.zeros((2, 5, 3, 7), np.float32)}), NotImplementedError, NO_STEPS)
    with contractor(ctr) as c:
        for bad in (0, 1025, -1, 2.0, "8", True):
            refusal(lambda: c.run_many(s, group=bad), ValueError, GROUP)
            refusal(lambda: c.many_bytes(2, group=bad), ValueError, GROUP)
        for bad in ([s[0], s[1], s[2]], {}, None, s[0]):
            refusal(lambda: c.run_many(bad), ValueError, STACKS)
        refusal(lambda: c.run_many({3: s[0]}), ValueError, "3 is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.run_many({"0": s[0]}), ValueError, "'0' is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.run_many({True: s[0]}), ValueError, "True is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.run_many({0: s[0], 1: torch.from_numpy(s[1])}), TypeError, KINDS)
        refusal(lambda: c.run_many({0: np.float32(1)}), ValueError, "the stack of leaf 0 has no set axis.")
        refusal(lambda: c.run_many({1: s[1][0]}), ValueError,
                "the stack of leaf 1 has the shape (2, 6) after its set axis, not the leaf's (7, 2, 6).")
        refusal(lambda: c.run_many({1: s[1][:, :, :1]}), ValueError,
                "the stack of leaf 1 has the shape (7, 1, 6) after its set axis, not the leaf's (7, 2, 6).")
        refusal(lambda: c.run_many({1: s[1][:0]}), ValueError, "the stack of leaf 1 holds no set.")
        refusal(lambda: c.run_many({0: s[0], 2: np.concatenate([s[2], s[2]])}), ValueError,
                "the stack of leaf 2 holds 4 sets, the first stack 2.")
        refusal(lambda: c.run_many({0: s[0].astype(np.float64)}), TypeError,
                "an array of dtype float64 does not cast safely to float32.")
        refusal(lambda: c.run_many({0: torch.from_numpy(s[0].astype(np.float64))}), TypeError,
                "a tensor of dtype torch.float64 does not widen exactly to float32.")
        refusal(lambda: c.run_many({0: torch.from_numpy(s[0])}), ValueError, "a tensor is on cpu, not on cuda:0.")
        refusal(lambda: c.run_many({0: torch.from_numpy(s[0].astype(np.complex64)).conj()}), TypeError,
                "a tensor of dtype torch.complex64 does not widen exactly to float32.")
        refusal(lambda: c.run_many({1: s[1], 2: s[2]}), ValueError, MISSING)
        c._bound = {0, 1, 2}  # (as after bind: the checks of `out` come last)
        shape = (2,) + tuple(c.plan.shape)
        refusal(lambda: c.run_many({1: s[1]}, out=np.zeros(shape, np.float64)), TypeError,
                "'out' must be of dtype float32, not float64.")
        for bad in (np.zeros(shape[1:], np.float32), np.zeros((3,) + shape[1:], np.float32), np.zeros(shape[::-1], np.float32).T):
            refusal(lambda: c.run_many({1: s[1]}, out=bad), ValueError, f"'out' must be C-contiguous and of shape {shape}.")
        refusal(lambda: c.run_many({1: s[1]}, out=[0.0]), TypeError, "'out' must be a numpy array or a torch tensor.")
        refusal(lambda: c.run_many({1: s[1]}, out=torch.zeros(shape)), ValueError, "'out' is on cpu, not on cuda:0.")


def test_a_lazily_conjugated_stack_is_refused(ctr, no_gpu):
    import torch
    s = stacks(dtype=np.complex64)
    with contractor(ctr, dtype=np.complex64) as c:
        t = torch.from_numpy(s[0])
        refusal(lambda: c.run_many({0: t.conj()}), ValueError, "a tensor is lazily conjugated (is_conj()): pass tensor.resolve_conj().")
        refusal(lambda: c.run_many({0: torch._neg_view(t)}), ValueError, "a tensor is lazily negated (is_neg()): pass tensor.resolve_neg().")


def test_the_order_of_the_refusals(ctr, no_gpu):
    """Each call breaks rule k and every later rule too: the text is rule k's."""
    import torch
    s = stacks()
    bad_out = np.zeros(3, np.float64)
    c = ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), accumulate="float64")
    every = dict(stacks=[], group=0, out=bad_out)
    c.close()
    refusal(lambda: c.run_many(**every), ValueError, CLOSED)
    with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), accumulate="float64") as c:
        refusal(lambda: c.run_many(**every), NotImplementedError, NO_PATH)
    with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), accumulate="float64", path_kernel=2) as c:
        refusal(lambda: c.run_many(**every), NotImplementedError, WIDE)
    with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), path_kernel=2) as c:
        refusal(lambda: c.run_many(**every), NotImplementedError, NO_STEPS)
    with contractor(ctr) as c:
        refusal(lambda: c.run_many(**every), ValueError, GROUP)
        refusal(lambda: c.run_many([], out=bad_out), ValueError, STACKS)
        refusal(lambda: c.run_many({7: s[0][0], 1: torch.from_numpy(s[1])}, out=bad_out), ValueError,
                "7 is not a leaf of the plan (0 to 2).")
        mixed = {1: s[1][0].astype(np.float64), 2: torch.from_numpy(s[2])}
        refusal(lambda: c.run_many(mixed, out=bad_out), TypeError, KINDS)
        refusal(lambda: c.run_many({1: s[1][0].astype(np.float64)}, out=bad_out), ValueError,
                "the stack of leaf 1 has the shape (2, 6) after its set axis, not the leaf's (7, 2, 6).")
        # (every shape before any dtype)
        refusal(lambda: c.run_many({1: s[1].astype(np.float64), 2: s[2][:, :1]}, out=bad_out), ValueError,
                "the stack of leaf 2 has the shape (1, 2, 6, 3) after its set axis, not the leaf's (2, 2, 6, 3).")
        refusal(lambda: c.run_many({1: s[1].astype(np.float64)}, out=bad_out), TypeError,
                "an array of dtype float64 does not cast safely to float32.")
        refusal(lambda: c.run_many({1: s[1]}, out=bad_out), ValueError, MISSING)


# ---- many_bytes ----------------------------------------------------------------------------------------------------------

def restated(p, R, group, leaves):
    """The terms of many_bytes, from the plan's numbers alone."""
    item, A = p.dtype.itemsize, p.slice_range[1] - p.slice_range[0]
    n_blocks = 1
    for x in p.block_inds:
        n_blocks *= p.shape[p.inds.index(x)]
    block = p.out_numel // n_blocks
    pad = lambda n: (int(n) + 63) // 64 * 64  # noqa: E731
    L, S = len(p.leaf_numel), len(p.steps)
    G = p.path_kernel
    handle = dict(leaves=item * sum(pad(n) for n in p.leaf_numel), arenas=item * G * p.arena_elems, staging=item * G * block,
                  output=item * p.out_numel, plan_tables=8 * (p.perms.size + p.leaf_sl.size + 2 * len(p.slice_dims)),
                  leaf_pointers=8 * L, path_tables=8 * (S * 16 + 2 * (S + 1) + A))
    members = min(group, R * A)
    call = dict(stacks=item * R * sum(int(p.leaf_numel[t]) for t in leaves),
                more_members=item * max(members - G, 0) * (p.arena_elems + block),
                outputs=item * R * p.out_numel, tables=16 * L)
    return handle, call


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
@pytest.mark.parametrize("R", [1, 5])
def test_many_bytes_term_by_term(ctr, no_gpu, R, dtype):
    for kw, groups in ((dict(path_kernel=5), (1, 3, 5, 6, 13, 1024, None)), (dict(path_kernel=1024), (5, 12, 13, 1024)),
                       (dict(path_kernel=5, slice_range=(1, 11)), (4, 11)), (dict(path_kernel=4, slices=()), (1, 3, 1024))):
        with contractor(ctr, dtype=dtype, **kw) as c:
            p = c.plan
            assert p.path_kernel == min(kw["path_kernel"], p.slice_range[1] - p.slice_range[0])
            for group in groups:
                for leaves in ((), (1,), (0, 2), (0, 1, 2)):
                    handle, call = restated(p, R, 1024 if group is None else group, leaves)
                    got = c.many_bytes(R, group=group, leaves=leaves)
                    assert got == sum(handle.values()) + sum(call.values()), (kw, group, leaves, handle, call)
            assert c.many_bytes(R) == c.many_bytes(R, group=1024, leaves=())  # (nothing was stacked yet)
            # beyond Plan.path_kernel every member costs an arena and a staging block; below it nothing
            G, A = p.path_kernel, p.slice_range[1] - p.slice_range[0]
            per_member = restated(p, 1, 1, ())[0]["arenas"] // G + restated(p, 1, 1, ())[0]["staging"] // G
            below, at = c.many_bytes(R, group=1), c.many_bytes(R, group=G)
            assert below == at
            if R * A > G:
                assert c.many_bytes(R, group=G + 1) - at == per_member > 0
            assert c.many_bytes(R, group=1024) == c.many_bytes(R, group=max(G, min(1024, R * A)))


def test_many_bytes_grows_with_the_sets(ctr, no_gpu):
    with contractor(ctr) as c:
        p = c.plan
        a, b = c.many_bytes(1, group=1, leaves=(1,)), c.many_bytes(2, group=1, leaves=(1,))
        assert b - a == 4 * (int(p.leaf_numel[1]) + p.out_numel)
        for bad in (0, -1, 1.0, True, "2"):
            refusal(lambda: c.many_bytes(bad), ValueError, "'n_sets' must be a positive integer.")
        refusal(lambda: c.many_bytes(1, leaves=(3,)), ValueError, "3 is not a leaf of the plan (0 to 2).")


# ---- the schedule --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lo, hi", [(0, 12), (1, 11), (0, 1), (3, 4)])
def test_the_schedule_against_enumeration(lo, hi):
    A = hi - lo
    for R in (1, 2, 5, 7):
        pairs = [(i, a) for i in range(R) for a in range(lo, hi)]  # set-major
        for group in (1, 2, 3, 5, 12, 13, 24, 1024):
            launches = mc.schedule(R, lo, hi, group)
            assert len(launches) == -(-R * A // min(group, R * A))
            seen = []
            for m0, n in launches:
                assert 1 <= n <= min(group, R * A)
                seen += [mc.member(m, lo, hi) for m in range(m0, m0 + n)]
            assert seen == pairs, (R, group)
            assert all(n == min(group, R * A) for _, n in launches[:-1])


def test_the_groups_of_the_grid_cut_the_sets_where_the_tests_say(ctr):
    ends = {g: [(m0 + n) % 12 for m0, n in mc.schedule(5, 0, 12, g)] for g in mc.GROUPS}
    assert 5 in ends[5] and set(ends[12]) == {0} and ends[13][0] == 1 and ends[1024] == [0]
    assert len(mc.schedule(5, 0, 12, 1)) == 60


# ---- the records ---------------------------------------------------------------------------------------------------------

def test_the_fields_of_the_results(ctr):
    names = lambda cls: [f.name for f in dataclasses.fields(cls)]  # noqa: E731
    assert names(ctr.ManyResult) == ["inds", "array", "sets", "group", "macs", "launches", "path_launches",
                                     "peak_device_bytes", "device_s"]
    assert names(ctr.ContractionResult) == [
        "inds", "array", "macs", "n_slices", "peak_device_bytes", "launches", "device_s", "fuse_macs", "kernel_launches",
        "row_kernel_launches", "scaling", "exponents", "narrow_launches", "slice_batch", "batch_launches", "compute",
        "split_launches", "path_kernel", "path_launches", "hoisted", "reused", "indirect", "indirect_launches", "matrix_launches"]
    assert names(ctr.Plan)[-1] == "accumulate" and len(names(ctr.Plan)) == 39
    r = ctr.ManyResult(("set", "i"), np.zeros((2, 3)), 2, 5, 10, 4, (2, 2), 100)
    assert r.device_s == 0.0
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.sets = 3
    assert "ManyResult" in ctr.__all__ and ctr.MAX_PATH_KERNEL == 1024
