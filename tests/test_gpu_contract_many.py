"""`Contractor.run_many` on the device: R leaf sets of one plan per call (csrc/contract_sets.h, ct_sets_path_kernel and
ct_sets_reduce_kernel; tnco_hip_contract_load_leaf_sets, tnco_hip_contract_run_sets).

The oracle is `c.run()` per set on the same Contractor: `array[i]` must be byte for byte its array.  Two equal wrong
answers would pass that, so a set is also held to numpy's einsum of the whole sliced sum in float64 / complex128 under
the bound of tests/test_gpu_contract_path.py,

    |got - ref| <= (c kt + 2) u (|A| |B| |C|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

with kt = K of the stored step + K of the output step + the assignments added into the element.  The leaves are those
of tests/path_cases.py, uniform in (0.5, 1.5) in both parts, a different seed per set (tests/many_cases.py); the leaves
that are not stacked are those of set 0, bound.  Every run stays under many_cases.MEMORY_CAP bytes of device memory."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as bc
from tests import many_cases as mc
from tests import path_cases as pc

pytestmark = pytest.mark.gpu

N = mc.N_ASSIGNMENTS
DTYPE_IDS = [np.dtype(d).name for d in mc.DTYPES]


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def contractor(ctr, chain, dtype, **kw):
    kw.setdefault("slices", mc.SLICES)
    kw.setdefault("path_kernel", 5)
    return ctr.Contractor(mc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, **kw)


def leaf_set(sets, stacked, i):
    """Leaf set i of a call that stacks the leaves `stacked`: those of set i, the others of set 0."""
    return [sets[i][t] if t in stacked else sets[0][t] for t in range(3)]


def oracles(c, sets, stacked):
    """c.run() per set, every leaf given (the leaves are bound no longer afterwards)."""
    return [c.run(leaf_set(sets, stacked, i)) for i in range(len(sets))]


def bind_shared(c, sets, stacked):
    c.bind({t: sets[0][t] for t in range(3) if t not in stacked})


def assert_many(c, r, want, R, group, what):
    """`r`, a run_many of R sets, against `want`, the runs of the sets one by one."""
    p = c.plan
    A = p.slice_range[1] - p.slice_range[0]
    launches = len(mc.schedule(R, *p.slice_range, group))
    got = host(r.array)
    assert r.inds == ("set",) + tuple(p.inds) and got.shape == (R,) + tuple(p.shape) and got.dtype == p.dtype, what
    assert np.isfinite(got).all(), what
    for i in range(R):
        assert np.array_equal(bits(got[i]), bits(want[i].array)), f"{what}: set {i} differs from run()"
    assert r.sets == R and r.group == min(group, R * A), what
    assert r.path_launches == (launches, launches) == (-(-R * A // r.group),) * 2 and r.launches == 2 * launches, what
    assert r.macs == sum(w.macs for w in want[:R]) == R * p.macs, what
    assert r.peak_device_bytes < mc.MEMORY_CAP, what


def assert_counters(ctr, c, r, R, group, what):
    """Nothing else was launched, and the three memory counts agree."""
    from tnco_amd import _lib
    L, h = c._handle()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    stats = np.zeros(4, np.int64)
    _lib.check(L.tnco_hip_contract_stats(h, ptr(stats)))
    assert r.peak_device_bytes == c.many_bytes(R, group=group) == int(stats[2]), what
    assert (int(stats[0]), int(stats[1])) == (r.macs, r.launches), what
    for entry, n in ((L.tnco_hip_contract_kernel_launches, len(ctr.KERNEL_PATHS)), (L.tnco_hip_contract_row_launches, 3),
                     (L.tnco_hip_contract_path_launches, 2), (L.tnco_hip_contract_batch_launches, 1),
                     (L.tnco_hip_contract_narrow_launches, 1)):
        counts = np.full(n, -1, np.int64)
        _lib.check(entry(h, ptr(counts)))
        assert not counts.any(), (what, entry)


def assert_einsum(chain, arrays, got, inds, dtype, what, kt=None):
    ref, mag = pc.einsum_reference(chain, arrays)
    got = got.transpose([inds.index(x) for x in chain.output])
    (_, _, k1), (_, _, k2) = chain.steps()
    kt = k1 + k2 + chain.summed if kt is None else kt
    u = float(np.finfo(dtype).eps) / 2
    bound = ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * u * mag
    err = np.abs(got.astype(ref.dtype) - ref)
    print(f"{what}: largest error / bound {float((err / bound).max()):.4f} (kt {kt})")
    assert got.shape == ref.shape and (err <= bound).all(), what


# ---- the kernel paths ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
@pytest.mark.parametrize("chain", pc.CASES, ids=[c.name for c in pc.CASES])
def test_every_shape_class_with_the_gathered_leaf_stacked(ctr, chain, dtype):
    R, group, stacked = 3, 5, (1,)
    sets = mc.fill_sets(chain, dtype, R, seed=81)
    what = f"{chain.name} {np.dtype(dtype).name}"
    with contractor(ctr, chain, dtype) as c:
        assert c.many_bytes(R, group=group, leaves=stacked) < mc.MEMORY_CAP
        want = oracles(c, sets, stacked)
        bind_shared(c, sets, stacked)
        r = c.run_many({1: mc.stack(sets, 1)}, group=group)
        assert isinstance(r.array, np.ndarray)
        assert_many(c, r, want, R, group, what)
        assert_counters(ctr, c, r, R, group, what)
        for i in (0, R - 1):
            assert_einsum(chain, leaf_set(sets, stacked, i), r.array[i], c.plan.inds, dtype, f"{what} set {i}")


# ---- groups that cut sets ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stacked", mc.STACKED, ids=["A", "B", "C", "ABC"])
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DTYPE_IDS)
def test_groups_that_end_inside_a_set_at_its_end_and_beyond_it(ctr, dtype, stacked):
    chain = pc.SMALL
    sets = mc.fill_sets(chain, dtype, max(mc.SETS), seed=82)
    with contractor(ctr, chain, dtype) as c:
        want = oracles(c, sets, stacked)
        assert len({bits(w.array).tobytes() for w in want}) == len(want)  # (the sets differ)
        bind_shared(c, sets, stacked)
        for R in mc.SETS:
            stacks = {t: mc.stack(sets[:R], t) for t in stacked}
            for group in mc.GROUPS:
                what = f"{np.dtype(dtype).name} stacked {stacked} R = {R} group = {group}"
                r = c.run_many(stacks, group=group)
                assert_many(c, r, want, R, group, what)
                assert_counters(ctr, c, r, R, group, what)
        r = c.run_many({t: mc.stack(sets, t) for t in stacked})  # (group=None: 1024)
        assert r.group == 5 * N and r.path_launches == (1, 1)
        for i in (0, 4):
            assert_einsum(chain, leaf_set(sets, stacked, i), r.array[i], c.plan.inds, dtype, f"stacked {stacked} set {i}")


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_three_sets_of_three_assignments_in_groups_of_two_and_four(ctr, dtype):
    """Every launch but the first starts inside a set, and both groups end inside one; the range (3, 6) holds the last
    assignment of block p = 0 and the first two of p = 1."""
    chain, R, stacked = pc.SMALL, 3, (0, 1, 2)
    sets = mc.fill_sets(chain, dtype, R, seed=90)
    with contractor(ctr, chain, dtype, slice_range=(3, 6)) as c:
        want = oracles(c, sets, stacked)
        stacks = {t: mc.stack(sets, t) for t in stacked}
        for group in (2, 4):
            what = f"{np.dtype(dtype).name} A = 3 R = 3 group = {group}"
            r = c.run_many(stacks, group=group)
            assert_many(c, r, want, R, group, what)
            assert_counters(ctr, c, r, R, group, what)
            assert r.path_launches == ((5, 5) if group == 2 else (3, 3)), what


# ---- block placement and ranges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slice_range", [None, (1, 11)], ids=["whole", "range-1-11"])
@pytest.mark.parametrize("variant", ["base", "summed", "placed"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_three_blocks_one_block_and_twelve_blocks(ctr, dtype, variant, slice_range):
    chain = bc.Chain(f"small-{variant}", bc.SMALL.sizes, bc.SMALL.classes, variant)
    R, stacked = 3, (1, 2)
    sets = mc.fill_sets(chain, dtype, R, seed=83)
    with contractor(ctr, chain, dtype, slice_range=slice_range) as c:
        p = c.plan
        assert p.out_numel // (p.out_numel // chain.n_blocks) == chain.n_blocks
        want = oracles(c, sets, stacked)
        bind_shared(c, sets, stacked)
        stacks = {t: mc.stack(sets, t) for t in stacked}
        for group in (4, 5, 1024):
            what = f"{chain.name} {np.dtype(dtype).name} {slice_range} group = {group}"
            r = c.run_many(stacks, group=group)
            assert_many(c, r, want, R, group, what)
            assert_counters(ctr, c, r, R, group, what)
        if slice_range is None:
            for i in range(R):
                assert_einsum(chain, leaf_set(sets, stacked, i), r.array[i], p.inds, dtype, f"{what} set {i}")
        elif variant == "placed":  # assignments 0 and 11 are not run: their blocks are zero in every set, the others are not
            a = r.array.transpose([0] + [1 + p.inds.index(x) for x in chain.output]).reshape(R, 12, -1)
            assert not a[:, 0].any() and not a[:, 11].any() and (a[:, 1:11] != 0).all()


def test_an_unsliced_plan(ctr):
    chain, dtype, R, group = pc.SMALL, np.complex64, 7, 3
    sets = mc.fill_sets(chain, dtype, R, seed=84)
    with contractor(ctr, chain, dtype, slices=(), path_kernel=4) as c:
        assert c.plan.path_kernel == 1 and c.plan.slice_range == (0, 1)
        want = oracles(c, sets, (0, 2))
        bind_shared(c, sets, (0, 2))
        r = c.run_many({0: mc.stack(sets, 0), 2: mc.stack(sets, 2)}, group=group)
        assert_many(c, r, want, R, group, "unsliced")
        assert_counters(ctr, c, r, R, group, "unsliced")
        assert r.path_launches == (3, 3) and r.group == 3
        _, K, J, _ = chain.sizes  # nothing is sliced: the stored step sums over k, the output step over t, u and j
        assert_einsum(chain, leaf_set(sets, (0, 2), 6), r.array[6], c.plan.inds, dtype, "unsliced set 6", kt=K + 4 * J)


# ---- sets do not leak ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_sets_do_not_leak_into_each_other(ctr, dtype):
    chain, R, stacked = pc.SMALL, 4, (1,)
    sets = mc.fill_sets(chain, dtype, R, seed=85)
    sets[2][1][...] = 0  # the stacked leaf of set 2: every product of that set is zero
    with contractor(ctr, chain, dtype) as c:
        want = oracles(c, sets, stacked)
        bind_shared(c, sets, stacked)
        stack = mc.stack(sets, 1)
        for group in (5, 13, 1024):
            r = c.run_many({1: stack}, group=group)
            assert_many(c, r, want, R, group, f"a zero set, group = {group}")
            assert not bits(r.array[2]).any() and all(r.array[i].all() for i in (0, 1, 3))
            back = c.run_many({1: stack[::-1]}, group=group)
            assert np.array_equal(bits(back.array), bits(r.array[::-1])), "the sets reversed"
            again = c.run_many({1: stack}, group=group)
            assert np.array_equal(bits(again.array), bits(r.array)), "a second identical call"


# ---- kinds of input --------------------------------------------------------------------------------------------------------

def test_numpy_and_torch_stacks_views_and_out(ctr, torch):
    chain, dtype, R = pc.SMALL, np.complex64, 3
    sets = mc.fill_sets(chain, dtype, R, seed=86)
    stacked = (1,)
    shape = chain.shapes()[1]  # (k, t, j)
    with contractor(ctr, chain, dtype) as c:
        want = oracles(c, sets, stacked)
        bind_shared(c, sets, stacked)
        stack = mc.stack(sets, 1)
        r = c.run_many({1: stack}, group=5)
        assert isinstance(r.array, np.ndarray)
        assert_many(c, r, want, R, 5, "numpy in, numpy out")
        t = on_device(torch, stack)
        r = c.run_many({1: t}, group=5)
        assert isinstance(r.array, torch.Tensor) and r.array.device.index == c.device and r.array.is_contiguous()
        assert_many(c, r, want, R, 5, "torch in, torch out")
        # views: the leaf's axes permuted, every second set of a larger stack, a stack that starts inside its storage
        permuted = on_device(torch, stack.transpose(0, 3, 2, 1)).permute(0, 3, 2, 1)
        wide = torch.zeros((2 * R,) + shape, dtype=t.dtype, device="cuda")
        wide[::2] = t
        tail = torch.zeros((R + 1,) + shape, dtype=t.dtype, device="cuda")
        tail[1:] = t
        for name, view in (("permuted", permuted), ("stepped", wide[::2]), ("offset", tail[1:])):
            assert tuple(view.shape) == stack.shape and (name == "offset" or not view.is_contiguous())
            assert (name != "offset" or view.storage_offset() > 0)
            assert_many(c, c.run_many({1: view}, group=13), want, R, 13, f"a {name} view")
        # an expanded set axis: R equal sets
        same = c.run_many({1: t[1:2].expand((R,) + shape)}, group=13)
        assert t[1:2].expand((R,) + shape).stride(0) == 0
        assert_many(c, same, [want[1]] * R, R, 13, "an expanded set axis")
        # out=, a second call into it, the other kind of out
        out = torch.full((R,) + tuple(c.plan.shape), 7, dtype=t.dtype, device="cuda")
        r = c.run_many({1: t}, group=12, out=out)
        assert r.array is out
        assert_many(c, r, want, R, 12, "out=")
        out.zero_()
        assert_many(c, c.run_many({1: stack}, group=12, out=out), want, R, 12, "numpy in, a second call into the same out")
        into = np.full((R,) + tuple(c.plan.shape), 7, dtype)
        r = c.run_many({1: t}, out=into)
        assert r.array is into
        assert_many(c, r, want, R, 1024, "torch in, numpy out")


def test_a_float32_stack_into_a_complex128_plan(ctr, torch):
    chain, R, stacked = pc.SMALL, 2, (2,)
    sets = mc.fill_sets(chain, np.complex128, R, seed=87)
    narrow = [pc.fill(chain, np.float32, 870 + i)[2] for i in range(R)]
    for i in range(R):
        sets[i][2] = narrow[i].astype(np.complex128)  # (exact)
    with contractor(ctr, chain, np.complex128) as c:
        want = oracles(c, sets, stacked)
        bind_shared(c, sets, stacked)
        for stack in (np.stack(narrow), on_device(torch, np.stack(narrow))):
            assert_many(c, c.run_many({2: stack}, group=5), want, R, 5, f"float32 -> complex128 ({type(stack).__name__})")


def test_a_bound_leaf_given_as_a_stack_stays_bound_and_untouched(ctr, torch):
    chain, dtype, R = pc.SMALL, np.float64, 3
    sets = mc.fill_sets(chain, dtype, R + 1, seed=88)
    bound = sets[R]  # the leaves that are bound: another set than any of the stack
    with contractor(ctr, chain, dtype) as c:
        want = [c.run([bound[0], sets[i][1], bound[2]]) for i in range(R)]
        c.bind(dict(enumerate(bound)))
        before = c.run()
        assert not np.array_equal(bits(before.array), bits(want[0].array))
        r = c.run_many({1: mc.stack(sets[:R], 1)}, group=5)
        assert_many(c, r, want, R, 5, "a bound leaf given as a stack")
        after = c.run()  # (leaf 1 is still bound, and holds what it held)
        assert np.array_equal(bits(after.array), bits(before.array))
        assert_many(c, c.run_many({1: on_device(torch, mc.stack(sets[:R], 1))}, group=5), want, R, 5, "the same from torch")
        assert np.array_equal(bits(c.run().array), bits(before.array))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_what_the_entry_points_refuse_and_that_the_handle_stays_as_it_was(ctr, torch):
    from tnco_amd import _lib
    L = _lib.load()
    chain, dtype, R = pc.SMALL, np.float32, 2
    sets = mc.fill_sets(chain, dtype, R, seed=89)
    stack = mc.stack(sets, 1)  # (2, 7, 2, 6): 168 elements
    t = on_device(torch, stack)
    wide = on_device(torch, stack.astype(np.float64))
    i64 = lambda *v: np.array(v, np.int64).ctypes.data_as(C.c_void_p)  # noqa: E731
    dev = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    hostp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def refused(rc_, text):
        assert rc_ == _lib.EINVAL and L.tnco_hip_last_error().decode() == text, (rc_, L.tnco_hip_last_error())

    load, run, launches = L.tnco_hip_contract_load_leaf_sets, L.tnco_hip_contract_run_sets, L.tnco_hip_contract_sets_launches
    torch.cuda.synchronize()
    with contractor(ctr, chain, dtype) as c:
        want = oracles(c, sets, (1,))
        bind_shared(c, sets, (1,))
        _, h = c._handle()
        n_out = c.plan.out_numel
        out_n = np.zeros((R, n_out), dtype)
        out_t = torch.zeros(R * n_out, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        stats0, counts = np.zeros(4, np.int64), np.full(2, -1, np.int64)
        assert L.tnco_hip_contract_stats(h, hostp(stats0)) == _lib.OK
        refused(launches(None, hostp(counts)), "null argument.")
        refused(launches(h, None), "null argument.")
        good = (1, 0, 1, i64(168), None)  # where, src_dtype, ndim, dims, strides of the stack on the device
        refused(load(None, 1, R, dev(t), *good), "null argument.")
        refused(load(h, 1, R, None, *good), "null argument.")
        refused(load(h, -1, R, dev(t), *good), "'leaf' is not a leaf of the plan.")
        refused(load(h, 3, R, dev(t), *good), "'leaf' is not a leaf of the plan.")
        refused(load(h, 1, 0, dev(t), *good), "'n_sets' must be at least 1.")
        refused(load(h, 1, -2, dev(t), *good), "'n_sets' must be at least 1.")
        refused(load(h, 1, 1 << 60, dev(t), *good), "'n_sets' is too large.")
        refused(load(h, 1, R, dev(t), 2, 0, 1, i64(168), None), "'where' must be 0 (host) or 1 (device).")
        refused(load(h, 1, R, dev(t), 1, 0, 33, i64(*([1] * 32), 168), None), "'ndim' must be from 0 to 32.")
        refused(load(h, 1, R, dev(t), 1, 0, -1, i64(168), None), "'ndim' must be from 0 to 32.")
        refused(load(h, 1, R, dev(t), 1, 0, 1, None, None), "null argument.")
        refused(load(h, 1, R, dev(t), 1, 0, 2, i64(0, 168), None), "dims must be positive.")
        refused(load(h, 1, R, dev(t), 1, 0, 2, i64(2, 84), i64(84, -1)), "a stride is negative.")
        refused(load(h, 1, R, dev(t), 1, 0, 1, i64(84), None), "dims do not multiply to the sets' elements.")
        refused(load(h, 1, R, dev(t), 1, 0, 2, i64(3, 84), None), "dims do not multiply to the sets' elements.")
        refused(load(h, 1, R, dev(t), 1, 0, 0, None, None), "dims do not multiply to the sets' elements.")
        refused(load(h, 1, R, hostp(stack), 0, 1, 1, i64(168), None), "a host stack must have the plan's dtype.")
        refused(load(h, 1, R, hostp(stack), 0, 0, 1, i64(168), i64(1)), "a host stack must be C-contiguous: 'strides' must be NULL.")
        for code in (1, 2, 3, 4, 7, -1, 8):  # (a narrowing, a storage code, no code at all)
            refused(load(h, 1, R, dev(wide), 1, code, 1, i64(168), None), "'src_dtype' does not widen to the plan's dtype.")
        dst = (1, 1, i64(R * n_out), i64(1))  # where, ndim, dims, dst_strides of a contiguous result on the device
        refused(run(None, R, 5, dev(out_t), *dst), "null argument.")
        refused(run(h, R, 5, None, *dst), "null argument.")
        refused(run(h, 0, 5, dev(out_t), *dst), "'n_sets' must be at least 1.")
        refused(run(h, 1 << 60, 5, dev(out_t), *dst), "'n_sets' is too large.")
        for group in (0, 1025, -1):
            refused(run(h, R, group, dev(out_t), *dst), "'group' must be from 1 to 1024.")
        refused(run(h, R, 5, dev(out_t), 2, 1, i64(R * n_out), i64(1)), "'where' must be 0 (host) or 1 (device).")
        refused(run(h, R, 5, dev(out_t), 1, 1, i64(R * n_out), None), "null argument.")
        refused(run(h, R, 5, dev(out_t), 1, 33, i64(*([1] * 32), R * n_out), i64(*([1] * 33))), "'ndim' must be from 0 to 32.")
        refused(run(h, R, 5, dev(out_t), 1, 2, i64(R, 0), i64(n_out, 1)), "dims must be positive.")
        refused(run(h, R, 5, dev(out_t), 1, 2, i64(R + 1, n_out), i64(n_out, 1)), "dims do not multiply to the sets' outputs.")
        refused(run(h, R, 5, dev(out_t), 1, 1, i64(n_out), i64(1)), "dims do not multiply to the sets' outputs.")
        refused(run(h, R, 5, dev(out_t), 1, 2, i64(R, n_out), i64(n_out, -1)), "a stride is negative.")
        refused(run(h, R, 5, dev(out_t), 1, 2, i64(R, n_out), i64(0, 1)), "a destination stride is 0.")
        # nothing ran, nothing was reserved, nothing was counted
        stats = np.zeros(4, np.int64)
        assert L.tnco_hip_contract_stats(h, hostp(stats)) == _lib.OK and tuple(stats[:3]) == tuple(stats0[:3])
        assert not out_t.any() and not out_n.any()
        # a stack of another number of sets names its leaf; the handle is as it was: the same stack runs with its own number
        assert load(h, 1, R, dev(t), *good) == _lib.OK
        refused(run(h, R + 1, 5, hostp(out_n), 0, 0, None, None), "leaf 1 has a stack of 2 sets loaded, not of 3.")
        assert run(h, R, 5, dev(out_t), *dst) == _lib.OK
        assert launches(h, hostp(counts)) == _lib.OK and tuple(counts) == (5, 5)
        got = host(out_t).reshape(R, n_out)
        # (a run reads the stacks once: the next one needs them again, here from the host)
        assert load(h, 1, R, hostp(stack), 0, 0, 1, i64(168), None) == _lib.OK
        assert run(h, R, 1024, hostp(out_n), 0, 0, None, None) == _lib.OK
        assert launches(h, hostp(counts)) == _lib.OK and tuple(counts) == (1, 1)
        assert np.array_equal(bits(got), bits(out_n))
        r = c.run_many({1: stack}, group=5)
        assert_many(c, r, want, R, 5, "after the refusals")
        # (where 0 gives the raw output buffers, [block axes][the others] per set, as run_loaded does for one)
        assert np.array_equal(bits(np.stack([ctr._host_layout(c.plan, out_n[i]) for i in range(R)])), bits(r.array))
        # after a run of another kind the counts of this one are zeros
        assert np.array_equal(bits(c.run(leaf_set(sets, (1,), 0)).array), bits(want[0].array))
        assert launches(h, hostp(counts)) == _lib.OK and tuple(counts) == (0, 0)
    # a leaf that was never loaded
    with contractor(ctr, chain, dtype) as c:
        _, h = c._handle()
        assert load(h, 1, R, dev(t), *good) == _lib.OK
        refused(run(h, R, 5, hostp(out_n), 0, 0, None, None), "leaf 0 was never loaded.")
    # handles that do not take leaf sets
    kinds = ((dict(path_kernel=None), "leaf sets need a path kernel: call tnco_hip_contract_set_path_kernel first."),
             (dict(accumulate="float64"), "leaf sets are not supported with wide accumulation."))
    for kw, text in kinds:
        with contractor(ctr, chain, dtype, **kw) as c:
            _, h = c._handle()
            refused(load(h, 1, R, dev(t), *good), text)
            refused(run(h, R, 5, hostp(out_n), 0, 0, None, None), text)
            assert np.array_equal(bits(c.run(sets[0]).array), bits(ctr.contract(mc.PATH, chain.ts, sets[0], chain.output,
                                                                               slices=mc.SLICES, **kw).array)), kw
    with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=dtype, slices=("s",), path_kernel=2) as c:
        _, h = c._handle()
        leaf = np.ones((5, 3, 7), dtype)
        refused(load(h, 0, 1, hostp(leaf), 0, 0, 1, i64(105), None), "leaf sets need a plan with steps.")
        refused(run(h, 1, 1, hostp(out_n), 0, 0, None, None), "leaf sets need a plan with steps.")
        assert c.run([leaf]).array.all()
    ts, shapes = [("a", "k"), ("k", "b")], [(3, 4), (4, 5)]
    with ctr.Contractor([(0, 1)], ts, shapes, ("a", "b"), dtype=dtype, sparse_inds=("a", "b"), projs=np.array([[0, 1], [2, 4]])) as c:
        _, h = c._handle()
        leaf = np.ones((2, 3, 4), dtype)
        refused(load(h, 0, 2, hostp(leaf), 0, 0, 1, i64(24), None), "leaf sets are not supported with row axes.")
        refused(run(h, 2, 1, hostp(out_n), 0, 0, None, None), "leaf sets are not supported with row axes.")
