"""`accumulate="float64"` on the device (csrc/contract_accumulate.h): the sum over slice assignments in float64.

The oracle is the engine as it stands plus numpy.  Every assignment `a` of a case is run alone, `slice_range=(a, a + 1)`
and no keyword: existing behaviour, and it yields the float32 / complex64 block of that assignment with zeros elsewhere.
The blocks are folded by `tests.accumulate_cases.model` -- float64 additions in assignment order, the first block placed,
one `astype` -- and the run with the keyword must give those bytes: equal for finite and infinite elements, NaN at the
same places.  The same bytes are asked of every way of grouping the assignments (`slice_batch`, `path_kernel`), so the
runs are also equal to one another.

The case that the engine gets wrong without the keyword: blocks 2^24, 1, 1, ... (64 ones), every product and every sum
inside a block exact.  float32 returns 2^24 (2^24 + 1 ties to even, 64 times), the keyword 2^24 + 64.
"""
import ctypes as C

import numpy as np
import pytest

from tests import accumulate_cases as ac
from tests import batch_cases as bc
from tests import gather_cases as gc
from tests import hoist_cases as hc
from tests import indirect_cases as ic
from tests import mode_cases as mc
from tests import reuse_cases as rc

pytestmark = pytest.mark.gpu

WIDE = dict(accumulate="float64")
SINGLES = (np.float32, np.complex64)
SINGLE_IDS = ("float32", "complex64")
BATCHES, GROUPS = (1, 5, 64), (1, 5, 1024)


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def fill(chain, dtype, seed):
    """Signed values of mixed magnitude: the float32 running sum of a block's summands rounds, so it differs from the
    float64 one in most elements."""
    rng = np.random.RandomState(seed)
    out = []
    for shape in chain.shapes():
        a = rng.standard_normal(shape) * np.exp2(rng.randint(-3, 4, shape))
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.standard_normal(shape) * np.exp2(rng.randint(-3, 4, shape))
        out.append(a.astype(dtype))
    return out


class Net:
    """A network and a mode: the calls of one case."""

    def __init__(self, ctr, path, ts, arrays, output, slices, **mode):
        self.ctr, self.args, self.mode = ctr, (list(path), [tuple(x) for x in ts], arrays, output), dict(mode, slices=slices)
        self.shapes = [a.shape for a in arrays]
        self.dtype = np.result_type(*arrays)
        self._parts = {}

    def plan(self, **kw):
        path, ts, _, output = self.args
        return self.ctr.plan(path, ts, self.shapes, output, dtype=self.dtype, **{**self.mode, **kw})

    def run(self, **kw):
        return self.ctr.contract(*self.args, **{**self.mode, **kw})

    def parts(self, **order):
        """(where, block) of every assignment, each from a run of that assignment alone without the keyword; once."""
        key = repr(order)
        if key not in self._parts:
            p = self.plan(**order)
            out = []
            for a in range(p.n_slices):
                r = self.run(slice_range=(a, a + 1), **order)
                assert r.inds == p.inds and r.n_slices == 1
                where = ac.where_of(p, a)
                rest = r.array.copy()
                rest[where] = 0
                assert not rest.any()  # (the blocks it does not reach stay zero)
                out.append((where, r.array[where].copy()))
            self._parts[key] = (p, out)
        return self._parts[key]

    def want(self, lo=None, hi=None, **order):
        p, parts = self.parts(**order)
        return ac.model(parts[lo:hi], p.shape, self.dtype)


def chain_net(ctr, chain, dtype, seed, **mode):
    return Net(ctr, bc.PATH, chain.ts, fill(chain, dtype, seed), chain.output, bc.SLICES, **mode)


def assert_is_model(r, want, what):
    assert r.array.dtype == want.dtype and r.array.shape == want.shape, what
    assert ac.same_bytes(r.array, want), f"{what}: not the float64 sum of the assignments' blocks, rounded once"


CHAINS = bc.PLAIN + [bc.SUMMED, bc.PLACED]


@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
@pytest.mark.parametrize("chain", CHAINS, ids=[c.name for c in CHAINS])
def test_every_output_step_class_and_every_grouping_give_the_model(ctr, chain, dtype):
    net = chain_net(ctr, chain, dtype, seed=71)
    want = net.want()
    plain = net.run()
    what = f"{chain.name} {np.dtype(dtype).name}"
    base = net.run(**WIDE)
    assert_is_model(base, want, what)
    assert by_class(ctr, base) == by_class(ctr, plain) and base.macs == plain.macs
    for B in BATCHES:
        assert_is_model(net.run(slice_batch=B, **WIDE), want, f"{what} slice_batch={B}")
    for G in GROUPS:
        assert_is_model(net.run(path_kernel=G, **WIDE), want, f"{what} path_kernel={G}")
    assert_is_model(net.run(slice_range=(1, 11), **WIDE), net.want(1, 11), f"{what} slice_range=(1, 11)")
    if chain.variant == "placed":  # every block visited once: the bytes of the run without the keyword
        assert np.array_equal(ac.bits(base.array), ac.bits(plain.array)), what
    else:  # (the case has something to say: the float32 running sum rounds otherwise)
        _, parts = net.parts()
        assert ac.same_bytes(plain.array, ac.running_float32(parts, want.shape, dtype)), what
        assert not np.array_equal(ac.bits(want), ac.bits(plain.array)), what


def by_class(ctr, r):
    k = dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))
    return dict(tiled=sum(v for n, v in k.items() if n.startswith("tiled")), dot=k["dot"], stream=k["stream"])


STORAGE_MODES = [dict(storage="bfloat16"), dict(storage="float16", scaling="tensor")]


@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
@pytest.mark.parametrize("mode", STORAGE_MODES, ids=["bfloat16", "float16-scaled"])
def test_storage_mode_writes_the_output_from_the_mfma_kernel(ctr, mode, dtype):
    chain = bc.HALF[0]
    arrays = [(a / np.float32(8)).astype(a.dtype) for a in fill(chain, dtype, seed=72)]
    net = Net(ctr, bc.PATH, chain.ts, arrays, chain.output, bc.SLICES, **mode)
    want = net.want()
    r = net.run(**WIDE)
    assert_is_model(r, want, f"{mode}")
    assert by_class(ctr, r)["tiled"] == 2 * bc.N_ASSIGNMENTS and np.isfinite(want).all() and want.any()
    assert_is_model(net.run(slice_batch=5, **WIDE), want, f"{mode} slice_batch=5")
    if "scaling" in mode:  # the narrowing passes of the stored step, and the one launch that rounds the accumulator
        assert r.narrow_launches == bc.N_ASSIGNMENTS + 1 and r.exponents == net.run().exponents


@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
@pytest.mark.parametrize("compute", ["bf16x3", "matrix"])
def test_the_matrix_core_compute_modes_write_the_output(ctr, compute, dtype):
    chain = bc.PLAIN[1]  # stream-tiled: the output step is of the tiled class
    net = chain_net(ctr, chain, dtype, seed=73, compute=compute)
    want = net.want()
    r = net.run(**WIDE)
    assert_is_model(r, want, compute)
    assert (r.split_launches if compute == "bf16x3" else r.matrix_launches) == bc.N_ASSIGNMENTS
    assert_is_model(net.run(slice_batch=5, **WIDE), want, f"{compute} slice_batch=5")


@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
def test_an_output_step_with_folded_operands(ctr, dtype):
    case = ic.case("stream-7x9x11-beta", "both", np.dtype(dtype).name)
    net = Net(ctr, case.path, case.ts_inds, mc.fill(case), case.output_inds, case.slices, indirect=True)
    p = net.plan()
    assert p.steps[-1][8] == ctr.OUT and all(ic.folded_sides(p)[-1]) and p.n_slices == 6
    want = net.want()
    r = net.run(**WIDE)
    assert_is_model(r, want, "indirect")
    assert sum(r.indirect_launches) == 6 and r.batch_launches == 6 and r.narrow_launches == 1
    assert r.launches == sum(r.kernel_launches) + sum(r.indirect_launches) + r.batch_launches + r.narrow_launches
    assert_is_model(net.run(slice_batch=5, **WIDE), want, "indirect slice_batch=5")
    # the order of the folds does not depend on how the operands are read
    assert_is_model(Net(ctr, case.path, case.ts_inds, mc.fill(case), case.output_inds, case.slices).run(**WIDE), want, "direct")


def test_hoisting_alone_and_in_a_slice_batch(ctr):
    case = hc.case("kept-first-stream-7-9-11")
    net = Net(ctr, case.path, case.ts_inds, mc.fill(case), case.output_inds, case.slices, hoist=True)
    want = net.want()
    r = net.run(**WIDE)
    assert r.hoisted == (1, 0)
    assert_is_model(r, want, "hoist")
    b = net.run(slice_batch=5, **WIDE)
    assert_is_model(b, want, "hoist slice_batch=5")
    assert (r.batch_launches, b.batch_launches) == (12, 3) and r.narrow_launches == b.narrow_launches == 1
    assert r.macs == b.macs == net.run().macs


@pytest.mark.parametrize("order", rc.ORDERS[:2], ids=rc.ORDER_IDS[:2])
def test_reuse_in_the_default_and_in_a_named_order(ctr, order):
    case = rc.case("nested")
    kw = rc.order_kw(case, order)
    net = Net(ctr, case.path, case.ts_inds, mc.fill(case), case.output_inds, case.slices, reuse=True)
    want = net.want(**kw)  # the model under the same order: the blocks are folded in its assignment order
    r = net.run(**WIDE, **kw)
    assert r.reused == (2, 0) or order is not None
    assert_is_model(r, want, f"reuse {order}")
    assert r.macs == net.run(**kw).macs and r.batch_launches == 12 and r.narrow_launches == 1
    # without reuse, same order: the same bytes
    assert_is_model(Net(ctr, case.path, case.ts_inds, mc.fill(case), case.output_inds, case.slices).run(**WIDE, **kw), want,
                    f"no reuse {order}")


GROUPINGS = [dict(), dict(slice_batch=64), dict(path_kernel=1024)]
GROUPING_IDS = ["unbatched", "slice_batch=64", "path_kernel=1024"]


@pytest.mark.parametrize("grouping", GROUPINGS, ids=GROUPING_IDS)
@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
def test_sixty_four_ones_after_two_to_the_24(ctr, dtype, grouping):
    """The case the plain engine gets wrong, and the one test of this file that cannot pass without the feature.  A
    network sliced over one summed index of dimension 65, small-integer data: block 0 is 4096 x 4096 = 2^24 in every
    element, blocks 1 .. 64 are 1 x 1.  With slice_batch=64 the groups are 64 + 1, with path_kernel=1024 one group."""
    path, ts, arrays, output, slices = ac.edge_network("ones-after-2^24", dtype)
    assert arrays[0].shape[0] == 65
    unit = (1 + 1j) if np.dtype(dtype).kind == "c" else 1
    call = lambda **kw: ctr.contract(path, ts, arrays, output, slices=slices, **grouping, **kw)  # noqa: E731
    # every assignment's block is exact (existing behaviour): 2^24, then ones
    for a, v in ((0, ac.TWO24), (1, 1.0), (64, 1.0)):
        assert np.array_equal(call(slice_range=(a, a + 1)).array, np.full((ac.EDGE_I, ac.EDGE_J), v * unit, dtype))
    plain = call()
    assert np.array_equal(plain.array, np.full((ac.EDGE_I, ac.EDGE_J), ac.TWO24 * unit, dtype))  # the case bites
    wide = call(**WIDE)
    assert wide.array.dtype == np.dtype(dtype)
    assert np.array_equal(wide.array, np.full((ac.EDGE_I, ac.EDGE_J), (ac.TWO24 + 64) * unit, dtype))
    assert wide.n_slices == 65 and wide.macs == plain.macs


@pytest.mark.parametrize("grouping", GROUPINGS, ids=GROUPING_IDS)
@pytest.mark.parametrize("name", [n for n in ac.EDGES if n != "ones-after-2^24"])
def test_the_narrowing_edges_are_numpys_astype(ctr, name, grouping):
    """Ties in both directions, overflow, inf - inf, -0.0, subnormal sums: the blocks as the engine computes them one by
    one are the designed float32 terms, and the run is the model of them (tests/accumulate_cases.py on what the
    definition cannot reach: half the smallest subnormal, a -0.0 factor)."""
    for dtype in SINGLES if name in ac.COMPLEX_EDGES else SINGLES[:1]:
        path, ts, arrays, output, slices = ac.edge_network(name, dtype)
        net = Net(ctr, path, ts, arrays, output, slices)
        _, parts = net.parts()
        terms = ac.edge_terms(name)
        unit = (1 + 1j) if np.dtype(dtype).kind == "c" else 1
        for (_, block), t in zip(parts, terms):  # the device computed the terms the case is designed on
            assert ac.same_bytes(block, np.full((ac.EDGE_I, ac.EDGE_J), t * unit if np.isfinite(t) else t, dtype)), (name, block, t)
        want = net.want()
        # numpy alone, from the designed terms: the same bytes
        alone = ac.model([((), t) for t in terms], (), np.float32)
        assert ac.same_bytes(want.real.astype(np.float32), np.full(want.shape, alone, np.float32)), name
        r = net.run(**grouping, **WIDE)
        assert_is_model(r, want, f"{name} {np.dtype(dtype).name}")
        differs = not ac.same_bytes(net.run(**grouping).array, want)
        assert differs == ac.EDGES[name][1], name


REDUCE = gc.BY_NAME["reduce-base"]


@pytest.fixture(scope="module")
def reduce_case():
    arrays = gc.fill(REDUCE, np.float32)
    want, _ = gc.expected(REDUCE, np.float32, arrays)  # integers: every sum is exact in float32 and in float64
    return arrays, want


@pytest.mark.parametrize("grouping", [dict(), dict(slice_batch=5), dict(path_kernel=5)],
                         ids=["unbatched", "slice_batch=5", "path_kernel=5"])
def test_a_block_past_one_trip_of_the_fold_and_of_the_narrowing(ctr, reduce_case, grouping):
    """The chain of tests/gather_cases.py with a block of 1030 x 513 = 528 390 elements, three blocks: more than the
    2048 x 256 lanes of a launch, so the last elements of a block and of the output are reached by the grid stride
    only."""
    arrays, want = reduce_case
    assert REDUCE.block_numel > gc.TRIP
    p = REDUCE.plan(np.float32, **grouping, **WIDE)
    assert p.peak_device_bytes < gc.MEMORY_CAP
    r = ctr.contract(list(REDUCE.path), REDUCE.ts, arrays, REDUCE.out_inds, **REDUCE.keywords(), **grouping, **WIDE)
    got = r.array.transpose([r.inds.index(x) for x in REDUCE.out_inds])
    assert np.array_equal(ac.bits(got), ac.bits(want))
    assert r.narrow_launches == 1
    # what the library reserves is what the plan states (their totals differ by the padding of leaves and tables, the same
    # few hundred bytes with and without the keyword)
    base = ctr.contract(list(REDUCE.path), REDUCE.ts, arrays, REDUCE.out_inds, **REDUCE.keywords(), **grouping)
    assert r.peak_device_bytes - base.peak_device_bytes == \
        p.peak_device_bytes - REDUCE.plan(np.float32, **grouping).peak_device_bytes >= 2 * 4 * 3 * REDUCE.block_numel


@pytest.mark.parametrize("dtype", SINGLES, ids=SINGLE_IDS)
def test_the_launch_counts_the_memory_and_a_second_call(ctr, dtype):
    chain = bc.SMALL
    net = chain_net(ctr, chain, dtype, seed=74)
    n = bc.N_ASSIGNMENTS
    plain = net.run()
    for kw, groups in ((dict(), n), (dict(slice_range=(1, 11)), 10), (dict(slice_batch=5), 3), (dict(slice_batch=64), 1),
                       (dict(slice_batch=4, slice_range=(1, 11)), 3)):
        base, r, p = net.run(**kw), net.run(**kw, **WIDE), net.plan(**kw, **WIDE)
        assert r.kernel_launches == base.kernel_launches and r.macs == base.macs == p.macs, kw
        assert r.batch_launches == groups and base.batch_launches == (groups if "slice_batch" in kw else 0), kw
        assert r.narrow_launches == 1 and base.narrow_launches == 0 and r.path_launches == (0, 0), kw
        assert r.launches == sum(r.kernel_launches) + r.batch_launches + r.narrow_launches, kw
        assert r.launches == base.launches + 1 + (0 if "slice_batch" in kw else groups), kw
        assert r.peak_device_bytes - base.peak_device_bytes == p.peak_device_bytes - net.plan(**kw).peak_device_bytes > 0, kw
        assert r.slice_batch == base.slice_batch and r.n_slices == base.n_slices, kw
        again = net.run(**kw, **WIDE)
        assert np.array_equal(ac.bits(again.array), ac.bits(r.array)), kw
    for G, groups in ((5, 3), (1024, 1)):
        base, r, p = net.run(path_kernel=G), net.run(path_kernel=G, **WIDE), net.plan(path_kernel=G, **WIDE)
        assert r.path_launches == base.path_launches == (groups, groups) and r.narrow_launches == 1
        assert r.batch_launches == 0 and r.kernel_launches == (0,) * len(ctr.KERNEL_PATHS)
        assert r.launches == 2 * groups + 1 == base.launches + 1 and r.macs == plain.macs
        assert r.peak_device_bytes - base.peak_device_bytes == p.peak_device_bytes - net.plan(path_kernel=G).peak_device_bytes > 0
        assert np.array_equal(ac.bits(net.run(path_kernel=G, **WIDE).array), ac.bits(r.array))
    # the growth the plan states is the growth the library reserves
    item, out = np.dtype(dtype).itemsize, plain.array.size
    assert net.run(**WIDE).peak_device_bytes - plain.peak_device_bytes == 2 * item * out + item * out // chain.n_blocks
    assert net.run(slice_batch=5, **WIDE).peak_device_bytes - net.run(slice_batch=5).peak_device_bytes == 2 * item * out


def test_unsliced_calls_and_plans_without_steps_return_the_bytes_of_none(ctr):
    chain = bc.SMALL
    arrays = fill(chain, np.complex64, seed=75)
    plain = ctr.contract(bc.PATH, chain.ts, arrays, chain.output)
    r = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, **WIDE)
    assert np.array_equal(ac.bits(r.array), ac.bits(plain.array)) and r.launches == plain.launches + 2
    assert (r.batch_launches, r.narrow_launches) == (1, 1)
    # a path that leaves several tensors: every part unsliced
    parts = ctr.contract([(0, 1)], chain.ts, arrays, **WIDE)
    plain_parts = ctr.contract([(0, 1)], chain.ts, arrays)
    assert all(np.array_equal(ac.bits(a), ac.bits(b)) for a, b in zip(parts.array, plain_parts.array))
    # a single leaf: blocks are placed, nothing is summed, nothing is reserved or launched on top
    a = arrays[0]
    one = ctr.contract([], [chain.ts[0]], [a], slices=("u",), **WIDE)
    one_plain = ctr.contract([], [chain.ts[0]], [a], slices=("u",))
    assert np.array_equal(ac.bits(one.array), ac.bits(one_plain.array))
    assert one.launches == one_plain.launches and one.peak_device_bytes == one_plain.peak_device_bytes
    assert (one.batch_launches, one.narrow_launches) == (0, 0)


def _handle(ctr, L, p):
    from tnco_amd import _lib
    d, keep = ctr._describe(p, 0)
    h = C.c_void_p()
    _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
    del keep
    return h


def _stats(L, h):
    from tnco_amd import _lib
    stats = np.zeros(4, np.int64)
    _lib.check(L.tnco_hip_contract_stats(h, stats.ctypes.data_as(C.c_void_p)))
    return stats


def test_the_setter_refuses_by_name_and_leaves_the_handle_as_it_was(ctr):
    from tnco_amd import _lib
    L = _lib.load()
    err = lambda: L.tnco_hip_last_error().decode()  # noqa: E731
    ts, shapes = [("s", "i", "k"), ("s", "k", "j")], [(3, 2, 4), (3, 4, 5)]
    mk = lambda **kw: ctr.plan([(0, 1)], ts, shapes, ("i", "j"), slices=("s",), **kw)  # noqa: E731

    def refused(call, text):
        assert call() == _lib.EINVAL and err() == text, (err(), text)

    counts = np.full(2, -1, np.int64)
    cp = counts.ctypes.data_as(C.c_void_p)
    for d in SINGLES:
        p = mk(dtype=d)
        item = np.dtype(d).itemsize
        h = _handle(ctr, L, p)
        try:
            bytes0 = int(_stats(L, h)[2])
            for bad in (2, -1, 64):
                refused(lambda: L.tnco_hip_contract_set_accumulate(h, bad), "'mode' must be 0 (off) or 1 (float64).")
            assert int(_stats(L, h)[2]) == bytes0
            assert L.tnco_hip_contract_set_accumulate(h, 1) == _lib.OK
            assert int(_stats(L, h)[2]) == bytes0 + 2 * item * 10 + item * 10  # the accumulator and the staging block
            refused(lambda: L.tnco_hip_contract_set_accumulate(h, 2), "'mode' must be 0 (off) or 1 (float64).")
            assert int(_stats(L, h)[2]) == bytes0 + 3 * item * 10  # (still on)
            assert L.tnco_hip_contract_accumulate_launches(h, cp) == _lib.OK and counts.tolist() == [0, 0]
            refused(lambda: L.tnco_hip_contract_accumulate_launches(h, None), "null argument.")
            # a slice batch set afterwards stages in its own buffer: the staging block is released
            assert L.tnco_hip_contract_set_slice_batch(h, 2) == _lib.OK
            batched = int(_stats(L, h)[2])
            assert L.tnco_hip_contract_set_accumulate(h, 0) == _lib.OK
            assert int(_stats(L, h)[2]) == batched - 2 * item * 10
            assert L.tnco_hip_contract_set_accumulate(h, 1) == _lib.OK and int(_stats(L, h)[2]) == batched
        finally:
            L.tnco_hip_contract_destroy(h)
    refused(lambda: L.tnco_hip_contract_set_accumulate(None, 1), "null argument.")
    refused(lambda: L.tnco_hip_contract_accumulate_launches(None, cp), "null argument.")
    rows = ctr.plan([(0, 1)], [("a", "i", "k"), ("k", "j", "b")], [(2, 3, 4), (4, 5, 2)], ("a", "b"), dtype=np.float32,
                    sparse_inds=("a", "b"), projs=np.array([[0, 1], [1, 1], [1, 0]]))
    for p, text in ((mk(dtype=np.float64), "wide accumulation needs a float32 or complex64 output."),
                    (mk(dtype=np.complex128), "wide accumulation needs a float32 or complex64 output."),
                    (rows, "row axes are not supported with wide accumulation.")):
        h = _handle(ctr, L, p)
        try:
            bytes0 = int(_stats(L, h)[2])
            for mode in (0, 1):
                refused(lambda: L.tnco_hip_contract_set_accumulate(h, mode), text)
            assert int(_stats(L, h)[2]) == bytes0
        finally:
            L.tnco_hip_contract_destroy(h)


@pytest.mark.parametrize("refuse", [False, True], ids=["taken", "refused"])
def test_a_refused_call_leaves_the_run_as_it_was(ctr, refuse):
    """Through the ABI, the setter before and after the slice batch: a handle that refused a mode runs as before it, on
    or off, and the counters say what ran."""
    from tnco_amd import _lib
    L = _lib.load()
    path, ts, arrays, output, slices = ac.edge_network("ones-after-2^24", np.float32)
    p = ctr.plan(path, ts, [a.shape for a in arrays], output, slices=slices, dtype=np.float32)
    want = {0: ac.TWO24, 1: ac.TWO24 + 64}
    for on, first in ((0, False), (1, False), (1, True)):
        h = _handle(ctr, L, p)
        try:
            if on and first:
                assert L.tnco_hip_contract_set_accumulate(h, 1) == _lib.OK
            assert L.tnco_hip_contract_set_slice_batch(h, 64) == _lib.OK
            if on and not first:
                assert L.tnco_hip_contract_set_accumulate(h, 1) == _lib.OK
            if refuse:
                assert L.tnco_hip_contract_set_accumulate(h, 7) == _lib.EINVAL
            out = np.empty(p.out_numel, p.dtype)
            ptrs = (C.c_void_p * 2)(*[a.ctypes.data for a in arrays])
            _lib.check(L.tnco_hip_contract_run(h, ptrs, out.ctypes.data_as(C.c_void_p)))
            counts = np.full(2, -1, np.int64)
            assert L.tnco_hip_contract_accumulate_launches(h, counts.ctypes.data_as(C.c_void_p)) == _lib.OK
            assert counts.tolist() == [2 * on, on]
            assert np.array_equal(out, np.full(p.out_numel, want[on], np.float32))
        finally:
            L.tnco_hip_contract_destroy(h)
