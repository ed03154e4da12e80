"""The refusals of the optimizer's constructor that need the device (the others: tests/test_tree_check_model.py).

* `tree_check_kernel` against the model of tests/tree_check_cases.py, tree for tree, through
  `tnco_hip_diag_tree_check(where=1)`: the 4^9 link arrays of three nodes in one launch, the named damages at every size
  (127 -> 129 nodes: one more trip of its lane loop, 4095: 64 trips), the random families.  Codes 1-6 as the host check;
  a tree of code 7 (not reachable from the root) gets 0 -- the one documented difference: the kernel follows no link
  chain.  The diagnostic runs that kernel alone.
* `create()` from links in device memory: trees the device greedy left there, damaged through
  `tnco_hip_copy_to_device`, refused with the message of the lowest damaged replica; put back, they build the batch that
  the same trees build as a host array.
  NOTHING here writes a tree that the kernel accepts and that is not a tree (code 7, the ring) into links that go to
  `create()`: it would reach build_kernel, whose later passes walk entries nobody wrote.  `_upload` asserts it.
* explicit `node_masks`, `leaf_masks` with a bit beyond `n_inds`, a dimension beyond the exponent tables, the two
  strides the Python layer cannot get wrong, a best tree too wide for `max_width` with its `min_slices`, a device the
  links are not on, a device that is not there.
  Wrong masks change values, never an address."""
import contextlib

import numpy as np
import pytest

from tests import helpers as H
from tests import tree_check_cases as tc
from tests.test_tree_check_model import host_status

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


@pytest.fixture(scope="module")
def lib():
    from tnco_amd import _lib
    return _lib


@contextlib.contextmanager
def patched_desc(core, **fields):
    """While active, tnco_hip_create gets its descriptor with these fields overwritten: descriptors core.py never writes."""
    L = core._lib.load()
    real = L.tnco_hip_create
    calls = []

    def create(dref, href):
        for k, v in fields.items():
            setattr(dref._obj, k, v)
        calls.append(1)
        return real(dref, href)

    L.tnco_hip_create = create
    try:
        yield
    finally:
        L.tnco_hip_create = real
    assert calls


def _raises(core, message, *a, exc=ValueError, **kw):
    with pytest.raises(exc) as e:
        core.BatchedOptimizer(*a, **kw)
    assert type(e.value) is exc and str(e.value) == message, (str(e.value), message)


# ---- tree_check_kernel against the model -------------------------------------------------------------------------------

@pytest.mark.parametrize("family", tc.FAMILY_NAMES)
def test_kernel_equals_the_model_tree_for_tree(lib, family):
    trees = tc.family(family)
    st = tc.library_status(trees)
    got = host_status(lib, trees, where=1)
    want = np.where(st == 7, 0, st)  # (the kernel has no check 7)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{family}: tree {bad[0]} {np.asarray(trees[bad[0]]).tolist()}: kernel {got[bad[0]]}, model {want[bad[0]]}"
    assert np.array_equal(want, tc.device_status(trees))
    if family in ("named N=9", "named N=129"):
        assert (st == 7).any()


# ---- create() from device links ----------------------------------------------------------------------------------------

def _upload(lib, dl, trees):
    """`trees` into the device links `dl` -- only trees, or what tree_check_kernel refuses."""
    trees = np.ascontiguousarray(trees, np.int32)
    assert trees.shape == dl.shape
    st, dev = tc.library_status(trees), tc.device_status(trees)
    assert not ((st != 0) & (dev == 0)).any(), "a non-tree that the kernel accepts must never go to create()"
    lib.check(lib.load().tnco_hip_copy_to_device(dl.ptr, trees.ctypes.data, trees.nbytes))


def test_create_refuses_damaged_device_links(core, lib):
    prob = H.regular_problem(16, graph_seed=3)
    n, N, R = 16, 31, 130
    seeds = H.replica_seeds(R, S=2)
    dl = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds, device=0, keep_on_device=True)
    orig = dl.numpy()
    assert orig.shape == (R, 3, N) and not tc.library_status(orig).any()
    plants = [("left=N", n), ("parent=-2", 0), ("right=INT32_MAX", N - 1), ("one child null", n), ("left == right", N - 1),
              ("parent == left", n), ("last node has a parent", N - 1), ("second root", 0), ("leaf slot with children", n - 1),
              ("internal node turned leaf", n), ("parent words exchanged", 0), ("child of two parents", N - 1),
              ("leaf named as parent", n)]
    assert {tc.DAMAGES[name][0] for name, _ in plants} == {1, 2, 3, 4, 5, 6}
    args = (prob.leaf_masks, dl, seeds)
    kw = dict(n_inds=prob.n_inds)
    damaged = {}
    try:
        for name, at in plants:
            code, f = tc.DAMAGES[name]
            for r in (0, 64, 129):
                batch = orig.copy()
                assert f(batch[r], at) and tc.device_status(batch[r:r + 1])[0] == code, (name, r)
                damaged.setdefault(code, batch[r].copy())
                _upload(lib, dl, batch)
                assert np.array_equal(dl.numpy(), batch)
                _raises(core, tc.MESSAGES[code], *args, **kw)
        # two damages in two replicas: the lower replica's message
        for (ra, ca), (rb, cb) in (((3, 5), (70, 2)), ((64, 6), (65, 1)), ((128, 2), (129, 4)), ((0, 3), (129, 6))):
            batch = orig.copy()
            batch[ra], batch[rb] = damaged[ca], damaged[cb]
            _upload(lib, dl, batch)
            _raises(core, tc.MESSAGES[ca], *args, **kw)
        # one tree shared by all replicas: the first tree of the same memory
        one = core.DeviceLinks(dl.ptr, (3, N), 0)
        for code in (1, 4, 6):
            batch = orig.copy()
            batch[0] = damaged[code]
            _upload(lib, dl, batch)
            _raises(core, tc.MESSAGES[code], prob.leaf_masks, one, seeds[:5], **kw)
        # links on a device other than the descriptor's (the library's own check: core.py has one of its own)
        _upload(lib, dl, orig)
        with patched_desc(core, device=1):
            _raises(core, "'links' are in the memory of another device.", *args, **kw)
    finally:
        _upload(lib, dl, orig)
    # the original trees back: the batch they build as a host array
    with core.BatchedOptimizer(*args, **kw) as a, core.BatchedOptimizer(prob.leaf_masks, orig, seeds, **kw) as b:
        for x, y in zip(a.costs(), b.costs()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        ids = np.arange(R)
        assert np.array_equal(a.trees(ids, which_min=False, contraction=False)[0], orig)
    with core.BatchedOptimizer(prob.leaf_masks, one, seeds[:5], **kw) as a, \
            core.BatchedOptimizer(prob.leaf_masks, orig[0], seeds[:5], **kw) as b:
        assert np.array_equal(a.costs()[0].view(np.uint64), b.costs()[0].view(np.uint64))


# ---- the other refusals that need the device ---------------------------------------------------------------------------

def _bit(p):
    return np.uint64(1 << (p % 64))


def _has(row, p):
    return bool((int(row[p // 64]) >> (p % 64)) & 1)


def test_explicit_node_masks_are_checked(core):
    prob = H.regular_problem(8, graph_seed=4)
    n, N, R = 8, 15, 3
    seeds = H.replica_seeds(R, S=1)
    links = prob.links(seeds)
    masks = np.stack([prob.node_masks(l, r) for l, r, _ in links]).astype(np.uint64)
    lm, om, kw = prob.leaf_masks, prob.output_mask, dict(n_inds=prob.n_inds)
    for r in range(R):
        assert tc.mask_status(links[r, 0], links[r, 1], masks[r], lm, om) == 0
    core.BatchedOptimizer(lm, links, seeds, node_masks=masks, **kw).close()
    core.BatchedOptimizer(lm, links[0], seeds, node_masks=masks[0], **kw).close()

    def damage(r, kind):
        m = masks[r].copy()
        l, rr = links[r, 0], links[r, 1]
        if kind == "leaf row":
            m[0, 0] ^= _bit(next(p for p in range(prob.n_inds) if _has(lm[0], p)))
            return m, 12
        node = N - 1 if kind == "extra leg at the root" else n
        a, b = m[l[node]], m[rr[node]]
        if kind.startswith("extra leg"):
            p = next(p for p in range(prob.n_inds) if not _has(a | b, p))
            m[node, p // 64] |= _bit(p)
        else:  # a leg that one child has and the node must keep
            p = next(p for p in range(prob.n_inds) if _has(a ^ b, p))
            assert _has(m[node], p)
            m[node, p // 64] &= ~_bit(p)
        return m, 11

    for kind in ("extra leg", "extra leg at the root", "missing leg", "leaf row"):
        for r in (0, R - 1):  # [R, N, W], the damage in the first and in the last replica
            m, want = damage(r, kind)
            assert tc.mask_status(links[r, 0], links[r, 1], m, lm, om) == want, kind
            batch = masks.copy()
            batch[r] = m
            _raises(core, tc.MASK_MESSAGES[want], lm, links, seeds, node_masks=batch, **kw)
        m, want = damage(0, kind)  # [N, W] with one shared tree
        _raises(core, tc.MASK_MESSAGES[want], lm, links[0], seeds, node_masks=m, **kw)
    assert tc.MASK_MESSAGES[11] == "Contraction is not valid." and tc.MASK_MESSAGES[12] == "'node_masks' leaves differ from 'leaf_masks'."


def test_leaf_masks_beyond_n_inds_a_dimension_beyond_the_tables_and_devices(core):
    prob = H.regular_problem(8, graph_seed=4)
    seeds = H.replica_seeds(2, S=1)
    links = prob.links(seeds)
    assert prob.n_inds == 12
    for p in (12, 63):
        lm = prob.leaf_masks.copy()
        lm[3, 0] |= _bit(p)
        _raises(core, "index position out of range in 'leaf_masks'.", lm, links, seeds, n_inds=prob.n_inds)
    dims = np.full(prob.n_inds, 2, np.uint64)
    dims[3] = 1 << 40  # (a power-of-two part up to 2^32 is taken: tests/test_gpu_parity.py::test_invalid_inputs)
    _raises(core, "an index dimension with a power-of-two part above 2^32 is not supported on the GPU path.",
            prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=dims, exc=NotImplementedError)
    with patched_desc(core, device=99):
        _raises(core, "'device' is not valid.", prob.leaf_masks, links, seeds, n_inds=prob.n_inds)
    with patched_desc(core, device=-1):
        _raises(core, "'device' is not valid.", prob.leaf_masks, links, seeds, n_inds=prob.n_inds)


def test_strides_below_a_row_are_refused(core):
    """`slices_stride` < W and `min_links_stride` < 3 N: through the C ABI, core.py writes 0 or the row length."""
    prob = H.regular_problem(48, graph_seed=8)
    assert prob.W == 2
    seeds = H.replica_seeds(4, S=3)
    links = prob.links(seeds)
    kw = dict(n_inds=prob.n_inds)
    with patched_desc(core, slices_stride=1):
        _raises(core, "'slices_stride' is not valid.", prob.leaf_masks, links, seeds, max_width=6,
                slices=np.zeros((4, 2), np.uint64), **kw)
    with patched_desc(core, slices_stride=-2):
        _raises(core, "'slices_stride' is not valid.", prob.leaf_masks, links, seeds, max_width=6, **kw)
    N = 2 * prob.n - 1
    for stride in (3 * N - 1, 1, -3 * N):
        with patched_desc(core, min_links_stride=stride):
            _raises(core, "'min_links_stride' is not valid.", prob.leaf_masks, links, seeds, min_links=links, **kw)


def _width(prob, links_r, slices_r):
    """log2 of the largest tensor of the tree once the sliced indices are removed (all dimensions 2): its open legs."""
    m = prob.node_masks(links_r[0], links_r[1]).astype(np.uint64) & ~np.asarray(slices_r, np.uint64)[None, :]
    return int(np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1).sum(1).max())


def test_best_tree_wider_than_max_width_is_refused(core):
    prob = H.regular_problem(16, graph_seed=2)
    R, max_width = 4, 4
    seeds = H.replica_seeds(R, S=5)
    links = prob.links(seeds)
    kw = dict(n_inds=prob.n_inds, max_width=max_width)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, **kw) as g:
        sl, _ = g.slices_many(np.arange(R))
    none = np.zeros_like(sl)
    assert all(_width(prob, links[r], sl[r]) <= max_width for r in range(R))
    wide = [_width(prob, links[r], none[r]) > max_width for r in range(R)]
    assert wide[R - 1] and any(wide)
    core.BatchedOptimizer(prob.leaf_masks, links, seeds, slices=sl, min_links=links, min_slices=sl, **kw).close()
    msg = "Width of the sliced minimum contraction is larger than 'max_width'."
    _raises(core, msg, prob.leaf_masks, links, seeds, slices=sl, min_links=links, min_slices=none, **kw)
    only_last = sl.copy()
    only_last[R - 1] = 0
    _raises(core, msg, prob.leaf_masks, links, seeds, slices=sl, min_links=links, min_slices=only_last, **kw)
