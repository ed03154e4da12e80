"""Every refusal of the optimizer's constructor that needs no device: the tree check (host `tree_check` of
csrc/tnco_hip.hip) against a model and against the real reference Tree, and the descriptor checks in code order.

tests/tree_check_cases.py holds the model (`reference_verdict`, `library_status`, `device_status`) and the trees: named
damages of four base trees at seven sizes, all 4^9 link arrays of three nodes, seeded random damage.  Here:

* the model of the reference against the REAL reference (oracle/_ref/libref_tree.so, or its recording
  tests/golden/tree_check.json where the reference sources are absent);
* the library's rule against the reference's: it accepts nothing the reference refuses, and what it refuses beyond the
  reference falls into named classes with pinned counts;
* the argument in the comment above `tree_check_kernel` (the host's two counters follow from checks 1-5 and the answered
  child links) on every tree of every family;
* the real host function (`tnco_hip_diag_tree_check(where=0)`) against the model, tree for tree;
* `BatchedOptimizer` with host links: the message of every damage, of the LOWEST damaged replica of a batch whatever
  the thread count, and of a ring of internal nodes (not a tree, yet every count and link is right);
* `check_input`'s refusals in code order, each with its exception type and text, the precedence between neighbours shown
  by descriptors that violate two at once.

The tests that need the device are in tests/test_gpu_tree_check.py, but for the ring as `min_links` (below, marked): the
host check of `min_links` runs once the handle is open.

Two messages tnco_hip_create can return are named by no test, both "finite width: candidate legs beyond the re-slice
scratch (internal error).": the status a re-slice kernel leaves when a tensor has more candidate legs than its scratch
holds.  `create` sizes that scratch from the network it is given, so no descriptor reaches them; they guard the kernels'
own bookkeeping."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from tests import tree_check_cases as tc

GOLDEN = Path(__file__).resolve().parent / "golden" / "tree_check.json"


def real_reference_verdicts(ref, trees):
    trees = np.ascontiguousarray(trees, np.int32)
    N = trees.shape[2]
    # (identical link arrays once: the exhaustive family is checked in a second or two)
    uniq, inv = np.unique(trees.reshape(len(trees), -1), axis=0, return_inverse=True)
    uniq = np.ascontiguousarray(uniq.reshape(-1, 3, N))
    ok = np.array([ref.ref_tree_is_valid(N, t[0], t[1], t[2]) == 1 for t in uniq], bool)
    return ok[inv.reshape(-1)]


@pytest.fixture(scope="module")
def fam():
    out = {}
    for name, trees in tc.families().items():
        q = tc.parts(trees)
        out[name] = (trees, q, tc.library_status(trees, q))
    return out


@pytest.fixture(scope="module")
def ref_verdicts(fam, oracle_lib):
    """family -> bool[T] of the real reference; the recording where the reference was not built (and both compared
    where both exist)."""
    golden = json.loads(GOLDEN.read_text())
    rec = {}
    for name, (trees, _, _) in fam.items():
        assert golden[name]["trees"] == len(trees), name
        ok = np.zeros(len(trees), bool)
        ok[golden[name]["accepted"]] = True
        rec[name] = ok
    ref = oracle_lib.ref_tree()
    if ref is None:
        return rec
    real = {name: real_reference_verdicts(ref, trees) for name, (trees, _, _) in fam.items()}
    for name in real:
        assert np.array_equal(real[name], rec[name]), f"{name}: tests/golden/tree_check.json is stale"
    return real


@pytest.fixture(scope="module")
def lib():
    from tnco_amd import _lib
    return _lib


def host_status(lib, trees, where=0, device=0):
    trees = np.ascontiguousarray(trees, np.int32)
    T, _, N = trees.shape
    out = np.full(T, -1, np.int32)
    lib.check(lib.load().tnco_hip_diag_tree_check(device, N, trees.ctypes.data, 3 * N, T, where, out.ctypes.data))
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", tc.SIZES)
def test_every_named_damage_fails_its_own_check_and_no_earlier_one(N):
    labels, codes, trees = tc.named_arrays(N)
    q = tc.parts(trees)
    st, dev = tc.library_status(trees, q), tc.device_status(trees, q)
    for k in np.flatnonzero(st != codes):
        pytest.fail(f"{labels[k]}: the model says {st[k]}, the table {codes[k]}")
    assert np.array_equal(dev, np.where(codes == 7, 0, codes))  # the kernel's rule: the same but for check 7
    assert set(codes) >= {1, 2, 3, 4, 5, 6} and (N not in (9, 129) or 7 in codes)
    for k, lab in enumerate(labels):
        if "parent words exchanged" in lab:
            assert not q["counters"][k] and q["links"][k], lab  # every count right: only the links tell
        if "ring" in lab:
            assert not (q["counters"][k] or q["links"][k]) and q["reach"][k], lab
    planted = {int(lab.rsplit("@", 1)[1]) for lab in labels if "@" in lab}
    assert planted == set(tc.positions(N))
    assert not tc.library_status(tc.valid_trees(N)).any() and tc.reference_verdict(tc.valid_trees(N)).all()


def test_random_damage_families_hold_every_code(fam):
    for n in (3, 4):
        assert set(fam[f"random n={n}"][2]) == {0, 1, 2, 3, 4, 5, 6}
    for n in (33, 65):  # (codes 4 and 5 are rare there by construction: the named damages cover them)
        assert set(fam[f"random n={n}"][2]) >= {0, 1, 2, 3, 6}


# ---- the model of the reference against the real reference -----------------------------------------------------------------

def test_reference_model_equals_the_real_reference(fam, ref_verdicts):
    for name, (trees, _, _) in fam.items():
        model = tc.reference_verdict(trees)
        bad = np.flatnonzero(model != ref_verdicts[name])
        assert len(bad) == 0, f"{name}: tree {bad[0]} {trees[bad[0]].tolist()}: model {model[bad[0]]}"


# What the reference accepts and the library refuses, per family: (a negative entry other than -1; check 6, i.e. a parent
# or child count that the strict rule refuses or a child link its child does not answer [of these: every count right,
# only a link unanswered -- the reference compares no link with a parent word]; not reachable from the root).
# Of the 4^9 arrays of three nodes both accept the same two: the reference's lenient counters need more nodes to matter.
STRICTER = {
    "exhaustive": (0, 0, 0, 0),
    "named N=3": (40, 0, 0, 0),
    "named N=5": (40, 12, 12, 0),
    "named N=7": (40, 12, 12, 0),
    "named N=9": (40, 12, 12, 1),
    "named N=127": (40, 12, 12, 0),
    "named N=129": (56, 16, 16, 2),
    "named N=4095": (72, 20, 20, 0),
    "random n=3": (590, 309, 14, 0),
    "random n=4": (413, 512, 8, 0),
    "random n=33": (11, 196, 0, 0),
    "random n=65": (5, 203, 0, 0),
}


def test_library_refuses_what_the_reference_refuses_and_three_classes_more(fam, ref_verdicts):
    got = {}
    for name, (trees, q, st) in fam.items():
        ref = ref_verdicts[name]
        assert not (~ref & (st == 0)).any(), f"{name}: the library accepts a tree the reference refuses"
        more = ref & (st != 0)
        assert set(st[more]) <= {1, 6, 7}, name
        neg = (np.asarray(trees) < -1).any(axis=(1, 2))
        assert np.array_equal(more & (st == 1), more & neg), name  # check 1 beyond the reference: only such entries
        got[name] = (int((more & (st == 1)).sum()), int((more & (st == 6)).sum()),
                     int((more & (st == 6) & ~q["counters"]).sum()), int((more & (st == 7)).sum()))
        print(f"{name}: reference accepts {int(ref.sum())}, library {int((st == 0).sum())}; refused beyond the reference: "
              f"negative entry {got[name][0]}, check 6 {got[name][1]} (links only {got[name][2]}), unreachable {got[name][3]}")
    assert got == STRICTER


# ---- the comment above tree_check_kernel -------------------------------------------------------------------------------

def test_answered_links_imply_the_hosts_counters(fam):
    """With checks 1-5 passed and every child link answered by the child's parent word, both counters are right: the
    kernel may drop them.  (So device_status == library_status but for check 7.)"""
    for name, (trees, q, st) in fam.items():
        early = q["c1"] | q["c2"] | q["c3"] | q["c4"] | q["c5"]
        assert not (~early & ~q["links"] & q["counters"]).any(), name
        assert np.array_equal(tc.device_status(trees, q), np.where(st == 7, 0, st)), name


# ---- the real host function --------------------------------------------------------------------------------------------

EXHAUSTIVE_CODES = [2, 258048, 2304, 1225, 504, 9, 52, 0]  # trees per code 0..7 among the 4^9 of three nodes


def test_host_check_equals_the_model_tree_for_tree(fam, lib):
    for name, (trees, _, st) in fam.items():
        got = host_status(lib, trees)
        bad = np.flatnonzero(got != st)
        assert len(bad) == 0, f"{name}: tree {bad[0]} {np.asarray(trees[bad[0]]).tolist()}: host {got[bad[0]]}, model {st[bad[0]]}"
    assert np.bincount(fam["exhaustive"][2], minlength=8).tolist() == EXHAUSTIVE_CODES


def test_diag_tree_check_refuses_bad_arguments(lib):
    L = lib.load()
    t = np.ascontiguousarray(tc.left_deep(2)[None], np.int32)
    out = np.zeros(1, np.int32)
    for args in ((3, None, 9, 1, 0, out.ctypes.data), (3, t.ctypes.data, 9, 1, 0, None), (4, t.ctypes.data, 12, 1, 0, out.ctypes.data),
                 (3, t.ctypes.data, 8, 1, 0, out.ctypes.data), (3, t.ctypes.data, 9, 0, 0, out.ctypes.data),
                 (3, t.ctypes.data, 9, 1, 2, out.ctypes.data)):
        assert L.tnco_hip_diag_tree_check(0, *args) == lib.EINVAL


# ---- through BatchedOptimizer, host links: refused before any device use ---------------------------------------------------

def _refused(links, message, R=None, **kw):
    from tnco_amd import core
    N = links.shape[-1]
    n = (N + 1) // 2
    R = len(links) if links.ndim == 3 else R
    with pytest.raises(ValueError) as e:
        core.BatchedOptimizer(np.zeros((n, 1), np.uint64), links, np.arange(R), n_inds=1, **kw)
    assert str(e.value) == message, (str(e.value), message)


@pytest.mark.parametrize("N", tc.SIZES)
def test_every_named_damage_is_refused_with_its_message(N):
    """One replica, and one tree shared by 64."""
    labels, codes, trees = tc.named_arrays(N)
    for k in range(len(labels)):
        _refused(trees[k:k + 1], tc.MESSAGES[int(codes[k])])
        _refused(trees[k], tc.MESSAGES[int(codes[k])], R=64)


def _one_per_damage(N):
    """One named case of every damage (and the rings), the position changing from one damage to the next."""
    labels, codes, trees = tc.named_arrays(N)
    seen, out = {}, []
    for k, lab in enumerate(labels):
        kind = lab.split(f"N={N} ", 1)[1].rsplit(" @", 1)[0] if "@" in lab else lab
        seen.setdefault(kind, []).append(k)
    for j, (kind, ks) in enumerate(seen.items()):
        out.append(ks[(5 * j) % len(ks)])
    return [(labels[k], int(codes[k]), trees[k]) for k in out]


@pytest.mark.parametrize("R", [64, 130, 1025])
@pytest.mark.parametrize("N", [9, 129])
def test_a_damaged_replica_anywhere_in_a_batch_is_found(N, R):
    good = tc.valid_trees(N)
    batch = np.ascontiguousarray(good[np.arange(R) % len(good)])
    for _, code, t in _one_per_damage(N):
        for where in (0, 64, R - 1):
            if where < R:
                links = batch.copy()
                links[where] = t
                _refused(links, tc.MESSAGES[code])


@pytest.mark.parametrize("R", [64, 130, 1025])
def test_the_lowest_damaged_replica_speaks(R):
    """Two damages with different messages in one batch: the lower replica's, whatever thread checked it.  (Replica r used
    to go to thread r % nth and the lowest THREAD's finding was reported: with two threads or more, replica 2's.)"""
    N = 129
    cases = {code: t for _, code, t in _one_per_damage(N)}
    good = tc.valid_trees(N)
    for first, second in ((3, 5), (5, 2), (6, 1), (1, 4), (2, 6), (4, 3)):
        for a, b in ((1, 2), (1, R - 1), (R - 2, R - 1), (63, 64)):
            links = np.ascontiguousarray(good[np.arange(R) % len(good)])
            if b < R:
                links[a], links[b] = cases[first], cases[second]
                _refused(links, tc.MESSAGES[first])


def test_a_ring_of_internal_nodes_is_no_tree():
    """N = 9: a root over two leaves, and three internal nodes that hold one another and a leaf each.  Every count and
    every link is right -- the reference accepts it -- but the traverse from the root reaches 3 of 9 nodes."""
    ring = tc.ring(9)
    assert tc.reference_verdict(ring)[0] and tc.device_status(ring)[0] == 0 and tc.library_status(ring)[0] == 7
    _refused(ring, "Tree is not valid.", R=1)
    _refused(ring[None], "Tree is not valid.")
    batch = np.ascontiguousarray(np.tile(tc.left_deep(5), (130, 1, 1)))
    batch[129] = ring
    _refused(batch, "Tree is not valid.")
    for base in ("left_deep", "balanced"):
        _refused(tc.ring(129, tc.BASES[base]), "Tree is not valid.", R=3)


@pytest.mark.gpu
def test_a_ring_as_min_links_is_refused():
    """The host check of `min_links` runs once the handle is open; the ring never reaches a kernel."""
    from tnco_amd import core
    from tnco_amd.synthetic import Problem, chain_tn
    prob = Problem(*chain_tn(5))
    links = tc.left_deep(5)
    for ml in (tc.ring(9), np.stack([links, tc.ring(9)])):
        with pytest.raises(ValueError) as e:
            core.BatchedOptimizer(prob.leaf_masks, links, [1, 2], n_inds=prob.n_inds, min_links=ml)
        assert str(e.value) == "Tree is not valid."
    core.BatchedOptimizer(prob.leaf_masks, links, [1, 2], n_inds=prob.n_inds, min_links=links).close()


# ---- check_input: the descriptor, in code order ------------------------------------------------------------------------

class _Args:
    """A descriptor that passes every check of check_input but the tree check (its links are damaged: nothing here may
    reach the device), and the arrays it points to."""

    def __init__(self, lib, n=2, W=1, R=2):
        N = 2 * n - 1
        self.keep = dict(leaf_masks=np.zeros((n, W), np.uint64), links=np.full((3, N), -1, np.int32), seeds=np.zeros(R, np.uint32),
                         prng=np.zeros((R, 625), np.uint32), dims=np.full(max(W * 64, 1), 2, np.uint64), sparse=np.ones(W, np.uint64))
        self.keep["links"][2, 0] = 7 * N  # check 1
        d = self.d = lib.Desc()
        d.n_leaves, d.n_inds, d.n_replicas = n, 1, R
        d.leaf_masks, d.links, d.seeds = (self.keep[k].ctypes.data for k in ("leaf_masks", "links", "seeds"))
        d.dim_uniform, d.cost_dtype, d.width_dtype, d.max_width = 2, lib.F64, lib.F32, float("nan")


NULL = object()

# (what is wrong, exception, message) in the order of check_input; a field `x` of the dict is set on the descriptor, a
# value naming an array of _Args.keep points the field there, NULL clears it
CHECKS = [
    (dict(n_leaves=1), ValueError, "Precision is too low."),
    (dict(n_replicas=0), ValueError, "'n_inds' / 'n_replicas' are not valid."),
    (dict(links=NULL), ValueError, "null input array."),
    (dict(prng_states="prng", bad_prng=True), ValueError, "prng position out of range."),
    (dict(cost_dtype=7), NotImplementedError, "cost_type must be float64 or float32."),
    (dict(n_inds=4097), NotImplementedError, "more than 4096 indices are not supported yet."),
    (dict(sparse_mask="sparse", n_projs=0), RuntimeError, "'n_projs' must be a positive number."),
    (dict(dims="dims", zero_dim=True), ValueError, "Dimensions must be positive numbers"),
    (dict(dim_uniform=0), ValueError, "Dimensions must be positive numbers"),
    (dict(n_leaves=32769, max_width=3.0), NotImplementedError, "finite width: more than 32768 tensors are not supported."),
    (dict(max_width=-1.0), RuntimeError, "'max_width' must be a non-negative number."),
    (dict(max_width=3.0, width_dtype=9), NotImplementedError, "finite width: width_type must be float32 or float64."),
    (dict(), ValueError, "Nodes are not valid"),
]
MORE_CHECKS = [
    (dict(n_inds=-1), ValueError, "'n_inds' / 'n_replicas' are not valid."),
    (dict(n_replicas=-3), ValueError, "'n_inds' / 'n_replicas' are not valid."),
    (dict(leaf_masks=NULL), ValueError, "null input array."),
    (dict(seeds=NULL), ValueError, "null input array."),
    (dict(n_leaves=0), ValueError, "Precision is too low."),
    (dict(n_leaves=-5), ValueError, "Precision is too low."),
]


def _create(lib, *wrong):
    n = max([w.get("n_leaves", 2) for w in wrong] + [2])
    W = 65 if any(w.get("n_inds", 0) > 4096 for w in wrong) else 1
    a = _Args(lib, n=n, W=W)
    for w in wrong:
        for k, v in w.items():
            if k == "bad_prng":
                a.keep["prng"][1, 624] = 625
            elif k == "zero_dim":
                a.keep["dims"][0] = 0
            else:
                setattr(a.d, k, None if v is NULL else a.keep[v].ctypes.data if isinstance(v, str) else v)
    h = C.c_void_p()
    rc = lib.load().tnco_hip_create(C.byref(a.d), C.byref(h))
    assert rc != lib.OK and not h.value
    lib.check(rc)


@pytest.mark.parametrize("k", range(len(CHECKS) + len(MORE_CHECKS)))
def test_check_input_refusals_type_and_text(lib, k):
    wrong, exc, msg = (CHECKS + MORE_CHECKS)[k]
    with pytest.raises(exc) as e:
        _create(lib, wrong)
    assert type(e.value) is exc and str(e.value) == msg


# two neighbours of CHECKS violated at once -> the index of the one that speaks.  (The two sites of the dimension check cannot
# both be violated -- one reads `dims`, the other runs where `dims` is uniform or absent: each is paired with the finite-width
# checks behind them.  Every descriptor here has a damaged tree besides: all of this precedes the tree check.)
PAIRS = [
    (0, dict(n_leaves=1, n_replicas=0)),
    (1, dict(n_replicas=0, links=NULL)),
    (2, dict(links=NULL, prng_states="prng", bad_prng=True)),
    (3, dict(prng_states="prng", bad_prng=True, cost_dtype=7)),
    (4, dict(cost_dtype=7, n_inds=4097)),
    (5, dict(n_inds=4097, sparse_mask="sparse", n_projs=0)),
    (6, dict(sparse_mask="sparse", n_projs=0, dims="dims", zero_dim=True)),
    (7, dict(dims="dims", zero_dim=True, n_leaves=32769, max_width=3.0)),
    (8, dict(dim_uniform=0, n_leaves=32769, max_width=3.0)),
    (9, dict(n_leaves=32769, max_width=-1.0)),
    (10, dict(max_width=-1.0, width_dtype=9)),
    (11, dict(max_width=3.0, width_dtype=9)),
]


@pytest.mark.parametrize("k", range(len(PAIRS)))
def test_check_input_refusals_come_in_code_order(lib, k):
    speaker, wrong = PAIRS[k]
    _, exc, msg = CHECKS[speaker]
    with pytest.raises(exc) as e:
        _create(lib, wrong)
    assert type(e.value) is exc and str(e.value) == msg


def test_null_descriptor(lib):
    h = C.c_void_p()
    assert lib.load().tnco_hip_create(None, C.byref(h)) == lib.EINVAL
    assert lib.load().tnco_hip_last_error() == b"null argument."
    d = lib.Desc()
    assert lib.load().tnco_hip_create(C.byref(d), None) == lib.EINVAL
    assert lib.load().tnco_hip_last_error() == b"null argument."
