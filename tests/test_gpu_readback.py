"""The read-back surface of a handle -- every entry point of csrc/tnco_hip.hip from tnco_hip_run to tnco_hip_diag_moves:
what each one refuses (status, the exact tnco_hip_last_error() text, nothing written), in the order it checks, and that the
getters that return the same thing in two ways (one replica / a list / all) agree bit for bit, on every layout they branch
on: child partials, the unified layout of hyper-indices, finite width with float32 and float64 widths, a restored best tree
(HBM kernel on a small tree) and a batch on two streams read without a sync().  The values themselves are held to the
oracle elsewhere (tests/test_gpu_parity.py, test_gpu_fw.py, test_gpu_restore.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import cost_range_cases as CR
from tests import helpers as H

pytestmark = pytest.mark.gpu

EINVAL = 1
BETAS = H.linear_betas(0, 60, 20)
TOPK_HOST = 4096 // 2  # tnco_hip_best sorts on the host beyond TOPK_CHUNK / 2 (csrc/extract_kernels.h)


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _make(core, kind, R=32):
    """A batch of `kind` after the 20-sweep schedule, with the arm of the getters it is meant to reach asserted."""
    kw, groups, fw = {}, 0, False
    if kind == "hyper":
        # (the smallest network with hyper-indices the suite builds; dims 2, so that no cost leaves the number range)
        prob = CR.problem(next(c for c in CR.CASES if c.name == "hyper_lds").with_param(1))
    elif kind.startswith("fw"):
        prob, fw, groups = H.regular_problem(40, graph_seed=8), True, 1
        kw = dict(max_width=5, width_type="float64" if kind == "fw64" else "float32")
    else:
        prob = H.regular_problem(16, graph_seed=3)
    seeds = H.replica_seeds(R, S=9)
    kw.update(n_inds=prob.n_inds, dims=prob.dims, output_mask=prob.output_mask)
    gpu = core.BatchedOptimizer(prob.leaf_masks, prob.links(seeds), seeds, **kw)
    gpu.run(BETAS)
    if kind == "restored":  # min_links= puts a small tree on the HBM kernel
        snap = gpu.snapshot()
        gpu.close()
        gpu = core.BatchedOptimizer.restore(snap, prob.leaf_masks, **kw)
        gpu.run(BETAS)
        groups = 1
    assert gpu.finite_width == fw and gpu.launch_groups == groups, (kind, gpu.finite_width, gpu.launch_groups)
    return gpu


@pytest.fixture(scope="module")
def batches(core):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _make(core, kind)
        return made[kind]

    yield get
    for g in made.values():
        g.close()


def _state(gpu, ids=None):
    ids = np.arange(gpu.n_replicas) if ids is None else np.asarray(ids)
    tot, mn = gpu.costs()
    st = dict(cur=gpu.trees(ids, which_min=False)[0], best=gpu.trees(ids, which_min=True)[0], tot=tot.view(np.uint64),
              mn=mn.view(np.uint64), prng=gpu.prng_states(ids), moves=gpu.moves_per_replica())
    if gpu.finite_width:
        st["slices"], st["min_slices"] = gpu.slices_many(ids)
    return st


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: (name, batch, call(L, h, R, a) -> status, message).  `a`: scratch arrays big enough for every output.
# The texts are those of the library before its entry points were rewritten.
# ---------------------------------------------------------------------------------------------------------------------
NULLH, NULLA = "null handle.", "null argument."
RANGE, NOFW = "'replica' out of range.", "handle was created without 'max_width'."
KIND, BET, KBAD, POS = "'prob_kind' is not valid.", "'betas' is not valid.", "'k' is not valid.", "prng position out of range."
NOTINT = "'node' is not an internal node."


class _Scratch:
    def __init__(self, gpu):
        R, N, W = gpu.n_replicas, gpu.n_nodes, gpu.n_words
        self.R, self.N, self.n, self.W = R, N, gpu.n_leaves, W
        self.betas = np.zeros(4)
        self.u64 = np.zeros((R + 1) * max(N * W, 8), np.uint64)
        self.u64b = np.zeros_like(self.u64)
        self.f64, self.f64b = np.zeros(max(R + 1, N)), np.zeros(max(R + 1, N))
        self.i32 = [np.zeros((R + 1) * 3 * N, np.int32) for _ in range(3)]
        self.i64 = np.zeros(R + 8, np.int64)
        self.st = gpu.prng_states()           # [R, 625], valid positions
        self.st_bad = self.st.copy()
        self.st_bad[0, 624] = 625
        self.st_bad_last = self.st.copy()
        self.st_bad_last[-1, 624] = 625
        self.out = np.zeros((R + 1, 625), np.uint32)
        self.ids = np.arange(R, dtype=np.int64)
        self.bad_first, self.bad_last, self.neg_last = self.ids.copy(), self.ids.copy(), self.ids.copy()
        self.bad_first[0], self.bad_last[-1], self.neg_last[-1] = R, R, -1
        self.prev = C.c_uint64(0)


def _poke(L, h, a, r, field, node=0, word=0, write=0, value=0):
    return L.tnco_hip_diag_poke(h, r, field, node, word, write, value & 0xFFFFFFFFFFFFFFFF, C.byref(a.prev))


def _rows():
    p = _ptr
    u = C.byref
    rows = [
        # tnco_hip_run (infinite memory) / tnco_hip_run_fw (finite width)
        ("run null", "plain", lambda L, h, a: L.tnco_hip_run(None, 2, p(a.betas), 4), NULLH),
        ("run kind 3", "plain", lambda L, h, a: L.tnco_hip_run(h, 3, p(a.betas), 4), KIND),
        ("run kind -1", "plain", lambda L, h, a: L.tnco_hip_run(h, -1, p(a.betas), 4), KIND),
        ("run n < 0", "plain", lambda L, h, a: L.tnco_hip_run(h, 2, p(a.betas), -1), BET),
        ("run no betas", "plain", lambda L, h, a: L.tnco_hip_run(h, 2, None, 4), BET),
        ("run kind before n", "plain", lambda L, h, a: L.tnco_hip_run(h, 3, None, -1), KIND),
        ("run on fw", "fw32", lambda L, h, a: L.tnco_hip_run(h, 2, p(a.betas), 4), "handle was created with 'max_width': use tnco_hip_run_fw."),
        ("run kind before fw", "fw32", lambda L, h, a: L.tnco_hip_run(h, 3, p(a.betas), 4), KIND),
        ("run betas before fw", "fw32", lambda L, h, a: L.tnco_hip_run(h, 2, None, 4), BET),
        ("run_fw null", "fw32", lambda L, h, a: L.tnco_hip_run_fw(None, 2, p(a.betas), 4, 10, 0), NULLH),
        ("run_fw on plain", "plain", lambda L, h, a: L.tnco_hip_run_fw(h, 2, p(a.betas), 4, 10, 0), "handle was created without 'max_width': use tnco_hip_run."),
        ("run_fw plain before kind", "plain", lambda L, h, a: L.tnco_hip_run_fw(h, 3, None, -1, 10, -1), "handle was created without 'max_width': use tnco_hip_run."),
        ("run_fw kind 3", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 3, p(a.betas), 4, 10, 0), KIND),
        ("run_fw kind before n", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 3, p(a.betas), -1, 10, -1), KIND),
        ("run_fw n < 0", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 2, p(a.betas), -1, 10, 0), BET),
        ("run_fw no betas", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 2, None, 4, 10, 0), BET),
        ("run_fw offset < 0", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 2, p(a.betas), 4, 10, -1), BET),
        ("run_fw offset < 0, no sweeps", "fw32", lambda L, h, a: L.tnco_hip_run_fw(h, 2, None, 0, 10, -1), BET),
        # slices
        ("slices null", "fw32", lambda L, h, a: L.tnco_hip_get_slices(None, 0, p(a.u64), p(a.u64b)), NULLH),
        ("slices plain", "plain", lambda L, h, a: L.tnco_hip_get_slices(h, 0, p(a.u64), p(a.u64b)), NOFW),
        ("slices plain before r", "plain", lambda L, h, a: L.tnco_hip_get_slices(h, -1, p(a.u64), p(a.u64b)), NOFW),
        ("slices r -1", "fw32", lambda L, h, a: L.tnco_hip_get_slices(h, -1, p(a.u64), p(a.u64b)), RANGE),
        ("slices r R", "fw32", lambda L, h, a: L.tnco_hip_get_slices(h, a.R, p(a.u64), p(a.u64b)), RANGE),
        ("slices_many null", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(None, 1, p(a.ids), p(a.u64), p(a.u64b)), NULLH),
        ("slices_many plain", "plain", lambda L, h, a: L.tnco_hip_get_slices_many(h, 1, p(a.ids), p(a.u64), p(a.u64b)), NOFW),
        ("slices_many plain before k", "plain", lambda L, h, a: L.tnco_hip_get_slices_many(h, -1, None, p(a.u64), p(a.u64b)), NOFW),
        ("slices_many k < 0", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(h, -1, p(a.ids), p(a.u64), p(a.u64b)), NULLA),
        ("slices_many no ids", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(h, a.R + 1, None, p(a.u64), p(a.u64b)), NULLA),
        ("slices_many bad first", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(h, a.R, p(a.bad_first), p(a.u64), p(a.u64b)), RANGE),
        ("slices_many bad last", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(h, a.R, p(a.bad_last), p(a.u64), p(a.u64b)), RANGE),
        ("slices_many -1 last", "fw32", lambda L, h, a: L.tnco_hip_get_slices_many(h, a.R, p(a.neg_last), p(a.u64), p(a.u64b)), RANGE),
        # diagnostics of the finite-width handle and the timers
        ("reslice_info null", "fw32", lambda L, h, a: L.tnco_hip_diag_reslice_info(None, p(a.i32[0]), p(a.i32[1])), NULLH),
        ("reslice_info plain", "plain", lambda L, h, a: L.tnco_hip_diag_reslice_info(h, p(a.i32[0]), p(a.i32[1])), "handle has no re-pricing re-slice."),
        ("fw_stats null", "fw32", lambda L, h, a: L.tnco_hip_diag_fw_stats(None, p(a.i64)), NULLA),
        ("fw_stats no out", "fw32", lambda L, h, a: L.tnco_hip_diag_fw_stats(h, None), NULLA),
        ("fw_stats plain", "plain", lambda L, h, a: L.tnco_hip_diag_fw_stats(h, p(a.i64)), NOFW),
        ("fw_stats no out before plain", "plain", lambda L, h, a: L.tnco_hip_diag_fw_stats(h, None), NULLA),
        ("kernel_time null", "plain", lambda L, h, a: L.tnco_hip_diag_kernel_time(None, None, None, 0), NULLH),
        ("kernel_times null", "plain", lambda L, h, a: L.tnco_hip_diag_kernel_times(None, p(a.f64), p(a.i64), 0), NULLH),
        # costs, trees, caches, validate
        ("costs null", "plain", lambda L, h, a: L.tnco_hip_get_costs(None, p(a.f64), p(a.f64b)), NULLH),
        ("tree null", "plain", lambda L, h, a: L.tnco_hip_get_tree(None, 0, 0, p(a.i32[0]), p(a.i32[1]), p(a.i32[2]), None), NULLH),
        ("tree r -1", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, -1, 0, p(a.i32[0]), p(a.i32[1]), p(a.i32[2]), None), RANGE),
        ("tree r R", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, a.R, 1, p(a.i32[0]), p(a.i32[1]), p(a.i32[2]), None), RANGE),
        ("tree r before outputs", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, a.R, 0, None, None, None, None), RANGE),
        ("tree no left", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, 0, 0, None, p(a.i32[1]), p(a.i32[2]), None), "null output array."),
        ("tree no right", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, 0, 1, p(a.i32[0]), None, p(a.i32[2]), None), "null output array."),
        ("tree no parent", "plain", lambda L, h, a: L.tnco_hip_get_tree(h, 0, 0, p(a.i32[0]), p(a.i32[1]), None, None), "null output array."),
        ("caches null", "plain", lambda L, h, a: L.tnco_hip_get_caches(None, 0, p(a.f64), p(a.f64b), p(a.u64)), NULLH),
        ("caches r -1", "plain", lambda L, h, a: L.tnco_hip_get_caches(h, -1, p(a.f64), p(a.f64b), p(a.u64)), RANGE),
        ("caches r R", "hyper", lambda L, h, a: L.tnco_hip_get_caches(h, a.R, p(a.f64), p(a.f64b), p(a.u64)), RANGE),
        ("validate null", "plain", lambda L, h, a: L.tnco_hip_validate(None, 1e-5, None, None), NULLH),
        ("trees null", "plain", lambda L, h, a: L.tnco_hip_get_trees(None, 1, p(a.ids), 0, p(a.i32[0]), None), NULLH),
        ("trees k < 0", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, -1, p(a.ids), 0, p(a.i32[0]), None), NULLA),
        ("trees no ids", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, a.R + 1, None, 0, p(a.i32[0]), None), NULLA),
        ("trees no links", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, 1, p(a.ids), 0, None, None), NULLA),
        ("trees which 2", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, 1, p(a.ids), 2, p(a.i32[0]), None), "'which' is not valid."),
        ("trees which before ids", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, a.R, p(a.bad_first), 2, p(a.i32[0]), None), "'which' is not valid."),
        ("trees null before which", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, 1, None, 2, p(a.i32[0]), None), NULLA),
        ("trees bad first", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, a.R, p(a.bad_first), 1, p(a.i32[0]), None), RANGE),
        ("trees bad last", "plain", lambda L, h, a: L.tnco_hip_get_trees(h, a.R, p(a.bad_last), 0, p(a.i32[0]), None), RANGE),
        ("trees -1 last", "fw32", lambda L, h, a: L.tnco_hip_get_trees(h, a.R, p(a.neg_last), 0, p(a.i32[0]), None), RANGE),
        # PRNG states
        ("prng null", "plain", lambda L, h, a: L.tnco_hip_get_prng(None, 0, p(a.out)), NULLA),
        ("prng no out", "plain", lambda L, h, a: L.tnco_hip_get_prng(h, 0, None), NULLA),
        ("prng no out before r", "plain", lambda L, h, a: L.tnco_hip_get_prng(h, -1, None), NULLA),
        ("prng r -1", "plain", lambda L, h, a: L.tnco_hip_get_prng(h, -1, p(a.out)), RANGE),
        ("prng r R", "plain", lambda L, h, a: L.tnco_hip_get_prng(h, a.R, p(a.out)), RANGE),
        ("set_prng null", "plain", lambda L, h, a: L.tnco_hip_set_prng(None, 0, p(a.st)), NULLA),
        ("set_prng no in", "plain", lambda L, h, a: L.tnco_hip_set_prng(h, 0, None), NULLA),
        ("set_prng r -1", "plain", lambda L, h, a: L.tnco_hip_set_prng(h, -1, p(a.st)), RANGE),
        ("set_prng r R", "plain", lambda L, h, a: L.tnco_hip_set_prng(h, a.R, p(a.st)), RANGE),
        ("set_prng position", "plain", lambda L, h, a: L.tnco_hip_set_prng(h, 0, p(a.st_bad)), POS),
        ("set_prng r before position", "plain", lambda L, h, a: L.tnco_hip_set_prng(h, a.R, p(a.st_bad)), RANGE),
        ("prng_many null", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(None, 1, p(a.ids), p(a.out)), NULLA),
        ("prng_many no out", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, 1, p(a.ids), None), NULLA),
        ("prng_many no out before k", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, a.R + 1, None, None), NULLA),
        ("prng_many k < 0", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, -1, p(a.ids), p(a.out)), KBAD),
        ("prng_many k > R", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, a.R + 1, None, p(a.out)), KBAD),
        ("prng_many bad first", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, a.R, p(a.bad_first), p(a.out)), RANGE),
        ("prng_many bad last", "plain", lambda L, h, a: L.tnco_hip_get_prng_many(h, a.R, p(a.bad_last), p(a.out)), RANGE),
        ("prng_many -1 last", "fw32", lambda L, h, a: L.tnco_hip_get_prng_many(h, a.R, p(a.neg_last), p(a.out)), RANGE),
        ("set_prng_many null", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(None, 1, p(a.ids), p(a.st)), NULLA),
        ("set_prng_many no in", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, 1, p(a.ids), None), NULLA),
        ("set_prng_many k < 0", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, -1, p(a.ids), p(a.st)), KBAD),
        ("set_prng_many k > R", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R + 1, None, p(a.st)), KBAD),
        ("set_prng_many bad first", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, p(a.bad_first), p(a.st)), RANGE),
        ("set_prng_many bad last", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, p(a.bad_last), p(a.st)), RANGE),
        ("set_prng_many position first", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, p(a.ids), p(a.st_bad)), POS),
        ("set_prng_many position last", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, None, p(a.st_bad_last)), POS),
        # (row by row: the id of a row, then its position, then the next row)
        ("set_prng_many id 0 before position 0", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, p(a.bad_first), p(a.st_bad)), RANGE),
        ("set_prng_many position 0 before last id", "plain", lambda L, h, a: L.tnco_hip_set_prng_many(h, a.R, p(a.bad_last), p(a.st_bad)), POS),
        # best, min_cost_device
        ("best null", "plain", lambda L, h, a: L.tnco_hip_best(None, 1, p(a.f64), p(a.i64)), NULLH),
        ("best k < 0", "plain", lambda L, h, a: L.tnco_hip_best(h, -1, p(a.f64), p(a.i64)), "'k' out of range."),
        ("best k R + 1", "plain", lambda L, h, a: L.tnco_hip_best(h, a.R + 1, p(a.f64), p(a.i64)), "'k' out of range."),
        ("best k R + 1, fw", "fw32", lambda L, h, a: L.tnco_hip_best(h, a.R + 1, p(a.f64), p(a.i64)), "'k' out of range."),
        ("min_cost_device null", "plain", lambda L, h, a: L.tnco_hip_min_cost_device(None, p(a.f64)), NULLA),
        ("min_cost_device no dst", "plain", lambda L, h, a: L.tnco_hip_min_cost_device(h, None), NULLA),
        # counters
        ("counters null", "plain", lambda L, h, a: L.tnco_hip_diag_counters(None, u(a.prev), None, None, None), NULLH),
        ("full_copies null", "plain", lambda L, h, a: L.tnco_hip_diag_full_copies(None, u(a.prev)), NULLA),
        ("full_copies no out", "plain", lambda L, h, a: L.tnco_hip_diag_full_copies(h, None), NULLA),
        ("stage_cycles null", "plain", lambda L, h, a: L.tnco_hip_diag_stage_cycles(None, p(a.u64)), NULLA),
        ("stage_cycles no out", "plain", lambda L, h, a: L.tnco_hip_diag_stage_cycles(h, None), NULLA),
        ("moves null", "plain", lambda L, h, a: L.tnco_hip_diag_moves(None, p(a.u64)), NULLA),
        ("moves no out", "plain", lambda L, h, a: L.tnco_hip_diag_moves(h, None), NULLA),
        # tnco_hip_diag_poke: fields 0 parent, 1 swap_children, 2 legs, 3 ccost, 4 partial, 5 / 6 partial_left / _right,
        # 7 total, 8 min_cost, 9 jmin, 10 slices, 11 min_slices, 12 width
        ("poke null", "plain", lambda L, h, a: _poke(L, None, a, 0, 8), NULLH),
        ("poke r -1", "plain", lambda L, h, a: _poke(L, h, a, -1, 8), RANGE),
        ("poke r R", "plain", lambda L, h, a: _poke(L, h, a, a.R, 8, write=1, value=7), RANGE),
        ("poke r before field", "plain", lambda L, h, a: _poke(L, h, a, a.R, 99), RANGE),
        ("poke unknown field", "plain", lambda L, h, a: _poke(L, h, a, 0, 13), "unknown 'field'."),
        ("poke field -1", "plain", lambda L, h, a: _poke(L, h, a, 0, -1), "unknown 'field'."),
        ("poke parent node -1", "plain", lambda L, h, a: _poke(L, h, a, 0, 0, node=-1), "'node' out of range."),
        ("poke parent node N", "plain", lambda L, h, a: _poke(L, h, a, 0, 0, node=a.N, write=1, value=a.n), "'node' out of range."),
        ("poke parent a leaf", "plain", lambda L, h, a: _poke(L, h, a, 0, 0, node=a.n, write=1, value=a.n - 1), "a parent must be an internal node."),
        ("poke parent N", "plain", lambda L, h, a: _poke(L, h, a, 0, 0, node=0, write=1, value=a.N), "a parent must be an internal node."),
        ("poke parent -1 below the root", "plain", lambda L, h, a: _poke(L, h, a, 0, 0, node=a.n, write=1, value=-1), "a parent must be an internal node."),
        ("poke swap a leaf", "plain", lambda L, h, a: _poke(L, h, a, 0, 1, node=a.n - 1, write=1), NOTINT),
        ("poke swap N", "plain", lambda L, h, a: _poke(L, h, a, 0, 1, node=a.N, write=1), NOTINT),
        ("poke legs a leaf", "plain", lambda L, h, a: _poke(L, h, a, 0, 2, node=0), NOTINT),
        ("poke legs word W", "plain", lambda L, h, a: _poke(L, h, a, 0, 2, node=a.n, word=a.W, write=1, value=1), "'word' out of range."),
        ("poke legs word -1", "plain", lambda L, h, a: _poke(L, h, a, 0, 2, node=a.n, word=-1), "'word' out of range."),
        ("poke legs node before word", "plain", lambda L, h, a: _poke(L, h, a, 0, 2, node=0, word=-1), NOTINT),
        ("poke ccost, child partials", "plain", lambda L, h, a: _poke(L, h, a, 0, 3, node=a.n), "the child-partial layout stores neither 'ccost' nor 'partial' of a node."),
        ("poke partial, child partials, a leaf", "plain", lambda L, h, a: _poke(L, h, a, 0, 4, node=0), "the child-partial layout stores neither 'ccost' nor 'partial' of a node."),
        ("poke ccost a leaf", "hyper", lambda L, h, a: _poke(L, h, a, 0, 3, node=a.n - 1), NOTINT),
        ("poke partial a leaf", "fw32", lambda L, h, a: _poke(L, h, a, 0, 4, node=a.N, write=1), NOTINT),
        ("poke partial_left, unified", "hyper", lambda L, h, a: _poke(L, h, a, 0, 5, node=a.n), "only the child-partial layout stores the partial costs of a node's children."),
        ("poke partial_right, split, a leaf", "fw32", lambda L, h, a: _poke(L, h, a, 0, 6, node=0), "only the child-partial layout stores the partial costs of a node's children."),
        ("poke partial_left a leaf", "plain", lambda L, h, a: _poke(L, h, a, 0, 5, node=a.n - 1), NOTINT),
        ("poke partial_right N", "plain", lambda L, h, a: _poke(L, h, a, 0, 6, node=a.N, write=1), NOTINT),
        ("poke total, unified", "hyper", lambda L, h, a: _poke(L, h, a, 0, 7), "only the child-partial layout keeps the root's partial cost in the replica record."),
        ("poke total, split", "fw32", lambda L, h, a: _poke(L, h, a, 0, 7, write=1), "only the child-partial layout keeps the root's partial cost in the replica record."),
        ("poke jmin beyond", "plain", lambda L, h, a: _poke(L, h, a, 0, 9, write=1, value=1 << 30), "'jmin' beyond the rotations the journal holds."),
        ("poke slices plain", "plain", lambda L, h, a: _poke(L, h, a, 0, 10), NOFW),
        ("poke min_slices plain, word", "plain", lambda L, h, a: _poke(L, h, a, 0, 11, word=-1), NOFW),
        ("poke slices word W", "fw32", lambda L, h, a: _poke(L, h, a, 0, 10, word=a.W, write=1, value=1), "'word' out of range."),
        ("poke min_slices word -1", "fw32", lambda L, h, a: _poke(L, h, a, 0, 11, word=-1), "'word' out of range."),
        ("poke width plain", "plain", lambda L, h, a: _poke(L, h, a, 0, 12, node=a.n), NOFW),
        ("poke width plain before node", "hyper", lambda L, h, a: _poke(L, h, a, 0, 12, node=0), NOFW),
        ("poke width a leaf", "fw32", lambda L, h, a: _poke(L, h, a, 0, 12, node=a.n - 1), NOTINT),
        ("poke width a leaf, float64", "fw64", lambda L, h, a: _poke(L, h, a, 0, 12, node=a.N, write=1), NOTINT),
    ]
    return rows


ROWS = _rows()


@pytest.mark.parametrize("kind", ["plain", "hyper", "fw32", "fw64"])
def test_refusals_status_text_and_nothing_written(core, batches, kind):
    gpu = batches(kind)
    L, h = gpu._L, gpu._h
    a = _Scratch(gpu)
    before = _state(gpu)
    rows = [r for r in ROWS if r[1] == kind]
    assert rows
    for name, _kind, call, text in rows:
        rc = call(L, h, a)
        got = L.tnco_hip_last_error().decode()
        assert (rc, got) == (EINVAL, text), f"{name}: status {rc}, '{got}'"
        assert _same(before, _state(gpu)), f"{name}: the refused call changed the state"
    # no handle, no error: the two getters that return a number
    assert L.tnco_hip_diag_launch_groups(None) == 0 and L.tnco_hip_diag_device_bytes(None) == 0
    assert gpu.validate() == (0, -1)


def test_what_is_no_refusal(core, batches):
    """Calls next to the refusals that succeed and do nothing: no sweeps, no outputs, an empty list -- and tnco_hip_get_tree,
    which takes every `which` but 0 as the best tree (tnco_hip_get_trees refuses 2)."""
    for kind in ("plain", "fw32"):
        gpu = batches(kind)
        L, h = gpu._L, gpu._h
        a = _Scratch(gpu)
        before = _state(gpu)
        p = _ptr
        calls = [lambda: L.tnco_hip_run(h, 2, None, 0), lambda: L.tnco_hip_get_costs(h, None, None),
                 lambda: L.tnco_hip_get_trees(h, 0, None, 1, None, None), lambda: L.tnco_hip_best(h, 0, None, None),
                 lambda: L.tnco_hip_get_prng_many(h, 0, None, None), lambda: L.tnco_hip_set_prng_many(h, 0, None, None),
                 lambda: L.tnco_hip_get_caches(h, 0, None, None, None)]
        if kind == "fw32":
            calls = calls[1:] + [lambda: L.tnco_hip_run_fw(h, 2, None, 0, 10, 0), lambda: L.tnco_hip_get_slices_many(h, 0, None, None, None),
                                 lambda: L.tnco_hip_get_slices_many(h, 1, p(a.ids), None, None), lambda: L.tnco_hip_get_slices(h, 0, None, None)]
        for i, c in enumerate(calls):
            assert c() == 0, (kind, i)
        assert _same(before, _state(gpu))
        best = gpu.tree(3, which_min=True)
        l, r, q = (np.empty(gpu.n_nodes, np.int32) for _ in range(3))
        assert L.tnco_hip_get_tree(h, 3, 2, p(l), p(r), p(q), None) == 0
        assert all(np.array_equal(x, y) for x, y in zip((l, r, q), best[:3]))


# ---------------------------------------------------------------------------------------------------------------------
# siblings
# ---------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64) if x.dtype == np.float64 else x


def _assert_siblings(gpu, picks):
    """One replica / a list of one / the whole batch: the same bits.  `picks`: the replicas compared one by one."""
    R, N, root = gpu.n_replicas, gpu.n_nodes, gpu.n_nodes - 1
    everyone = np.arange(R)
    tot, mn = gpu.costs()
    states = gpu.prng_states()
    assert states.shape == (R, 625)
    assert (states[picks, 624] < 624).any(), "no picked replica in the middle of an mt19937 block"
    some = gpu.prng_states(picks)
    if gpu.finite_width:
        all_s, all_m = gpu.slices_many(everyone)
    cur_all = {w: gpu.trees(picks, which_min=w) for w in (False, True)}
    for j, r in enumerate(picks):
        one = gpu.prng_state(r)
        assert np.array_equal(one, gpu.prng_states([r])[0]) and np.array_equal(one, states[r]) and np.array_equal(one, some[j]), f"prng {r}"
        for w in (False, True):
            l, rr, p, _m = gpu.tree(r, which_min=w)
            links, con = gpu.trees([r], which_min=w)
            assert np.array_equal(np.stack([l, rr, p]), links[0]), f"tree {r} which={w}"
            assert np.array_equal(links[0], cur_all[w][0][j]) and np.array_equal(con[0], cur_all[w][1][j]), f"trees {r} which={w}"
        cc, pc, hy = gpu.caches(r)
        assert _bits(pc)[root] == _bits(tot)[r], f"total cost {r}: caches {pc[root]!r}, costs {tot[r]!r}"
        if gpu.finite_width:
            s, m = gpu.slices(r)
            s1, m1 = gpu.slices_many([r])
            assert np.array_equal(s, s1[0]) and np.array_equal(m, m1[0]), f"slices {r}"
            assert np.array_equal(s, all_s[r]) and np.array_equal(m, all_m[r]), f"slices {r} of all"
    order = np.lexsort((everyone, mn))  # ascending cost, ties by replica number
    for k in sorted({1, min(4, R), min(R, TOPK_HOST), R}):
        c, ids = gpu.best(k)
        assert np.array_equal(ids, order[:k]) and np.array_equal(_bits(c), _bits(mn[order[:k]])), f"best({k})"
    assert gpu.counters()["moves"] == int(gpu.moves_per_replica().sum())
    assert gpu.moves_per_replica().shape == (R,) and (gpu.moves_per_replica() > 0).all()


@pytest.mark.parametrize("kind", ["plain", "hyper", "fw32", "fw64", "restored"])
def test_sibling_getters_agree(core, batches, kind):
    gpu = batches(kind)
    R = gpu.n_replicas
    _assert_siblings(gpu, list(range(0, R, 3)) + [R - 1])
    if kind == "hyper":  # the unified layout stores ccost / partial, and the hyper cache is the stored legs'
        cc, pc, hy = gpu.caches(1)
        l, r, _p, m = gpu.tree(1)
        n = gpu.n_leaves
        assert hy[n:].any() and not hy[:n].any()
        assert np.array_equal(hy[n:], m[n:] & m[l[n:]] & m[r[n:]])
        assert cc[n:].all() and pc[gpu.n_nodes - 1] == gpu._poke(1, "partial", node=gpu.n_nodes - 1)
        assert cc[n] == gpu._poke(1, "ccost", node=n)
    assert gpu.validate() == (0, -1)


@pytest.mark.parametrize("kind", ["plain", "fw32"])
def test_prng_setters_agree(core, batches, kind):
    """set_prng_state against set_prng_states with and without ids, each read back by both getters."""
    gpu = batches(kind)
    R = gpu.n_replicas
    orig = gpu.prng_states()
    before = _state(gpu)
    try:
        a = np.roll(orig, 1, axis=0)
        gpu.set_prng_states(a)
        assert np.array_equal(gpu.prng_states(), a) and all(np.array_equal(gpu.prng_state(r), a[r]) for r in range(R))
        ids = np.array([R - 1, 0, 5, 4])
        b = np.roll(orig, 2, axis=0)
        gpu.set_prng_states(b[ids], ids)
        want = a.copy()
        want[ids] = b[ids]
        assert np.array_equal(gpu.prng_states(), want) and np.array_equal(gpu.prng_states(ids), b[ids])
        assert all(np.array_equal(gpu.prng_state(r), want[r]) for r in range(R))
        gpu.set_prng_states(b[:3])  # (ids = NULL, k < R: replicas 0 .. k-1)
        want[:3] = b[:3]
        assert np.array_equal(gpu.prng_states(), want)
        c = np.roll(orig, 3, axis=0)
        for r in (0, 7, R - 1):
            gpu.set_prng_state(r, c[r])
            want[r] = c[r]
            assert np.array_equal(gpu.prng_state(r), c[r])
        assert np.array_equal(gpu.prng_states(), want) and np.array_equal(gpu.prng_states(np.arange(R)), want)
    finally:
        gpu.set_prng_states(orig)
    assert _same(before, _state(gpu))


def test_best_on_the_device_and_on_the_host(core):
    """More replicas than TOPK_CHUNK / 2: best(k) selects on the device up to that k and sorts on the host beyond it; both
    are the host's argsort with ties broken by the replica number (16 leaves: many replicas share a best cost)."""
    prob = H.regular_problem(16, graph_seed=3)
    R = TOPK_HOST + 64
    seeds = H.replica_seeds(R, S=9)
    with core.BatchedOptimizer(prob.leaf_masks, prob.links(seeds), seeds, n_inds=prob.n_inds) as gpu:
        gpu.run(BETAS)
        assert not gpu.finite_width and gpu.launch_groups == 0
        tot, mn = gpu.costs()
        assert len(np.unique(mn)) < R, "no ties to break"
        order = np.lexsort((np.arange(R), mn))
        for k in (1, 5, TOPK_HOST, TOPK_HOST + 1, R):
            c, ids = gpu.best(k)
            assert np.array_equal(ids, order[:k]) and np.array_equal(c.view(np.uint64), mn[order[:k]].view(np.uint64)), f"best({k})"
        root = gpu.n_nodes - 1
        for r in (0, R // 2, R - 1):
            assert gpu.caches(r)[1][root] == tot[r]
        assert gpu.counters()["moves"] == int(gpu.moves_per_replica().sum())


TWO_STREAMS = {
    "80 x 16385, TNCO_HIP_GROUPS=2": (80, 11, 16385, {}, {"TNCO_HIP_GROUPS": "2"}),
    "fw 40 x 8200": (40, 8, 8200, dict(max_width=5), {}),
}


@pytest.mark.parametrize("shape", list(TWO_STREAMS))
def test_two_streams_read_without_a_sync(core, monkeypatch, shape):
    """The getters join the group streams themselves: run() returns with kernels in flight on two streams, and the first
    call after it is a getter.  16 replicas against their siblings, first and last block included."""
    n, gs, R, kw, env = TWO_STREAMS[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = H.regular_problem(n, graph_seed=gs)
    seeds = H.replica_seeds(R, S=5)
    with core.BatchedOptimizer(prob.leaf_masks, prob.links(seeds), seeds, n_inds=prob.n_inds, **kw) as gpu:
        assert gpu.launch_groups == 2 and gpu.finite_width == bool(kw)
        picks = [int(x) for x in np.linspace(0, R - 1, 16)]
        for first in ("costs", "tree", "prng_states", "trees", "best"):
            gpu.run(BETAS[:4])
            if first == "costs":
                tot, _mn = gpu.costs()
                assert tot[R - 1] == gpu.caches(R - 1)[1][gpu.n_nodes - 1]
            elif first == "tree":
                t = gpu.tree(R - 1)
                assert np.array_equal(np.stack(t[:3]), gpu.trees([R - 1], which_min=False)[0][0])
            elif first == "prng_states":
                s = gpu.prng_states()
                assert np.array_equal(s[R - 1], gpu.prng_state(R - 1))
            elif first == "trees":
                t = gpu.trees([R - 1], which_min=True)[0][0]
                assert np.array_equal(t, np.stack(gpu.tree(R - 1, which_min=True)[:3]))
            else:
                c, ids = gpu.best(4)
                assert np.array_equal(c, gpu.costs()[1][ids])
        _assert_siblings(gpu, picks)
        assert gpu.validate() == (0, -1)
