"""The checker checked: tnco_hip_validate (build_kernel, compare_kernel, fw_check_kernel, materialize_min_kernel and the
host loop that chunks the replicas and merges the verdicts) must say "bad" for every kind of damaged replica state, count
the bad replicas exactly and name the smallest one -- in every lane layout the library dispatches, the three node layouts,
finite width, and across the seams of its staging chunks.

Every case: build a handle, run a few sweeps, validate() == (0, -1); damage single fields of chosen replicas through
BatchedOptimizer._poke (tnco_hip_diag_poke: host copies, links stay a tree); read the damaged replicas back through the
getters; the expected (n_bad, first_bad) comes from tests/validate_cases.py, a plain restatement of the reference's
is_valid that tests/test_validate_model.py holds to the oracle; validate(atol) must return exactly that; the old values
go back and validate() == (0, -1) again.  Where the direction is known in advance (a cost off by exp(2 atol) is bad, by
exp(atol / 2) it is not) the test asserts it of the restatement too.

Lane layouts: the validator's kernels are instantiated for 4 x 1 ... 4 x 4, 8 x 3, 8 x 4, 16 x 3, 16 x 4 lanes x words
(networks of one or two mask words run as 4 x 1; there is no 1 x 1 or 2 x 1 instantiation of these kernels)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import validate_cases as V
from tnco_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


def _lanes(W):
    """Lanes that own a replica (W <= 16 -> 4, <= 32 -> 8, <= 64 -> 16); a block has 256 threads."""
    return 4 if W <= 16 else 8 if W <= 32 else 16


def _model(prob, **kw):
    return V.Model(prob.leaf_masks, prob.n_inds, dims=prob.dims, output_mask=prob.output_mask, sparse_mask=prob.sparse_mask, **kw)


def _scale(f):
    return lambda old: old * f


def _out(f):
    """Scaled out of the tolerance; the 0 a leaf child's slot holds becomes 1."""
    return lambda old: old * f if old != 0 else 1.0


def _const(v):
    return lambda old: v


def _flip(bit):
    return lambda old: old ^ (1 << bit)


def _case(gpu, model, damage, atol=1e-5, layout=None, bad=None, note=""):
    """damage: [(replica, field, dict(node=, word=), new value from old)].  Applies it, takes the expected verdicts of
    the damaged replicas from the restatement, asserts validate(atol), restores, asserts a clean validate().  `bad`: the
    replicas that MUST be the bad ones whatever the restatement says (None: the restatement decides).  Returns them."""
    undo = []
    try:
        for r, field, kw, fn in damage:
            if field == "swap_children":
                gpu._poke(r, field, **kw)
                undo.append((r, field, kw, None))
            else:
                old = gpu._poke(r, field, **kw)
                undo.append((r, field, kw, old))
                gpu._poke(r, field, fn(old), **kw)
        touched = sorted({d[0] for d in damage})
        ok = V.verdicts(model, [V.gpu_state(gpu, r, layout) for r in touched], atol)
        want = [r for r, v in zip(touched, ok) if not v]
        got = gpu.validate(atol)
        print(f"validate {note} atol={atol}: got {got}, restatement {V.expected_validate(want)}, bad replicas {want}")
        assert got == V.expected_validate(want), f"{note}: validate() {got}, restatement says {want}"
        if bad is not None:
            assert want == sorted(bad), f"{note}: the restatement's bad replicas {want}, required {sorted(bad)}"
    finally:
        for r, field, kw, old in reversed(undo):
            gpu._poke(r, field, old, **kw)
    assert gpu.validate(atol) == (0, -1), f"{note}: not clean after the restore"
    return want


def _pool(R, gpb):
    """Distinct replicas: first and last lane group of the first block, the block seam, the middle, the first and the last
    replica of the last, partly filled block."""
    assert R % gpb != 0 and R > 4 * gpb
    last0 = R // gpb * gpb
    head = [0, gpb - 1, gpb, 2 * gpb - 1, last0 - 1, last0, R - 2, R - 1, R // 2]
    rest = [x for x in range(3 * gpb + 1, R, max(1, R // 97)) if x not in head]
    return head + rest


def _other_internal(parent, x, n):
    """An internal node that is not x's parent (nor x)."""
    return next(c for c in range(n, len(parent)) if c != parent[x] and c != x)


def _partial_field(layout, gpu, r, node):
    """The field that holds a partial cost in node's header: under child partials the slot of an internal child if it
    has one (its own partial cost lives in its parent)."""
    if layout != "child-partial":
        return "partial"
    l, _, _, _ = gpu.tree(r, with_masks=False)
    return "partial_left" if l[node] >= gpu.n_leaves else "partial_right"


def _legs_and_links(gpu, model, layout, prob, replicas, note):
    """A leg bit in word 0 and the highest index of the network (last used word), the parent of a leaf and of an internal
    node, each in a replica of its own: all bad, in whatever layout the handle keeps its nodes."""
    n, N, W = prob.n, 2 * prob.n - 1, prob.W
    r_w0, r_wl, r_leaf, r_int = replicas
    hi = prob.n_inds - 1
    assert hi // 64 == W - 1
    leaf, inner = n - 1, n + 5
    damage = [(r_w0, "legs", dict(node=n + 1, word=0), _flip(0)),
              (r_wl, "legs", dict(node=N - 2, word=W - 1), _flip(hi % 64)),
              (r_leaf, "parent", dict(node=leaf), _const(_other_internal(gpu.tree(r_leaf, with_masks=False)[2], leaf, n))),
              (r_int, "parent", dict(node=inner), _const(_other_internal(gpu.tree(r_int, with_masks=False)[2], inner, n)))]
    _case(gpu, model, damage, 1e-5, layout, bad=list(replicas), note=note)


LANE_CASES = [(130, 3, 12300), (200, 4, 12300), (512, 3, 12300), (600, 3, 12300), (900, 3, 8200), (1300, 3, 8200),
              (2048, 3, 4100), (2600, 3, 1500)]


@pytest.mark.parametrize("n,deg,R", LANE_CASES)
def test_every_lane_layout_sees_damage_wherever_it_sits(core, n, deg, R):
    """4 x 1, 4 x 2, 4 x 3, 4 x 4, 8 x 3, 8 x 4, 16 x 3, 16 x 4 (4, 7, 12, 15, 22, 31, 48, 61 mask words), child-partial
    layout, batches of full wavefronts.  Damaged: the header of a node of every residue i mod L (the lanes of a replica
    share the nodes out that way), the first internal node, the root, the last node below it; a leg bit in word 0 and the
    highest index of the network (last used word); the root total; min_cost; the parents of a leaf, an internal node and
    the root; exchanged children -- each in a replica of its own: first / last lane group of a block, the seam of two
    blocks, the last, partly filled block, R - 1."""
    prob = H.regular_problem(n, graph_seed=n % 89, degree=deg)
    L = _lanes(prob.W)
    gpb = 256 // L
    seeds = H.replica_seeds(R, S=n)
    links = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds)
    model = _model(prob)
    N, W, atol = 2 * n - 1, prob.W, 1e-5
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        gpu.run(H.linear_betas(0, 60, 6))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        assert layout == "child-partial"
        for f in ("ccost", "partial", "slices", "min_slices", "width"):  # (fields this layout does not store)
            with pytest.raises(ValueError):
                gpu._poke(0, f, node=n)
        pool = iter(_pool(R, gpb))
        nodes = [n + j for j in range(L)] + [N - 2, N - 1]
        costs = []
        for node in nodes:
            r = next(pool)
            costs.append((r, _partial_field(layout, gpu, r, node), dict(node=node)))
        r_tot, r_min = next(pool), next(pool)
        costs += [(r_tot, "total", {}), (r_min, "min_cost", {})]
        # inside the tolerance: nobody is bad
        _case(gpu, model, [(r, f, kw, _scale(np.exp(0.5 * atol))) for r, f, kw in costs], atol, layout, bad=[], note="x exp(atol/2)")
        # outside: every one of them
        _case(gpu, model, [(r, f, kw, _out(np.exp(2 * atol))) for r, f, kw in costs], atol, layout,
              bad=[r for r, _, _ in costs], note="x exp(2 atol)")
        # legs and links
        r_w0, r_wl, r_leaf, r_int, r_root, r_swap = (next(pool) for _ in range(6))
        hi = prob.n_inds - 1
        assert hi // 64 == W - 1
        par = gpu.tree(r_leaf, with_masks=False)[2]
        leaf = n - 1
        par_i = gpu.tree(r_int, with_masks=False)[2]
        inner = n + L + 1
        l_s, r_s, _, _ = gpu.tree(r_swap, with_masks=False)
        swap_node = next(x for x in range(N - 1, n - 1, -1) if l_s[x] >= n and r_s[x] >= n)
        damage = [(r_w0, "legs", dict(node=n + 1, word=0), _flip(0)),
                  (r_wl, "legs", dict(node=N - 2, word=W - 1), _flip(hi % 64)),
                  (r_leaf, "parent", dict(node=leaf), _const(_other_internal(par, leaf, n))),
                  (r_int, "parent", dict(node=inner), _const(_other_internal(par_i, inner, n))),
                  (r_root, "parent", dict(node=N - 1), _const(n)),
                  (r_swap, "swap_children", dict(node=swap_node), None)]
        want = _case(gpu, model, damage, atol, layout, note="legs and links")
        assert set(want) >= {r_w0, r_wl, r_leaf, r_int, r_root}
        # (exchanged children under child partials: bad exactly where the two slots differ)
        pl, pr = gpu._poke(r_swap, "partial_left", node=swap_node), gpu._poke(r_swap, "partial_right", node=swap_node)
        assert (r_swap in want) == (not V.is_logclose(pl, pr, atol))


def _layout_problem(kind):
    if kind.startswith("hyper"):
        ts, _dims, out = syn.random_hyper_tn(120, 200, k=3, n_output=5, seed=12)
        return H.Problem(ts, 2, out), {}
    prob = H.regular_problem(128, graph_seed=5)
    if kind == "dims 3":
        return H.Problem(prob.ts_inds, 3, []), {}
    return prob, (dict(cost_type="float32") if kind == "float32" else {})


@pytest.mark.parametrize("kind", ["child-partial", "hyper", "dims 3", "float32"])
def test_every_cost_field_both_directions_two_tolerances(core, kind):
    """Child-partial layout (plain dims 2) and the unified layout (hyper-indices; dims 3; float32 cost): every cost field
    scaled by exp(atol / 2) stays valid and by exp(2 atol) does not, at atol 1e-5 and 1e-3; sign flipped, inf and NaN are
    bad; an exact zero is what is_logclose makes of it.  Fields the layout does not store are refused."""
    prob, kw = _layout_problem(kind)
    n, N, R = prob.n, 2 * prob.n - 1, 3000
    seeds = H.replica_seeds(R, S=77)
    links = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds)
    model = _model(prob, **kw)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims, output_mask=prob.output_mask,
                               **kw) as gpu:
        gpu.run(H.linear_betas(0, 40, 8))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        assert layout == ("child-partial" if kind == "child-partial" else "unified")
        refused = ("ccost", "partial") if layout == "child-partial" else ("partial_left", "partial_right", "total")
        for f in refused + ("slices", "min_slices", "width"):
            with pytest.raises(ValueError):
                gpu._poke(5, f, node=n + 2)
        for args in (dict(node=N), dict(node=n - 1), dict(node=-1)):  # (not an internal node)
            with pytest.raises(ValueError):
                gpu._poke(5, "legs", **args)
        for bad_call in (lambda: gpu._poke(R, "min_cost"), lambda: gpu._poke(-1, "min_cost"),
                         lambda: gpu._poke(5, "legs", node=n, word=prob.W), lambda: gpu._poke(5, "parent", n - 1, node=n),
                         lambda: gpu._poke(5, "parent", N, node=0), lambda: gpu._poke(5, "parent", -1, node=n),
                         lambda: gpu._poke(5, "jmin", 1 << 30)):
            with pytest.raises(ValueError):
                bad_call()
        assert gpu.validate() == (0, -1)  # (nothing was written)
        if layout == "child-partial":
            fields = [("partial_left", N - 1), ("partial_right", N - 1), ("partial_left", N - 2), ("partial_right", N - 2),
                      ("total", 0), ("min_cost", 0)]
        else:
            fields = [("ccost", n), ("partial", n), ("ccost", N - 1), ("partial", N - 1), ("ccost", N - 2), ("partial", n + 9),
                      ("min_cost", 0)]
        where = []
        for k, (f, node) in enumerate(fields):
            r = 7 + 131 * k
            if f in ("partial_left", "partial_right"):  # (the slot of an INTERNAL child: a leaf's holds 0)
                links_r = gpu.tree(r, with_masks=False)
                node = next(x for x in range(node, n - 1, -1) if links_r[f == "partial_right"][x] >= n)
            where.append((r, f, dict(node=node) if node else {}))
        for atol in (1e-5, 1e-3):
            _case(gpu, model, [(r, f, a, _scale(np.exp(0.5 * atol))) for r, f, a in where], atol, layout, bad=[], note=f"{kind} up, inside")
            _case(gpu, model, [(r, f, a, _scale(np.exp(-0.5 * atol))) for r, f, a in where], atol, layout, bad=[], note=f"{kind} down, inside")
            _case(gpu, model, [(r, f, a, _scale(np.exp(2 * atol))) for r, f, a in where], atol, layout,
                  bad=[r for r, _, _ in where], note=f"{kind} up, outside")
            _case(gpu, model, [(r, f, a, _scale(np.exp(-2 * atol))) for r, f, a in where], atol, layout,
                  bad=[r for r, _, _ in where], note=f"{kind} down, outside")
        for name, v in (("sign", None), ("inf", np.inf), ("nan", np.nan)):
            fn = _scale(-1.0) if v is None else _const(v)
            _case(gpu, model, [(r, f, a, fn) for r, f, a in where], 1e-5, layout, bad=[r for r, _, _ in where], note=f"{kind} {name}")
        _case(gpu, model, [(r, f, a, _const(0.0)) for r, f, a in where], 1e-5, layout, note=f"{kind} zero")
        # a replica damaged twice counts once; exchanged children of the unified layout change nothing (caches per node)
        r2 = 1234
        twice = [(r2, "min_cost", {}, _scale(2.0)), (r2, where[0][1], where[0][2], _scale(2.0)), (R - 1, "min_cost", {}, _const(np.nan))]
        _case(gpu, model, twice, 1e-5, layout, bad=[r2, R - 1], note=f"{kind} twice")
        l, rr, _, _ = gpu.tree(99, with_masks=False)
        node = next(x for x in range(N - 1, n - 1, -1) if l[x] >= n and rr[x] >= n)
        want = _case(gpu, model, [(99, "swap_children", dict(node=node), None)], 1e-5, layout, note=f"{kind} exchanged children")
        if layout == "unified":
            assert want == []
        _legs_and_links(gpu, model, layout, prob, [0, 63, R - 2, R - 1], f"{kind} legs and links")


def test_best_tree_cost_and_journal_prefix(core):
    """min_cost and the best tree are checked against each other: a journal prefix shortened by a rotation gives another
    best tree -- bad where its cost differs from min_total_cost, still valid where it does not (the restatement prices the
    tree get_tree returns for the shortened prefix)."""
    prob = H.regular_problem(512, graph_seed=11)
    R = 6000
    seeds = H.replica_seeds(R, S=5)
    links = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds)
    model = _model(prob)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        gpu.run(H.linear_betas(5, 60, 12))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        cand = [r for r in list(range(0, 40)) + list(range(R - 40, R)) if gpu._poke(r, "jmin") > 0]
        assert len(cand) >= 8
        with pytest.raises(ValueError):  # beyond the rotations the journal holds
            gpu._poke(cand[0], "jmin", 1 << 20)
        cut1 = [(r, "jmin", {}, lambda old: old - 1) for r in cand[:6] + cand[-6:]]
        want = _case(gpu, model, cut1, 1e-5, layout, note="jmin - 1")
        cut0 = [(r, "jmin", {}, _const(0)) for r in cand[:6] + cand[-6:]]
        want0 = _case(gpu, model, cut0, 1e-5, layout, note="jmin = 0")
        assert want or want0, "no shortened journal changed the best tree's cost"
        print("best tree: unchanged cost after jmin - 1 in", sorted(set(c[0] for c in cut1) - set(want)))


def _fw_vec():
    ts, dims, out = syn.random_hyper_tn(28, 60, k=3, n_output=3, seed=7, dims_choices=(2, 3, 4, 6))
    return H.Problem(ts, np.array(dims, np.uint64), out)


FW_CASES = {
    "dims 2": (lambda: H.regular_problem(40, graph_seed=8), dict(max_width=6)),
    "dims 2, float64 widths": (lambda: H.regular_problem(40, graph_seed=8), dict(max_width=6, width_type="float64")),
    "per-index dims": (_fw_vec, dict(max_width=9.5)),
    "per-index dims, float64 widths": (_fw_vec, dict(max_width=9.5, width_type="float64")),
}


def _needed_slice(model, legs, slices):
    """(bit, node): a sliced index without which some tensor is wider than max_width, or None."""
    for i in sorted(range(model.N), key=lambda i: -V.width(model, legs[i] & ~slices)):
        for b in V.bits(legs[i] & slices):
            s2 = slices.copy()
            s2[b // 64] &= ~(np.uint64(1) << np.uint64(b % 64))
            if V.width(model, legs[i] & ~s2) > model.max_width:
                return b
    return None


@pytest.mark.parametrize("kind", list(FW_CASES))
def test_finite_width_checks_and_the_merge_of_verdicts(core, monkeypatch, kind):
    """Split layout.  A slice a widest tensor needs, dropped from `slices` (the current tree too wide, and its sliced costs
    wrong) and from `min_slices` (only the best tree too wide, its cost wrong); the width cache at +-atol/2 (valid) and
    +-2 atol, NaN (bad), float32 and float64 widths, uniform and per-index dims (the re-slice in one wavefront and the
    walk + full rebuild form); the cost cache; damage that only the finite-width check sees, damage that only the
    comparison sees, and both in one replica, which counts once; leg bits and parents in this layout's addressing."""
    wave = kind.startswith("dims 2")
    if wave:  # (the library leaves the one-wavefront form while many replicas fall back: pinned, as tests/test_gpu_fw.py does)
        monkeypatch.setenv("TNCO_HIP_FW_WAVE", "1")
    mk, fkw = FW_CASES[kind]
    prob = mk()
    n, N, R = prob.n, 2 * prob.n - 1, 700
    seeds = H.replica_seeds(R, S=21)
    links = prob.links(seeds)
    model = _model(prob, **fkw)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims, output_mask=prob.output_mask,
                               **fkw) as gpu:
        gpu.run(H.linear_betas(0, 40, 25), update_slices_every=10)
        assert gpu.validate() == (0, -1)
        st = gpu.fw_stats()  # which form of the re-slice ran (sweeps 0, 10 and 20 re-slice)
        if wave:
            assert st["repriced"] > 0 and st["full_rebuild_form"] == 0
            assert (gpu.reslice_info()[1] >= 0).any()  # (fw_wave_kernel left its change counts)
        else:
            assert st["repriced"] == 0 and st["full_rebuild_form"] > 0
            with pytest.raises(ValueError):
                gpu.reslice_info()  # (no re-pricing form for this cost model)
        layout = V.gpu_layout(gpu)
        assert layout == "split"
        _legs_and_links(gpu, model, layout, prob, [1, 63, 64, R - 3], f"{kind} legs and links")
        for f in ("partial_left", "partial_right", "total"):
            with pytest.raises(ValueError):
                gpu._poke(0, f, node=n)
        atol = 1e-5
        # width cache, both directions, every residue of the node index by four lanes, first and last internal node
        nodes = [n, n + 1, n + 2, n + 3, N - 2, N - 1]
        where = [(3 + 97 * k, "width", dict(node=x)) for k, x in enumerate(nodes)]
        for w_atol, sgn in [(1e-5, +1), (1e-5, -1), (1e-3, +1), (1e-3, -1)]:  # (a float32 width near 8 resolves 5e-7)
            _case(gpu, model, [(r, f, a, (lambda old, s=sgn: old + s * 0.5 * w_atol)) for r, f, a in where], w_atol, layout, bad=[],
                  note=f"{kind} width {sgn:+d} atol/2")
            _case(gpu, model, [(r, f, a, (lambda old, s=sgn: old + s * 2 * w_atol)) for r, f, a in where], w_atol, layout,
                  bad=[r for r, _, _ in where], note=f"{kind} width {sgn:+d} 2 atol")
        _case(gpu, model, [(r, f, a, _const(np.nan)) for r, f, a in where], atol, layout, bad=[r for r, _, _ in where], note=f"{kind} width NaN")
        # cost cache of the split layout
        cw = [(11, "ccost", dict(node=n)), (R - 1, "partial", dict(node=N - 1)), (R - 2, "ccost", dict(node=N - 2)), (500, "min_cost", {})]
        _case(gpu, model, [(r, f, a, _scale(np.exp(0.5 * atol))) for r, f, a in cw], atol, layout, bad=[], note=f"{kind} costs inside")
        _case(gpu, model, [(r, f, a, _scale(np.exp(2 * atol))) for r, f, a in cw], atol, layout, bad=[r for r, _, _ in cw], note=f"{kind} costs outside")
        # slices
        found = []
        for r in list(range(0, 60)) + list(range(R - 60, R)):
            legs = gpu.tree(r)[3]
            sl, msl = gpu.slices(r)
            b = _needed_slice(model, legs, sl)
            mlegs = gpu.tree(r, which_min=True)[3]
            mb = _needed_slice(model, mlegs, msl)
            if b is not None and mb is not None:
                found.append((r, b, mb))
            if len(found) >= 4:
                break
        assert len(found) >= 4, "no replica whose slices are all needed"
        (ra, ba, _), (rb, _, mbb), (rc, bc, _), (rd, _, mbd) = found
        drop = [(ra, "slices", dict(word=ba // 64), lambda old, b=ba: old & ~(1 << (b % 64))),
                (rb, "min_slices", dict(word=mbb // 64), lambda old, b=mbb: old & ~(1 << (b % 64)))]
        _case(gpu, model, drop, atol, layout, bad=[ra, rb], note=f"{kind} dropped slices")
        # ... and with min_cost set to what the best tree costs under the damaged min_slices: nothing but the width of
        # the best tree is wrong then, the current state is untouched
        ml, mr, _, mlegs = gpu.tree(rd, which_min=True)
        msl = gpu.slices(rd)[1].copy()
        msl[mbd // 64] &= ~(np.uint64(1) << np.uint64(mbd % 64))
        new_min = V.cost_cache(model, ml, mr, mlegs, V.traverse(ml, mr), msl)[2]
        only_w = [(rd, "min_slices", dict(word=mbd // 64), lambda old, b=mbd: old & ~(1 << (b % 64))), (rd, "min_cost", {}, _const(new_min))]
        _case(gpu, model, only_w, atol, layout, bad=[rd], note=f"{kind} best tree too wide, nothing else")
        # merge: only the width check (rc: width cache), only the comparison (rd: partial cost), both (ra), the best
        # tree's side only (rb); and a clean replica in between stays clean
        both = [(ra, "width", dict(node=n + 1), _const(1e3)), (ra, "partial", dict(node=N - 1), _scale(3.0)),
                (rc, "width", dict(node=N - 1), lambda old: old + 1.0),
                (rd, "partial", dict(node=n + 2), _scale(1.5)),
                (rb, "min_slices", dict(word=mbb // 64), lambda old, b=mbb: old & ~(1 << (b % 64)))]
        _case(gpu, model, both, atol, layout, bad=[ra, rb, rc, rd], note=f"{kind} merge")


def _spread_case(gpu, model, layout, picks, note):
    atol = 1e-5
    _case(gpu, model, [(r, "min_cost", {}, _scale(np.exp(2 * atol))) for r in picks], atol, layout, bad=list(picks), note=note)


def test_counts_across_staging_chunks(core):
    """2 048 leaves x 4 100 replicas: the node blocks alone are 3.5 GB, so the validator's 1 GiB of staging takes the batch
    in at least four chunks.  n_bad and first_bad (the smallest damaged replica) must be exact for one bad replica at the
    very end, for a spread over the whole batch, and for sets that begin in a later chunk."""
    n, R = 2048, 4100
    prob = H.regular_problem(n, graph_seed=n % 89)
    seeds = H.replica_seeds(R, S=n)
    links = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds)
    model = _model(prob)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        W = prob.W
        assert R * (n - 1) * ((32 + 8 * W + 31) // 32 * 32) >= 3 << 30  # (R (n - 1) BS, DESIGN section 2: >= 3 chunks of 1 GiB)
        gpu.run(H.linear_betas(0, 60, 4))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        _spread_case(gpu, model, layout, [R - 1], "last replica only")
        _spread_case(gpu, model, layout, [R - 300, R - 1], "last chunk only")
        spread = sorted({int(x) for x in np.linspace(0, R - 1, 30)})
        _spread_case(gpu, model, layout, spread, "spread")
        _spread_case(gpu, model, layout, spread[11:], "spread, from a later chunk")
        _spread_case(gpu, model, layout, spread[22:], "spread, the last quarter")
        # another kind of damage, seen by compare_kernel rather than the host's min_cost term, in later chunks
        N = 2 * n - 1
        dmg = [(r, _partial_field(layout, gpu, r, N - 1), dict(node=N - 1), _scale(2.0)) for r in (R // 2 + 1, R - 700, R - 2)]
        _case(gpu, model, dmg, 1e-5, layout, bad=[R // 2 + 1, R - 700, R - 2], note="partials in later chunks")


def test_counts_on_the_headline_shape(core):
    """512 leaves x 65 536 replicas (the benchmark's shape: ~4.3 GB of node blocks, several chunks)."""
    n, R = 512, 65536
    prob = H.regular_problem(n, graph_seed=11)
    seeds = H.replica_seeds(R, S=5)
    links = core.greedy_trees(prob.ts_inds, prob.n_inds, seeds, device=0, keep_on_device=True)
    model = _model(prob)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        gpu.run(H.linear_betas(0, 100, 5))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        _spread_case(gpu, model, layout, [R - 1], "last replica only")
        spread = sorted({int(x) for x in np.linspace(0, R - 1, 30)})
        _spread_case(gpu, model, layout, spread, "spread")
        _spread_case(gpu, model, layout, spread[11:], "spread, from a later chunk")
        N = 2 * n - 1
        dmg = [(r, "total", {}, _scale(1.0 + 1e-3)) for r in (R // 3, R - 64, R - 1)] + \
              [(40000, "legs", dict(node=N - 2, word=prob.W - 1), _flip((prob.n_inds - 1) % 64))]
        _case(gpu, model, dmg, 1e-5, layout, bad=[R // 3, 40000, R - 64, R - 1], note="totals and legs")
    core.greedy_release()


def test_the_first_nodes_of_a_tiny_tree(core):
    """Three leaves: the internal nodes are nodes 3 and 4, inside the first stride of the lanes' node loop."""
    prob = H.regular_problem(3, graph_seed=3, degree=2)
    R = 70
    seeds = H.replica_seeds(R, S=3)
    model = _model(prob)
    with core.BatchedOptimizer(prob.leaf_masks, prob.links(seeds), seeds, n_inds=prob.n_inds) as gpu:
        gpu.run(H.linear_betas(0, 80, 30))
        assert gpu.validate() == (0, -1)
        layout = V.gpu_layout(gpu)
        dmg = [(0, _partial_field(layout, gpu, 0, 3), dict(node=3), _out(2.0)), (R - 1, _partial_field(layout, gpu, R - 1, 4), dict(node=4), _out(2.0)),
               (33, "legs", dict(node=3, word=0), _flip(0))]
        _case(gpu, model, dmg, 1e-5, layout, bad=[0, 33, R - 1], note="three leaves")
