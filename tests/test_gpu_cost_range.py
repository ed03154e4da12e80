"""The annealing kernels where costs leave the cost type's range (tests/cost_range_cases.py): every sweep kernel of the
library -- the two LDS-resident kernels, the HBM sweep kernel in the child-partial layout (spread and in full
wavefronts), the general instantiations, both forms of the finite-width re-slice -- against the oracle, chunk by chunk,
on pairs of which some cross to +inf, some come back and some stay finite in the same wavefront; and the constructors
from both sides of the edge.

Costs are compared bit for bit, +inf included.  A NaN equals a NaN of any sign or payload (x86 and the GPU make different
default NaNs from inf - inf); a NaN on one side only fails.  Where a NaN can be stored at all, from oracle/tnco_oracle.c: a
contraction cost is pow() of positive numbers, a product of positive numbers, or such a product times min(., n_projs):
+inf at most; a partial sum adds non-negative costs; min_total_cost takes a total that compared less than it, which a NaN
never does; widths are finite.  Only the delta of a move and the running total of a walk can be NaN, and neither is
stored.  So no stored field can be NaN, and the comparison asserts that none is, on either side.
"""
import numpy as np
import pytest

from tests import cost_range_cases as C
from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = C.resolved()
CTORS = C.ctor_cases()
BEST = C.best_tree_cases()


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


def assert_costs_equal(got, want, what):
    """Bit for bit, except that a NaN equals any NaN."""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: a NaN on one side only"
    same = got.view(np.uint64) == want.view(np.uint64)
    assert np.all(same | gn), f"{what}: {got[~(same | gn)][:4]} != {want[~(same | gn)][:4]}"


def assert_replica_equal(gpu, r, o, fw):
    """helpers.assert_replica_equal with the cost comparison above, plus slices and best slices at finite width."""
    for which in (False, True):
        for name, g, w in zip(("left", "right", "parent", "legs"), gpu.tree(r, which_min=which), o.tree(which_min=which)):
            assert np.array_equal(g, w), f"replica {r} {name} (min={which})"
    cc, pc, hy = gpu.caches(r)
    occ, opc, ohy = o.caches()
    assert_costs_equal(cc, occ, f"replica {r} ccost")
    assert_costs_equal(pc, opc, f"replica {r} partial")
    assert not np.isnan(cc).any() and not np.isnan(pc).any(), f"replica {r}: a stored NaN"
    assert np.array_equal(hy, ohy), f"replica {r} hyper"
    assert np.array_equal(gpu.prng_state(r), o.prng_state()), f"replica {r} prng"
    if fw:
        for name, g, w in zip(("slices", "min_slices"), gpu.slices(r), o.slices()):
            assert np.array_equal(g, w), f"replica {r} {name}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cost_range(core, oracle_lib, monkeypatch, case):
    for k in ("TNCO_HIP_FW_WAVE", "TNCO_HIP_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    prob = C.problem(case)
    P = len(case.pairs)
    links, seeds, who = C.batch(case, prob, case.pairs)
    R = len(seeds)
    ids = C.checked_replicas(case, R, P)
    oracles = [C.make_oracle(oracle_lib, case, prob, links[k], case.pairs[k][1]) for k in range(P)]
    saw = dict(nonfinite=0, back=0, finite=0)
    was_bad = [False] * P
    ever_bad = [False] * P
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims, output_mask=prob.output_mask,
                               sparse_mask=prob.sparse_mask, **case.kw) as gpu:
        # the kernel the case names
        if case.resident:
            assert gpu.launch_groups == 0
        else:
            assert gpu.launch_groups >= 1
        done = 0
        for k in range(len(case.chunks)):
            gpu.run(case.betas(k), case.chunks[k][0], update_slices_every=case.every)
            for o in oracles:
                C.advance(o, case, k, done)
            done += len(case.betas(k))
            tot, mn = gpu.costs()
            moves = gpu.moves_per_replica()
            assert not np.isnan(tot).any() and not np.isnan(mn).any()
            for r in ids:
                o = oracles[who[r]]
                assert_replica_equal(gpu, r, o, case.fw)
                assert_costs_equal(tot[r], o.total_cost, f"replica {r} total after chunk {k}")
                assert_costs_equal(mn[r], o.min_total_cost, f"replica {r} best total after chunk {k}")
                assert int(moves[r]) == o.counters()["moves"], f"replica {r} moves after chunk {k}"
            for p, o in enumerate(oracles):  # (what the GPU just agreed with is the edge itself)
                bad = not np.isfinite(o.total_cost)
                saw["back"] += was_bad[p] and not bad
                was_bad[p] = bad
                ever_bad[p] |= C.state_flags(o)[0]
        saw["nonfinite"], saw["finite"] = sum(ever_bad), P - sum(ever_bad)
        assert saw["nonfinite"] == case.counts["crossed"] and saw["finite"] == case.counts["finite"] and saw["back"] >= 2
        # the end: the oracle's verdicts, the totals of the whole batch, the best of it
        verdicts = [o.is_valid() != 0 for o in oracles]
        assert [p for p, v in enumerate(verdicts) if v] == case.counts["invalid"]
        assert gpu.validate() == H.expected_validate([verdicts[p] for p in who])
        tot, mn = gpu.costs()
        assert_costs_equal(tot, np.array([o.total_cost for o in oracles])[who], "totals of the batch")
        assert_costs_equal(mn, np.array([o.min_total_cost for o in oracles])[who], "best totals of the batch")
        kbest = min(R, 16)
        c, bid = gpu.best(kbest)
        assert_costs_equal(c, np.sort(mn, kind="stable")[:kbest], "best(k)")
        assert np.array_equal(mn[bid], c) and len(set(bid.tolist())) == kbest
        if case.fw:
            st = gpu.fw_stats()
            if case.form is not None:  # (as tests/test_gpu_fw.py tells the pinned forms apart)
                wave = case.form == "wave"
                assert (st["repriced"] > 0) == wave and (st["full_rebuild_form"] > 0) == (not wave)
                if wave:  # (the change lists of the last re-slices were recorded: the walk-free form ran)
                    _how, nch = gpu.reslice_info()
                    assert (nch >= 0).any()
                else:  # (a handle pinned to the walk + full rebuild has no re-pricing to report on)
                    with pytest.raises(ValueError, match="no re-pricing re-slice"):
                        gpu.reslice_info()
            if case.cost_range:  # the re-pricing met a new exponent field >= 2047 and left the replica to the full rebuild
                assert st["fell_back"] >= st["cost_range"] > 0
    for o in oracles:
        o.close()


@pytest.mark.parametrize("variant", list(C.CTOR_VARIANTS))
@pytest.mark.parametrize("ctor", CTORS, ids=[c.name for c in CTORS])
def test_constructors_at_the_edge(core, oracle_lib, ctor, variant):
    """BatchedOptimizer constructs the batch exactly when the oracle constructs every tree of it (one replica over: the
    whole create is refused, as "Precision is too low."); a batch that constructs has the oracle's totals."""
    prob = ctor.problem()
    links = ctor.links(prob)
    kw = dict(C.CTOR_VARIANTS[variant], cost_type=ctor.cost_type)
    seeds = [7 + r for r in range(len(links))]
    oracles, refused = [], 0
    for r, (l, rr, p) in enumerate(links):
        okw = dict(kw, min_tree=(l, rr, p, prob.node_masks(l, rr))) if variant == "min_links" else kw
        try:
            oracles.append(oracle_lib.Oracle(l, rr, p, prob.node_masks(l, rr), n_inds=prob.n_inds, dims=prob.dims, seed=seeds[r], **okw))
        except ValueError as e:
            assert "Precision is too low" in str(e)
            refused += 1
    if variant != "fw_sliced":  # (with slices drawn the oracle alone decides; else the integer totals say the same)
        assert (refused == 0) == ctor.ok
    gkw = dict(kw, min_links=links) if variant == "min_links" else kw
    if refused:
        with pytest.raises(ValueError, match="Precision is too low"):
            core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims, **gkw)
        return
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims, **gkw) as gpu:
        tot, mn = gpu.costs()
        for r, o in enumerate(oracles):
            assert_replica_equal(gpu, r, o, variant.startswith("fw"))
            assert_costs_equal(tot[r], o.total_cost, f"replica {r} total")
            assert_costs_equal(mn[r], o.min_total_cost, f"replica {r} best total")
        assert np.isfinite(tot).all() and gpu.validate() == (0, -1)


@pytest.mark.parametrize("case", BEST, ids=[b.name for b in BEST])
def test_best_tree_at_the_edge(core, oracle_lib, case):
    """`min_links` (and `min_slices`) whose cost alone decides: the current tree constructs, so only the check of
    get_cost(min_ctree[, min_slices]) can refuse -- as the oracle does; a case that constructs has the oracle's best tree and
    best total."""
    prob = case.problem()
    cur, best = case.trees(prob)
    kw = dict(case.kw, cost_type=case.cost_type)
    args = (prob.leaf_masks, cur[None], [3])
    with core.BatchedOptimizer(*args, n_inds=prob.n_inds, dims=prob.dims, **kw) as alone:  # the current tree on its own
        assert alone.validate() == (0, -1)
    gkw = dict(kw, min_links=best[None], min_slices=case.min_slices_mask(prob))
    okw = dict(kw, min_tree=(best[0], best[1], best[2], prob.node_masks(best[0], best[1])), min_slices=case.min_slices_mask(prob))
    make = lambda: oracle_lib.Oracle(cur[0], cur[1], cur[2], prob.node_masks(cur[0], cur[1]), n_inds=prob.n_inds, dims=prob.dims,  # noqa: E731
                                     seed=3, **okw)
    if not case.ok:
        with pytest.raises(ValueError, match="Precision is too low"):
            make()
        with pytest.raises(ValueError, match="Precision is too low"):
            core.BatchedOptimizer(*args, n_inds=prob.n_inds, dims=prob.dims, **gkw)
        return
    o = make()
    with core.BatchedOptimizer(*args, n_inds=prob.n_inds, dims=prob.dims, **gkw) as gpu:
        tot, mn = gpu.costs()
        assert_replica_equal(gpu, 0, o, bool(case.kw))
        assert_costs_equal(tot[0], o.total_cost, "total")
        assert_costs_equal(mn[0], o.min_total_cost, "best total")
        assert np.isfinite(mn).all() and gpu.validate() == (0, -1)
