"""The child-partial node layout (plain handles: no hyper-indices, dims 2^k, infinite memory).

A node's header holds the partial costs of its two children, the root's own partial cost is kept with the replica and
the contraction cost is derived from the legs (sa_kernels.h).  get_caches(), validate(), costs() and the trees must give
what the oracle gives, bit for bit, at every mask width W = 1 ... 12 and beyond, through every kernel that reads or
writes the blocks: the sweep kernel, the LDS-resident kernels of a small batch, extraction, snapshot / restore.  Handles
with hyper-indices or a general cost model keep the layout with the node's own costs and must be unaffected."""
import numpy as np
import pytest

from tests import helpers as H
from tnco_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# 3-regular networks: 1.5 n indices -> W = 1, 2, ..., 12 mask words, and 22
SIZES = [8, 64, 120, 160, 200, 250, 290, 330, 380, 420, 460, 512, 900]


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


def _same_costs(gpu, rows, oracles):
    tot, mn = gpu.costs()
    for q, o in zip(rows, oracles):
        assert tot[q] == o.total_cost and mn[q] == o.min_total_cost, q


@pytest.mark.parametrize("n", SIZES)
def test_plain_layout_matches_oracle_through_every_kernel(core, oracle_lib, n):
    orc = oracle_lib
    prob = H.regular_problem(n, graph_seed=n % 89 + 1)
    assert prob.W == (1.5 * n + 63) // 64
    R = 2048
    seeds = H.replica_seeds(R, S=n)
    links = prob.links(seeds)
    b1, b2 = H.linear_betas(0, 60, 40), H.linear_betas(60, 100, 30)
    kw = dict(n_inds=prob.n_inds, dims=2)
    check = [0, R // 2 + 1, R - 1]
    oracles = [H.make_oracle(orc, prob, links[r], seeds[r]) for r in check]
    for o in oracles:
        o.run(orc.PROB_MH, b1)

    # the sweep kernel
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, **kw) as big:
        big.run(b1)
        assert big.validate() == (0, -1)
        for r, o in zip(check, oracles):
            H.assert_replica_equal(big, r, o)
        _same_costs(big, check, oracles)
        # extraction: current and best trees of several replicas in one device pass
        ids = np.array(check, np.int64)
        cur, _ = big.trees(ids, which_min=False)
        best, _ = big.trees(ids, which_min=True)
        for q, o in enumerate(oracles):
            for got, which in ((cur, False), (best, True)):
                l, rr, p, _m = o.tree(which)
                assert np.array_equal(got[q, 0], l) and np.array_equal(got[q, 1], rr) and np.array_equal(got[q, 2], p)
        snap = big.snapshot()

    # snapshot / restore: caches rebuilt from the trees, then more sweeps -- against oracles restored the same way (a
    # rebuilt partial cost may round differently from the one the moves maintained: costs here exceed 2^53)
    restored = []
    for o in oracles:
        l, rr, p, m = o.tree(False)
        restored.append(orc.Oracle(l, rr, p, m, n_inds=prob.n_inds, dims=2, mt_state=o.prng_state(), min_tree=o.tree(True)))
    with core.BatchedOptimizer.restore(snap, prob.leaf_masks, **kw) as again:
        assert again.validate() == (0, -1)
        _same_costs(again, check, restored)
        again.run(b2)
        assert again.validate() == (0, -1)
        for o in restored:
            o.run(orc.PROB_MH, b2)
        for r, o in zip(check, restored):
            H.assert_replica_equal(again, r, o)
        _same_costs(again, check, restored)

    # a small batch of the same replicas, fresh (no best-tree checkpoint, so the LDS-resident kernels may take it)
    sl = [snap["links"][r] for r in check]
    with core.BatchedOptimizer(prob.leaf_masks, np.stack(sl), None, prng_states=snap["prng_states"][check], **kw) as small:
        assert small.validate() == (0, -1)
        small.run(b2)
        assert small.validate() == (0, -1)
        for q, o in enumerate(oracles):
            l, rr, p, m = o.tree(False)
            o2 = orc.Oracle(l, rr, p, m, n_inds=prob.n_inds, dims=2, mt_state=o.prng_state())
            o2.run(orc.PROB_MH, b2)
            H.assert_replica_equal(small, q, o2, check_min=False)
            assert small.costs()[0][q] == o2.total_cost


@pytest.mark.parametrize("case", ["hyper", "dims3", "f32"])
def test_other_layouts_unaffected(core, oracle_lib, case):
    orc = oracle_lib
    okw = {}
    if case == "hyper":
        ts, _d, out = syn.random_hyper_tn(120, 200, k=3, n_output=3, seed=5)
        prob = H.Problem(ts, 2, out)
    else:
        prob = H.regular_problem(200, graph_seed=3)
        if case == "dims3":
            prob.dims = 3
        else:
            okw = dict(cost_type="float32")
    R = 1024
    seeds = H.replica_seeds(R, S=9)
    links = prob.links(seeds)
    betas = H.linear_betas(0, 50, 40)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=prob.dims,
                               output_mask=prob.output_mask, **okw) as gpu:
        gpu.run(betas)
        assert gpu.validate() == (0, -1)
        for r in (0, R - 1):
            o = H.make_oracle(orc, prob, links[r], seeds[r], **okw)
            o.run(orc.PROB_MH, betas)
            H.assert_replica_equal(gpu, r, o)
        snap = gpu.snapshot()
    with core.BatchedOptimizer.restore(snap, prob.leaf_masks, n_inds=prob.n_inds, dims=prob.dims,
                                       output_mask=prob.output_mask, **okw) as again:
        assert again.validate() == (0, -1)
