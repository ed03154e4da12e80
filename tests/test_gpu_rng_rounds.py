"""The refill rounds of the sweep kernel's mt19937 producer (csrc/sa_sweep.h: MT_ROUND_RING, MT_ROUND_LOW) on the GPU:
the child-partial instantiations of `sa_run_kernel` in full wavefronts (batches too large for the LDS-resident kernels)
and in the SPREAD form, bit for bit against the oracle -- trees, best trees, costs and generator state.  Forty-eight
sweeps as launches of 1, 2, 5 and 40: several generation wraps of every replica's generator, launches that begin and end
at arbitrary ring positions; and generator states imported at positions around the block and the generation boundaries
into the replicas of ONE wavefront, whose rings then refill in common rounds from unrelated positions.
(The rule itself, against numpy's MT19937 from every start position: tests/test_rng_rounds_model.py.)"""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

SWEEPS = 48
LAUNCHES = (1, 2, 5, 40)


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


@functools.lru_cache(maxsize=None)
def _batch(n, deg, R):
    from tnco_amd import core as c
    prob = H.regular_problem(n, graph_seed=n % 89, degree=deg)
    seeds = H.replica_seeds(R, S=n + 1)
    return prob, seeds, c.greedy_trees(prob.ts_inds, prob.n_inds, seeds)


def _checked(R):
    """The first whole wavefront (16 consecutive replicas), three from the middle, the last three."""
    return list(range(16)) + [R // 2 - 1, R // 2, R // 2 + 1] + [R - 3, R - 2, R - 1]


@pytest.mark.parametrize("n,deg,R", [(130, 3, 12300), (512, 3, 12300), (512, 3, 3000)],
                         ids=["4x1 lanes x words", "4x3 (the headline)", "4x3 SPREAD"])
def test_launches_of_1_2_5_40_sweeps_against_the_oracle(core, oracle_lib, n, deg, R):
    prob, seeds, links = _batch(n, deg, R)
    betas = H.linear_betas(0, 60, SWEEPS)
    assert sum(LAUNCHES) == SWEEPS
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        assert gpu.launch_groups >= 1
        at = 0
        for k in LAUNCHES:
            gpu.run(betas[at:at + k])
            at += k
        tot, mn = gpu.costs()
        moves = gpu.moves_per_replica()
        for r in _checked(R):
            o = H.make_oracle(oracle_lib, prob, links[r], seeds[r])
            o.run(oracle_lib.PROB_MH, betas)
            H.assert_replica_equal(gpu, r, o)
            assert tot[r] == o.total_cost and mn[r] == o.min_total_cost
            assert int(moves[r]) == o.counters()["moves"]
        # (two words per move at the least: every checked generator ran through its 624 words and wrapped)
        assert int(moves[_checked(R)].min()) * 2 > 624
        assert gpu.validate() == (0, -1)


POSITIONS = (0, 1, 15, 16, 17, 575, 576, 607, 608, 609, 623, 624)


def _state_at(pos, seed):
    """625 words (key, position) of a seeded numpy MT19937 advanced to `pos` of its third generation; position 0 is the
    generation of position 1 with nothing drawn yet."""
    bg = np.random.MT19937(seed)
    bg.random_raw(624 - bg.state["state"]["pos"])  # (to the end of the seeded generation)
    bg.random_raw(2 * 624 + max(pos, 1))
    s = bg.state["state"]
    assert s["pos"] == max(pos, 1)
    return np.concatenate([s["key"].astype(np.uint32), np.array([pos], np.uint32)])


def test_imported_states_at_the_block_and_generation_boundaries(core, oracle_lib):
    n, deg, R = 512, 3, 12300
    prob, seeds, links = _batch(n, deg, R)
    betas = H.linear_betas(0, 60, 3)
    first = 32  # (the third wavefront: replicas 32..47)
    states = {first + i: _state_at(p, 77 + i) for i, p in enumerate(POSITIONS)}
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds) as gpu:
        assert gpu.launch_groups >= 1
        for r, st in states.items():
            gpu.set_prng_state(r, st)
            assert np.array_equal(gpu.prng_state(r), st)
        gpu.run(betas)
        tot, mn = gpu.costs()
        for r in range(first, first + 16):  # (the four replicas behind the twelve: their seeded states)
            o = H.make_oracle(oracle_lib, prob, links[r], seeds[r], mt_state=states.get(r))
            o.run(oracle_lib.PROB_MH, betas)
            H.assert_replica_equal(gpu, r, o)
            assert tot[r] == o.total_cost and mn[r] == o.min_total_cost
        assert gpu.validate() == (0, -1)
