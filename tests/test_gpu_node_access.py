"""How the child-partial instantiations of the sweep kernel read and write a node (csrc/sa_sweep.h, TNCO_NODE_ACCESS;
csrc/sa_kernels.h, View<..., PAIRS>): the header as one 8-byte piece per lane of a quad, the legs in pairs of words per
lane -- the same bytes in HBM, another lane for each word.  Bit for bit against the oracle at the mask widths where the
pair map can go wrong and tests/test_gpu_child_partials.py (W = 1 ... 12, 22) does not reach: a pair half filled (odd W),
a lane without a word, the single row of an odd K partly filled, in every (lanes, words per lane) class above 4 x 3.

A batch of 256 replicas with a best-tree checkpoint given: the LDS-resident kernels leave it alone and the sweep kernel
runs it, spread over the wavefront slots (`launch_groups` >= 1).  The same check in full wavefronts at one width of the
4 x 4, 8 x 3 and 16 x 3 classes, in the spread form of more than one replica per wavefront at W = 12 and W = 10, and on a
tree of 8 leaves, where the children whose parent word an accepted move rewrites are mostly leaves."""
import functools

import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

SWEEPS = 30
LAUNCHES = (1, 2, 27)  # (state leaves and re-enters the kernel)


def leaves_for(W):
    """The largest 3-regular network (an even number of tensors, 1.5 n indices of dimension 2) of W mask words."""
    n = (64 * W * 2 // 3) & ~1
    assert (3 * n // 2 + 63) // 64 == W
    return n


@pytest.fixture(scope="module")
def core():
    from tnco_amd import core as c
    return c


@functools.lru_cache(maxsize=None)
def _batch(n, R):
    from tnco_amd import core as c
    prob = H.regular_problem(n, graph_seed=n % 89 + 2)
    seeds = H.replica_seeds(R, S=n + 3)
    return prob, seeds, c.random_trees(prob.ts_inds, prob.n_inds, seeds)


def _run_and_check(core, orc, n, R, W):
    prob, seeds, links = _batch(n, R)
    assert prob.W == W
    betas = H.linear_betas(0, 60, SWEEPS)
    assert sum(LAUNCHES) == SWEEPS
    # (min_links: the best tree so far is the initial one, as in a fresh handle -- given, it keeps the LDS-resident kernels out)
    with core.BatchedOptimizer(prob.leaf_masks, links, seeds, n_inds=prob.n_inds, dims=2, min_links=links) as gpu:
        assert gpu.launch_groups >= 1
        at = 0
        for k in LAUNCHES:
            gpu.run(betas[at:at + k])
            at += k
        assert gpu.validate() == (0, -1)
        tot, mn = gpu.costs()
        for r in (0, R // 2, R - 1):
            o = H.make_oracle(orc, prob, links[r], seeds[r])
            o.run(orc.PROB_MH, betas)
            H.assert_replica_equal(gpu, r, o)
            assert tot[r] == o.total_cost and mn[r] == o.min_total_cost, r


# W -> (lanes per replica, words per lane) as csrc/tnco_hip.hip, choose_lanes, picks them: the kernel instantiation a case runs
WIDTHS = [(13, (4, 4)), (14, (4, 4)), (15, (4, 4)), (16, (4, 4)), (17, (8, 3)), (23, (8, 3)), (24, (8, 3)),
          (25, (8, 4)), (32, (8, 4)), (33, (16, 3)), (47, (16, 3)), (48, (16, 3))]


@pytest.mark.parametrize("W,lanes_words", WIDTHS, ids=[f"W={w} ({l}x{k})" for w, (l, k) in WIDTHS])
def test_256_replicas_1_2_27_sweeps_against_the_oracle(core, oracle_lib, W, lanes_words):
    _run_and_check(core, oracle_lib, leaves_for(W), 256, W)


@pytest.mark.parametrize("W,lanes_words", [(15, (4, 4)), (23, (8, 3)), (47, (16, 3))], ids=["W=15 (4x4)", "W=23 (8x3)", "W=47 (16x3)"])
def test_full_wavefronts_against_the_oracle(core, oracle_lib, W, lanes_words):
    """12 300 replicas: 64 / lanes replicas in every wavefront, the form the benchmark runs."""
    _run_and_check(core, oracle_lib, leaves_for(W), 12300, W)


@pytest.mark.parametrize("W", [12, 10])
def test_spread_form_against_the_oracle(core, oracle_lib, W):
    """3 000 replicas of a 4 x 3 network: below the kernel's wavefront slots and too many for the LDS-resident kernels
    (as tests/test_gpu_rng_rounds.py arranges it) -- several replicas per wavefront, the other lane groups shadowing."""
    _run_and_check(core, oracle_lib, leaves_for(W), 3000, W)


def test_eight_leaves_parents_of_leaves(core, oracle_lib):
    """8 leaves, W = 1: C and E of a move are leaves more often than not, so the one store per parent word goes to the
    leaf-parent array for both words of many moves, and to a header and the array for others."""
    _run_and_check(core, oracle_lib, 8, 256, 1)
