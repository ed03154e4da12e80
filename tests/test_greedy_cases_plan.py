"""The plan side of tests/greedy_cases.py, without a GPU: every named network selects, by the restated dispatch rule, the
kernel instantiation it is meant for; the cases together (with those of tests/test_gpu_greedy.py) reach every instantiation
the host can launch; the restated `supported` is the library's; and the host generator equals the Python spec
(ctree.greedy_contraction) on the small hyper networks -- indices on five and six tensors, which tests/test_host.py's
networks (three and four holders) do not have."""
import numpy as np
import pytest

from tests import greedy_cases as gc
from tnco_amd import core, ctree as ct


def _lib_supported(net):
    from tnco_amd import _lib
    off, _hold = core.holders_csr(net.ts, net.n_inds)
    return bool(_lib.load().tnco_hip_diag_greedy_device_supported(net.n, net.n_inds, off.ctypes.data))


@pytest.mark.parametrize("case", gc.CASES, ids=[c.name for c in gc.CASES])
def test_every_case_selects_the_variant_it_is_meant_for(case):
    net = case.build()
    assert gc.supported(net.ts, net.n_inds) and _lib_supported(net)
    assert net.max_holders() == case.holders <= gc.GREEDY_MAXH
    assert gc.set_need(net.ts, net.n_inds, net.out_keep) == case.w_m1
    for form, want in case.expect.items():
        got = gc.dispatch(net.ts, net.n_inds, net.out_keep, form)
        assert tuple(got[:3]) == want, (form, got)
        assert 0 < got.lds <= gc.LDS_PER_WORKGROUP
    # a form the case leaves out launches nothing the forms it has do not
    for form in set(gc.FORMS) - set(case.expect):
        assert tuple(gc.dispatch(net.ts, net.n_inds, net.out_keep, form)[:3]) in case.expect.values()
    assert case.spec == (net.n <= 60)
    assert case.draws == (net.n >= 900)


def test_the_figures_the_cases_are_chosen_by():
    d = lambda name, form: gc.dispatch(*gc.CASE_BY_NAME[name].build(), form)  # noqa: E731
    # 1000 tensors: E = I = 1500, the last row of <24>; the set form with its queue in LDS would take 32 KB, four trees
    # per CU: the 24 rows in registers are taken, 20.5 KB
    net = gc.regular(1000)
    assert (net.n_inds, gc.graph_tables(*net)[0]) == (1500, 1500)
    assert d("regular-1000", "set-lds-queue").lds == 32792 and gc.LDS_PER_CU // 32792 == 4
    assert d("regular-1000", "set").lds == 32792 - 1536 * 8 == 20504
    # 700 tensors: 17 rows of candidates, one past <16>, in both forms
    assert gc.graph_tables(*gc.regular(700))[0] == 1050 and -(-1050 // 64) == 17
    # <0> by the rule: need 20 (the 24 rows are not taken: the queue in LDS leaves more than eight trees per CU), need 25
    assert d("hyper-40-200-k6", "default").lds < gc.LDS_PER_CU // 8 and 4 * 5 == 20
    assert 5 * 5 == 25 > 24
    # 900 tensors, 1100 indices: 18 words, need 36, about 32 KB
    assert 31 * 1024 < d("hyper-900-1100-k3", "default").lds < 33 * 1024
    # one mask word with six holders, on ten indices
    net = gc.CASE_BY_NAME["hyper-24-30-k6"].build()
    assert sum(len(h) == 6 for h in gc.holders_of(net.ts, net.n_inds)) == 10 and net.n_inds <= 64
    # registers rows with d0 >= 64 and M1 >= 2: dims past the first word, several candidates each
    for name in ("hyper-40-100-k4", "hyper-40-130-k5", "hyper-40-150-k6"):
        net = gc.CASE_BY_NAME[name].build()
        assert any(len(h) >= 3 for h in gc.holders_of(net.ts, net.n_inds)[64:])


def test_the_cases_reach_every_instantiation_the_host_can_launch():
    greedy, shuffle = set(), set()
    for build, expect in [(c.build, c.expect) for c in gc.CASES] + list(gc.EXISTING.values()):
        net = build()
        for form, want in expect.items():
            assert tuple(gc.dispatch(net.ts, net.n_inds, net.out_keep, form)[:3]) == want
            greedy.add(want[:2])
            shuffle.add(want[2])
    assert greedy == gc.ALL_GREEDY and shuffle == gc.ALL_SHUFFLE
    # the new cases alone: every large one, the set form's rows with several candidates per index, the queue in LDS by the rule
    new = {(f, c.expect[f]) for c in gc.CASES for f in c.expect}
    assert {(gc.GRAPH, 24), (gc.SET, 24), (gc.SET, 8), (gc.SET, 12), (gc.SET, 16)} <= {v[:2] for _, v in new}
    assert ("default", (gc.SET, 0, 16)) in new and ("default", (gc.SET, 0, 8)) in new and ("default", (gc.GRAPH, 24, 8)) in new
    # py_shuffle_lds_kernel<4> has no network: 8 trees per workgroup fit up to 2848 tensors, the kernel takes 2000
    assert gc.shuffle_kernel(gc.MAX_LEAVES) == 8 and gc.shuffle_kernel(2848) == 8 and gc.shuffle_kernel(2849) == 4


def test_limit_networks():
    """tests/test_gpu_greedy_variants.py's limits, from inside: what the rule makes of them."""
    for net, want in [(gc.star(6), (gc.SET, 8, 16)), (gc.chain(3), (gc.GRAPH, 4, 16)), (gc.chain(2000), (gc.SET, 0, 8)),
                      (gc.regular(1360), (gc.SET, 0, 8))]:
        assert gc.supported(net.ts, net.n_inds) and _lib_supported(net)
        assert tuple(gc.dispatch(net.ts, net.n_inds, net.out_keep)[:3]) == want
    assert gc.star(6).max_holders() == 6 and gc.star(7).max_holders() == 7
    assert not gc.supported(*gc.star(7)[:2]) and not _lib_supported(gc.star(7))
    assert gc.dispatch(*gc.star(7)) == gc.Variant(gc.HOST, 0, 0, 0)
    # the chain of 2000 is no graph for the kernel (1999 contractible indices, 24 rows hold 1536) and within 64 KB as sets
    assert gc.graph_tables(*gc.chain(2000)) is None and gc.dispatch(*gc.chain(2000)).lds < gc.LDS_PER_WORKGROUP
    # n_inds at GREEDY_KEY_MAX_EXP: the 3-regular graph of 1360 tensors has 2040 indices, 32 mask words, 40 KB of LDS;
    # one more index and the network is the host's
    net = gc.regular(1360)
    assert net.n_inds == gc.GREEDY_KEY_MAX_EXP and gc.dispatch(*net).lds < gc.LDS_PER_WORKGROUP
    more = gc.regular(1362)
    assert more.n_inds == 2043 and not gc.supported(*more[:2]) and not _lib_supported(more)
    for n in (2, 2001):
        assert not gc.supported(*gc.chain(n)[:2]) and not _lib_supported(gc.chain(n))


def test_hand_back_networks():
    """The two networks whose trees the graph form hands back (all of them: a list past 255 entries; some: a tensor past
    255 legs) are the graph form's by the rule."""
    for net, want in [(gc.hub_ring(255), (gc.GRAPH, 8, 16)), (gc.regular(300, 1, 6), (gc.GRAPH, 16, 16))]:
        assert gc.supported(net.ts, net.n_inds) and _lib_supported(net)
        assert tuple(gc.dispatch(net.ts, net.n_inds, net.out_keep)[:3]) == want
    assert len(gc.hub_ring(255).ts[0]) == 255 and gc.hub_ring(255).n == 256


def test_restated_supported_is_the_librarys_on_random_networks():
    rng = np.random.RandomState(5)
    seen = set()
    for s in range(60):
        n = int(rng.randint(3, 400))
        net = gc.hyper(n, int(n * rng.uniform(1.0, 6.0)), int(rng.randint(2, 9)), seed=s)
        seen.add(gc.supported(net.ts, net.n_inds))
        assert gc.supported(net.ts, net.n_inds) == _lib_supported(net), (net.n, net.n_inds)
    assert seen == {True, False}


@pytest.mark.parametrize("case", [c for c in gc.CASES if c.spec], ids=[c.name for c in gc.CASES if c.spec])
def test_host_generator_equals_the_python_spec_on_the_small_hyper_cases(case):
    net = case.build()
    seeds = gc.seeds48()[:8]
    om = ct.pack_masks([list(net.out_keep)], net.n_inds)[0]
    links = core.greedy_trees(net.ts, net.n_inds, seeds, output_mask=om)
    for k, s in enumerate(seeds):
        con = ct.greedy_contraction(net.ts, net.out_keep, int(s))
        assert np.array_equal(links[k], np.stack(ct.tree_from_contraction(con, net.n))), (case.name, int(s))
