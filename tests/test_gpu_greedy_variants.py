"""Every instantiation of the device generator of the initial trees (csrc/greedy_device.hip), the second and third tree of
a wavefront, trees handed back to the host one by one, and the kernel's limits from inside: device == host generator
(csrc/host_greedy.cpp), tree for tree -- `np.array_equal` on the links and on `draws`, no tolerance anywhere -- and the
library's own account of what it launched (tnco_hip_diag_greedy_device_last) equal to what tests/greedy_cases.py's
restatement of the dispatch rule predicts.

Which test reaches which instantiation (asserted from the diagnostic in the test named; the rule itself is asserted
without a GPU in tests/test_greedy_cases_plan.py):

    greedy_graph_kernel<4>     test_the_small_variants_are_reached_as_recorded[regular-8-default]
    greedy_graph_kernel<8>     test_the_small_variants_are_reached_as_recorded[regular-200-gs3-default]
    greedy_graph_kernel<12>    test_the_small_variants_are_reached_as_recorded[regular-512-gs11-default]
    greedy_graph_kernel<16>    test_the_small_variants_are_reached_as_recorded[sycamore-20-default]
    greedy_graph_kernel<24>    test_every_variant_by_the_rule[regular-1000-default], [regular-700-default]
    greedy_kernel<4>           test_the_small_variants_are_reached_as_recorded[regular-8-set]
    greedy_kernel<8>           test_every_variant_by_the_rule[hyper-40-100-k4-default], [hyper-24-30-k6-default]
    greedy_kernel<12>          test_every_variant_by_the_rule[hyper-40-130-k5-default]
    greedy_kernel<16>          test_every_variant_by_the_rule[hyper-40-150-k6-default]
    greedy_kernel<24>          test_every_variant_by_the_rule[regular-1000-set], [regular-700-set]
    greedy_kernel<0>           test_every_variant_by_the_rule[hyper-40-200-k6-default], [hyper-60-260-k6-default],
                               [hyper-900-1100-k3-default] (by the rule); [...-set-lds-queue] (forced)
    py_shuffle_kernel          every [...-set] and [...-set-lds-queue] run; at n = 1000 in [regular-1000-set]
    py_shuffle_lds_kernel<16>  every [...-default] run of at most 800 tensors
    py_shuffle_lds_kernel<8>   test_every_variant_by_the_rule[regular-1000-default], [hyper-900-1100-k3-default]

(tests/test_gpu_greedy.py runs the small graph and set variants too -- test_regular_graphs and
test_config5_topology_and_many_seeds, on the networks of test_the_small_variants_are_reached_as_recorded -- without
looking at what was launched.)

Host time of the reference of the large-state case (3 589 trees of 1 000 tensors, csrc/host_greedy.cpp on 8 CPU
threads): 1.5 s, computed once for both forms; the 6 149 trees of 300 tensors of the hand-back case: 1.1 s; the 8 197
trees of 256 tensors of the case in which every tree is handed back: 1.4 s.
"""
from typing import NamedTuple

import numpy as np
import pytest

from tests import greedy_cases as gc
from tnco_amd import core, ctree as ct, synthetic as syn

pytestmark = pytest.mark.gpu


class Diag(NamedTuple):
    form: int
    rows: int
    shuffle: int
    G: int
    lds: int
    R: int
    redone: int
    mask: int


def diag() -> Diag:
    from tnco_amd import _lib
    out = np.zeros(8, np.int64)
    assert _lib.load().tnco_hip_diag_greedy_device_last(out.ctypes.data) == 0
    return Diag(*(int(v) for v in out))


def set_form(monkeypatch, form):
    for name in gc.FORMS["set-lds-queue"]:
        monkeypatch.delenv(name, raising=False)
    for name, value in gc.FORMS[form].items():
        monkeypatch.setenv(name, value)


def _mask(net):
    return ct.pack_masks([list(net.out_keep)], net.n_inds)[0]


_HOST = {}


def host_trees(key, net, seeds, draws=None):
    """(links, draws afterwards) of the host generator: computed once per `key`, shared, never written to."""
    if key not in _HOST:
        d = None if draws is None else draws.copy()
        links = core.greedy_trees(net.ts, net.n_inds, seeds, output_mask=_mask(net), draws=d)
        for a in (links, d):
            if a is not None:
                a.setflags(write=False)
        _HOST[key] = (links, d)
    return _HOST[key]


def device_trees(net, seeds, draws=None, keep_on_device=False):
    d = None if draws is None else draws.copy()
    links = core.greedy_trees(net.ts, net.n_inds, seeds, output_mask=_mask(net), draws=d, device=0, keep_on_device=keep_on_device)
    return links, d, diag()


def assert_same_trees(host, dev, G):
    bad = np.flatnonzero((host != dev).reshape(len(host), -1).any(axis=1))
    assert bad.size == 0, (f"{bad.size} of {len(host)} trees differ; first: tree {int(bad[0])}, "
                           f"trip {int(bad[0]) // G} of its wavefront (G = {G}), wavefront {int(bad[0]) % G}")


def assert_spec(net, seeds, dev):
    for k, s in enumerate(seeds):
        con = ct.greedy_contraction(net.ts, net.out_keep, int(s))
        assert np.array_equal(dev[k], np.stack(ct.tree_from_contraction(con, net.n))), int(s)


# --- 1. every variant, by the rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", gc.RUNS, ids=gc.RUN_IDS)
def test_every_variant_by_the_rule(case, form, monkeypatch):
    net = case.build()
    seeds = gc.seeds48()
    draws = gc.draws_for(len(seeds)) if case.draws else None
    host, d_host = host_trees((case.name, "48"), net, seeds, draws)
    set_form(monkeypatch, form)
    dev, d_dev, d = device_trees(net, seeds, draws)
    want = gc.dispatch(net.ts, net.n_inds, net.out_keep, form)
    assert tuple(want[:3]) == case.expect[form]
    assert (d.form, d.rows, d.shuffle, d.lds) == tuple(want), d
    assert (d.R, d.G, d.redone, d.mask) == (len(seeds), len(seeds), 0, 1), d
    assert_same_trees(host, dev, d.G)
    if draws is not None:
        assert np.array_equal(d_host, d_dev) and np.all(d_host >= draws + np.uint64(net.n - 1))
    if case.spec:
        assert_spec(net, seeds[:8], dev)


@pytest.mark.parametrize("name,form", [(n, f) for n, (_b, e) in gc.EXISTING.items() for f in e],
                         ids=[f"{n}-{f}" for n, (_b, e) in gc.EXISTING.items() for f in e])
def test_the_small_variants_are_reached_as_recorded(name, form, monkeypatch):
    """The networks of tests/test_gpu_greedy.py: that they launch the small instantiations is asserted here."""
    build, expect = gc.EXISTING[name]
    net = build()
    seeds = gc.seeds48()[:8]
    host, _ = host_trees((name, "8"), net, seeds)
    set_form(monkeypatch, form)
    dev, _, d = device_trees(net, seeds)
    assert (d.form, d.rows, d.shuffle) == expect[form] and d.lds == gc.dispatch(net.ts, net.n_inds, net.out_keep, form).lds
    assert (d.redone, d.mask) == (0, 1)
    assert_same_trees(host, dev, d.G)


# --- 2. the second and third tree of a wavefront ------------------------------------------------------------------------------
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


PERSISTENT = [("regular-24", lambda: gc.regular(24), "default", (gc.GRAPH, 4)),
              ("regular-24", lambda: gc.regular(24), "set", (gc.SET, 4)),
              ("hyper-24-30-k6", lambda: gc.CASE_BY_NAME["hyper-24-30-k6"].build(), "default", (gc.SET, 8)),
              ("hyper-40-200-k6", lambda: gc.CASE_BY_NAME["hyper-40-200-k6"].build(), "default", (gc.SET, 0))]


@pytest.mark.parametrize("name,build,form,kernel", PERSISTENT, ids=[f"{p[0]}-{p[2]}" for p in PERSISTENT])
def test_a_wavefront_does_a_second_and_a_third_tree(name, build, form, kernel, monkeypatch):
    """R = 33 x CUs + 7 trees on at most 16 x CUs wavefronts: every wavefront goes round its loop at least twice, some three
    times -- the per-tree clears (the set form's queue, table, counts, ssa ids and neighbour rows; the graph form's cells,
    records, marks and its lkey / lrow, which live outside the loop) after a tree that used them."""
    net = build()
    R = 33 * _cus() + 7
    seeds = np.array(syn.replica_seeds(R), np.uint64)
    host, _ = host_trees((name, "33cus"), net, seeds)
    set_form(monkeypatch, form)
    dev, _, d = device_trees(net, seeds)
    print(f"{name} {form}: R = {d.R}, G = {d.G} wavefronts, {d.lds} B of LDS each")
    assert (d.form, d.rows) == kernel and d.R == R
    assert d.R > 2 * d.G, d  # (a condition of the test, not a measurement)
    assert (d.redone, d.mask) == (0, 1)
    assert_same_trees(host, dev, d.G)


@pytest.mark.parametrize("form,kernel", [("default", (gc.GRAPH, 24)), ("set", (gc.SET, 24))])
def test_a_wavefront_does_a_second_and_a_third_tree_with_large_state(form, kernel, monkeypatch):
    """1 000 tensors, 1 500 indices: 23 KB of LDS per tree in the graph form, 24 rows of queue cells in registers in both.
    G is read from a first call large enough to fill the card, then R = 2 G + 5."""
    net = gc.regular(1000)
    set_form(monkeypatch, form)
    _, _, d0 = device_trees(net, np.array(syn.replica_seeds(16 * _cus()), np.uint64), keep_on_device=True)
    G = d0.G
    assert (d0.form, d0.rows) == kernel and G < d0.R  # (G = CUs x trees per CU, not the batch)
    R = 2 * G + 5
    seeds = np.array(syn.replica_seeds(R), np.uint64)
    host, _ = host_trees(("regular-1000", R), net, seeds)
    dev, _, d = device_trees(net, seeds)
    print(f"regular-1000 {form}: R = {d.R}, G = {d.G} wavefronts, {d.lds} B of LDS each")
    assert (d.form, d.rows, d.G, d.R) == (*kernel, G, R) and d.R > 2 * d.G
    assert (d.redone, d.mask) == (0, 1)
    assert_same_trees(host, dev, d.G)


# --- 3. trees handed back one by one -------------------------------------------------------------------------------------------
def _widest(net, links):
    """legs of the widest intermediate tensor of every tree"""
    lm = ct.pack_masks(net.ts, net.n_inds)
    out = []
    for k in range(len(links)):
        m = ct.derive_inds(links[k, 0], links[k, 1], lm, None)
        out.append(int(np.unpackbits(np.ascontiguousarray(m[net.n:]).view(np.uint8), axis=1).sum(axis=1).max()))
    return np.array(out)


def test_trees_are_handed_back_one_by_one(monkeypatch):
    """The 6-regular graph of 300 tensors: the graph form counts a tensor's legs in eight bits, and the widest intermediate
    tensor of a greedy tree of this network has 230 to 265 legs -- about two trees in five pass 255 and end with status 9,
    the others are the kernel's.  Which trees: replayed on the host from the widths of the host generator's trees.  With
    G = R (64 trees) and with R = 2 G + 5; `draws` passed; links in host memory and left on the device: the merge of the
    redone trees -- runs of consecutive trees copied at once, isolated ones, gaps between them -- and the tree a
    wavefront does after one it gave up."""
    net = gc.regular(300, 1, 6)
    set_form(monkeypatch, "default")
    want = gc.dispatch(net.ts, net.n_inds, net.out_keep)
    assert (want.form, want.rows) == (gc.GRAPH, 16)
    _, _, d0 = device_trees(net, np.array(syn.replica_seeds(16 * _cus()), np.uint64), keep_on_device=True)
    G = d0.G
    assert G < d0.R
    R = 2 * G + 5
    seeds = np.array(syn.replica_seeds(R), np.uint64)
    draws = gc.draws_for(R)
    host, d_host = host_trees(("regular-300-6", R), net, seeds, draws)
    # the replay: status 9 <=> a merged tensor of more than 255 legs (no other status occurs: asserted from the mask)
    back = _widest(net, host[:64]) > 255
    runs = "".join("9" if b else "." for b in back)
    print(f"regular-300-6: handed back among the first 64 trees: {runs}")
    padded = f".{runs}."
    assert "99" in padded and ".9." in padded and 0 < back.sum() < 64
    for n_trees in (64, R):
        dev, d_dev, d = device_trees(net, seeds[:n_trees], draws[:n_trees])
        print(f"regular-300-6: R = {d.R}, G = {d.G}, {d.redone} trees redone on the host, statuses {d.mask:#x}")
        assert (d.form, d.rows, d.R) == (gc.GRAPH, 16, n_trees) and d.G == min(n_trees, G)
        assert d.mask == (1 << 0) | (1 << 9) and 0 < d.redone < n_trees
        assert (d.redone == back.sum()) if n_trees == 64 else (back.sum() <= d.redone <= n_trees - (64 - back.sum()))
        assert_same_trees(host[:n_trees], dev, d.G)
        assert np.array_equal(d_host[:n_trees], d_dev)
        kept, d_kept, d2 = device_trees(net, seeds[:n_trees], draws[:n_trees], keep_on_device=True)
        assert isinstance(kept, core.DeviceLinks) and d2 == d
        assert_same_trees(host[:n_trees], kept.numpy(), d.G)
        assert np.array_equal(d_host[:n_trees], d_kept)
    # the set form has no such limit: every tree is the kernel's
    set_form(monkeypatch, "set")
    dev, d_dev, d = device_trees(net, seeds[:64], draws[:64])
    assert (d.form, d.redone, d.mask) == (gc.SET, 0, 1)
    assert_same_trees(host[:64], dev, d.G)
    assert np.array_equal(d_host[:64], d_dev)


def test_every_tree_handed_back_and_a_wavefront_goes_on(monkeypatch):
    """Status 7, a neighbour list past its capacity: a hub with 255 neighbours that form a ring.  The first two ring
    tensors that meet make a tensor the hub takes at once (cost -16), its 255 entries and the other's three together: in
    every tree, whatever the shuffle -- no network was found in which this limit binds in some trees only (the shuffle
    decides between equal costs alone, and a list this long means costs hundreds of bits apart).  Here with R = 2 G + 5:
    every wavefront starts two trees after one it gave up, and the whole batch comes back to the device in one copy."""
    net = gc.hub_ring(255)
    set_form(monkeypatch, "default")
    assert gc.dispatch(net.ts, net.n_inds, net.out_keep)[:2] == (gc.GRAPH, 8)
    R0 = 16 * _cus()
    seeds = np.array(syn.replica_seeds(2 * R0 + 5), np.uint64)
    dev0, _, d0 = device_trees(net, seeds[:R0])
    G = d0.G
    R = 2 * G + 5
    host, _ = host_trees(("hub-255", R), net, seeds[:R])
    assert (d0.form, d0.rows, d0.redone, d0.mask) == (gc.GRAPH, 8, R0, 1 << 7), d0
    assert_same_trees(host[:R0], dev0, G)
    kept, _, d = device_trees(net, seeds[:R], keep_on_device=True)
    print(f"hub-255: R = {d.R}, G = {d.G}, {d.redone} trees redone on the host, statuses {d.mask:#x}")
    assert (d.form, d.rows, d.G, d.R, d.redone, d.mask) == (gc.GRAPH, 8, G, R, R, 1 << 7) and R > 2 * G
    assert_same_trees(host, kept.numpy(), G)


# --- 4. limits, from inside ------------------------------------------------------------------------------------------------------
LIMITS = [
    ("six-holders", lambda: gc.star(6), (gc.SET, 8, 16)),                   # GREEDY_MAXH tensors on one index
    ("three-tensors", lambda: gc.chain(3), (gc.GRAPH, 4, 16)),              # the fewest the kernel takes
    ("three-tensors-ring", lambda: gc.Network(((0, 1), (1, 2), (2, 0)), 3, ()), (gc.GRAPH, 4, 16)),
    ("2000-tensors", lambda: gc.chain(2000), (gc.SET, 0, 8)),               # the most; 1 999 indices, no graph for the kernel
    ("2040-indices", lambda: gc.regular(1360), (gc.SET, 0, 8)),             # GREEDY_KEY_MAX_EXP: 32 mask words, 40 KB of LDS
]


@pytest.mark.parametrize("name,build,kernel", LIMITS, ids=[x[0] for x in LIMITS])
def test_limits_from_inside(name, build, kernel, monkeypatch):
    net = build()
    seeds = gc.seeds48()[:8]
    host, _ = host_trees((name, "8"), net, seeds)
    set_form(monkeypatch, "default")
    dev, _, d = device_trees(net, seeds)
    want = gc.dispatch(net.ts, net.n_inds, net.out_keep)
    assert tuple(want[:3]) == kernel and (d.form, d.rows, d.shuffle, d.lds) == tuple(want), d
    assert (d.redone, d.mask) == (0, 1)
    assert_same_trees(host, dev, d.G)
    if net.n <= 60:
        assert_spec(net, seeds, dev)


def test_seven_holders_next_to_six_go_to_the_host():
    net = gc.star(7)
    seeds = gc.seeds48()[:8]
    host, _ = host_trees(("seven-holders", "8"), net, seeds)
    dev, _, d = device_trees(net, seeds)
    assert d == Diag(gc.HOST, 0, 0, 0, 0, 8, -1, 0)
    assert_same_trees(host, dev, 1)
