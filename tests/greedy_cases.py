"""Networks that select each instantiation of the device generator of the initial trees (csrc/greedy_device.hip), and
the rule that selects them, restated in plain Python.

`tnco_hip_greedy_trees_device` picks among twelve kernel instantiations by properties of the network: the graph form
`greedy_graph_kernel<4, 8, 12, 16, 24>` (ROWS = queue cells per lane, 64 ROWS >= contractible indices), the set form
`greedy_kernel<4, 8, 12, 16, 24>` (queue in registers: ROWS >= mask words x (holders of an index - 1)) and
`greedy_kernel<0>` (queue in LDS), and for the shuffle `py_shuffle_kernel` (state in memory) or
`py_shuffle_lds_kernel<16, 8>`.  `dispatch()` below is that rule; CASES names the networks (all from
tnco_amd/synthetic.py) with the variant each is MEANT to reach in each form.  tests/test_greedy_cases_plan.py asserts,
without a GPU, that dispatch() says so -- a retuned rule fails there first -- and tests/test_gpu_greedy_variants.py asserts
that the library's own account of the launch (tnco_hip_diag_greedy_device_last) agrees with dispatch() and that the trees
are the host generator's.

The environment variables of the three forms (tests/test_gpu_greedy.py's `form` fixture):
    default         the rule alone
    set             TNCO_HIP_GREEDY_GRAPH=0 TNCO_HIP_SHUFFLE_LDS=0: the set form and the in-memory shuffle for every network
    set-lds-queue   ... and TNCO_HIP_GREEDY_LDS_QUEUE=1: greedy_kernel<0>
"""
from __future__ import annotations

from functools import lru_cache
from typing import Callable, NamedTuple

import numpy as np

from tnco_amd import synthetic as syn

# csrc/greedy_wave.h, greedy_key.h, greedy_graph.h
GREEDY_MAXH = 6
GREEDY_LCAP = 256
GREEDY_KEY_MAX_EXP = 2040
MAX_LEAVES = 2000
LDS_PER_WORKGROUP = 64 * 1024
LDS_PER_CU = 160 * 1024

HOST, SET, GRAPH = 0, 1, 2  # out8[0] of tnco_hip_diag_greedy_device_last
FORMS = {
    "default": {},
    "set": {"TNCO_HIP_GREEDY_GRAPH": "0", "TNCO_HIP_SHUFFLE_LDS": "0"},
    "set-lds-queue": {"TNCO_HIP_GREEDY_GRAPH": "0", "TNCO_HIP_SHUFFLE_LDS": "0", "TNCO_HIP_GREEDY_LDS_QUEUE": "1"},
}


class Variant(NamedTuple):
    """What one call launches: form (HOST: nothing, the host version does the batch), ROWS of the greedy kernel (set form:
    0 = queue in LDS), the shuffle kernel (0 = in memory, else 8 or 16 trees per workgroup), LDS bytes per wavefront."""
    form: int
    rows: int
    shuffle: int
    lds: int


def holders_of(ts, n_inds):
    h = [[] for _ in range(n_inds)]
    for t, xs in enumerate(ts):
        for i in xs:
            h[i].append(t)
    return h


def set_lds_bytes(W, SMAX, I, QC, TS):
    """lds_bytes(): queue | four broadcast rows | ssa | neighbour list | slot of an ssa id [2n] | holders per dim | table."""
    return QC * 8 + 4 * W * 8 + SMAX * 2 + GREEDY_LCAP * 2 + (SMAX - 8) * 2 + I * 2 + TS * 2 + 16


def graph_lds_bytes(n, CAP):
    return 256 + 13 * n + 3 * CAP + 16


def _set_sizes(n, n_inds, holders):
    q = sum(max(0, len(h) - 1) for h in holders)
    W, SMAX = (n_inds + 63) // 64, 2 * n + 8
    TS = 64
    while 4 * TS < 5 * SMAX:
        TS <<= 1
    return q, W, SMAX, TS, (q + 63) & ~63


def supported(ts, n_inds) -> bool:
    """tnco_hip_diag_greedy_device_supported."""
    n = len(ts)
    if n < 3 or n > MAX_LEAVES or n_inds < 1 or n_inds > GREEDY_KEY_MAX_EXP:
        return False
    holders = holders_of(ts, n_inds)
    if any(len(h) > GREEDY_MAXH for h in holders):
        return False
    _q, W, SMAX, TS, QC = _set_sizes(n, n_inds, holders)
    return set_lds_bytes(W, SMAX, n_inds, QC, TS) <= LDS_PER_WORKGROUP


def graph_tables(ts, n_inds, out_keep=()):
    """build_graph() without the environment variable: (E, L, CAP) where the network is a multigraph the graph form takes,
    else None."""
    n = len(ts)
    if n < 3 or n > 2040:
        return None
    out = set(out_keep)
    holders = holders_of(ts, n_inds)
    fp = [0] * n
    pairs = {}
    E = 0
    for i, h in enumerate(holders):
        if len(h) > 2 or (i in out and len(h) > 1):
            return None  # a hyper-index
        for t in h:
            fp[t] += 1
        if len(h) == 2:
            a, b = min(h), max(h)
            if a == b:
                return None
            pairs[(a, b)] = pairs.get((a, b), 0) + 1
            E += 1
    if max(fp) > 255 or E < 1:
        return None
    if any(w == fp[a] == fp[b] for (a, b), w in pairs.items()):
        return None  # equal index sets among the inputs
    L = 2 * len(pairs)
    if L + 256 > 0x7FFF:
        return None
    CAP = max(L + 256, n)
    if E > 64 * 24 or graph_lds_bytes(n, CAP) > LDS_PER_WORKGROUP:
        return None
    return E, L, CAP


def shuffle_kernel(n, shuffle_lds=True) -> int:
    per_tree = 624 * 4 + 2 * n
    if not shuffle_lds or 4 * per_tree > LDS_PER_WORKGROUP:
        return 0
    if 16 * per_tree <= LDS_PER_WORKGROUP:
        return 16
    if 8 * per_tree <= LDS_PER_WORKGROUP:
        return 8
    return 4  # (not reachable: supported() stops at 2000 tensors, <8> fits up to 2848)


def set_need(ts, n_inds, out_keep=()):
    """(W, m1): mask words, and the candidates a contractible index can start with (its holders - 1)."""
    out = set(out_keep)
    holders = holders_of(ts, n_inds)
    m1 = max([1] + [len(h) - 1 for i, h in enumerate(holders) if i not in out])
    return (n_inds + 63) // 64, m1


def dispatch(ts, n_inds, out_keep=(), form="default") -> Variant:
    """The rule of tnco_hip_greedy_trees_device under the environment of FORMS[form]."""
    env = FORMS[form]
    n = len(ts)
    if not supported(ts, n_inds):
        return Variant(HOST, 0, 0, 0)
    shuffle = shuffle_kernel(n, env.get("TNCO_HIP_SHUFFLE_LDS") != "0")
    g = None if env.get("TNCO_HIP_GREEDY_GRAPH") == "0" else graph_tables(ts, n_inds, out_keep)
    if g is not None:
        E, _L, CAP = g
        rows = next(rw for rw in (4, 8, 12, 16, 24) if (E + 63) // 64 <= rw)
        return Variant(GRAPH, rows, shuffle, graph_lds_bytes(n, CAP))
    holders = holders_of(ts, n_inds)
    _q, W, SMAX, TS, QC = _set_sizes(n, n_inds, holders)
    rows = 0
    if env.get("TNCO_HIP_GREEDY_LDS_QUEUE", "0") == "0":
        _W, m1 = set_need(ts, n_inds, out_keep)
        need = W * m1
        rows = next((rw for rw in (4, 8, 12, 16) if need <= rw), 0)
        # 24 rows only where the queue in LDS would leave fewer than eight trees per CU
        if rows == 0 and need <= 24 and LDS_PER_CU // set_lds_bytes(W, SMAX, n_inds, QC, TS) < 8:
            rows = 24
    return Variant(SET, rows, shuffle, set_lds_bytes(W, SMAX, n_inds, 0 if rows else QC, TS))


# --- the networks ---------------------------------------------------------------------------------------------------------
class Network(NamedTuple):
    ts: tuple
    n_inds: int
    out_keep: tuple  # output legs with a single holder (the reference drops the others, tn.py:175-178)

    @property
    def n(self):
        return len(self.ts)

    def max_holders(self):
        return max(len(h) for h in holders_of(self.ts, self.n_inds))


def _freeze(ts, n_inds, out=()):
    cnt = [0] * n_inds
    for xs in ts:
        for i in xs:
            cnt[i] += 1
    return Network(tuple(tuple(int(i) for i in xs) for xs in ts), int(n_inds), tuple(int(i) for i in out if cnt[i] <= 1))


@lru_cache(maxsize=None)
def regular(n, graph_seed=1, degree=3) -> Network:
    p = syn.regular_problem(n, graph_seed=graph_seed, degree=degree)
    return _freeze(p.ts_inds, p.n_inds)


@lru_cache(maxsize=None)
def hyper(n, n_inds, k, seed=1, n_output=3) -> Network:
    ts, _d, out = syn.random_hyper_tn(n, n_inds, k=k, n_output=n_output, seed=seed)
    return _freeze(ts, 1 + max(i for xs in ts for i in xs), out)


@lru_cache(maxsize=None)
def chain(n) -> Network:
    ts, _d, _o = syn.chain_tn(n)
    return _freeze(ts, n - 1)


def star(m) -> Network:
    """A ring of m + 2 tensors (indices 1..m + 2) with index 0 on the first m of them -- not on all: an index common to
    every tensor joins the output and is no hyper-index any more."""
    n = m + 2
    return _freeze([[i + 1, (i + 1) % n + 1] + ([0] if i < m else []) for i in range(n)], n + 1)


def hub_ring(m) -> Network:
    """A hub with m neighbours that form a ring.  m = 255: the first two ring tensors that meet make a tensor the hub
    takes at once (cost -16), its 255 list entries and the other's three together -- past the graph form's 255 in every
    tree, whatever the shuffle (status 7)."""
    return _freeze([list(range(m))] + [[k, m + k, m + (k + 1) % m] for k in range(m)], 2 * m)


class Case(NamedTuple):
    name: str
    build: Callable[[], Network]
    expect: dict           # form -> (form code, ROWS, shuffle kernel): what the network is meant to reach
    w_m1: tuple | None     # (W, m1) of the set form, where the case is about them
    holders: int           # the most tensors on one index
    spec: bool = False     # small enough for the Python spec
    draws: bool = False    # run with generator outputs already consumed (across a twist of the state)


CASES = [
    # graph <24> at E = 1500; set <24> (W 24, m1 1; 20.5 KB of LDS, the queue in LDS would make it 32 KB); set <0> forced;
    # the LDS shuffle with 8 trees per workgroup, and the in-memory shuffle, at n = 1000
    Case("regular-1000", lambda: regular(1000), {"default": (GRAPH, 24, 8), "set": (SET, 24, 0), "set-lds-queue": (SET, 0, 0)},
         (24, 1), 2, draws=True),
    # E = 1050: 17 rows, one past <16>; the set form at need 17
    Case("regular-700", lambda: regular(700), {"default": (GRAPH, 24, 16), "set": (SET, 24, 0), "set-lds-queue": (SET, 0, 0)},
         (17, 1), 2),
    Case("hyper-40-100-k4", lambda: hyper(40, 100, 4), {"default": (SET, 8, 16), "set": (SET, 8, 0), "set-lds-queue": (SET, 0, 0)},
         (2, 3), 4, spec=True),
    Case("hyper-40-130-k5", lambda: hyper(40, 130, 5), {"default": (SET, 12, 16), "set": (SET, 12, 0), "set-lds-queue": (SET, 0, 0)},
         (3, 4), 5, spec=True),
    Case("hyper-40-150-k6", lambda: hyper(40, 150, 6), {"default": (SET, 16, 16), "set": (SET, 16, 0), "set-lds-queue": (SET, 0, 0)},
         (3, 5), 6, spec=True),
    # <0> by the rule: need 20 with a small LDS footprint; need 25
    Case("hyper-40-200-k6", lambda: hyper(40, 200, 6), {"default": (SET, 0, 16), "set": (SET, 0, 0)}, (4, 5), 6, spec=True),
    Case("hyper-60-260-k6", lambda: hyper(60, 260, 6), {"default": (SET, 0, 16), "set": (SET, 0, 0)}, (5, 5), 6, spec=True),
    # W 18, need 36, 32 KB of LDS, the LDS shuffle with 8 trees per workgroup
    Case("hyper-900-1100-k3", lambda: hyper(900, 1100, 3), {"default": (SET, 0, 8), "set": (SET, 0, 0)}, (18, 2), 3, draws=True),
    # one mask word, six holders
    Case("hyper-24-30-k6", lambda: hyper(24, 30, 6, seed=3), {"default": (SET, 8, 16), "set": (SET, 8, 0), "set-lds-queue": (SET, 0, 0)},
         (1, 5), 6, spec=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}

# (case, form) pairs of the device test
RUNS = [(c, f) for c in CASES for f in c.expect]
RUN_IDS = [f"{c.name}-{f}" for c, f in RUNS]

# the variants the EXISTING device tests reach (tests/test_gpu_greedy.py), by the same rule: network -> form -> variant
EXISTING = {
    "regular-8": (lambda: regular(8), {"default": (GRAPH, 4, 16), "set": (SET, 4, 0), "set-lds-queue": (SET, 0, 0)}),
    "regular-512-gs11": (lambda: regular(512, 11), {"default": (GRAPH, 12, 16), "set": (SET, 12, 0), "set-lds-queue": (SET, 0, 0)}),
    "regular-200-gs3": (lambda: regular(200, 3), {"default": (GRAPH, 8, 16), "set": (SET, 8, 0), "set-lds-queue": (SET, 0, 0)}),
    "sycamore-20": (lambda: _freeze(*(lambda p: (p.ts_inds, p.n_inds))(syn.sycamore_problem(20))),
                    {"default": (GRAPH, 16, 16), "set": (SET, 16, 0), "set-lds-queue": (SET, 0, 0)}),
}

# every instantiation the host can launch
ALL_GREEDY = {(GRAPH, r) for r in (4, 8, 12, 16, 24)} | {(SET, r) for r in (4, 8, 12, 16, 24, 0)}
ALL_SHUFFLE = {0, 16, 8}


def seeds48():
    return np.array([0, 1, 2**32 - 1] + list(syn.replica_seeds(45, S=7)), np.uint64)


def draws_for(R):
    """Outputs of Random(seed) consumed before the shuffle: none, and counts either side of the state's 624 words and beyond
    several twists."""
    return np.resize(np.array([0, 623, 624, 625, 5000], np.uint64), R)
