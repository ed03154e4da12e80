"""Annealing where costs leave the cost type's range: the cases shared by tests/test_cost_range_model.py (no GPU: the
oracle alone) and tests/test_gpu_cost_range.py (every sweep kernel of the library against the oracle, bit for bit).

What the reference does at that edge (infinite_memory/cost_model/simple.hpp, optimizer.hpp; restated in
oracle/tnco_oracle.c): a contraction cost pow(dims, count) beyond the cost type is +inf; a partial sum that holds one is
+inf; delta = (new_B - old_B) + (new_A - old_A) is NaN where inf - inf occurs and goes through the acceptance rule as C's
pow treats it (pow(NaN, -0.0) = 1: accepted at beta 0; u <= NaN is false otherwise); the partial sums of a walk are
re-added from the children, so a later move brings a total back to a finite number; a constructor whose total is not
finite raises "Precision is too low.".

A case = a network (tnco_amd.synthetic), dims, the cost type, optional finite-width / sparse arguments, a schedule as a
list of chunks (rule, betas), and an explicit list of (tree seed, replica seed) PAIRS.  A batch larger than the list is
the list repeated: replica r is the oracle's run of pair r mod len(pairs).  Every case meets, by the oracle alone:
  (a) the oracle constructs every pair;
  (b) in at least a quarter of the pairs some contraction cost or the total is non-finite at some chunk boundary;
  (c) in at least two pairs the total is finite at a later chunk boundary than one where it was not (the way back);
  (d) in at least two pairs the state is finite at every chunk boundary.
The pairs (and, where the case leaves it open, the dims parameter) come from search() below, which anyone can run again:
`python -c "from tests import cost_range_cases as C; C.print_table()"` prints TABLE as it stands in this file.  The counts
the search found are data here; tests/test_cost_range_model.py recomputes them.

Nothing here imports the device library.
"""
from __future__ import annotations

import numpy as np

from tnco_amd import ctree as ct
from tnco_amd import synthetic as syn

KIND = {"base": 0, "greedy": 1, "mh": 2}
HOT = ("mh", 0.0, 0.0)  # beta 0: pow(x, -0.0) = 1, every move is accepted -- a random walk over the trees


class Case:
    """One row of CASES.  `net`: ("regular", leaves, graph_seed) | ("hyper", tensors, indices, k, n_output, seed).
    `dims`: (family, *args) of make_dims; the LAST argument is the parameter search() may vary (`params`).
    `chunks`: (rule, beta0, beta1, sweeps) each -- linear_betas(beta0, beta1, sweeps).  `kw`: what the optimizer gets beyond
    the network (cost_type, max_width, width_type, n_projs, max_number_new_slices).  `resident`, `form`, `cost_range`: what
    the GPU test asserts about the kernel the handle runs; `env`: variables it pins while the handle is created and run;
    `start`: "random" (Problem.tree), "greedy" (the reference's starts) or "mixed" (greedy for an odd tree seed)."""

    def __init__(self, name, net, dims, chunks, *, kw=None, sparse=(), start="random", every=5, replicas=None,
                 resident=None, env=None, plan=None, params=(), cost_range=False, form=None, inf_at=None):
        self.name, self.net, self.dims, self.chunks = name, net, tuple(dims), [tuple(c) for c in chunks]
        self.kw = dict(kw or {})
        self.sparse, self.start, self.every = tuple(sparse), start, every
        self.replicas = replicas
        self.resident = resident      # True: launch_groups == 0 (an LDS-resident kernel); False: >= 1 (the HBM sweep kernel)
        self.env = dict(env or {})
        self.plan = dict(plan or {})  # words, lanes, words_per_lane, cost_mode
        self.params = tuple(params)
        self.cost_range = cost_range  # fw_stats()["cost_range"] > 0: the re-pricing left a cost to the full rebuild
        self.form = form              # finite width: "wave" | "rebuild"
        self.inf_at = inf_at          # a boundary at which the pairs that cross must hold a non-finite cost (search())

    @property
    def cost_type(self):
        return self.kw.get("cost_type", "float64")

    @property
    def fw(self):
        return "max_width" in self.kw

    def with_param(self, p):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.dims = self.dims[:-1] + (p,)
        return c

    def betas(self, k):
        _rule, b0, b1, n = self.chunks[k]
        return np.full(n, float(b0)) if b0 == b1 else syn.linear_betas(b0, b1, n)


# ---------------------------------------------------------------------------------------------------------------------
# networks, dims, trees
# ---------------------------------------------------------------------------------------------------------------------
def make_dims(spec, n_inds):
    """("uniform", d) -> d; ("uniform_pow2", k) -> 2^k.  Per-index families, drawn from RandomState(seed), exponent a in
    max(1, emax - 7) ... emax per index:
    ("pow2", seed, emax): 2^a, index 0 at 2^32 (the largest power-of-two part the library takes) -- pow2_product;
    ("odd_single", seed, emax): 2^a or 3 * 2^a -- one odd part: the table of 3^t times ldexp;
    ("odd_multi", seed, emax): {1, 3, 5, 7} * 2^a -- the rounded chain over the odd parts, then ldexp."""
    fam = spec[0]
    if fam == "uniform":
        return int(spec[1])
    if fam == "uniform_pow2":
        return 1 << int(spec[1])
    _fam, seed, emax = spec
    rng = np.random.RandomState(seed)
    a = rng.randint(max(1, emax - 7), emax + 1, size=n_inds)
    if fam == "pow2":
        a[0] = 32
        odd = np.ones(n_inds, np.int64)
    elif fam == "odd_single":
        odd = np.where(rng.randint(0, 2, size=n_inds) == 1, 3, 1)
    else:
        odd = np.array([1, 3, 5, 7])[rng.randint(0, 4, size=n_inds)]
    return np.array([int(o) << int(e) for o, e in zip(odd, a)], np.uint64)


def problem(case):
    if case.net[0] == "regular":
        _k, n, gs = case.net
        ts, _d, out = syn.random_regular_tn(n, 3, gs)
    else:
        _k, n, n_inds, k, n_out, seed = case.net
        ts, _d, out = syn.random_hyper_tn(n, n_inds, k=k, n_output=n_out, seed=seed)
    n_inds = 1 + max(i for xs in ts for i in xs)
    return syn.Problem(ts, make_dims(case.dims, n_inds), out, sparse_inds=case.sparse)


def plan_facts(prob):
    """What tnco_hip_create derives from a problem before it touches the device (csrc/tnco_hip.hip: choose_lanes,
    Params::cost_mode), restated: mask words, lanes per replica x words per lane, and the cost path -- 0: uniform dims 2^k
    (pow2_cost), 1: uniform dims, a table of pow(d, count), 2: per-index dims with odd parts (seq_product), 3: per-index
    powers of two (pow2_product)."""
    W = prob.W
    lanes, k = (4, (W + 3) // 4) if W <= 16 else (8, 3 if W <= 24 else 4) if W <= 32 else (16, 3 if W <= 48 else 4)
    d = prob.dims
    if np.ndim(d) == 0 or len(set(int(x) for x in d)) == 1:
        u = int(d) if np.ndim(d) == 0 else int(d[0])
        mode = 0 if u & (u - 1) == 0 else 1
    else:
        mode = 3 if all(int(x) & (int(x) - 1) == 0 for x in d) else 2
    return dict(words=W, lanes=lanes, words_per_lane=k, cost_mode=mode)


def start_tree(case, prob, tree_seed):
    if case.start == "greedy" or (case.start == "mixed" and int(tree_seed) % 2):
        out = ct.unpack_mask(prob.output_mask)
        return ct.tree_from_contraction(ct.greedy_contraction(prob.ts_inds, out, int(tree_seed)), prob.n)
    return prob.tree(tree_seed)


def batch(case, prob, pairs):
    """(links [R, 3, N], seeds [R], pair of every replica [R]) of the case's batch: the pairs repeated."""
    trees = np.stack([np.stack(start_tree(case, prob, t)) for t, _s in pairs]).astype(np.int32)
    R = case.replicas or len(pairs)
    who = np.arange(R) % len(pairs)
    return np.ascontiguousarray(trees[who]), [int(pairs[k][1]) for k in who], who


def checked_replicas(case, R, P):
    """All replicas of a small batch; of a repeated one the first, some middle and the last -- every pair among them."""
    if R <= 96:
        return list(range(R))
    mid = R // 2 - (R // 2) % 64
    return sorted(set(list(range(P)) + [63, 64, 65] + list(range(mid - 1, mid + 2)) + list(range(R - P - 1, R))))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's run of a pair, chunk by chunk
# ---------------------------------------------------------------------------------------------------------------------
def make_oracle(orc, case, prob, tree, seed):
    """Raises ValueError("Precision is too low.") as the reference's constructor does."""
    l, r, p = tree
    return orc.Oracle(l, r, p, prob.node_masks(l, r), n_inds=prob.n_inds, dims=prob.dims, sparse=prob.sparse_mask,
                      seed=int(seed) & 0xFFFFFFFF, **case.kw)


def advance(o, case, k, steps_done):
    """Chunk k on oracle `o`; finite width re-slices at sweep n (counted over all chunks) when n % every == 0, as
    BatchedOptimizer.run counts it."""
    rule = KIND[case.chunks[k][0]]
    betas = case.betas(k)
    if not case.fw:
        o.run(rule, betas)
    else:
        for i, b in enumerate(betas):
            o.update(rule, float(b), update_slices=(steps_done + i) % case.every == 0)
    return steps_done + len(betas)


def state_flags(o):
    """(some stored cost is non-finite, the total is finite, some stored cost is NaN) of an oracle's state."""
    cc, pc, _hy = o.caches()
    tot, mn = o.total_cost, o.min_total_cost
    allv = np.concatenate([cc, pc, [tot, mn]])
    return (not np.all(np.isfinite(allv))), bool(np.isfinite(tot)), bool(np.any(np.isnan(allv)))


def trace(orc, case, prob, pair):
    """None if the oracle refuses the pair; else dict(nonfinite=[per boundary], total_finite=[...], nan=bool, verdict=int):
    boundary 0 is the constructed state, boundary k + 1 the state after chunk k; verdict = is_valid() at the end."""
    try:
        o = make_oracle(orc, case, prob, start_tree(case, prob, pair[0]), pair[1])
    except ValueError as e:
        assert "Precision is too low" in str(e)
        return None
    nf, tf, nan, done = [], [], False, 0
    for k in range(-1, len(case.chunks)):
        if k >= 0:
            done = advance(o, case, k, done)
        a, b, c = state_flags(o)
        nf.append(a); tf.append(b); nan |= c
    v = o.is_valid()
    o.close()
    return dict(nonfinite=nf, total_finite=tf, nan=nan, verdict=int(v))


def classify(tr):
    """(crossed, came back, finite throughout) of a trace."""
    crossed = any(tr["nonfinite"])
    first_bad = next((i for i, f in enumerate(tr["total_finite"]) if not f), None)
    back = first_bad is not None and any(tr["total_finite"][first_bad + 1:])
    return crossed, back, not crossed


def counts(traces):
    cl = [classify(t) for t in traces]
    return dict(crossed=sum(c[0] for c in cl), came_back=sum(c[1] for c in cl), finite=sum(c[2] for c in cl),
                invalid=[k for k, t in enumerate(traces) if t["verdict"] != 0])


def meets_conditions(n_pairs, cnt):
    return 4 * cnt["crossed"] >= n_pairs and cnt["came_back"] >= 2 and cnt["finite"] >= 2


def search(orc, case, n_candidates=48, want=(3, 3, 2)):
    """The pairs of a case: for each dims parameter of case.params (or the one in case.dims), candidate pair k is (tree seed
    1000 + k, replica seed replica_seeds(.., S=11)[k]); of the pairs the oracle constructs, the first want[0] that came
    back, the first want[1] that stay finite and the first want[2] others that crossed, in candidate order.  The first
    parameter whose selection meets (a)-(d) wins.  Returns (param, pairs, counts) or None."""
    seeds = syn.replica_seeds(n_candidates, S=11)
    for p in (case.params or (case.dims[-1],)):
        c = case.with_param(p)
        prob = problem(c)
        back, fin, other = [], [], []
        for k in range(n_candidates):
            pair = (1000 + k, int(seeds[k]))
            tr = trace(orc, c, prob, pair)
            if tr is None:
                continue
            crossed, came_back, finite = classify(tr)
            if crossed and c.inf_at is not None and not tr["nonfinite"][c.inf_at]:
                continue  # (the state a greedy or base phase starts from must hold the non-finite cost)
            if came_back and len(back) < want[0]:
                back.append((k, pair, tr))
            elif finite and len(fin) < want[1]:
                fin.append((k, pair, tr))
            elif crossed and not came_back and len(other) < want[2]:
                other.append((k, pair, tr))
            if len(back) == want[0] and len(fin) == want[1] and len(other) == want[2]:
                break
        sel = sorted(back + fin + other)
        pairs = [x[1] for x in sel]
        cnt = counts([x[2] for x in sel])
        if pairs and meets_conditions(len(pairs), cnt):
            return p, pairs, cnt
    return None


def print_table(names=None):
    """Runs search() for every case (or those named) and prints the rows of TABLE."""
    from oracle import oracle as orc
    orc.build()
    for c in CASES:
        if names and c.name not in names:
            continue
        got = search(orc, c)
        if got is None:
            print(f"    # {c.name}: no parameter of {c.params or c.dims[-1:]} meets the conditions")
            continue
        p, pairs, cnt = got
        print(f"    {c.name!r}: dict(param={p!r}, pairs={pairs!r},\n        counts={cnt!r}),")


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _hot(n_chunks, sweeps):
    return [HOT + (sweeps,)] * n_chunks


_RAMP = [HOT + (6,)] * 3 + [("mh", 0.5, 8.0, 6), ("mh", 8.0, 16.0, 6), ("mh", 16.0, 24.0, 6)]
_P2 = (20, 24, 28, 32, 36, 40, 44)  # log2 of uniform dims the search tries on the 64- to 130-leaf networks
_PLAN_SMALL = dict(words=2, lanes=4, words_per_lane=1, cost_mode=0)

CASES = [
    # 1-3: the LDS-resident kernels: costs are stored as exponents there
    Case("small63", ("regular", 64, 7), ("uniform_pow2", 36), _hot(6, 5), resident=True, plan=_PLAN_SMALL, params=_P2),
    Case("small127", ("regular", 84, 11), ("uniform_pow2", 28), _hot(6, 5), resident=True, plan=_PLAN_SMALL, params=_P2),
    Case("lds_k1", ("regular", 128, 39), ("uniform_pow2", 20), _hot(6, 4), resident=True,
         plan=dict(words=3, lanes=4, words_per_lane=1, cost_mode=0), params=(12, 16, 20, 24, 28)),
    Case("lds_k3", ("regular", 512, 11), ("uniform_pow2", 6), _hot(6, 5), start="mixed", resident=True,
         plan=dict(words=12, lanes=4, words_per_lane=3, cost_mode=0), params=(5, 6, 7)),
    # ... and with a greedy tail from a state that holds an inf: in the child-partial layout the stored exponent only enters
    # the delta of a move, which the hot chunks accept whatever it is
    Case("small127_greedy", ("regular", 84, 11), ("uniform_pow2", 28), _hot(3, 5) + [("greedy", 0.0, 0.0, 4)] * 3, resident=True,
         plan=_PLAN_SMALL, params=_P2, inf_at=3),
    Case("lds_k1_greedy", ("regular", 128, 39), ("uniform_pow2", 20), _hot(3, 4) + [("greedy", 0.0, 0.0, 4)] * 3, resident=True,
         plan=dict(words=3, lanes=4, words_per_lane=1, cost_mode=0), params=(12, 16, 20, 24, 28), inf_at=3),
    Case("lds_k3_greedy", ("regular", 512, 11), ("uniform_pow2", 6), _hot(3, 5) + [("greedy", 0.0, 0.0, 4)] * 3, start="mixed",
         resident=True, plan=dict(words=12, lanes=4, words_per_lane=3, cost_mode=0), params=(5, 6, 7), inf_at=3),
    # 4: the HBM sweep kernel, child-partial layout, spread form (3 000 replicas of 512 leaves: four per wavefront)
    Case("cpl_spread", ("regular", 512, 11), ("uniform_pow2", 6), _hot(6, 5), start="mixed", replicas=3000, resident=False,
         plan=dict(words=12, lanes=4, words_per_lane=3, cost_mode=0), params=(5, 6, 7)),
    # 5: ... in full wavefronts
    Case("cpl_full_4x1", ("regular", 130, 41), ("uniform_pow2", 20), _hot(5, 4), replicas=12300, resident=False,
         plan=dict(words=4, lanes=4, words_per_lane=1, cost_mode=0), params=(12, 16, 20, 24, 28)),
    Case("cpl_full_8x3", ("regular", 900, 10), ("uniform_pow2", 4), [HOT + (1,)] * 3 + [("greedy", 0.0, 0.0, 3)] * 2,
         start="mixed", replicas=8200, resident=False, plan=dict(words=22, lanes=8, words_per_lane=3, cost_mode=0),
         params=(3, 4)),
    # 6: the general instantiations
    Case("f32_dims2", ("regular", 384, 5), ("uniform_pow2", 1), _hot(6, 4), start="mixed", kw=dict(cost_type="float32"),
         resident=False, plan=dict(words=9, cost_mode=0)),
    Case("f32_dims16", ("regular", 64, 7), ("uniform_pow2", 4), _hot(6, 5), kw=dict(cost_type="float32"), resident=False,
         plan=dict(words=2, cost_mode=0)),
    Case("f32_dims3", ("regular", 224, 5), ("uniform", 3), _hot(6, 4), start="mixed", kw=dict(cost_type="float32"),
         resident=False, plan=dict(words=6, cost_mode=1)),
    Case("vec_pow2", ("regular", 84, 11), ("pow2", 3, 32), _hot(6, 5), resident=False, plan=dict(words=2, cost_mode=3),
         params=(32, 30, 28)),
    Case("vec_odd_single", ("regular", 84, 11), ("odd_single", 4, 32), _hot(6, 5), resident=False,
         plan=dict(words=2, cost_mode=2), params=(32, 30, 28)),
    Case("vec_odd_multi", ("regular", 84, 11), ("odd_multi", 5, 32), _hot(6, 5), resident=False,
         plan=dict(words=2, cost_mode=2), params=(32, 30, 28)),
    Case("vec_odd_multi_f32", ("regular", 64, 7), ("odd_multi", 6, 4), _hot(6, 5), kw=dict(cost_type="float32"),
         resident=False, plan=dict(words=2, cost_mode=2), params=(2, 3, 4, 5)),
    Case("sparse_projs", ("regular", 128, 39), ("uniform_pow2", 52), _hot(6, 5), kw=dict(n_projs=1 << 20),
         sparse=tuple(i for i in range(192) if i % 3), resident=False, plan=dict(words=3, cost_mode=0), params=(52, 56, 60)),
    # (hyper-indices keep a handle off sa_small_kernel only: a batch that fits the LDS runs sa_lds_kernel<1>, a large one the
    #  hyper instantiation of the sweep kernel -- 12 300 replicas, as tests/test_gpu_parity.py reaches it)
    Case("hyper_lds", ("hyper", 60, 110, 3, 4, 21), ("uniform_pow2", 14), _hot(6, 5), resident=True,
         plan=dict(words=2, lanes=4, words_per_lane=1, cost_mode=0), params=(12, 14, 16)),
    Case("hyper", ("hyper", 60, 110, 3, 4, 21), ("uniform_pow2", 14), _hot(6, 5), replicas=12300, resident=False,
         plan=dict(words=2, lanes=4, words_per_lane=1, cost_mode=0), params=(12, 14, 16)),
    # 7: finite width
    Case("fw_wave", ("regular", 96, 21), ("uniform_pow2", 24), _hot(6, 5), kw=dict(max_width=30 * 24.0), resident=False,
         env=dict(TNCO_HIP_FW_WAVE="1"), form="wave", cost_range=True, plan=dict(words=3, cost_mode=0)),
    Case("fw_rebuild", ("regular", 96, 21), ("uniform_pow2", 24), _hot(6, 5), kw=dict(max_width=30 * 24.0), resident=False,
         env=dict(TNCO_HIP_FW_WAVE="0"), form="rebuild", plan=dict(words=3, cost_mode=0)),
    Case("fw_f32", ("regular", 96, 21), ("uniform_pow2", 3), _hot(6, 5), kw=dict(max_width=30 * 3.0, cost_type="float32"),
         resident=False, form="rebuild", plan=dict(words=3, cost_mode=0)),
    Case("fw_new_slices", ("regular", 96, 21), ("uniform_pow2", 24), _hot(6, 5),
         kw=dict(max_width=30 * 24.0, max_number_new_slices=2), resident=False, plan=dict(words=3, cost_mode=0)),
    # 8: the rules, from a state that already holds an inf; a real annealing ramp after the hot phase
    Case("rule_greedy", ("regular", 64, 7), ("uniform_pow2", 36), _hot(3, 6) + [("greedy", 0.0, 0.0, 4)] * 3, resident=True, inf_at=3,
         plan=_PLAN_SMALL, params=_P2),
    Case("rule_greedy_hbm", ("regular", 130, 41), ("uniform_pow2", 20), _hot(3, 5) + [("greedy", 0.0, 0.0, 4)] * 3,
         resident=False, replicas=12300, plan=dict(words=4, lanes=4, words_per_lane=1, cost_mode=0), inf_at=3,
         params=(12, 16, 20, 24, 28)),
    Case("rule_base", ("regular", 64, 7), ("uniform_pow2", 36), _hot(2, 6) + [("base", 0.0, 0.0, 5)] * 4, resident=True, inf_at=2,
         plan=_PLAN_SMALL, params=_P2),
    Case("rule_mh_ramp", ("regular", 64, 7), ("uniform_pow2", 36), _RAMP, resident=True, plan=_PLAN_SMALL, params=_P2, inf_at=3),
    Case("rule_mh_ramp_f32", ("regular", 64, 7), ("uniform_pow2", 5), _RAMP, start="mixed", kw=dict(cost_type="float32"), resident=False, inf_at=3,
         plan=dict(words=2, cost_mode=0), params=(3, 4, 5)),
    Case("rule_mh_ramp_hbm", ("regular", 130, 41), ("uniform_pow2", 20), _RAMP, resident=False, replicas=12300,
         plan=dict(words=4, lanes=4, words_per_lane=1, cost_mode=0), inf_at=3, params=(12, 16, 20, 24, 28)),
]


# What search() found (print_table() prints these rows): the dims parameter, the pairs, and of the pairs how many crossed,
# came back and stayed finite, and which the oracle's is_valid() rejects at the end (positions in `pairs`).
TABLE = {
    'small63': dict(param=32, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1040, 1354105336), (1041, 986407536), (1043, 301607634)],
        counts={'crossed': 3, 'came_back': 3, 'finite': 3, 'invalid': []}),
    'small127': dict(param=28, pairs=[(1000, 1942955387), (1001, 2404204091), (1004, 2181161659), (1013, 3477396796), (1020, 676431987), (1026, 129203736), (1027, 1992583338), (1035, 1194700557)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [4, 6]}),
    'lds_k1': dict(param=20, pairs=[(1001, 2404204091), (1002, 3969454232), (1003, 1999951822), (1004, 2181161659), (1005, 2522798630), (1011, 1303098500), (1012, 389426993), (1038, 3608698306)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [6, 7]}),
    'lds_k3': dict(param=6, pairs=[(1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1007, 2198630863), (1009, 3405809733), (1011, 1303098500), (1013, 3477396796), (1021, 64427674)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [2, 4, 7]}),
    'small127_greedy': dict(param=28, pairs=[(1000, 1942955387), (1001, 2404204091), (1004, 2181161659), (1041, 986407536), (1046, 3636048969)],
        counts={'crossed': 2, 'came_back': 2, 'finite': 3, 'invalid': []}),
    'lds_k1_greedy': dict(param=20, pairs=[(1001, 2404204091), (1002, 3969454232), (1003, 1999951822), (1010, 404257166), (1014, 2978295604), (1019, 2643821684), (1024, 816938268), (1033, 2845199074)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [6, 7]}),
    'lds_k3_greedy': dict(param=6, pairs=[(1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1009, 3405809733), (1027, 1992583338), (1029, 3618196966), (1033, 2845199074), (1045, 1719704067)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [3, 6]}),
    'cpl_spread': dict(param=6, pairs=[(1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1007, 2198630863), (1009, 3405809733), (1011, 1303098500), (1013, 3477396796), (1021, 64427674)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [2, 4, 7]}),
    'cpl_full_4x1': dict(param=20, pairs=[(1000, 1942955387), (1001, 2404204091), (1006, 793110137), (1008, 2705325683), (1009, 3405809733), (1010, 404257166), (1016, 4218488620), (1024, 816938268)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [1, 2, 7]}),
    'cpl_full_8x3': dict(param=4, pairs=[(1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1007, 2198630863), (1009, 3405809733), (1015, 179874675), (1019, 2643821684)],
        counts={'crossed': 4, 'came_back': 2, 'finite': 3, 'invalid': [1, 6]}),
    'f32_dims2': dict(param=1, pairs=[(1001, 2404204091), (1002, 3969454232), (1003, 1999951822), (1005, 2522798630), (1007, 2198630863), (1011, 1303098500), (1013, 3477396796), (1017, 4143603118)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [0, 4]}),
    'f32_dims16': dict(param=4, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1018, 2808575895), (1040, 1354105336), (1047, 1660062978)],
        counts={'crossed': 3, 'came_back': 2, 'finite': 3, 'invalid': [3]}),
    'f32_dims3': dict(param=3, pairs=[(1001, 2404204091), (1002, 3969454232), (1003, 1999951822), (1004, 2181161659), (1005, 2522798630), (1007, 2198630863), (1009, 3405809733), (1021, 64427674)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [1, 3, 5]}),
    'vec_pow2': dict(param=32, pairs=[(1000, 1942955387), (1001, 2404204091), (1004, 2181161659), (1013, 3477396796), (1020, 676431987), (1021, 64427674), (1026, 129203736), (1032, 2146509344)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [4, 7]}),
    'vec_odd_single': dict(param=32, pairs=[(1000, 1942955387), (1001, 2404204091), (1004, 2181161659), (1006, 793110137), (1013, 3477396796), (1016, 4218488620), (1020, 676431987), (1021, 64427674)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [5, 6, 7]}),
    'vec_odd_multi': dict(param=32, pairs=[(1000, 1942955387), (1001, 2404204091), (1004, 2181161659), (1006, 793110137), (1009, 3405809733), (1017, 4143603118), (1021, 64427674), (1027, 1992583338)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [1, 4]}),
    'vec_odd_multi_f32': dict(param=4, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1005, 2522798630), (1011, 1303098500), (1012, 389426993), (1014, 2978295604), (1016, 4218488620)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [4, 6]}),
    'sparse_projs': dict(param=52, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1004, 2181161659), (1008, 2705325683), (1011, 1303098500), (1019, 2643821684), (1024, 816938268)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [4, 5]}),
    'hyper_lds': dict(param=14, pairs=[(1000, 1942955387), (1002, 3969454232), (1003, 1999951822), (1004, 2181161659), (1005, 2522798630), (1006, 793110137), (1008, 2705325683), (1036, 4284900753)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [3, 7]}),
    'hyper': dict(param=14, pairs=[(1000, 1942955387), (1002, 3969454232), (1003, 1999951822), (1004, 2181161659), (1005, 2522798630), (1006, 793110137), (1008, 2705325683), (1036, 4284900753)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [3, 7]}),
    'fw_wave': dict(param=24, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1016, 4218488620), (1032, 2146509344), (1036, 4284900753)],
        counts={'crossed': 3, 'came_back': 3, 'finite': 3, 'invalid': []}),
    'fw_rebuild': dict(param=24, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1016, 4218488620), (1032, 2146509344), (1036, 4284900753)],
        counts={'crossed': 3, 'came_back': 3, 'finite': 3, 'invalid': []}),
    'fw_f32': dict(param=3, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1009, 3405809733), (1016, 4218488620), (1032, 2146509344), (1036, 4284900753)],
        counts={'crossed': 4, 'came_back': 3, 'finite': 3, 'invalid': [3]}),
    'fw_new_slices': dict(param=24, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1003, 1999951822), (1015, 179874675), (1019, 2643821684), (1043, 301607634), (1047, 1660062978)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [6, 7]}),
    'rule_greedy': dict(param=36, pairs=[(1000, 1942955387), (1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1011, 1303098500), (1018, 2808575895), (1040, 1354105336)],
        counts={'crossed': 4, 'came_back': 3, 'finite': 3, 'invalid': [6]}),
    'rule_greedy_hbm': dict(param=20, pairs=[(1001, 2404204091), (1006, 793110137), (1008, 2705325683), (1009, 3405809733), (1010, 404257166), (1015, 179874675), (1029, 3618196966)],
        counts={'crossed': 4, 'came_back': 3, 'finite': 3, 'invalid': [5]}),
    'rule_base': dict(param=32, pairs=[(1000, 1942955387), (1001, 2404204091), (1002, 3969454232), (1040, 1354105336), (1041, 986407536)],
        counts={'crossed': 2, 'came_back': 2, 'finite': 3, 'invalid': []}),
    'rule_mh_ramp': dict(param=36, pairs=[(1000, 1942955387), (1001, 2404204091), (1003, 1999951822), (1005, 2522798630), (1011, 1303098500), (1018, 2808575895), (1040, 1354105336)],
        counts={'crossed': 4, 'came_back': 3, 'finite': 3, 'invalid': [6]}),
    'rule_mh_ramp_f32': dict(param=5, pairs=[(1001, 2404204091), (1003, 1999951822), (1004, 2181161659), (1005, 2522798630), (1006, 793110137), (1013, 3477396796), (1014, 2978295604), (1016, 4218488620)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [3, 7]}),
    'rule_mh_ramp_hbm': dict(param=20, pairs=[(1001, 2404204091), (1006, 793110137), (1008, 2705325683), (1009, 3405809733), (1010, 404257166), (1015, 179874675), (1016, 4218488620), (1038, 3608698306)],
        counts={'crossed': 5, 'came_back': 3, 'finite': 3, 'invalid': [5, 7]}),
}


def resolved():
    """The cases with the dims parameter of TABLE in place and `pairs` / `counts` attached."""
    out = []
    for c in CASES:
        row = TABLE[c.name]
        r = c.with_param(row["param"])
        r.pairs, r.counts = [tuple(x) for x in row["pairs"]], dict(row["counts"])
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the constructors, from both sides of the edge: tiny hand-made trees whose costs are exact powers of two
# ---------------------------------------------------------------------------------------------------------------------
TOP = {"float64": 1024, "float32": 128}  # 2^TOP is the first power of two the cost type does not hold


def _split(e):
    """Exponents of per-index dims (each at most 32, the library's limit) that sum to e; e = 0: one index of dimension 1."""
    return [32] * (e // 32) + ([e % 32] if e % 32 or e == 0 else [])


class Ctor:
    """ts_inds / dims (uint64 per index, or an int) / trees (one contraction, or one per replica) of a constructor case;
    `total`: per tree, the exact costs in traverse order as Python integers (exact_costs below gives the same from the
    legs); `ok`: whether the reference constructs it."""

    def __init__(self, name, ts_inds, dims, contractions, cost_type, totals, ok):
        self.name, self.ts_inds, self.dims, self.contractions = name, ts_inds, dims, contractions
        self.cost_type, self.totals, self.ok = cost_type, totals, ok

    def problem(self):
        return syn.Problem(self.ts_inds, self.dims)

    def links(self, prob):
        return np.stack([np.stack(ct.tree_from_contraction(c, prob.n)) for c in self.contractions]).astype(np.int32)


def exact_costs(ts_inds, dims, contraction, slices=()):
    """The contraction costs of a tree, in the order of `contraction`, as Python integers: the product of dims over
    legs(child 0) | legs(child 1) | slices; an index is a leg of a node while a leaf outside its subtree holds it."""
    n = len(ts_inds)
    n_inds = 1 + max(i for xs in ts_inds for i in xs)
    d = [int(dims)] * n_inds if np.ndim(dims) == 0 else [int(x) for x in dims]
    leaves = {t: {t} for t in range(n)}
    holders = {i: {t for t in range(n) if i in ts_inds[t]} for i in range(n_inds)}

    def legs(x):
        return {i for t in leaves[x] for i in ts_inds[t] if holders[i] - leaves[x]}

    out = []
    for a, b, new in contraction:
        c = 1
        for i in legs(a) | legs(b) | set(slices):
            c *= d[i]
        out.append(c)
        leaves[new] = leaves[a] | leaves[b]
    return out


def fits(costs, cost_type):
    """Whether the reference's sum of these power-of-two costs stays finite: every running sum below 2^TOP (the sums of the
    cases here are exact in the cost type or round up to a power of two: no rounding decides)."""
    return sum(costs) < 2 ** TOP[cost_type]


def _chain3(a_exp, b_exp):
    """t0 = A, t1 = A + B, t2 = B; ((t0, t1), t2): costs 2^(a + b), 2^b."""
    A, B = _split(a_exp), _split(b_exp)
    ia = list(range(len(A)))
    ib = list(range(len(A), len(A) + len(B)))
    return [ia, ia + ib, ib], np.array([1 << e for e in A + B], np.uint64), [(0, 1, 3), (2, 3, 4)]


def _chain4(a, b, c):
    """t0 = A, t1 = A + B, t2 = B + C, t3 = C.  Tree X = ((t0, t1), (t2, t3)): 2^(a + b), 2^(b + c), 2^b; tree Y =
    (((t1, t2), t0), t3): 2^(a + b + c), 2^(a + c), 2^c."""
    A, B, Cc = _split(a), _split(b), _split(c)
    ia = list(range(len(A)))
    ib = list(range(len(A), len(A) + len(B)))
    ic = list(range(len(A) + len(B), len(A) + len(B) + len(Cc)))
    ts = [ia, ia + ib, ib + ic, ic]
    X = [(0, 1, 4), (2, 3, 5), (4, 5, 6)]
    Y = [(1, 2, 4), (0, 4, 5), (3, 5, 6)]
    return ts, np.array([1 << e for e in A + B + Cc], np.uint64), X, Y


def ctor_cases():
    out = []
    for ctype, T in TOP.items():
        # per-index power-of-two dims (pow2_product): A = one index of dimension 1, so both costs are 2^b
        # (float32, two costs of 2^127: their sum is finite in double and rounds to +inf in float)
        for name, b, totals, ok in (("total_at_top_minus_1", T - 2, [2 ** (T - 2)] * 2, True),
                                    ("two_costs_finite_sum_not", T - 1, [2 ** (T - 1)] * 2, False),
                                    ("both_costs_over", T, [2 ** T] * 2, False)):
            ts, dims, con = _chain3(0, b)
            out.append(Ctor(f"{ctype}-vec-{name}", ts, dims, [con], ctype, [totals], ok))
        # a single cost over, the other far below; and the same tree one index of dimension 2 lower
        ts, dims, con = _chain3(T - 40, 40)
        out.append(Ctor(f"{ctype}-vec-single_cost_over", ts, dims, [con], ctype, [[2 ** T, 2 ** 40]], False))
        ts, dims, con = _chain3(T - 41, 40)
        out.append(Ctor(f"{ctype}-vec-single_cost_below", ts, dims, [con], ctype, [[2 ** (T - 1), 2 ** 40]], True))
        # uniform power-of-two dims (pow2_cost): three tensors that hold the same s hyper-indices, both costs 2^(k s)
        for name, k, s, ok in (("total_at_top_minus_1",) + {1024: (14, 73), 128: (14, 9)}[T] + (True,),
                               ("two_costs_finite_sum_not",) + {1024: (33, 31), 128: (1, 127)}[T] + (False,),
                               ("both_costs_over",) + {1024: (16, 64), 128: (16, 8)}[T] + (False,)):
            ts = [list(range(s))] * 3
            out.append(Ctor(f"{ctype}-uniform-{name}", ts, 1 << k, [[(0, 1, 3), (2, 3, 4)]], ctype, [[2 ** (k * s)] * 2], ok))
        # a batch in which only the last replica is over: tree X five times (and alone: constructs), then tree Y
        ts, dims, X, Y = _chain4(T - 80, 40, 40)
        tx = [2 ** (T - 40), 2 ** 80, 2 ** 40]
        ty = [2 ** T, 2 ** (T - 40), 2 ** 40]
        out.append(Ctor(f"{ctype}-batch-all_below", ts, dims, [X] * 5, ctype, [tx] * 5, True))
        out.append(Ctor(f"{ctype}-batch-last_replica_over", ts, dims, [X] * 5 + [Y], ctype, [tx] * 5 + [ty], False))
    return out


# how a constructor case is built: infinite memory, a best tree given (min_links = the trees), finite width with a loose
# bound (no slices) and with one that needs slices (the sliced costs count: a sliced index is in every contraction)
CTOR_VARIANTS = {"plain": {}, "min_links": {}, "fw_loose": dict(max_width=4096.0), "fw_sliced": dict(max_width=48.0)}


class BestTree:
    """A constructor case whose CURRENT tree constructs and whose BEST tree (`min_links`, and at finite width `min_slices`)
    decides: the check of get_cost(min_ctree[, min_slices]) is the only one that can refuse it.  The network of _chain4: the
    current tree is X, the best tree Y.  `min_slices`: index positions, or None; `kw`: max_width at finite width.
    `cur_costs` / `best_costs`: the exact costs as Python integers (exact_costs gives the same)."""

    def __init__(self, name, a, b, c, cost_type, kw, min_slices, ok):
        self.name, self.cost_type, self.kw, self.ok = name, cost_type, dict(kw), ok
        self.ts_inds, self.dims, self.cur, self.best = _chain4(a, b, c)
        nb0 = len(_split(a))
        self.min_slices = None if min_slices is None else (list(range(nb0, nb0 + len(_split(b)))) if min_slices == "B" else [])
        sl = 2 ** b if min_slices == "B" else 1  # (B is in the first cost of Y already; it multiplies the other two)
        self.cur_costs = [2 ** (a + b), 2 ** (b + c), 2 ** b]
        self.best_costs = [2 ** (a + b + c), 2 ** (a + c) * sl, 2 ** c * sl]

    def problem(self):
        return syn.Problem(self.ts_inds, self.dims)

    def trees(self, prob):
        return tuple(np.stack(ct.tree_from_contraction(c, prob.n)).astype(np.int32) for c in (self.cur, self.best))

    def min_slices_mask(self, prob):
        return None if self.min_slices is None else ct.pack_masks([self.min_slices], prob.n_inds)[0]


def best_tree_cases():
    out = []
    loose = dict(max_width=4096.0)  # (no tensor is wider: no slices are drawn, none is needed for the best tree)
    for ctype, T in TOP.items():
        for tag, kw, msl in (("", {}, None), ("-fw", loose, None), ("-fw_min_slices_empty", loose, "none")):
            # Y's first cost is 2^T: refused, whatever the current tree; one index of dimension 2 lower it constructs
            out.append(BestTree(f"{ctype}-best_tree_over{tag}", T - 80, 40, 40, ctype, kw, msl, False))
            out.append(BestTree(f"{ctype}-best_tree_below{tag}", T - 81, 40, 40, ctype, kw, msl, True))
        # ... and over only through its slices: B sliced makes Y's second cost 2^(T - 1) too
        out.append(BestTree(f"{ctype}-best_tree_over_by_its_slices", T - 81, 40, 40, ctype, loose, "B", False))
    return out
