"""The tree check of tnco_hip_create as a model, and the trees it is tested on (no GPU, no library).

Two rules over link arrays [3, N] (rows: left, right, parent; null = -1; leaves in slots 0..n-1, N = 2n - 1):

* `reference_verdict`: Node::Node + Node::is_valid (include/tnco/node.hpp:45-106) and Tree::is_valid
  (include/tnco/tree.hpp:57-139) AS WRITTEN.  The constructor maps every negative entry to null before anything is
  checked.  The two counter lambdas read `c == node.is_leaf() ? 0 : 2` and `c == node.is_root() ? 0 : 1`, which parse as
  `(c == is_leaf) ? 0 : 2` and `(c == is_root) ? 0 : 1`: a node passes when its count DIFFERS from the flag (a leaf may be
  named as parent by any number of nodes but one, an internal node by any number but none).  No child link is compared
  with the child's parent word.  `n_leaves()` asserts the leaf count unless NDEBUG is defined; oracle/_ref is built
  without it, so the rule refuses there (`assertions=True`).
* `library_status`: 0, or the number of the first failing check of the host `tree_check` (csrc/tnco_hip.hip): 1-5 as the
  reference, entries strictly -1 or in range; 6 = the two counters as the reference's COMMENTS say (a leaf is nobody's
  parent, another node is the parent of two; every node but the root is one node's child) and every child link answered
  by the child's parent word; 7 = the traverse from the root reaches all N nodes.
  `device_status` is `tree_check_kernel`'s rule: 1-5, then 6 from the child links alone, no 7.

The rules work on batches [T, 3, N]; `parts` returns the single conditions, which the tests combine.
"""
from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
L, R, P = 0, 1, 2

MESSAGES = {
    1: "Nodes are not valid",
    2: "Last node should be root.",
    3: "There should be only one root.",
    4: "All leaves should be first.",
    5: "Number of nodes is not constenst with the number of leaves.",
    6: "Tree is not valid.",
    7: "Tree is not valid.",
}

SIZES = (3, 5, 7, 9, 127, 129, 4095)  # 127 -> 129: one more trip of the kernel's `i += 64` lane loop; 4095: 64 trips


# ---- the two rules -----------------------------------------------------------------------------------------------------

def _counts(l, r, p, N):
    """cp[t, i]: nodes of tree t whose parent word is i; cc[t, i]: child links of tree t that name i (entries out of range
    are not counted: check 1 has refused such a tree)."""
    T = l.shape[0]
    rows = np.broadcast_to(np.arange(T)[:, None], l.shape)
    cp, cc = np.zeros((T, N), np.int64), np.zeros((T, N), np.int64)
    inner = (l >= 0) & (l < N) & (r >= 0) & (r < N)
    np.add.at(cc, (rows[inner], l[inner]), 1)
    np.add.at(cc, (rows[inner], r[inner]), 1)
    hasp = (p >= 0) & (p < N)
    np.add.at(cp, (rows[hasp], p[hasp]), 1)
    return cp, cc


def _reached(l, r, N):
    """Nodes the traverse from the root visits (utils.hpp:34-51 restated: a stack, every node expanded once)."""
    seen = np.zeros(N, bool)
    stack = [N - 1]
    while stack:
        i = stack.pop()
        if seen[i]:
            continue
        seen[i] = True
        if l[i] >= 0:
            stack += [int(l[i]), int(r[i])]
    return int(seen.sum())


def parts(trees):
    """The conditions of the strict rule on every tree of [T, 3, N] (true = the check FAILS): c1..c5, `counters` and
    `links` (the two halves of check 6), `reach` (check 7; evaluated where nothing earlier fails, false elsewhere)."""
    t = np.asarray(trees, np.int64)
    t = t.reshape((-1,) + t.shape[-2:])
    T, _, N = t.shape
    n = (N + 1) // 2
    l, r, p = t[:, L], t[:, R], t[:, P]

    def in_range(x):
        return (x == -1) | ((x >= 0) & (x < N))

    bad = ~(in_range(l) & in_range(r) & in_range(p)) | ((l < 0) != (r < 0)) | ((l >= 0) & (l == r)) \
        | ((l >= 0) & (p >= 0) & ((p == l) | (p == r)))
    out = dict(c1=bad.any(1), c2=p[:, N - 1] != -1, c3=(p < 0).sum(1) != 1, c4=(l[:, :n] >= 0).any(1), c5=(l < 0).sum(1) != n)
    cp, cc = _counts(l, r, p, N)
    out["counters"] = ((cp != np.where(l < 0, 0, 2)) | (cc != np.where(p < 0, 0, 1))).any(1)
    lc, rc = np.clip(l, 0, N - 1), np.clip(r, 0, N - 1)
    me = np.arange(N)[None, :]
    unanswered = (l >= 0) & (r >= 0) & ((np.take_along_axis(p, lc, 1) != me) | (np.take_along_axis(p, rc, 1) != me))
    out["links"] = unanswered.any(1)
    early = out["c1"] | out["c2"] | out["c3"] | out["c4"] | out["c5"] | out["counters"] | out["links"]
    out["reach"] = np.zeros(T, bool)
    for k in np.flatnonzero(~early):
        out["reach"][k] = _reached(l[k], r[k], N) != N
    return out


def _first(conds):
    st = np.zeros(len(conds[0][1]), np.int32)
    for code, c in reversed(conds):
        st[c] = code
    return st


def library_status(trees, q=None):
    q = q or parts(trees)
    return _first([(1, q["c1"]), (2, q["c2"]), (3, q["c3"]), (4, q["c4"]), (5, q["c5"]), (6, q["counters"] | q["links"]), (7, q["reach"])])


def device_status(trees, q=None):
    q = q or parts(trees)
    return _first([(1, q["c1"]), (2, q["c2"]), (3, q["c3"]), (4, q["c4"]), (5, q["c5"]), (6, q["links"])])


def reference_verdict(trees, assertions=True):
    """bool[T]: Tree(nodes) of the reference is constructed and is_valid()."""
    t = np.asarray(trees, np.int64)
    t = t.reshape((-1,) + t.shape[-2:])
    T, _, N = t.shape
    t = np.where(t < 0, -1, t)  # Node::Node
    l, r, p = t[:, L], t[:, R], t[:, P]
    leaf, root = l == -1, p == -1
    node_ok = ~((l < 0) ^ (r < 0)) & ~(~leaf & (l == r)) & ~(~leaf & ~root & ((p == l) | (p == r)))  # Node::is_valid
    node_ok &= (l < N) & (r < N) & (p < N)  # Tree::is_valid, the lambda of "Nodes are not valid"
    ok = node_ok.all(1) & root[:, N - 1] & (root.sum(1) == 1)
    n = (N + 1) // 2  # n_leaves(): (size() + 1) / 2, with ASSERT(count of leaves == that)
    if assertions:
        ok &= leaf.sum(1) == n
    ok &= leaf[:, :n].all(1)
    ok &= N == 2 * n - 1
    cp, cc = _counts(l, r, p, N)
    ok &= (cp != leaf.astype(np.int64)).all(1)  # (c == is_leaf) ? 0 : 2  -> true where they differ
    ok &= (cc != root.astype(np.int64)).all(1)  # (c == is_root) ? 0 : 1
    return ok


# ---- valid trees -------------------------------------------------------------------------------------------------------

def from_pairs(n, pairs):
    """links [3, N] of the tree whose k-th internal node n + k joins the nodes pairs[k]."""
    N = 2 * n - 1
    t = np.full((3, N), -1, np.int32)
    for k, (a, b) in enumerate(pairs):
        t[L, n + k], t[R, n + k] = a, b
        t[P, a] = t[P, b] = n + k
    return t


def left_deep(n):
    return from_pairs(n, [(0, 1)] + [(n + k - 1, k + 1) for k in range(1, n - 1)])


def right_deep(n):
    return from_pairs(n, [(0, 1)] + [(k + 1, n + k - 1) for k in range(1, n - 1)])


def balanced(n):
    level, nxt, pairs = list(range(n)), n, []
    while len(level) > 1:
        up = []
        for k in range(0, len(level) - 1, 2):
            pairs.append((level[k], level[k + 1]))
            up.append(nxt)
            nxt += 1
        level = up + ([level[-1]] if len(level) % 2 else [])
    return from_pairs(n, pairs)


def native_random(n, seed=12345):
    """One tree of core.random_trees (host code of the library, no GPU) on an open chain of n tensors."""
    from tnco_amd import core
    from tnco_amd.synthetic import chain_tn
    return core.random_trees(chain_tn(n)[0], n - 1, [seed])[0]


def random_merges(n, rng):
    live, pairs = list(range(n)), []
    for k in range(n - 1):
        a = live.pop(int(rng.randint(len(live))))
        b = live.pop(int(rng.randint(len(live))))
        pairs.append((a, b))
        live.append(n + k)
    return from_pairs(n, pairs)


BASES = {"left_deep": left_deep, "right_deep": right_deep, "balanced": balanced, "native_random": native_random}


def ring(N, base=left_deep):
    """Not a tree, yet checks 1-6 pass: a valid tree over the leaves 0..n-4 (root N - 1) and, beside it, the internal
    nodes A, B, C = n, n + 1, n + 2 in a ring -- A holds (B, leaf n - 3), B holds (C, leaf n - 2), C holds (A, leaf n - 1),
    each the parent of the next.  N = 9: the root over two leaves plus the ring."""
    n = (N + 1) // 2
    m = n - 3  # leaves of the valid part; its internal node m + k becomes n + 3 + k
    sub = base(m).astype(np.int64)
    t = np.full((3, N), -1, np.int32)
    move = lambda x: np.where(x >= m, x + (n + 3 - m), x)  # noqa: E731
    for i in range(2 * m - 1):
        j = int(move(np.int64(i)))
        t[:, j] = np.where(sub[:, i] >= 0, move(sub[:, i]), -1)
    a, b, c = n, n + 1, n + 2
    for node, nxt, leaf, par in ((a, b, n - 3, c), (b, c, n - 2, a), (c, a, n - 1, b)):
        t[L, node], t[R, node], t[P, node] = nxt, leaf, par
        t[P, leaf] = node
    return t


# ---- named damages -----------------------------------------------------------------------------------------------------
# name -> (code, f(t, at) -> bool): `t` [3, N], a valid tree, is damaged in place at node `at`; False: not applicable there

def _set(field, value):
    def f(t, at):
        N = t.shape[1]
        t[field, at] = N if value == "N" else value
        return True
    return f


def _one_child_null(t, at):
    N = t.shape[1]
    if t[L, at] >= 0:
        t[L, at] = -1
    else:
        t[R, at] = N - 1
    return True


def _same_children(t, at):
    N = t.shape[1]
    if t[L, at] >= 0:
        t[R, at] = t[L, at]
    else:
        t[L, at] = t[R, at] = N - 1
    return True


def _parent_is(child):
    def f(t, at):
        if t[L, at] < 0:
            return False
        t[P, at] = t[child, at]
        return True
    return f


def _last_gets_parent(t, at):
    N = t.shape[1]
    if at != N - 1:
        return False
    t[P, at] = next(x for x in range(N) if x not in (t[L, at], t[R, at]))  # (N = 3: the root itself)
    return True


def _second_root(t, at):
    if at == t.shape[1] - 1:
        return False
    t[P, at] = -1
    return True


def _leaf_with_children(t, at):
    N = t.shape[1]
    if t[L, at] >= 0:
        return False
    cand = [x for x in range(min(N, 8)) if x != t[P, at]]
    cand = [x for x in cand if x != at] + [at]  # (N = 3 leaves one node besides the parent and the leaf itself)
    t[L, at], t[R, at] = cand[0], cand[1]
    return True


def _internal_to_leaf(t, at):
    if t[L, at] < 0:
        return False
    t[L, at] = t[R, at] = -1
    return True


def _swap_parent_words(t, at):
    """the parent words of `at` and of a child of another parent exchanged: every count stays, two links lie"""
    N = t.shape[1]
    if at == N - 1:
        return False
    mine = (t[L, at], t[R, at])
    for b in range(N - 1):
        theirs = (t[L, b], t[R, b])
        if b != at and t[P, b] != t[P, at] and t[P, b] not in mine and t[P, at] not in theirs:
            t[P, at], t[P, b] = t[P, b], t[P, at]
            return True
    return False


def _child_of_two(t, at):
    N = t.shape[1]
    if t[L, at] < 0:
        return False
    for c in range(N - 1):
        if c != at and t[P, c] != at and c != t[R, at] and c != t[P, at]:
            t[L, at] = c
            return True
    return False


def _leaf_as_parent(t, at):
    N = t.shape[1]
    if at == N - 1:
        return False
    n = (N + 1) // 2
    for leaf in range(n):
        if leaf != at and leaf not in (t[L, at], t[R, at]):
            t[P, at] = leaf
            return True
    return False


DAMAGES = {}
for _fname, _field in (("parent", P), ("left", L), ("right", R)):
    for _vname, _v in (("N", "N"), ("-2", -2), ("INT32_MIN", INT32_MIN), ("INT32_MAX", INT32_MAX)):
        DAMAGES[f"{_fname}={_vname}"] = (1, _set(_field, _v))
DAMAGES.update({
    "one child null": (1, _one_child_null),
    "left == right": (1, _same_children),
    "parent == left": (1, _parent_is(L)),
    "parent == right": (1, _parent_is(R)),
    "last node has a parent": (2, _last_gets_parent),
    "second root": (3, _second_root),
    "leaf slot with children": (4, _leaf_with_children),
    "internal node turned leaf": (5, _internal_to_leaf),
    "parent words exchanged": (6, _swap_parent_words),
    "child of two parents": (6, _child_of_two),
    "leaf named as parent": (6, _leaf_as_parent),
})


def positions(N):
    n = (N + 1) // 2
    return sorted({x for x in (0, 63, 64, n - 1, n, N - 1) if 0 <= x < N})


_named = {}


def named(N):
    """[(label, code, links[3, N])]: every damage at every position of every base tree of size N it applies to, and the
    rings (code 7) at N = 9 and N = 129.  Built once per size; callers copy before they write."""
    if N not in _named:
        n = (N + 1) // 2
        out = []
        for bname, base in BASES.items():
            tree = base(n)
            for dname, (code, f) in DAMAGES.items():
                for at in positions(N):
                    t = tree.copy()
                    if f(t, at):
                        out.append((f"{bname} N={N} {dname} @{at}", code, t))
        if N == 9:
            out.append(("ring N=9", 7, ring(9)))
        if N == 129:
            out += [(f"ring below {b} N=129", 7, ring(129, BASES[b])) for b in ("left_deep", "balanced")]
        for _, _, t in out:
            t.setflags(write=False)
        _named[N] = out
    return _named[N]


def named_arrays(N):
    cases = named(N)
    return [c[0] for c in cases], np.array([c[1] for c in cases], np.int32), np.stack([c[2] for c in cases])


def valid_trees(N):
    n = (N + 1) // 2
    return np.stack([b(n) for b in BASES.values()])


# ---- families ----------------------------------------------------------------------------------------------------------

def exhaustive():
    """All 4^9 link arrays of N = 3 with entries in {-1, 0, 1, 2}; tree k has the base-4 digits of k (entry 0 lowest)."""
    k = np.arange(4**9, dtype=np.int64)
    return np.stack([(k >> (2 * j)) & 3 for j in range(9)], 1).reshape(-1, 3, 3).astype(np.int32) - 1


RANDOM_FAMILIES = {3: 20000, 4: 20000, 33: 3000, 65: 3000}  # leaves -> trees
_random = {}


def random_damage(n, seed=2024):
    """RANDOM_FAMILIES[n] trees of n leaves (random merges), 1-3 entries of each replaced by draws from {-2, ..., N}."""
    if n not in _random:
        rng = np.random.RandomState(seed + n)
        N, T = 2 * n - 1, RANDOM_FAMILIES[n]
        out = np.empty((T, 3, N), np.int32)
        for k in range(T):
            t = random_merges(n, rng)
            for _ in range(rng.randint(1, 4)):
                t[rng.randint(3), rng.randint(N)] = rng.randint(-2, N + 1)
            out[k] = t
        out.setflags(write=False)
        _random[n] = out
    return _random[n]


FAMILY_NAMES = ["exhaustive"] + [f"named N={N}" for N in SIZES] + [f"random n={n}" for n in RANDOM_FAMILIES]
_families = {}


def family(name):
    """trees [T, 3, N] of one family (built once)."""
    if name not in _families:
        kind, _, arg = name.partition("=")
        if name == "exhaustive":
            t = exhaustive()
        elif kind == "named N":
            t = np.concatenate([named_arrays(int(arg))[2], valid_trees(int(arg))])
        else:
            t = random_damage(int(arg))
        _families[name] = t
    return _families[name]


def families():
    """name -> trees [T, 3, N]: what the model, the host check, the kernel and the reference are compared on."""
    return {name: family(name) for name in FAMILY_NAMES}


# ---- the two mask conditions of ContractionTree::is_valid (include/tnco/ctree.hpp:101-152) ---------------------------------

def mask_status(left, right, node_masks, leaf_masks, output_mask, check_shared=True):
    """What build_kernel reports for explicit `node_masks` [N, W] on a valid tree: 0; 10 a contraction of two tensors that
    share no index; 11 a node's legs are not (a ^ b) plus shared legs that stay open, i.e. it has a leg neither child has
    or misses one that only one child has ("Contraction is not valid." both); 12 a leaf row differs from `leaf_masks`."""
    N, n = len(left), len(leaf_masks)
    if not np.array_equal(node_masks[:n], leaf_masks):
        return 12
    for i in range(n, N):
        a, b, x = node_masks[left[i]], node_masks[right[i]], node_masks[i]
        if check_shared and not (a & b).any():
            return 10
        if (((a ^ b) & ~x) | (x & ~(a | b))).any():
            return 11
    return 0


MASK_MESSAGES = {10: "Contraction is not valid.", 11: "Contraction is not valid.", 12: "'node_masks' leaves differ from 'leaf_masks'."}
