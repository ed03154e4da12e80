"""A plain restatement of the reference's `is_valid(atol)` over the state a replica's getters return, and the readers
that collect that state from an oracle replica and from a GPU replica.  numpy / float64, no device code: the expected
verdicts of tests/test_gpu_validate.py, held to `oracle.is_valid()` by tests/test_validate_model.py.

Restated: include/tnco/optimize/infinite_memory/optimizer.hpp:223-251 and finite_width/greedy/optimizer.hpp:392-444
(`is_valid`), include/tnco/utils.hpp:78-87 (`is_logclose`), include/tnco/ctree.hpp:101-152 (the leg rule of every
contraction), the cost and width models of cost_model/simple*.hpp.  Two things are stricter than the reference, as the
product is: child and parent links must agree node by node (the reference's counters accept some
trees whose links disagree, include/tnco/tree.hpp:113-131), and the stored legs must EQUAL the legs derived from the
leaves (tnco/ctree.py:163-189) -- the device stores no HyperCache to compare, its hyper legs are a function of the legs.
"""
from __future__ import annotations

import numpy as np

U64 = np.uint64


class Model:
    """The problem description the verdict depends on (the constructor arguments of the optimizer)."""

    def __init__(self, leaf_masks, n_inds, *, dims=2, output_mask=None, sparse_mask=None, n_projs=0, cost_type="float64",
                 disable_shared_inds=False, max_width=None, width_type="float32"):
        self.leaf_masks = np.ascontiguousarray(leaf_masks, U64)
        self.n, self.W = self.leaf_masks.shape
        self.N = 2 * self.n - 1
        self.n_inds = n_inds
        self.output_mask = np.zeros(self.W, U64) if output_mask is None else np.ascontiguousarray(output_mask, U64)
        self.dim_uniform, self.dims_vec = None, None
        if np.ndim(dims) == 0:
            self.dim_uniform = int(dims)
        else:
            dv = np.asarray(dims, U64)
            if len(dv) and np.all(dv == dv[0]):  # ctree.hpp:79-89: all-equal dims collapse to the scalar form
                self.dim_uniform = int(dv[0])
            else:
                self.dims_vec = np.zeros(64 * self.W, U64)
                self.dims_vec[:len(dv)] = dv
        self.sparse = None if sparse_mask is None or not np.any(sparse_mask) else np.ascontiguousarray(sparse_mask, U64)
        self.n_projs = int(n_projs)
        self.ct = np.float64 if cost_type == "float64" else np.float32
        self.disable_shared_inds = bool(disable_shared_inds)
        self.fw = max_width is not None
        self.wt = np.float32 if width_type == "float32" else np.float64
        self.max_width = None if max_width is None else float(self.wt(max_width))


def bits(mask) -> list:
    """Set positions of a [W] mask, ascending (Bitset::visit order)."""
    b = np.unpackbits(np.ascontiguousarray(mask, "<u8").view(np.uint8), bitorder="little")
    return np.flatnonzero(b).tolist()


def popcount(mask) -> int:
    return int(np.unpackbits(np.ascontiguousarray(mask, "<u8").view(np.uint8)).sum())


def traverse(left, right) -> list:
    """Post-order of include/tnco/utils.hpp:34-51, None when the links do not form a tree of N nodes."""
    N = len(left)
    order, stack, seen = [], [N - 1], np.zeros(N, bool)
    while stack:
        pos = stack[-1]
        if seen[pos] or left[pos] < 0:
            stack.pop()
            order.append(pos)
        else:
            seen[pos] = True
            stack.append(int(right[pos]))
            stack.append(int(left[pos]))
        if len(order) + len(stack) > 2 * N:
            return None
    return order if len(order) == N and len(set(order)) == N else None


def links_consistent(left, right, parent) -> bool:
    """Node::is_valid + Tree::is_valid (node.hpp:72-107, tree.hpp:58-139) with the counters read as they are meant:
    one root, the last node; leaves first; every internal node has two different children, each of which names it as
    its parent; every node but the root is the child of exactly one node."""
    left, right, parent = (np.asarray(x, np.int64) for x in (left, right, parent))
    N = len(left)
    n = (N + 1) // 2
    for x in (left, right, parent):
        if np.any((x < -1) | (x >= N)):
            return False
    if np.any((left < 0) != (right < 0)) or np.any((left >= 0) & (left == right)):
        return False
    if np.any((left >= 0) & (parent >= 0) & ((parent == left) | (parent == right))):
        return False
    if parent[N - 1] != -1 or np.count_nonzero(parent < 0) != 1:
        return False
    if np.any(left[:n] >= 0) or np.any(left[n:] < 0):
        return False
    inner = np.arange(n, N)
    if np.any(parent[left[inner]] != inner) or np.any(parent[right[inner]] != inner):
        return False
    child_of = np.bincount(np.concatenate([left[inner], right[inner]]), minlength=N)
    named = np.bincount(parent[parent >= 0], minlength=N)
    want_children = np.where(np.arange(N) == N - 1, 0, 1)
    want_named = np.where(left < 0, 0, 2)
    return bool(np.all(child_of == want_children) and np.all(named == want_named))


def derive_legs(model: Model, left, right, order):
    """Legs of every node from the leaves: z = (x ^ y) | (x & y & outside(z)), outside(z) = the output legs and the legs
    of the leaves that are not below z (tnco/ctree.py:163-189 restated over sets)."""
    n, N, W = model.n, model.N, model.W
    below = np.zeros((N, W), U64)
    below[:n] = model.leaf_masks
    for p in order:
        if left[p] >= 0:
            below[p] = below[left[p]] | below[right[p]]
    outside = np.zeros((N, W), U64)
    outside[N - 1] = model.output_mask
    for p in reversed(order):
        if left[p] >= 0:
            outside[left[p]] = outside[p] | below[right[p]]
            outside[right[p]] = outside[p] | below[left[p]]
    legs = np.zeros((N, W), U64)
    legs[:n] = model.leaf_masks
    for p in order:
        if left[p] >= 0:
            a, b = legs[left[p]], legs[right[p]]
            legs[p] = (a ^ b) | (a & b & outside[p])
    return legs


def contraction_valid(model: Model, left, right, legs) -> bool:
    """ctree.hpp:101-152: (a ^ b) <= out <= (a | b) at every contraction, and a & b non-empty unless disabled."""
    for p in range(model.n, model.N):
        a, b, o = legs[left[p]], legs[right[p]], legs[p]
        if not model.disable_shared_inds and not np.any(a & b):
            return False
        if np.any((a ^ b) & ~o) or np.any(o & ~(a | b)):
            return False
    return True


def _get_cost(model: Model, mask):
    """cost_model/simple.hpp:37-55: pow(dims, count) in double converted to cost_type; per-index dims: the running
    product in cost_type over ascending positions."""
    ct = model.ct
    with np.errstate(over="ignore"):
        if model.dims_vec is None:
            return ct(np.float64(model.dim_uniform) ** np.float64(popcount(mask)))
        c = ct(1)
        for p in bits(mask):
            c = ct(c * ct(model.dims_vec[p]))
        return c


def contraction_cost(model: Model, a, b, slices=None):
    """simple.hpp:66-83, simple_sparse_inds.hpp:37-49; finite width: the sliced indices joined in
    (finite_width/cost_model/simple.hpp:127-147)."""
    u = a | b if slices is None else a | b | slices
    if model.sparse is None:
        return _get_cost(model, u)
    c1, c2 = _get_cost(model, u & ~model.sparse), _get_cost(model, u & model.sparse)
    np_ = model.ct(model.n_projs)
    with np.errstate(over="ignore", invalid="ignore"):
        return model.ct(c1 * (c2 if c2 < np_ else np_))


def cost_cache(model: Model, left, right, legs, order, slices=None):
    """CostCache (infinite_memory/utils.hpp:31-57) and get_cost (:102-116) in the reference's association order:
    partial = (c + partial[left]) + partial[right]; total = the costs summed in traverse order; all in cost_type."""
    ct = model.ct
    cc, pc = np.zeros(model.N, np.float64), np.zeros(model.N, np.float64)
    total = ct(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in order:
            if left[p] < 0:
                continue
            c = contraction_cost(model, legs[left[p]], legs[right[p]], slices)
            cc[p] = c
            pc[p] = ct(ct(c + ct(pc[left[p]])) + ct(pc[right[p]]))
            total = ct(total + c)
    return cc, pc, float(total)


def is_logclose(x, y, atol) -> bool:
    """include/tnco/utils.hpp:78-87."""
    x, y = float(x), float(y)
    if x < 0 or y < 0:
        return False
    if x == 0 or y == 0:
        return x == y
    with np.errstate(all="ignore"):
        return bool(abs(np.log(np.float64(x)) - np.log(np.float64(y))) <= atol)  # (NaN: not close)


def _width_simple(model: Model, mask) -> float:
    """finite_width/cost_model/simple.hpp:38-57."""
    wt = model.wt
    if model.dims_vec is None:
        return float(wt(np.log2(np.float64(model.dim_uniform)) * np.float64(popcount(mask))))
    w = wt(0)
    for p in bits(mask):
        w = wt(np.float64(w) + np.log2(np.float64(model.dims_vec[p])))
    return float(w)


def width(model: Model, mask) -> float:
    """... and simple_sparse_inds.hpp:38-52: width(inds - S) + min(width(inds & S), log2(n_projs))."""
    if model.sparse is None:
        return _width_simple(model, mask)
    w1, w2 = _width_simple(model, mask & ~model.sparse), _width_simple(model, mask & model.sparse)
    l2 = float(np.log2(np.float64(model.n_projs)))
    return float(model.wt(w1 + (w2 if w2 < l2 else float(model.wt(l2)))))


def is_valid(model: Model, s: dict, atol: float = 1e-5) -> bool:
    """The verdict for one replica.  `s`: left, right, parent [N], legs [N, W], ccost, partial [N] of the current tree;
    min_left, min_right, min_parent of the best tree; min_total_cost; finite width: slices, min_slices [W] and widths [N]
    (NaN where the replica caches none)."""
    l, r, p = s["left"], s["right"], s["parent"]
    ml, mr, mp = s["min_left"], s["min_right"], s["min_parent"]
    # the trees (optimize/optimizer.hpp base is_valid: ctree and min_ctree)
    if not links_consistent(l, r, p) or not links_consistent(ml, mr, mp):
        return False
    order, morder = traverse(l, r), traverse(ml, mr)
    if order is None or morder is None:
        return False
    legs = derive_legs(model, l, r, order)
    if not np.array_equal(legs, np.asarray(s["legs"], U64)) or not contraction_valid(model, l, r, legs):
        return False
    mlegs = derive_legs(model, ml, mr, morder)
    if not contraction_valid(model, ml, mr, mlegs):
        return False
    sl = np.asarray(s["slices"], U64) if model.fw else None
    msl = np.asarray(s["min_slices"], U64) if model.fw else None
    # the best tree's cost
    if not is_logclose(cost_cache(model, ml, mr, mlegs, morder, msl)[2], s["min_total_cost"], atol):
        return False
    # widths after slicing
    if model.fw:
        for i in range(model.N):
            if width(model, legs[i] & ~sl) > model.max_width or width(model, mlegs[i] & ~msl) > model.max_width:
                return False
    # CostCache
    cc, pc, _ = cost_cache(model, l, r, legs, order, sl)
    for i in range(model.N):
        if not is_logclose(cc[i], s["ccost"][i], atol) or not is_logclose(pc[i], s["partial"][i], atol):
            return False
    # WidthCache: is_close, |x - y| <= atol (utils.hpp:74-76)
    if model.fw:
        for i in range(model.N):
            c = s["widths"][i]
            if i < model.n and np.isnan(c):
                continue  # (the device caches the widths of internal nodes only)
            if not abs(width(model, legs[i]) - c) <= atol:
                return False
    return True


def verdicts(model: Model, states, atol: float = 1e-5) -> np.ndarray:
    """True = valid, one per state."""
    return np.array([is_valid(model, s, atol) for s in states], bool)


def expected_validate(bad_ids) -> tuple:
    """(n_bad, first_bad) of tnco_hip_validate for the set of replicas that are not valid."""
    bad = sorted(int(x) for x in bad_ids)
    return (len(bad), bad[0] if bad else -1)


def oracle_state(o) -> dict:
    l, r, p, m = o.tree()
    ml, mr, mp, _ = o.tree(which_min=True)
    cc, pc, _ = o.caches()
    s = dict(left=l, right=r, parent=p, legs=m, ccost=cc, partial=pc, min_left=ml, min_right=mr, min_parent=mp,
             min_total_cost=o.min_total_cost)
    if o.fw:
        s["slices"], s["min_slices"] = o.slices()
        s["widths"] = o.widths()
    return s


def gpu_layout(gpu) -> str:
    """"child-partial", "unified" or "split" (finite width), found by asking for the fields only one of them stores."""
    if gpu.finite_width:
        return "split"
    try:
        gpu._poke(0, "total")
        return "child-partial"
    except ValueError:
        return "unified"


def gpu_state(gpu, r: int, layout: str | None = None) -> dict:
    """The same through the GPU handle's getters.  What no getter returns is read through the poke entry point without
    writing: min_total_cost of one replica, the cached widths, and -- child-partial layout -- the slot a parent keeps
    for the partial cost of a LEAF child (get_caches reports the 0 a leaf has, whatever the slot holds)."""
    layout = layout or gpu_layout(gpu)
    n, N = gpu.n_leaves, gpu.n_nodes
    l, rr, p, m = gpu.tree(r)
    ml, mr, mp, _ = gpu.tree(r, which_min=True, with_masks=False)
    cc, pc, _ = gpu.caches(r)
    if layout == "child-partial":
        for x in range(n):
            par = int(p[x])
            if n <= par < N and (l[par] == x or rr[par] == x):
                pc[x] = gpu._poke(r, "partial_left" if l[par] == x else "partial_right", node=par)
    s = dict(left=l, right=rr, parent=p, legs=m, ccost=cc, partial=pc, min_left=ml, min_right=mr, min_parent=mp,
             min_total_cost=gpu._poke(r, "min_cost"))
    if gpu.finite_width:
        s["slices"], s["min_slices"] = gpu.slices(r)
        w = np.full(N, np.nan)
        for i in range(n, N):
            w[i] = gpu._poke(r, "width", node=i)
        s["widths"] = w
    return s
