"""The case table of the `indirect=True` tests (tests/test_contraction_indirect_plan.py,
tests/test_gpu_contract_indirect.py): networks whose step operands lie in an order that fits neither [h][m][k] nor
[h][k][m], so that the plain plan permutes them and the plan with the keyword reads them in place.  No GPU and no device
import.

One-step networks (`one_step`): A holds (m1, [h], k, m2) and B (n1, k, [h], n2) when folded -- M = m1 m2 around k -- and
([h], m1, m2, k) / ([h], k, n1, n2) when direct; `fold` says which of the two is interleaved.  With `sliced` both carry
p (2, held by the output: block placement) and u (3, summed: beta = 1) outermost, so that they are leaves read in place
at the slice offset of the assignment.

Chains: the three-tensor chains of tests/batch_cases.py, whose leaf B (k, t, j) is not dense after slicing over t (the
plain plan gathers it in every assignment), and `reordered`, whose intermediate Z (i1, i2, j1, j2) is summed over
(i1, j1) by the next step and whose slice-free leaf (j1, k, j2) is a permute that `hoist=True` runs once.

`launch_counts(p)` is what a call launches, from the plan alone; `interpret` runs the tables with numpy on one flat
arena.
"""
from __future__ import annotations

import math

import numpy as np

from tests import batch_cases as bc
from tests import mode_cases as mc
from tnco_amd import contraction as ctr

DTYPES = ("float32", "float64", "complex64", "complex128")
FOLDS = ("a", "b", "both")
BATCHES = (1, 5, 64)


def one_step(name, M, N, K, H=1, fold="both", sliced=False, dtype="float32"):
    """M, N: (first factor, second factor) of the two axes that make up m and n."""
    h = ("h",) if H > 1 else ()
    lead = ("p", "u") if sliced else ()
    a = ("m1",) + h + ("k", "m2") if fold in ("a", "both") else h + ("m1", "m2", "k")
    b = ("n1", "k") + h + ("n2",) if fold in ("b", "both") else h + ("k", "n1", "n2")
    dims = dict(m1=M[0], m2=M[1], n1=N[0], n2=N[1], k=K)
    if H > 1:
        dims["h"] = H
    out = h + ("m1", "m2", "n1", "n2")
    if sliced:
        dims.update(p=2, u=3)
        out = ("p",) + out
    return mc.Case(name, (lead + a, lead + b), tuple(dims.items()), out, ((0, 1),), lead, dtype, "uniform")


# name -> (M factors, N factors, K, H, sliced, the shape class): every size at which the dispatch takes another kernel
SHAPES = {
    "tiled-64x64x33": ((8, 8), (8, 8), 33, 1, False, "tiled"),
    "tiled-65x129x48": ((5, 13), (3, 43), 48, 1, False, "tiled"),
    "tiled-64x64x33-h3": ((8, 8), (8, 8), 33, 3, False, "tiled"),
    "tiled-65x64x33-beta": ((5, 13), (8, 8), 33, 1, True, "tiled"),
    "dot-4x5x512": ((2, 2), (5, 1), 512, 1, False, "dot"),
    "dot-32x256x512": ((4, 8), (16, 16), 512, 1, False, "dot"),  # 8192 outputs: the last shape of the dot class
    "stream-33x256x512": ((3, 11), (16, 16), 512, 1, False, "stream"),  # 8448 outputs: beyond it
    "stream-4x5x511": ((2, 2), (5, 1), 511, 1, False, "stream"),  # K = 511: below the dot class
    "stream-63x64x33": ((7, 9), (8, 8), 33, 1, False, "stream"),
    "stream-7x9x11-h3": ((7, 1), (3, 3), 11, 3, False, "stream"),
    "stream-7x9x11-beta": ((7, 1), (3, 3), 11, 1, True, "stream"),
    "dot-3x5x512-h3-beta": ((3, 1), (5, 1), 512, 3, True, "dot"),
}
ONE_STEP = tuple((name, fold) for name in SHAPES for fold in FOLDS)
# stream: more outputs than one trip of the grid-stride loop covers (256 x 65536), the shape of tests/contract_cases.py
# with k = 3 inside the first operand (k = 2 leaves the tables 24 bytes larger than the copy: rule (b)); float32 only
# (64 MiB of output)
SECOND_TRIP = "stream-second_trip"


def case(name, fold="both", dtype="float32"):
    if name == SECOND_TRIP:
        return mc.Case(name, (("m1", "k", "m2"), ("k", "j")), (("m1", 41), ("k", 3), ("m2", 100), ("j", 4100)),
                       ("m1", "m2", "j"), ((0, 1),), (), "float32", "uniform")
    if name in CHAINS:
        return CHAINS[name].with_(dtype=dtype)
    M, N, K, H, sliced, _ = SHAPES[name]
    return one_step(f"{name}-{fold}", M, N, K, H, fold, sliced, dtype)


def _batch_chain(chain, slice_range=None):
    return mc.Case("chain-" + chain.name + ("" if slice_range is None else "-range"), tuple(chain.ts),
                   tuple(chain.dims.items()), chain.output, tuple(bc.PATH), bc.SLICES, "float32", "uniform", slice_range)


def reordered(name, slice_range=None):
    ts = (("p", "u", "i1", "i2", "k"), ("j1", "k", "j2"), ("u", "i1", "j1", "l"))
    dims = dict(p=3, u=2, i1=4, i2=5, k=6, j1=3, j2=7, l=2)
    return mc.Case(name, ts, tuple(dims.items()), ("p", "i2", "j2", "l"), ((0, 1), (0, 1)), ("p", "u"), "float32",
                   "uniform", slice_range)


# name -> case: 12 (reordered: 6) assignments; a range that starts at 1
CHAINS = {c.name: c for c in [_batch_chain(q) for q in bc.PLAIN] +
          [_batch_chain(bc.SMALL, (1, 11)), reordered("reordered"), reordered("reordered-range", (1, 6))]}
# name -> (operands folded without hoist, with hoist=True)
CHAIN_FOLDS = {**{name: (1, 1) for name in CHAINS if name.startswith("chain-")},
               "reordered": (2, 1), "reordered-range": (2, 1)}


def folded_sides(p):
    """Per step: (A is folded, B is folded)."""
    if p.ind_steps is None:
        return [(False, False)] * len(p.steps)
    return [(bool(r[0] >= 0), bool(r[3] >= 0)) for r in p.ind_steps]


def launch_counts(p):
    """(once, per): what the hoisted phase of a call launches and what one assignment (one group of a slice batch)
    launches, each (kernel_launches in KERNEL_PATHS order, indirect_launches in INDIRECT_KERNEL_PATHS order): a gather
    launch per permute group that has rows of the kind, a step with a folded operand in the slot of its class among the
    indirect kernels, every other step in its slot of the plain ones."""
    hoisting = p.hoisted is not None
    step_flags = p.step_hoist if hoisting else np.zeros(len(p.steps), np.int64)
    perm_flags = p.perm_hoist if hoisting else np.zeros(len(p.perms), np.int64)
    plain = [dict.fromkeys(ctr.KERNEL_PATHS, 0), dict.fromkeys(ctr.KERNEL_PATHS, 0)]  # [per, once]
    through = [dict.fromkeys(ctr.INDIRECT_KERNEL_PATHS, 0), dict.fromkeys(ctr.INDIRECT_KERNEL_PATHS, 0)]
    for g in set(p.perms[:, 6].tolist()):
        for kind in set(perm_flags[p.perms[:, 6] == g].tolist()):
            plain[kind]["gather"] += 1
    for sig, f, sides in zip(mc.signature(p), step_flags, folded_sides(p)):
        if any(sides):
            through[int(f)]["ix_" + sig[0]] += 1
        else:
            plain[int(f)][mc.kernel_slot(sig)] += 1
    return tuple((tuple(plain[q][n] for n in ctr.KERNEL_PATHS), tuple(through[q][n] for n in ctr.INDIRECT_KERNEL_PATHS))
                 for q in (1, 0))


def groups(n, B):
    """Launches of a step of the loop over n assignments: one per assignment, or per group of a slice batch."""
    return n if B is None else -(-n // min(B, n))


def interpret(p, arrays):
    """The plan's tables run with numpy on one flat arena, in double precision: the arena is NaN before the hoisted
    phase and, outside the kept buffers, after each assignment; a folded operand is read through ind_maps, a direct one
    through its strides.  A table that points at a buffer the plan has released or not yet written leaves a NaN."""
    wide = np.complex128 if any(np.iscomplexobj(a) for a in arrays) else np.float64
    leaves = [np.ascontiguousarray(a, wide).reshape(-1) for a in arrays]
    arena = np.full(max(p.arena_elems, 1), np.nan, wide)
    n_blocks = math.prod(p.shape[p.inds.index(x)] for x in p.block_inds)
    block = p.out_numel // n_blocks
    out = np.zeros(p.out_numel, wide)
    place = [math.prod(p.slice_dims[s + 1:]) for s in range(len(p.slice_dims))]
    hoisting = p.hoisted is not None
    step_h = p.step_hoist if hoisting else np.zeros(len(p.steps), np.int64)
    perm_h = p.perm_hoist if hoisting else np.zeros(len(p.perms), np.int64)
    outside = np.ones(len(arena), bool)
    for off, numel in p.kept:
        outside[off:off + numel] = False

    def slice_offset(leaf, sid):
        ls = p.leaf_sl[leaf]
        return sum(((sid // place[int(ls[1 + j])]) % p.slice_dims[int(ls[1 + j])]) * int(ls[1 + ctr.MAX_AXES + j])
                   for j in range(int(ls[0])))

    def gather(row, sid, out_off):
        nd = int(row[4])
        dims, strides = row[8:8 + nd], row[8 + ctr.MAX_AXES:8 + ctr.MAX_AXES + nd]
        idx = np.zeros(tuple(int(d) for d in dims), np.int64)
        for k in range(nd):
            shape = [1] * nd
            shape[k] = int(dims[k])
            idx = idx + (np.arange(int(dims[k])) * int(strides[k])).reshape(shape)
        idx = idx.reshape(-1)
        if row[0] == ctr.LEAF:
            vals = leaves[int(row[1])][idx + slice_offset(int(row[1]), sid)]
        else:
            vals = arena[idx + int(row[1])]
        if row[2] == ctr.ARENA:
            arena[int(row[3]):int(row[3]) + int(row[5])] = vals
        else:
            out[out_off:out_off + block] = vals

    def operand(k, side, sid, H, R, Kc):
        """[H][R][Kc] of operand `side` of step k: rows m of A, n of B."""
        st = [int(v) for v in p.steps[k]]
        kind, ref = st[4 * side], st[4 * side + 1]
        base = leaves[ref][slice_offset(ref, sid):] if kind == ctr.LEAF else arena[ref:]
        if folded_sides(p)[k][side]:
            assert st[4 * side + 2] == st[4 * side + 3] == 0
            o = [int(v) for v in p.ind_steps[k, 3 * side:3 * side + 3]]
            th = p.ind_maps[o[0]:o[0] + H]
            # (the tables of A: h, m, k; of B: h, k, n)
            tr, tk = (p.ind_maps[o[2]:o[2] + R], p.ind_maps[o[1]:o[1] + Kc]) if side else \
                (p.ind_maps[o[1]:o[1] + R], p.ind_maps[o[2]:o[2] + Kc])
            assert len(th) == H and len(tr) == R and len(tk) == Kc
            idx = th.reshape(-1, 1, 1) + tr.reshape(1, -1, 1) + tk.reshape(1, 1, -1)
        else:
            sr, sk = (st[7], st[6]) if side else (st[2], st[3])
            idx = (np.arange(H) * R * Kc).reshape(-1, 1, 1) + (np.arange(R) * sr).reshape(1, -1, 1) + \
                (np.arange(Kc) * sk).reshape(1, 1, -1)
        return base[idx]

    def step(k, sid, out_off, beta):
        st = [int(v) for v in p.steps[k]]
        H, M, N, K = st[10:14]
        A = operand(k, 0, sid, H, M, K)
        Bm = operand(k, 1, sid, H, N, K)
        Cm = np.einsum("hmk,hnk->hmn", A, Bm).reshape(-1)
        if st[8] == ctr.ARENA:
            arena[st[9]:st[9] + H * M * N] = Cm
        else:
            out[out_off:out_off + block] = out[out_off:out_off + block] + Cm if beta else Cm

    def run(sid, out_off, beta, hoisted):
        for g in [-1] + list(range(len(p.steps))):
            for r in np.nonzero((p.perms[:, 6] == g) & (perm_h == hoisted))[0]:
                gather(p.perms[r], sid, out_off)
            if g >= 0 and step_h[g] == hoisted:
                step(g, sid, out_off, beta)

    if hoisting and any(p.hoisted):
        run(p.slice_range[0], 0, 0, 1)
    visited = set()
    for sid in range(*p.slice_range):
        blk = 0
        for x in p.block_inds:
            s = p.slice_inds.index(x)
            blk = blk * p.slice_dims[s] + (sid // place[s]) % p.slice_dims[s]
        run(sid, blk * block, blk in visited, 0)
        visited.add(blk)
        arena[outside] = np.nan
    return ctr._host_layout(p, out)
