"""The case table of the path-kernel tests (tests/test_gpu_contract_path.py, tests/test_contraction_path_plan.py):
three-tensor chains for `contraction.contract(..., path_kernel=G)`.

The base network is that of tests/batch_cases.py, sizes (I, K, J, L):

    A (p, u, i, k)   B (k, t, j)   C (t, u, j, l)   ->   (p, i, l)         path [(0, 1), (0, 1)]

sliced over p (3), u (2), t (2): 12 assignments, p placing blocks, u and t summed; B is gathered per assignment, A and C
are read in place.  The stored step has M, N, K = I, J, K, the output step I, L, J.  With a group of 2 the block of p = 0
is written by the groups (0, 1) and (2, 3): the second one adds to what an earlier launch left (beta from the table).

Each shape class of the dispatch (csrc/contract.hip launch_gemm; csrc/contract_path.h ct_path_step) is there as the
stored step and as the output step, at its smallest edge:
    tiled   M = N = 64 with K = 33 (the least K of the class, a k tail of 1 in the tiled kernel's 16-wide stage) and
            M = N = 65 with K = 48 (a second tile of one row and one column, no k tail);
    dot     K = 512 (the least) with 1 output (three quarters of the block idle), 5 (a second trip with one quarter at
            work) and 8192 outputs (the most); K = 515 with 5 outputs: a third trip over k that 3 lanes of a quarter take;
    stream  fewer outputs than the 1024 lanes of a block, and 1200: a second trip of the element loop.
Two more index patterns:
    "batch"     an index h (3) held by A, B, C and the output: both steps have H = 3;
    "permuted"  i is split into i1, i2 and the output step sums over i1 and j: the stored Z (i1, i2, j) is permuted arena
                to arena before the output step (a permute group between two steps, barriers on both sides).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import batch_cases as bc

PATH, SLICES, N_ASSIGNMENTS, DTYPES = bc.PATH, bc.SLICES, bc.N_ASSIGNMENTS, bc.DTYPES
GROUPS = (1, 2, 5, 12, 1024)


@dataclass(frozen=True)
class Batch(bc.Chain):
    """sizes (I, K, J, L) and h = 3 on every tensor: H = 3 in both steps."""

    @property
    def ts(self):
        return [("p", "u", "h", "i", "k"), ("k", "t", "h", "j"), ("t", "u", "h", "j", "l")]

    @property
    def output(self):
        return ("p", "h", "i", "l")

    @property
    def dims(self):
        return dict(super().dims, h=3)


@dataclass(frozen=True)
class Permuted(bc.Chain):
    """sizes (I2, K, J, L) and i1 = 3: Z (i1, i2, j), the output step sums over i1 and j."""

    @property
    def ts(self):
        return [("p", "u", "a", "i", "k"), ("k", "t", "j"), ("t", "u", "a", "j", "l")]

    @property
    def output(self):
        return ("p", "i", "l")

    @property
    def dims(self):
        return dict(super().dims, a=3)

    def steps(self):
        I, K, J, L = self.sizes
        return (3 * I, J, K), (I, L, 3 * J)


CASES = [
    bc.Chain("tiled-64x64x33-stored", (64, 33, 64, 3), ("tiled", "stream")),
    bc.Chain("tiled-65x65x48-stored", (65, 48, 65, 3), ("tiled", "stream")),
    bc.Chain("tiled-64x64x33-output", (64, 8, 33, 64), ("stream", "tiled")),
    bc.Chain("tiled-65x65x48-output", (65, 8, 48, 65), ("stream", "tiled")),
    bc.Chain("dot-1-stored", (1, 512, 1, 3), ("dot", "stream")),
    bc.Chain("dot-5-stored", (5, 512, 1, 3), ("dot", "stream")),
    bc.Chain("dot-8192-stored", (32, 512, 256, 3), ("dot", "stream")),
    bc.Chain("dot-1-output", (1, 5, 512, 1), ("stream", "dot")),
    bc.Chain("dot-5-output", (5, 5, 512, 1), ("stream", "dot")),
    bc.Chain("dot-8192-output", (32, 5, 512, 256), ("stream", "dot")),
    bc.Chain("stream-30-15", (5, 7, 6, 3), ("stream", "stream")),
    bc.Chain("stream-1200-1200", (40, 7, 30, 30), ("stream", "stream")),
    Batch("batch-h3", (5, 7, 6, 4), ("stream", "stream")),
    Permuted("permuted-intermediate", (5, 7, 6, 4), ("stream", "stream")),
    bc.Chain("dot-5-k515-stored", (5, 515, 1, 3), ("dot", "stream")),
]
SMALL = CASES[10]
DOT_TAIL, STREAM_TRIPS = CASES[14], CASES[11]  # a k tail in the dot class; a second trip of the element loop
SUMMED, PLACED = bc.SUMMED, bc.PLACED

for _c in CASES:
    assert tuple(bc.klass(*s) for s in _c.steps()) == _c.classes, _c.name
_outs = {c.name: tuple(m * n for m, n, _ in c.steps()) for c in CASES}
assert [_outs[f"dot-{n}-stored"][0] for n in (1, 5, 8192)] == [1, 5, 8192]
assert [_outs[f"dot-{n}-output"][1] for n in (1, 5, 8192)] == [1, 5, 8192]
assert _outs["stream-30-15"] == (30, 15) and _outs["stream-1200-1200"] == (1200, 1200)


def fill(chain, dtype, seed):
    """Leaves uniform in (0.5, 1.5) in both parts: no exact zeros, no cancellation."""
    rng = np.random.RandomState(seed)
    out = []
    for shape in chain.shapes():
        a = rng.uniform(0.5, 1.5, shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * rng.uniform(0.5, 1.5, shape)
        out.append(a.astype(dtype))
    return out


def einsum_reference(chain, arrays):
    """(the whole sliced sum, the same of the moduli) in double precision, axes in chain.output order."""
    sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in chain.ts for x in xs))}
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    args = lambda ws: [q for w, xs in zip(ws, chain.ts) for q in (w, [sym[x] for x in xs])]  # noqa: E731
    res = [sym[x] for x in chain.output]
    return np.einsum(*args(wide), res, optimize=True), np.einsum(*args([np.abs(w) for w in wide]), res, optimize=True)
