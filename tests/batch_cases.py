"""The case table of the slice-batch tests (tests/test_gpu_contract_batch.py): three-tensor chains for
`contraction.contract(..., slice_batch=B)`.

The base network, sizes (I, K, J, L):

    A (p, u, i, k)   B (k, t, j)   C (t, u, j, l)   ->   (p, i, l)         path [(0, 1), (0, 1)]

sliced over p (dim 3), u (2), t (2), in that order (p the most significant digit): 12 assignments.  p is held by the
result and places blocks, u and t are summed.  p and u are the outermost axes of A, t and u of C: both are read in
place at an offset that depends on the assignment; t is an inner axis of B, which is gathered per assignment.  The first
step Z (i, j) = A B has M, N, K = I, J, K and is stored to the arena, the second, Z C, has M, N, K = I, L, J and writes
the output.  With a batch of 5 the batches are assignments 0..4 (blocks 0 0 0 0 1: members that share a block, and a
batch that splits over two), 5..9 (1 1 1 2 2) and 10..11 (partial), and every batch straddles a wrap of the low digits.

Variants of the index pattern:
    "summed"  p is also held by C, (p, t, u, j, l), and not by the output (i, l): one block, every member adds to it;
    "placed"  the output holds every sliced index, (p, u, t, i, l): 12 blocks, beta is never 1.

The shape classes are those of the dispatch in csrc/contract.hip: tiled M, N >= 64 and K > 32; dot K >= 512 and at most
8192 outputs; stream everything else.  `classes` names the class of the stored step and of the output step.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

PATH = [(0, 1), (0, 1)]
SLICES = ("p", "u", "t")
SLICE_DIMS = (3, 2, 2)
N_ASSIGNMENTS = 12
BATCHES = (1, 2, 5, 12, 64)


@dataclass(frozen=True)
class Chain:
    name: str
    sizes: tuple  # I, K, J, L
    classes: tuple  # of the stored step, of the output step: "tiled" / "dot" / "stream"
    variant: str = "base"

    @property
    def ts(self):
        c = ("p", "t", "u", "j", "l") if self.variant == "summed" else ("t", "u", "j", "l")
        return [("p", "u", "i", "k"), ("k", "t", "j"), c]

    @property
    def output(self):
        return {"base": ("p", "i", "l"), "summed": ("i", "l"), "placed": ("p", "u", "t", "i", "l")}[self.variant]

    @property
    def dims(self):
        I, K, J, L = self.sizes
        return dict(p=3, u=2, t=2, i=I, k=K, j=J, l=L)

    def shapes(self):
        return [tuple(self.dims[x] for x in xs) for xs in self.ts]

    @property
    def n_blocks(self):
        return {"base": 3, "summed": 1, "placed": 12}[self.variant]

    @property
    def summed(self):  # assignments added into one element of the result
        return N_ASSIGNMENTS // self.n_blocks

    def steps(self):
        """(M, N, K) of the stored step and of the output step."""
        I, K, J, L = self.sizes
        return (I, J, K), (I, L, J)


def klass(M, N, K):
    if M >= 64 and N >= 64 and K > 32:
        return "tiled"
    return "dot" if K >= 512 and M * N <= 8192 else "stream"


# each class as the stored step and as the output step, at the smallest shapes that reach it
PLAIN = [
    Chain("tiled-stream", (65, 33, 65, 3), ("tiled", "stream")),
    Chain("stream-tiled", (65, 8, 33, 65), ("stream", "tiled")),
    Chain("dot-stream", (3, 512, 4, 5), ("dot", "stream")),
    Chain("stream-dot", (3, 5, 512, 4), ("stream", "dot")),
    Chain("stream-stream", (5, 7, 6, 3), ("stream", "stream")),
]
# storage mode: both steps on the MFMA kernel, M, N in {64, 65}, K in {33, 65}
HALF = [
    Chain("mfma-64x65x33-64x65x65", (64, 33, 65, 65), ("tiled", "tiled")),
    Chain("mfma-65x65x65-65x64x65", (65, 65, 65, 64), ("tiled", "tiled")),
]
# scaling: the MFMA kernel, the dot and the stream class as the stored step (staging, max word, narrowing pass)
SCALED = [HALF[0], PLAIN[2], PLAIN[4]]
SUMMED = Chain("summed-stream", (5, 7, 6, 3), ("stream", "stream"), "summed")
PLACED = Chain("placed-stream", (5, 7, 6, 3), ("stream", "stream"), "placed")
SMALL = PLAIN[4]

for _c in PLAIN + HALF + [SUMMED, PLACED]:
    assert tuple(klass(*s) for s in _c.steps()) == _c.classes, _c.name
assert {s[0] for c in HALF for s in c.steps()} == {64, 65} and {s[1] for c in HALF for s in c.steps()} == {64, 65}
assert {s[2] for c in HALF for s in c.steps()} == {33, 65}

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
