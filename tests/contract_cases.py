"""The case table of the contraction kernels' edge tests: one-step networks for `contraction.contract()`, each chosen
so that `plan()` gives one (H, M, N, K, operand forms, permutes) and the dispatcher of csrc/contract.hip one kernel
path.  tests/test_contraction_plan.py checks the plan side of every case without a GPU;
tests/test_gpu_contract_kernels.py runs them, checks the launch counts and compares the numbers element by element.

`ops`: what plan() must give for the single step -- H, M, N, K, form_a (0: A [m][k], 1: A [k][m]), form_b (0: B [k][n],
1: B [n][k]) and the number of permute rows.  `kernels`: the launches of the whole call per kernel path
(contraction.KERNEL_PATHS), every path not named being zero.  `kt`: products summed into one result element, K of the
step times the slice assignments accumulated into it; the per-element error bound grows with it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
ALL = (F32, F64, C64, C128)
DOUBLES = (F64, C128)
# With uniform(0.5, 1.5) fills one dropped product moves an element by about 0.11 / kt relative; the float32 bound
# (kt + 2) 2^-24 separates that from rounding while kt stays under roughly 900.  Single precision runs up to this kt.
KT_SINGLE = 600


@dataclass(frozen=True)
class Case:
    name: str
    ts: tuple
    dims: dict
    output: tuple | None
    slices: tuple
    ops: dict
    kernels: dict
    kt: int
    dtypes: tuple = ()  # () -> by the kt rule

    def run_dtypes(self):
        return self.dtypes or (ALL if self.kt <= KT_SINGLE else DOUBLES)

    def shapes(self):
        return [tuple(self.dims[x] for x in xs) for xs in self.ts]

    def n_slices(self):
        return int(np.prod([self.dims[x] for x in self.slices], dtype=np.int64))


def _op(H, M, N, K, form_a, form_b, perms=0):
    return dict(H=H, M=M, N=N, K=K, form_a=form_a, form_b=form_b, perms=perms)


def _tiled(form_a, form_b):
    return "tiled_" + ("mk" if form_a == 0 else "km") + "_" + ("kn" if form_b == 0 else "nk")


def _cases():
    out = []
    # tiled: the four operand layouts x the tile edges.  (64, 64, 33): the smallest step the dispatcher sends here;
    # (65, 127, 48): one past a tile / one short of two, K a multiple of the k tile; (128, 64, 49): K one past;
    # (70, 200, 515): many k tiles and a tail of 3
    for fa, la in ((0, ("i", "k")), (1, ("k", "i"))):
        for fb, lb in ((0, ("k", "j")), (1, ("j", "k"))):
            for M, N, K in ((64, 64, 33), (65, 127, 48), (128, 64, 49), (70, 200, 515)):
                out.append(Case(f"{_tiled(fa, fb)}-{M}x{N}x{K}", (la, lb), dict(i=M, j=N, k=K), None, (),
                                _op(1, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # tiled with batches, both operands in place: the batch offsets h M K, h K N, h M N
    out.append(Case("tiled_batched-mk_kn", (("h", "i", "k"), ("h", "k", "j")), dict(h=3, i=65, j=127, k=33),
                    ("h", "i", "j"), (), _op(3, 65, 127, 33, 0, 0), {"tiled_mk_kn": 1}, 33))
    out.append(Case("tiled_batched-km_nk", (("h", "k", "i"), ("h", "j", "k")), dict(h=3, i=65, j=127, k=33),
                    ("h", "i", "j"), (), _op(3, 65, 127, 33, 1, 1), {"tiled_km_nk": 1}, 33))
    # tiled, beta = 1: the leaves read in place at a slice offset, the one step writes the output five times
    out.append(Case("tiled_beta-in_place", (("s", "i", "k"), ("s", "k", "j")), dict(s=5, i=70, j=64, k=40), None,
                    ("s",), _op(1, 70, 64, 40, 0, 0), {"tiled_mk_kn": 5}, 200))
    # tiled fed by a gather of an inner sliced axis: two rows of different sizes in one launch, then beta = 1
    out.append(Case("tiled_beta-gathered", (("i", "s", "k"), ("k", "j", "s")), dict(s=3, i=1100, j=700, k=90), None,
                    ("s",), _op(1, 1100, 700, 90, 0, 0, perms=2), {"gather": 3, "tiled_mk_kn": 3}, 270))
    # block placement: sliced indices the result holds, in the middle of it (two gathers per assignment) and
    # outermost (no permute at all); six assignments, each writing its own block once
    out.append(Case("blocks-inner", (("a", "b", "c"), ("c", "d", "e")), dict(a=64, b=3, c=40, d=2, e=64), None,
                    ("b", "d"), _op(1, 64, 64, 40, 0, 0, perms=2), {"gather": 6, "tiled_mk_kn": 6}, 40))
    out.append(Case("blocks-outer", (("b", "a", "c"), ("d", "c", "e")), dict(a=64, b=3, c=40, d=2, e=64), None,
                    ("b", "d"), _op(1, 64, 64, 40, 0, 0), {"tiled_mk_kn": 6}, 40))
    # dot: the K threshold from both sides
    out.append(Case("dot-K512", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=512), None, (),
                    _op(1, 4, 5, 512, 0, 0), {"dot": 1}, 512))
    out.append(Case("stream-K511", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=511), None, (),
                    _op(1, 4, 5, 511, 0, 0), {"stream": 1}, 511))
    # dot with batches and beta = 1: K not a multiple of the block, and a long one.  kt = 3108 and 280000: the double
    # types see every term; the single types run the shorter one for beta and the batch offsets, not for single terms
    for K, dtypes in ((777, ALL), (70000, DOUBLES)):
        out.append(Case(f"dot_batched_beta-K{K}", (("s", "h", "k"), ("s", "h", "k", "j")), dict(s=4, h=3, j=5, k=K),
                        ("h", "j"), ("s",), _op(3, 1, 5, K, 0, 0), {"dot": 4}, 4 * K, dtypes))
    # dot: the output threshold from both sides (128 x 64 would go to the tiled kernel first)
    out.append(Case("dot-8192_outputs", (("i", "k"), ("k", "j")), dict(i=256, j=32, k=600), None, (),
                    _op(1, 256, 32, 600, 0, 0), {"dot": 1}, 600))
    out.append(Case("stream-8193_outputs", (("i", "k"), ("k",)), dict(i=8193, k=600), None, (),
                    _op(1, 8193, 1, 600, 0, 0), {"stream": 1}, 600))
    # stream: more outputs than one trip of the grid-stride loop covers (256 x 65536)
    out.append(Case("stream-second_trip", (("i",), ("j",)), dict(i=4100, j=4100), None, (),
                    _op(1, 4100, 4100, 1, 0, 0), {"stream": 1}, 1, (F32, F64)))
    out.append(Case("stream-just_misses_tiled", (("i", "k"), ("k", "j")), dict(i=63, j=64, k=40), None, (),
                    _op(1, 63, 64, 40, 0, 0), {"stream": 1}, 40))
    out.append(Case("stream-K32_misses_tiled", (("k", "i"), ("j", "k")), dict(i=64, j=64, k=32), None, (),
                    _op(1, 64, 64, 32, 1, 1), {"stream": 1}, 32))
    out.append(Case("stream_batched_outer_beta", (("s", "h", "i"), ("s", "h", "j")), dict(s=3, h=4, i=33, j=47),
                    ("h", "i", "j"), ("s",), _op(4, 33, 47, 1, 0, 0), {"stream": 3}, 3))
    # stream: degenerate steps
    out.append(Case("stream-K1", (("i",), ("j",)), dict(i=7, j=5), None, (), _op(1, 7, 5, 1, 0, 0), {"stream": 1}, 1))
    out.append(Case("stream-M1", (("k",), ("k", "j")), dict(j=9, k=6), None, (),
                    _op(1, 1, 9, 6, 0, 0), {"stream": 1}, 6))
    out.append(Case("stream-N1", (("i", "k"), ("k",)), dict(i=9, k=6), None, (),
                    _op(1, 9, 1, 6, 0, 0), {"stream": 1}, 6))
    out.append(Case("stream-N1_transposed", (("k", "i"), ("k",)), dict(i=9, k=6), None, (),
                    _op(1, 9, 1, 6, 1, 0), {"stream": 1}, 6))
    out.append(Case("stream-scalar_leaf", ((), ("j",)), dict(j=11), None, (), _op(1, 1, 11, 1, 0, 0), {"stream": 1}, 1))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# a second fill, standard_normal: signs and the complex cross terms (the bound holds, it is looser against one term)
NORMAL_FILL = ("tiled_km_nk-70x200x515", "tiled_mk_nk-65x127x48", "tiled_batched-km_nk", "tiled_beta-in_place",
               "blocks-inner", "dot_batched_beta-K777", "dot-8192_outputs", "stream-just_misses_tiled",
               "stream_batched_outer_beta")
