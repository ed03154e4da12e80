"""The row-mapped contraction kernels of csrc/contract.hip (ct_rows_tiled / ct_rows_dot / ct_rows_stream) at their
edges, element by element, in the manner of tests/test_gpu_contract_kernels.py.

Every case is a one-step network with sparse indices handed to `contraction.contract(..., sparse_inds=, projs=)`.  A
test asserts which kernel path ran, from `ContractionResult.row_kernel_launches` (the plain paths of `kernel_launches`
all zero except the gathers of the permutes), then compares every element with numpy in float64 / complex128: the
up-cast operands indexed at each projection's values of their sparse indices and multiplied per projection -- nothing
of tnco_amd.contraction is part of the reference.  The bound is the project's own, as it stands:

    |got - ref| <= (c kt + 2) u (|A| @ |B|)      u = eps / 2 of the real type, c = 1 real, c = 2 complex

with kt the products summed into an element.  Fills are uniform(0.5, 1.5): a dropped or doubled product, or a row read
through a wrong map entry, moves an element far over the bound while kt <= contract_cases.KT_SINGLE in single
precision, always in double.

`sparse` lists the sparse indices in column order; with ("t", "s") and the first operand holding s, the map of A is
neither the identity nor monotone (the rows of the result are sorted by t first).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np
import pytest

from tests import contract_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@dataclass(frozen=True)
class Case:
    name: str
    ts: tuple
    dims: dict
    output: tuple
    sparse: tuple
    P: object  # rows of projs: a number (random rows, seeded), "all", or ("distinct", n)
    rows: str  # the row-mapped path the step must take
    size: tuple  # (R, H, M, N, K) of the step
    slices: tuple = ()
    gathers: int = 0  # launches of the gather kernel, all assignments
    dtypes: tuple = ()

    @property
    def n_slices(self):
        return int(np.prod([self.dims[x] for x in self.slices], dtype=np.int64))

    @property
    def kt(self):
        held = set(self.output)
        return self.size[4] * int(np.prod([self.dims[x] for x in self.slices if x not in held], dtype=np.int64))

    def run_dtypes(self):
        return self.dtypes or (cc.ALL if self.kt <= cc.KT_SINGLE else cc.DOUBLES)

    def projs(self):
        every = np.array(list(itertools.product(*(range(self.dims[x]) for x in self.sparse))), np.int64)
        rng = np.random.RandomState(len(self.name))
        if self.P == "all":
            return every[rng.permutation(len(every))]
        if isinstance(self.P, tuple):
            return every[rng.permutation(len(every))[:self.P[1]]]
        return every[rng.randint(0, len(every), self.P)]


def _cases():
    out = []
    st = dict(s=5, t=3)
    # tiled: the four operand layouts x tile edges and k tails, both operands through maps
    for fa, la in ((0, ("s", "i", "k")), (1, ("s", "k", "i"))):
        for fb, lb in ((0, ("t", "k", "j")), (1, ("t", "j", "k"))):
            for M, N, K in ((64, 64, 33), (65, 127, 48), (70, 200, 515)):
                name = "tiled_" + ("mk" if fa == 0 else "km") + "_" + ("kn" if fb == 0 else "nk") + f"-{M}x{N}x{K}"
                out.append(Case(name, (la, lb), dict(st, i=M, j=N, k=K), ("s", "t", "i", "j"), ("t", "s"), 11,
                                "rows_tiled", (None, 1, M, N, K)))
    # tiled with batches (H > 1), and with only B mapped (A holds every sparse index: its rows in place)
    out.append(Case("tiled_batched", (("s", "h", "i", "k"), ("t", "h", "k", "j")), dict(st, h=3, i=65, j=64, k=33),
                    ("s", "t", "h", "i", "j"), ("t", "s"), 11, "rows_tiled", (None, 3, 65, 64, 33)))
    out.append(Case("tiled_only_B_mapped", (("s", "t", "i", "k"), ("t", "j", "k")), dict(st, i=64, j=70, k=40),
                    ("s", "t", "i", "j"), ("s", "t"), 11, "rows_tiled", (None, 1, 64, 70, 40)))
    # beta = 1 under a summed slice (the sliced axis lies inside the leaves' rows: two gathers per assignment), and
    # block placement under a slice the result holds
    out.append(Case("tiled_beta", (("s", "q", "i", "k"), ("t", "q", "k", "j")), dict(st, q=4, i=70, j=64, k=40),
                    ("s", "t", "i", "j"), ("t", "s"), 11, "rows_tiled", (None, 1, 70, 64, 40), ("q",), 4))
    out.append(Case("stream_beta", (("s", "q", "i", "k"), ("t", "q", "k", "j")), dict(st, q=3, i=9, j=7, k=5),
                    ("s", "t", "i", "j"), ("t", "s"), 11, "rows_stream", (None, 1, 9, 7, 5), ("q",), 3))
    out.append(Case("stream_blocks", (("s", "b", "i", "k"), ("t", "k", "j")), dict(st, b=3, i=9, j=7, k=5),
                    ("s", "t", "b", "i", "j"), ("t", "s"), 11, "rows_stream", (None, 1, 9, 7, 5), ("b",), 3))
    out.append(Case("tiled_blocks", (("s", "b", "i", "k"), ("t", "k", "j")), dict(st, b=2, i=64, j=64, k=33),
                    ("s", "t", "b", "i", "j"), ("t", "s"), 11, "rows_tiled", (None, 1, 64, 64, 33), ("b",), 2))
    # R = 1 (one projection: both maps are [0]); R a prime; many rows of the result reading one row of A
    out.append(Case("stream-R1", (("s", "i", "k"), ("t", "k", "j")), dict(st, i=7, j=5, k=6), ("s", "t", "i", "j"),
                    ("t", "s"), 1, "rows_stream", (1, 1, 7, 5, 6)))
    out.append(Case("tiled-R1", (("s", "i", "k"), ("t", "k", "j")), dict(st, i=64, j=65, k=34), ("s", "t", "i", "j"),
                    ("t", "s"), 1, "rows_tiled", (1, 1, 64, 65, 34)))
    out.append(Case("stream-R37", (("s", "i", "k"), ("t", "k", "j")), dict(s=7, t=11, i=3, j=5, k=6),
                    ("s", "t", "i", "j"), ("t", "s"), ("distinct", 37), "rows_stream", (37, 1, 3, 5, 6)))
    out.append(Case("stream-repeated", (("s", "i", "k"), ("t", "k", "j")), dict(s=2, t=40, i=3, j=5, k=6),
                    ("s", "t", "i", "j"), ("t", "s"), "all", "rows_stream", (80, 1, 3, 5, 6)))
    # fewer than 64 elements per row (a wavefront covers several rows), one element per row
    out.append(Case("stream-MN1", (("s", "k"), ("t", "k")), dict(s=7, t=11, k=6), ("s", "t"), ("t", "s"), "all",
                    "rows_stream", (77, 1, 1, 1, 6)))
    # H > 1 on the stream kernel; A's rows in place and B one row for every r (no map at all, H > 1: not folded)
    out.append(Case("stream_batched", (("s", "h", "i", "k"), ("h", "t", "k", "j")), dict(st, h=4, i=5, j=3, k=7),
                    ("s", "t", "h", "i", "j"), ("t", "s"), 11, "rows_stream", (None, 4, 5, 3, 7)))
    out.append(Case("stream_batched-no_maps", (("s", "h", "i", "k"), ("h", "k", "j")), dict(st, h=4, i=5, j=3, k=7),
                    ("s", "h", "i", "j"), ("s",), 11, "rows_stream", (None, 4, 5, 3, 7)))
    out.append(Case("stream-only_B_rows", (("i", "k"), ("s", "k", "j")), dict(st, i=5, j=3, k=7),
                    ("s", "i", "j"), ("s",), 11, "rows_stream", (None, 1, 5, 3, 7)))
    # dot: the K threshold and the output threshold from both sides (outputs = R H M N)
    d32 = dict(s=8, t=4)
    out.append(Case("dot-K512", (("s", "i", "k"), ("t", "k", "j")), dict(st, i=4, j=5, k=512), ("s", "t", "i", "j"),
                    ("t", "s"), 11, "rows_dot", (None, 1, 4, 5, 512)))
    out.append(Case("stream-K511", (("s", "i", "k"), ("t", "k", "j")), dict(st, i=4, j=5, k=511), ("s", "t", "i", "j"),
                    ("t", "s"), 11, "rows_stream", (None, 1, 4, 5, 511)))
    out.append(Case("dot-8192_outputs", (("s", "i", "k"), ("t", "k", "j")), dict(d32, i=16, j=16, k=600),
                    ("s", "t", "i", "j"), ("t", "s"), "all", "rows_dot", (32, 1, 16, 16, 600)))
    out.append(Case("stream-8193_outputs", (("s", "h", "i", "k"), ("t", "h", "k")), dict(s=3, t=1, h=1, i=2731, k=600),
                    ("s", "t", "h", "i"), ("t", "s"), "all", "rows_stream", (3, 1, 2731, 1, 600)))
    out.append(Case("dot_batched-K777", (("s", "h", "k"), ("t", "h", "k", "j")), dict(st, h=3, j=5, k=777),
                    ("s", "t", "h", "j"), ("t", "s"), 11, "rows_dot", (None, 3, 1, 5, 777), (), 0, cc.DOUBLES))
    # stream: more outputs than one trip of the grid-stride loop covers (256 x 65536): 41 rows of 640 x 640
    out.append(Case("stream-second_trip", (("s", "i"), ("t", "j")), dict(s=7, t=11, i=640, j=640), ("s", "t", "i", "j"),
                    ("t", "s"), ("distinct", 41), "rows_stream", (41, 1, 640, 640, 1), (), 0, (cc.F32, cc.F64)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _fill(case, dtype, seed, normal=False):
    rng = np.random.RandomState(seed)
    draw = (lambda s: rng.standard_normal(s)) if normal else (lambda s: rng.uniform(0.5, 1.5, s))
    out = []
    for xs in case.ts:
        shape = tuple(case.dims[x] for x in xs)
        a = draw(shape)
        if np.dtype(dtype).kind == "c":
            a = a + 1j * draw(shape)
        out.append(np.asarray(a).astype(dtype))
    return out


def _result_inds(case):
    """Axes of the projected one step: "proj", then [shared indices that stay][rest of the first][rest of the
    second] without the sparse ones."""
    a, b = case.ts
    shared = set(a) & set(b)
    keep = shared & set(case.output)
    full = tuple(x for x in a if x in keep) + tuple(x for x in a if x not in shared) + \
        tuple(x for x in b if x not in shared)
    return ("proj",) + tuple(x for x in full if x not in case.sparse)


def _at_projs(a, xs, case, projs):
    """[P][the non-sparse axes of a]: a at each projection's values of the sparse indices it holds."""
    held = [x for x in case.sparse if x in xs]
    if not held:
        return np.broadcast_to(a, (len(projs),) + a.shape)
    front = np.moveaxis(a, [xs.index(x) for x in held], range(len(held)))
    return front[tuple(projs[:, case.sparse.index(x)] for x in held)]


def _reference(case, arrays, projs, inds):
    """(the result, the same of the moduli), in double precision: one product of the two operands per projection."""
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    dense = [tuple(x for x in xs if x not in case.sparse) for xs in case.ts]
    sym = {x: k + 1 for k, x in enumerate(dict.fromkeys(dense[0] + dense[1]))}
    subs = [[0] + [sym[x] for x in xs] for xs in dense]
    res = [0] + [sym[x] for x in inds[1:]]
    at = [_at_projs(a, xs, case, projs) for a, xs in zip(wide, case.ts)]
    ref = np.einsum(at[0], subs[0], at[1], subs[1], res, optimize=True)
    mag = np.einsum(np.abs(at[0]), subs[0], np.abs(at[1]), subs[1], res, optimize=True)
    return ref, mag


def _bound(mag, kt, dtype):
    u = float(np.finfo(dtype).eps) / 2
    return ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * u * mag


def _assert_within(got, ref, bound, what):
    """|got - ref| <= bound in every element; an element that is not a number does not satisfy it."""
    assert got.shape == ref.shape == bound.shape, what
    err = np.abs(got.astype(ref.dtype) - ref)
    bad = ~(err <= bound)
    ratio = np.divide(err, bound, out=np.zeros_like(bound), where=bound > 0)
    ratio[bad & ~(ratio > 1)] = np.inf
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    print(f"{what}: largest error / bound {float(ratio[at]):.4f} at {at}")
    if bad.any():
        where = np.argwhere(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound, "
                             f"{int(np.isnan(err).sum())} of them not a number; first at "
                             f"{tuple(where[0].tolist())}, last at {tuple(where[-1].tolist())}, worst at {at}: got "
                             f"{got[at]}, reference {ref[at]}, error / bound {float(ratio[at]):.3g}")


def _assert_paths(ctr, r, case, n_slices, what):
    want = tuple(n_slices * (name == case.rows) for name in ctr.ROW_KERNEL_PATHS)
    assert r.row_kernel_launches == want, f"{what}: {dict(zip(ctr.ROW_KERNEL_PATHS, r.row_kernel_launches))}"
    gathers = case.gathers * n_slices // case.n_slices
    assert r.kernel_launches == (gathers,) + (0,) * 6, f"{what}: {dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))}"
    assert r.launches == sum(r.kernel_launches) + sum(r.row_kernel_launches)


def _run_case(ctr, case, dtype, seed, normal=False):
    arrays, projs = _fill(case, dtype, seed, normal), case.projs()
    what = f"{case.name} {np.dtype(dtype).name}"
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, sparse_inds=case.sparse, projs=projs)
    inds = _result_inds(case)
    assert r.inds == inds and r.n_slices == case.n_slices and r.array.dtype == np.dtype(dtype), what
    _assert_paths(ctr, r, case, case.n_slices, what)
    R, H, M, N, K = case.size
    rows = len(np.unique(projs, axis=0))  # (the result holds every sparse index)
    assert R in (None, rows), what
    assert r.macs == case.n_slices * rows * H * M * N * K, what
    ref, mag = _reference(case, arrays, projs, inds)
    _assert_within(r.array, ref, _bound(mag, case.kt, dtype), f"{what}: kt {case.kt}")
    return arrays, projs, r


_RUNS = [pytest.param(c, d, id=f"{c.name}-{np.dtype(d).name}") for c in CASES for d in c.run_dtypes()]
_NORMAL = ("tiled_km_nk-70x200x515", "tiled_mk_kn-65x127x48", "tiled_batched", "tiled_beta", "stream_blocks",
           "dot_batched-K777", "dot-8192_outputs", "stream_batched", "stream-repeated")


@pytest.mark.parametrize("case,dtype", _RUNS)
def test_row_kernel_path_and_every_element(ctr, case, dtype):
    _run_case(ctr, case, dtype, seed=21)


@pytest.mark.parametrize("case,dtype", [pytest.param(BY_NAME[n], d, id=f"{n}-{np.dtype(d).name}")
                                        for n in _NORMAL for d in BY_NAME[n].run_dtypes()])
def test_row_kernel_path_and_every_element_with_signs(ctr, case, dtype):
    _run_case(ctr, case, dtype, seed=22, normal=True)


def test_the_maps_of_the_cases_are_what_they_were_chosen_for(ctr):
    """No GPU work: the tiled cases run under a map that is neither the identity nor monotone, `repeated` has many rows
    of the result on one row of A, `only_B_mapped` and `no_maps` carry the maps their names say."""
    def ops(case):
        p = ctr.plan([(0, 1)], case.ts, [tuple(case.dims[x] for x in xs) for xs in case.ts], case.output,
                     slices=case.slices, sparse_inds=case.sparse, projs=case.projs())
        (op,) = p.ops
        assert not op["folded"] and (op["H"], op["M"], op["N"], op["K"]) == case.size[1:]
        return op
    for case in CASES:
        op = ops(case)
        if case.name.startswith("tiled_") and "only_B" not in case.name:
            a = op["a_map"]
            assert (np.diff(a) < 0).any() and (np.diff(a) > 0).any() and not np.array_equal(a, np.arange(len(a)))
            assert op["b_map"] is not None and len(set(op["b_map"].tolist())) < len(op["b_map"])
    assert np.bincount(ops(BY_NAME["stream-repeated"])["a_map"]).tolist() == [40, 40]
    op = ops(BY_NAME["tiled_only_B_mapped"])
    assert op["a_map"] is None and op["b_map"] is not None
    op = ops(BY_NAME["stream_batched-no_maps"])
    assert op["a_map"] is None and op["b_map"] is None and op["R"] > 1
    op = ops(BY_NAME["stream-R1"])
    assert op["R"] == 1 and op["a_map"].tolist() == [0] and op["b_map"].tolist() == [0]


@pytest.mark.parametrize("name", ["tiled_beta", "stream_beta"])
@pytest.mark.parametrize("dtype", cc.DOUBLES + (cc.F32,))
def test_slice_range_parts_add_up_to_the_whole(ctr, name, dtype):
    case = BY_NAME[name]
    (s,) = case.slices
    n, K = case.dims[s], case.size[4]
    arrays, projs = _fill(case, dtype, seed=23), case.projs()
    inds = _result_inds(case)
    total, total_bound = 0, 0
    for lo, hi in ((0, 1), (1, n)):
        r = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, slice_range=(lo, hi),
                         sparse_inds=case.sparse, projs=projs)
        assert r.n_slices == hi - lo
        _assert_paths(ctr, r, case, hi - lo, f"{name} [{lo}, {hi})")
        part = [np.take(a, range(lo, hi), axis=xs.index(s)) for a, xs in zip(arrays, case.ts)]
        ref, mag = _reference(case, part, projs, inds)
        _assert_within(r.array, ref, _bound(mag, K * (hi - lo), dtype), f"{name} [{lo}, {hi})")
        total = total + r.array.astype(ref.dtype)
        total_bound = total_bound + _bound(mag, K * (hi - lo), dtype)
    ref, _ = _reference(case, arrays, projs, inds)
    _assert_within(total, ref, total_bound, f"{name}: the parts added")


@pytest.mark.parametrize("name,dtype", [("tiled_beta", np.float32), ("tiled_batched", np.complex64),
                                        ("dot_batched-K777", np.float64), ("dot-8192_outputs", np.complex128),
                                        ("stream_beta", np.float32), ("stream_blocks", np.complex128)])
def test_runs_are_bit_identical_per_row_kernel_path(ctr, name, dtype):
    case = BY_NAME[name]
    arrays, projs, first = _run_case(ctr, case, dtype, seed=24)
    again = ctr.contract([(0, 1)], case.ts, arrays, case.output, slices=case.slices, sparse_inds=case.sparse,
                         projs=projs)
    assert again.row_kernel_launches == first.row_kernel_launches
    assert np.array_equal(again.array, first.array)


def test_duplicate_projections_give_duplicate_slabs(ctr):
    case = BY_NAME["stream_batched"]
    arrays, projs = _fill(case, np.float64, seed=25), case.projs()
    twice = np.concatenate([projs, projs[::-1]])
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, sparse_inds=case.sparse, projs=twice)
    once = ctr.contract([(0, 1)], case.ts, arrays, case.output, sparse_inds=case.sparse, projs=projs)
    assert r.macs == once.macs and r.array.shape[0] == 2 * len(projs)
    assert np.array_equal(r.array, np.concatenate([once.array, once.array[::-1]]))


def test_a_folded_step_runs_the_plain_kernels(ctr):
    """Only the first operand has rows, stored [r][m][k], H = 1: a plain GEMM with R M rows, no row-mapped launch."""
    case = Case("folded", (("s", "i", "k"), ("k", "j")), dict(s=5, i=30, j=64, k=40), ("s", "i", "j"), ("s",), 9,
                "", (None, 1, 30, 64, 40))
    arrays, projs = _fill(case, np.float64, seed=26), case.projs()
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, sparse_inds=case.sparse, projs=projs)
    R = len(np.unique(projs, axis=0))
    assert R * 30 >= 64 and r.row_kernel_launches == (0, 0, 0)
    assert dict(zip(ctr.KERNEL_PATHS, r.kernel_launches))["tiled_mk_kn"] == 1 and r.launches == 1
    ref, mag = _reference(case, arrays, projs, ("proj", "i", "j"))
    _assert_within(r.array, ref, _bound(mag, 40, np.float64), "folded")


def test_a_result_that_is_not_a_number_fails(ctr):
    case = BY_NAME["stream-R37"]
    arrays, projs, r = _run_case(ctr, case, np.float32, seed=27)
    inds = _result_inds(case)
    ref, mag = _reference(case, arrays, projs, inds)
    broken = r.array.copy()
    broken[17, 1, 2] = np.nan
    with pytest.raises(AssertionError, match="1 of them not a number"):
        _assert_within(broken, ref, _bound(mag, case.kt, np.float32), "nan")
    arrays[0][3, 1, 2] = np.nan  # ... and one in an operand reaches the result and fails there
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, sparse_inds=case.sparse, projs=projs)
    assert np.isnan(r.array).any()
    with pytest.raises(AssertionError, match="not a number"):
        _assert_within(r.array, ref, _bound(mag, case.kt, np.float32), "nan in")
