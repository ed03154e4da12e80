"""The case table of the gather, reduce and narrowing tests (tests/test_contraction_gather_plan.py without a GPU,
tests/test_gpu_contract_gather.py on one): the kernels of csrc/contract.hip that only move numbers -- ct_gather_body
(ct_gather_kernel, ct_half_gather_kernel, ct_half_gather_scaled_kernel), ct_path_permutes, ct_batch_reduce_kernel,
ct_path_reduce_kernel, ct_scale_narrow_kernel -- past the first trip of their grid-stride loops.  No device import.

These kernels copy, add in a fixed order or round once, so every case has an expectation in bytes, from numpy alone:
a gathered operand is observed through a step that sums exact products of small integers (or through no step at all: a
network of one tensor), a stored tensor through the product with a scalar leaf 1.  `fill` gives the leaves, `expected`
the result in the axis order of `Case.out_inds`.

Groups:
  leaf       leaf -> output gathers: a network of one tensor, 0, 4 and 34 axes
  transpose  leaf -> arena gathers that transpose: two rows of one launch on both sides of one block
  permute    an arena -> arena permute between two steps
  storage    the groups above under storage= (the 16-bit moves, the widening and the scaled widening gather)
  reduce     ct_batch_reduce_kernel / ct_path_reduce_kernel on a block above one trip (the chain of tests/batch_cases.py)
  narrow     ct_scale_narrow_kernel: tail only, quads and a tail, above one trip
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import batch_cases as bc
from tnco_amd import contraction as ctr

# csrc/contract.hip launch_gathers: blocks = min((largest + 255) / 256, 2048), 256 lanes each, and the same cap in the
# launches of ct_batch_reduce_kernel (run_steps) and ct_path_reduce_kernel (run_path): an element number of TRIP or
# more is reached by `e += gridDim.x * blockDim.x` only
TRIP = 2048 * 256
# ... the launch of ct_scale_narrow_kernel: min(max((quads + 255) / 256, 1), 2048) blocks, four float32 parts per lane
# and trip (a complex element is two parts); the n % 4 parts after the last quad one lane each
NARROW_TRIP = 4 * TRIP
BLOCK = 256  # lanes of a block: a row of at most this many elements leaves every other block of its launch idle

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
ALL = (F32, F64, C64, C128)
SINGLES = (F32, C64)
STORAGES = ("float16", "bfloat16")
# peak_device_bytes of every run stays under about 64 MB (the cards are shared)
MEMORY_CAP = 70 * 10 ** 6

LEAF, ARENA, OUT = ctr.LEAF, ctr.ARENA, ctr.OUT
# the planted defects of the plan test (tests/test_contraction_gather_plan.py): a row stops after its first TRIP
# elements; two axes' strides of a row are swapped; the narrowing pass drops the n % 4 parts after the last quad
DEFECTS = ("one_trip", "swapped_strides", "no_tail")


@dataclass(frozen=True)
class Case:
    name: str
    group: str
    ts: tuple
    dims: tuple  # (index, dimension) pairs
    path: tuple
    out_inds: tuple  # the axes `expected` is given in; also the output_inds of the call
    fill: str  # "index", "ints", "values", "narrow"
    # what the case is for, asserted from plan()'s tables: (source kind, destination kind, ndim, numel, group) per row
    rows: tuple
    dtypes: tuple = ALL
    slices: tuple = ()
    slice_range: tuple = None
    mode: tuple = ()  # (keyword, value) pairs of storage= / scaling=
    batching: tuple = ()  # (keyword, value) pairs: each is one more run, byte-equal to the run without the keyword
    block_numel: int = None  # elements of a block of the output
    stored: tuple = ()  # elements of every step result that goes to the arena
    classes: tuple = ()  # shape class of every step: "tiled" / "dot" / "stream"
    bites: tuple = ()  # the planted defects that must change the bytes of this case; the others must not
    large: bool = True  # a case above a trip size: it must fail under at least one defect

    @property
    def dim(self) -> dict:
        return dict(self.dims)

    def shapes(self):
        return [tuple(self.dim[x] for x in xs) for xs in self.ts]

    def keywords(self) -> dict:
        kw = dict(self.mode, slices=self.slices)
        if self.slice_range is not None:
            kw["slice_range"] = self.slice_range
        return kw

    def plan(self, dtype, **more):
        return ctr.plan(list(self.path), self.ts, self.shapes(), self.out_inds, dtype=dtype, **self.keywords(), **more)

    def assignments(self) -> range:
        n = math.prod(self.dim[x] for x in self.slices)
        return range(*(self.slice_range or (0, n)))

    def run_dtypes(self):
        return tuple(d for d in self.dtypes if not self.mode or d in SINGLES)

    @property
    def storage(self):
        return dict(self.mode).get("storage")

    @property
    def scaling(self):
        return dict(self.mode).get("scaling")


def _d(**dims):
    return tuple(dims.items())


def _modes():
    """(tag, mode) of the storage runs, both types; _scaled_modes: with scaling="tensor"."""
    return [(s, (("storage", s),)) for s in STORAGES]


def _scaled_modes():
    return [(s + "-scaled", (("storage", s), ("scaling", "tensor"))) for s in STORAGES]


# --- leaf: a network of one tensor -----------------------------------------------------------------------------------
LEAF4 = _d(a=7, b=101, c=3, d=251)  # four odd dims, 532 371 elements: the second trip covers a part of the grid only
LEAF4_NUMEL = 7 * 101 * 3 * 251
# 34 axes: 21 of dimension 2 and 11 of dimension 1 after the two sliced ones (x0 outermost, x17 in the middle) are
# dropped -- a row of MAX_AXES axes and 2^21 elements: four trips, dimension-1 axes inside the div/mod chain
WIDE_ONES = (2, 5, 8, 11, 14, 19, 22, 25, 28, 31, 33)
WIDE_SLICED = ("x0", "x17")
WIDE = tuple((f"x{k}", 1 if k in WIDE_ONES else 2) for k in range(34))
assert sum(d == 2 for x, d in WIDE if x not in WIDE_SLICED) == 21 and len(WIDE) - 2 == ctr.MAX_AXES


def _leaf_cases():
    names = tuple(x for x, _ in LEAF4)
    wide = tuple(x for x, _ in WIDE)
    return [
        Case("leaf-0-axes", "leaf", ((),), (), (), (), "index", ((LEAF, OUT, 0, 1, -1),), large=False),
        Case("leaf-4-axes", "leaf", (names,), LEAF4, (), names, "index", ((LEAF, OUT, 4, LEAF4_NUMEL, -1),),
             bites=("one_trip", "swapped_strides")),
        # sliced on an inner axis, four of its 101 values: blocks placed, the others of the output stay zero
        Case("leaf-4-axes-sliced", "leaf", (names,), LEAF4, (), names, "index", ((LEAF, OUT, 3, 7 * 3 * 251, -1),),
             slices=("b",), slice_range=(3, 7), block_numel=7 * 3 * 251, bites=("swapped_strides",), large=False),
        Case("leaf-34-axes", "leaf", (wide,), WIDE, (), wide, "index", ((LEAF, OUT, ctr.MAX_AXES, 1 << 21, -1),),
             dtypes=(F32,), slices=WIDE_SLICED, block_numel=1 << 21, bites=("one_trip", "swapped_strides")),
    ]


# --- transpose: A (i, s, k) B (k, j, s) -> (i, j), sliced on s --------------------------------------------------------
# Neither leaf is dense once s is dropped, so both are gathered in the launch before step 0: a row of 4133 x 127 =
# 524 891 elements and one of 127 x 2 = 254.  The launch is sized by the larger row; the blocks that the smaller one does
# not need must write nothing.  The step has 4133 x 2 x 127 multiply-adds: within what path_kernel= takes.  Both leaves
# hold integers 1 ... 7 in every part: an element of the result is an exact sum that every gathered element of its row
# and every element of B's column enters
TR_DIMS = _d(i=4133, s=3, k=127, j=2)
TR_TS = (("i", "s", "k"), ("k", "j", "s"))
TR_ROWS = ((LEAF, ARENA, 2, 4133 * 127, -1), (LEAF, ARENA, 2, 127 * 2, -1))
TR_BATCHING = (("slice_batch", 2), ("path_kernel", 2))


def _transpose_cases():
    plain = Case("transpose-two-rows", "transpose", TR_TS, TR_DIMS, ((0, 1),), ("i", "j"), "ints", TR_ROWS, slices=("s",),
                 batching=TR_BATCHING, block_numel=4133 * 2, classes=("stream",), bites=("one_trip", "swapped_strides"))
    half = [Case(f"transpose-two-rows-{tag}", "storage", TR_TS, TR_DIMS, ((0, 1),), ("i", "j"), "ints", TR_ROWS,
                 dtypes=SINGLES, slices=("s",), mode=mode, batching=TR_BATCHING[:1], block_numel=4133 * 2,
                 classes=("stream",), bites=("one_trip", "swapped_strides")) for tag, mode in _modes()]
    return [plain] + half


# --- permute: T0 (a, b, c) T1 (c, d) T2 (b, n), path [(0, 1), (0, 1)] --------------------------------------------------
# Step 0 leaves Z (a, b, d), 130 x 41 x 101 = 538 330 elements, in the arena; step 1 sums over b, so Z is permuted to
# (a, d, b) arena to arena in the launch before it
PM_DIMS = _d(a=130, b=41, c=2, d=101, n=3)
PM_NUMEL = 130 * 41 * 101
PERMUTE = Case("permute-arena", "permute", (("a", "b", "c"), ("c", "d"), ("b", "n")), PM_DIMS, ((0, 1), (0, 1)),
               ("a", "d", "n"), "ints", ((ARENA, ARENA, 3, PM_NUMEL, 1),), batching=(("path_kernel", 1),),
               block_numel=130 * 101 * 3, stored=(PM_NUMEL,), classes=("stream", "stream"),
               bites=("one_trip", "swapped_strides"))


# --- storage: the widening gather of a single leaf, plain and scaled -------------------------------------------------
def _widen_cases():
    names = tuple(x for x, _ in LEAF4)
    return [Case(f"leaf-4-axes-{tag}", "storage", (names,), LEAF4, (), names, "values", ((LEAF, OUT, 4, LEAF4_NUMEL, -1),),
                 dtypes=SINGLES, mode=mode, bites=("one_trip", "swapped_strides")) for tag, mode in _modes() + _scaled_modes()]


# --- reduce: the chain of tests/batch_cases.py with a block of 1030 x 513 = 528 390 elements --------------------------
RD_SIZES = (1030, 2, 3, 513)  # I, K, J, L: both steps are stream class
RD_BLOCK = 1030 * 513
RD_SLICE_BATCH, RD_PATH_KERNEL = (1, 5, 64), (1, 5, 1024)
RD_OFF_RANGE = (1, 11)  # with groups of 4: 1..4, 5..8, 9..10 -- it starts off a multiple of the group


def _reduce_cases():
    out = []
    for variant in ("base", "summed", "placed"):
        chain = bc.Chain(f"reduce-{variant}", RD_SIZES, ("stream", "stream"), variant)
        every = tuple((kw, v) for kw, vs in (("slice_batch", RD_SLICE_BATCH), ("path_kernel", RD_PATH_KERNEL)) for v in vs)
        # (a member's block of the staging buffer is 8 MB in complex128: groups of up to 5 keep a run under the cap)
        few = tuple((kw, v) for kw, v in every if v <= 5)
        rows = ((LEAF, ARENA, 2, 2 * 3, -1),)  # B (k, t, j) gathered per assignment; A and C are read in place
        common = dict(slices=bc.SLICES, block_numel=RD_BLOCK, stored=(1030 * 3,), classes=chain.classes,
                      bites=("swapped_strides",))
        args = (tuple(chain.ts), tuple(chain.dims.items()), tuple(bc.PATH), chain.output, "ints", rows)
        out.append(Case(chain.name, "reduce", *args, dtypes=(F32,), batching=every, **common))
        if variant != "placed":  # (twelve blocks of the output are 101 MB in complex128)
            out.append(Case(chain.name + "-complex128", "reduce", *args, dtypes=(C128,), batching=few, **common))
    chain = bc.Chain("reduce-base-off-range", RD_SIZES, ("stream", "stream"))
    out.append(Case(chain.name, "reduce", tuple(chain.ts), tuple(chain.dims.items()), tuple(bc.PATH), chain.output, "ints",
                    ((LEAF, ARENA, 2, 2 * 3, -1),), dtypes=(F32, C128), slice_range=RD_OFF_RANGE,
                    batching=(("slice_batch", 4), ("path_kernel", 4)), slices=bc.SLICES, block_numel=RD_BLOCK,
                    stored=(1030 * 3,), classes=chain.classes, bites=("swapped_strides",)))
    return out


# --- narrow: A (i, k) B (k, j) -> Z (i, j) stored, then Z times the scalar leaf 1 -------------------------------------
# Every element of Z is one product of two values that are exact in storage, so the float32 sum is exact and the
# stored bits are one rounding of it; the second step, M = I J and N = K = 1, returns the stored Z at its exponent.
NR_TS = (("i", "k"), ("k", "j"), ())
NR_PATH = ((0, 1), (0, 1))
NR_SMALL_REAL, NR_SMALL_COMPLEX = (1, 2, 3, 4, 5, 7), (1, 3)  # elements: tail only, one quad, one quad and a tail
NR_LARGE = {False: (1030, 2051), True: (1031, 1021)}  # (I, J): 2 112 530 and 2 x 1 052 651 = 2 105 302 parts, n % 4 == 2
NR_K = {"stream": 2, "tiled": 33}


def _narrow_cases():
    out = []
    for tag, mode in _scaled_modes():
        for cplx, sizes in ((False, NR_SMALL_REAL), (True, NR_SMALL_COMPLEX)):
            for n in sizes:
                out.append(Case(f"narrow-{n}-{'complex' if cplx else 'real'}-{tag}", "narrow", NR_TS, _d(i=1, k=2, j=n),
                                NR_PATH, ("i", "j"), "narrow", (), dtypes=(C64 if cplx else F32,), mode=mode,
                                block_numel=n, stored=(n,), classes=("stream", "stream"),
                                bites=("no_tail",) if (2 * n if cplx else n) % 4 else (), large=False))
        for cplx, (I, J) in NR_LARGE.items():
            for cls, K in NR_K.items():
                out.append(Case(f"narrow-{I}x{J}-{'complex' if cplx else 'real'}-{cls}-{tag}", "narrow", NR_TS,
                                _d(i=I, k=K, j=J), NR_PATH, ("i", "j"), "narrow", (), dtypes=(C64 if cplx else F32,),
                                mode=mode, block_numel=I * J, stored=(I * J,), classes=(cls, "stream"), bites=("no_tail",)))
        # two assignments, A sliced on its outermost axis and read in place, the result holds the sliced index: as a
        # batch of two, each member has its own staging buffer, exponent slots and max word
        I, J = NR_LARGE[False]
        out.append(Case(f"narrow-{I}x{J}-real-stream-sliced-{tag}", "narrow", (("s", "i", "k"), ("k", "j"), ()),
                        _d(s=2, i=I, k=2, j=J), NR_PATH, ("s", "i", "j"), "narrow", (), dtypes=(F32,), slices=("s",),
                        mode=mode, batching=(("slice_batch", 2),), block_numel=I * J, stored=(I * J,),
                        classes=("stream", "stream"), bites=("no_tail",)))
    return out


CASES = _leaf_cases() + _transpose_cases() + [PERMUTE] + _widen_cases() + _reduce_cases() + _narrow_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c, np.dtype(d)) for c in CASES for d in c.run_dtypes()]
RUN_IDS = [f"{c.name}-{d.name}" for c, d in RUNS]


def klass(M, N, K):
    return bc.klass(M, N, K)


# --- fills ------------------------------------------------------------------------------------------------------------
def _complex(re, im, dtype):
    return (re + 1j * im).astype(dtype) if np.dtype(dtype).kind == "c" else re.astype(dtype)


def _significands(rng, shape, storage):
    """Non-zero values that are exact in the storage type with every significand bit in use: +- m 2^x, m an integer of
    the type's full significand width, x in -3 ... 3 around 1."""
    p = {"float16": 11, "bfloat16": 8}[storage]
    m = rng.randint(1 << (p - 1), 1 << p, shape).astype(np.float64)
    return rng.choice([-1.0, 1.0], shape) * np.ldexp(m, rng.randint(-3, 4, shape) - (p - 1))


def fill(case, dtype) -> list:
    """The leaves of a case in `dtype`, seeded by the case's name; none of them holds a zero."""
    dtype = np.dtype(dtype)
    rng = np.random.RandomState(sum(case.name.encode()) + 977)
    cplx = dtype.kind == "c"
    out = []
    for t, shape in enumerate(case.shapes()):
        n = math.prod(shape)
        if case.fill == "index":  # flat index + 1 (imaginary part: twice that), exact in float32 below 2^24
            assert (2 if cplx else 1) * n <= 1 << 24
            re = np.arange(1, n + 1, dtype=np.float64).reshape(shape)
            a = _complex(re, 2 * re, dtype)
        elif case.fill == "ints":  # 1 ... 7 in both parts: every sum of the case is an integer far below 2^24
            a = _complex(rng.randint(1, 8, shape).astype(np.float64), rng.randint(1, 8, shape).astype(np.float64), dtype)
        elif case.fill == "values":  # seeded, non-zero, exact in the storage type
            a = ctr.round_to_storage(_complex(rng.standard_normal(shape), rng.standard_normal(shape), dtype), case.storage)
        else:
            a = _narrow_leaf(case, t, shape, rng, dtype)
        assert a.dtype == dtype and a.shape == shape
        assert (a.real != 0).all() and (not cplx or (a.imag != 0).all()) or case.fill == "narrow"
        out.append(a)
    return out


def _narrow_leaf(case, t, shape, rng, dtype):
    """The leaves of the narrowing chain: row i of A holds one a_i, at column i % K, and zeros; B has no zero; the third
    leaf is 1.  With the sliced axis: assignment 1 of A is another draw, 2^5 up."""
    if not shape:
        return np.ones((), dtype)
    if case.ts[t][-2:] != ("i", "k"):  # B
        return _complex(_significands(rng, shape, case.storage), _significands(rng, shape, case.storage), dtype)
    I, K = shape[-2:]
    a = np.zeros((math.prod(shape[:-2]), I, K), np.float64)
    for s in range(len(a)):
        a[s, np.arange(I), np.arange(I) % K] = _significands(rng, I, case.storage) * 2.0 ** (5 * s)
    return a.reshape(shape).astype(dtype)  # (real in a complex case too: a part of Z is a_i times a part of b)


# --- expectations -----------------------------------------------------------------------------------------------------
def digits(case, sid) -> dict:
    """The values of the sliced indices at assignment `sid`: the first of `slices` the most significant digit."""
    dims = [case.dim[x] for x in case.slices]
    return {x: (sid // math.prod(dims[k + 1:])) % dims[k] for k, x in enumerate(case.slices)}


def parts(a):
    """The real parts of an array as one more axis of 2 (a real array: itself)."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(a.real.dtype).reshape(a.shape + (2,)) if a.dtype.kind == "c" else a


def narrow_exponent(z) -> int:
    """The documented rule: e = floor(log2 m) - 14, m the largest |part| of the tensor (finite, non-zero here)."""
    m = float(np.abs(parts(z)).max())
    assert m > 0 and np.isfinite(m)
    return math.frexp(m)[1] - 1 - 14


def narrowed(z, storage):
    """(float32 / complex64 `z` as a scaled step stores it and a later step reads it: round_to_storage(ldexp(z, -s))
    scaled back by 2^s, the exponent s)."""
    s = narrow_exponent(z)
    x = parts(z)
    stored = ctr.round_to_storage(np.ldexp(x, -s).astype(np.float32), storage)
    back = np.ldexp(stored, s).astype(np.float32)
    return (back.reshape(-1).view(np.complex64).reshape(z.shape) if z.dtype.kind == "c" else back), s


def expected(case, dtype, arrays):
    """(the result of the case in `dtype`, axes in case.out_inds order, from numpy alone; under scaling the exponent of
    every assignment's stored tensor -- of a network of one tensor: of the leaf -- else None).  The assignments of
    `slice_range` are added in assignment order, or placed where the result holds the sliced index; what no assignment
    writes is zero."""
    dtype = np.dtype(dtype)
    wide = np.complex128 if dtype.kind == "c" else np.float64
    total = np.zeros(tuple(case.dim[x] for x in case.out_inds), dtype)
    exps = []
    sym = {x: k for k, x in enumerate(case.dim)}
    for sid in case.assignments():
        at = digits(case, sid)
        leaves = [a[tuple(at.get(x, slice(None)) for x in xs)] for xs, a in zip(case.ts, arrays)]
        inds = [tuple(x for x in xs if x not in at) for xs in case.ts]
        rest = [x for x in case.out_inds if x not in at]
        where = tuple(at.get(x, slice(None)) for x in case.out_inds)
        if case.group == "narrow":  # Z = A B exactly (one product per part), stored once, times 1
            z = np.einsum(leaves[0].astype(wide), [sym[x] for x in inds[0]], leaves[1].astype(wide), [sym[x] for x in inds[1]],
                          [sym[x] for x in rest])
            assert np.array_equal(z.astype(dtype), z)  # (exact in float32)
            part, s = narrowed(z.astype(dtype), case.storage)
            exps.append(s)
        elif not case.path:  # one tensor: itself (under scaling: as the leaf is held, one exponent for the whole leaf)
            if case.scaling is not None:
                whole, e = ctr.scale_to_storage(arrays[0], case.storage)
                assert e == narrow_exponent(arrays[0])
                leaves, exps = [whole[tuple(at.get(x, slice(None)) for x in case.ts[0])]], exps + [e]
            part = leaves[0].transpose([inds[0].index(x) for x in rest])
        else:  # integers: the einsum in double precision is exact, and so is every partial sum in `dtype`
            args = [q for a, xs in zip(leaves, inds) for q in (a.astype(wide), [sym[x] for x in xs])]
            part = np.einsum(*args, [sym[x] for x in rest], optimize=True)
            assert np.abs(parts(part)).max() * len(case.assignments()) < 1 << 24
        total[where] += part.astype(dtype)
    return total, (exps if case.scaling is not None else None)


# --- what a run must launch -------------------------------------------------------------------------------------------
def launches(case, p, keyword=None, value=None) -> dict:
    """The launch counts of a run of plan `p`: gather launches (one per permute group and assignment), the steps by shape
    class, the narrowing passes, the reduce kernel, the two path kernels.  With a batching keyword a group of
    assignments is what an assignment is without."""
    n = len(case.assignments())
    groups = n if keyword is None else -(-n // min(value, n))
    want = dict(gather=0, tiled=0, dot=0, stream=0, narrow=0, batch=0, path=(0, 0))
    if keyword == "path_kernel":
        return dict(want, path=(groups, groups))
    want["gather"] = groups * len(set(p.perms[:, 6].tolist()))
    for st in p.steps:
        want[klass(*(int(v) for v in st[11:14]))] += groups
    want["narrow"] = groups * len(case.stored) if case.scaling is not None else 0
    want["batch"] = groups if keyword == "slice_batch" else 0
    return want
