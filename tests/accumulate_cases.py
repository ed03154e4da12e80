"""What the accumulate tests share (tests/test_contraction_accumulate_plan.py without a GPU,
tests/test_gpu_contract_accumulate.py and tests/test_gpu_contract_accumulate_network.py on one): the numpy model of
`accumulate="float64"`, the designed sums, and the small network they are run through.  No device import.

The definition (tnco_amd/contraction.py, "Wide accumulation"): with b_0, b_1, ... the float32 / complex64 blocks that hit
one output block, in assignment order,

    r = float32(((float64(b_0) + float64(b_1)) + float64(b_2)) + ...)

each part (re, im) on its own, the first block placed, one rounding to nearest even at the end; an output block that no
assignment reaches is zero.

The designed sums (EDGES): lists of float32 terms, a term given as the pair (a, b) of float32 factors whose product it
is -- the network below computes a block as one product per element, so the term is exact unless it is meant not to be
(the product that underflows to -0.0).  Two things the definition cannot reach are left out on purpose, because they do
not exist, not because they are hard:
  * a sum of half the smallest float32 subnormal: every float32 is a multiple of 2^-149 and so is every float64 sum of
    them, so the accumulator never holds 2^-150.  The reachable neighbours are here: sums that land on the smallest
    subnormal and on an odd multiple of it, after cancellation from the normal range;
  * a -0.0 block from a -0.0 factor: a step starts every sum at +0.0 and fma(-0.0, 1, +0.0) is +0.0.  A block of -0.0
    does arise when a negative product underflows, fma(-2^-100, 2^-100, +0.0) = -0.0, and that one is here.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32, C64 = np.dtype(np.float32), np.dtype(np.complex64)
TWO24 = float(1 << 24)
BIG = 1.5 * 2.0 ** 127  # finite in float32; twice it is finite in float64 only
TINY = 2.0 ** -149  # the smallest float32 subnormal


def wide_of(dtype):
    return np.dtype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)


def model(parts, shape, dtype):
    """The definition, literally.  parts: (where, block) in assignment order, `where` an index into the result (integers
    for the axes of the sliced indices the result holds, slices for the others), block: what that assignment computes."""
    dtype = np.dtype(dtype)
    acc, seen = np.zeros(shape, wide_of(dtype)), set()
    with np.errstate(over="ignore", invalid="ignore"):
        for where, block in parts:
            b = np.asarray(block, dtype).astype(acc.dtype)  # exact
            if repr(where) in seen:
                acc[where] = acc[where] + b  # one IEEE float64 addition per part
            else:
                acc[where] = b
                seen.add(repr(where))
        return acc.astype(dtype)  # one rounding, to nearest even


def running_float32(parts, shape, dtype):
    """What `accumulate=None` does with the same blocks (ct_store with beta 1): the running sum in the blocks' own type."""
    dtype = np.dtype(dtype)
    out, seen = np.zeros(shape, dtype), set()
    with np.errstate(over="ignore", invalid="ignore"):
        for where, block in parts:
            b = np.asarray(block, dtype)
            out[where] = out[where] + b if repr(where) in seen else b
            seen.add(repr(where))
    return out


def round_to_float32_bits(x: Fraction) -> int:
    """The bit pattern of the float32 nearest to the rational x, ties to even, in integer arithmetic: subnormals, and inf
    beyond the range.  x == 0 gives +0.0 (a rational has no sign of zero)."""
    sign = 0x80000000 if x < 0 else 0
    x = abs(x)
    if x == 0:
        return sign
    e = x.numerator.bit_length() - x.denominator.bit_length()  # floor(log2 x), or one above it
    if Fraction(2) ** e > x:
        e -= 1
    e = max(e, -126)  # (below the normal range the last place stays 2^-149)
    ulp = Fraction(2) ** (e - 23)
    q, rest = divmod(x, ulp)
    q = int(q)
    if rest * 2 > ulp or (rest * 2 == ulp and q & 1):
        q += 1
    if q == 1 << 24:  # the rounding carried into the next exponent
        q, e = 1 << 23, e + 1
    if q < 1 << 23:  # subnormal (e is -126), zero included
        return sign | q
    return sign | 0x7F800000 if e + 127 >= 255 else sign | ((e + 127) << 23) | (q - (1 << 23))


def f32(v) -> np.float32:
    out = np.float32(v)
    assert float(out) == float(v) or not np.isfinite(out), v  # the factors of the table are float32 numbers
    return out


# name -> (the terms as (a, b) factor pairs, True when the float32 running sum gives other bits than the model)
EDGES = {
    # the case of the issue: 2^24 then 64 ones.  float32: 2^24 + 1 ties to even, 64 times; float64: 2^24 + 64
    "ones-after-2^24": ([(4096.0, 4096.0)] + [(1.0, 1.0)] * 64, True),
    # the narrowing ties: 2^24 + 1 goes down to 2^24 (the running sum agrees), 2^24 + 3 goes up to 2^24 + 4 (it does not)
    "tie-to-even-down": ([(4096.0, 4096.0), (1.0, 1.0)], False),
    "tie-to-even-up": ([(4096.0, 4096.0)] + [(1.0, 1.0)] * 3, True),
    # two blocks of 1.5 2^127: finite in float64, +inf in float32, in both sums; taken back by a third block, the float64
    # sum is finite again and the float32 one stays inf
    "overflow": ([(BIG, 1.0), (BIG, 1.0)], False),
    "overflow-taken-back": ([(BIG, 1.0), (BIG, 1.0), (-BIG, 1.0)], True),
    "inf-minus-inf": ([(np.inf, 1.0), (-np.inf, 1.0)], False),
    "minus-zero-alone": ([(-2.0 ** -100, 2.0 ** -100)], False),
    "minus-zero-then-zero": ([(-2.0 ** -100, 2.0 ** -100), (0.0, 1.0)], False),  # -0.0 + 0.0 = +0.0 in both types
    # subnormal sums: the smallest subnormal left over from the normal range, an odd multiple built from subnormal blocks
    "subnormal-after-cancellation": ([(2.0 ** -126, 1.0), (-(2.0 ** -126 - TINY), 1.0)], False),
    "subnormal-odd-multiple": ([(TINY, 1.0)] * 3, False),
    # 2^-96 + 2^-149 needs 54 bits: the float64 addition itself ties to even, and the narrowing is exact
    "float64-tie": ([(2.0 ** -96, 1.0), (TINY, 1.0)], False),
    # 1 + 2^-24 + 2^-24: float32 drops each half ulp, float64 holds both and the sum rounds to 1 + 2^-23
    "two-half-ulps": ([(1.0, 1.0), (2.0 ** -24, 1.0), (2.0 ** -24, 1.0)], True),
}
# the edges whose terms mean the same in both parts of a complex network (finite factors; see edge_network)
COMPLEX_EDGES = tuple(n for n in EDGES if n not in ("inf-minus-inf", "minus-zero-alone", "minus-zero-then-zero"))


def edge_terms(name) -> list:
    """The float32 terms of an edge, each as the device computes it: fma(a, b, +0.0) in float32."""
    with np.errstate(under="ignore", over="ignore"):
        return [np.float32(f32(a) * f32(b)) for a, b in EDGES[name][0]]


EDGE_I, EDGE_J = 3, 2


def edge_network(name, dtype):
    """(path, ts_inds, arrays, output_inds, slices): A (s, i, k) B (s, k, j) -> (i, j) with k of dimension 1, sliced over
    the summed s, one term per value of s: assignment s computes the block a_s b_s in every element, one product each.
    complex64: A holds a_s (1 + i) and B holds b_s, so both parts of the block are a_s b_s (re = a b - a 0, im = a 0 + a b)."""
    dtype = np.dtype(dtype)
    terms = EDGES[name][0]
    a = np.array([f32(t[0]) for t in terms], np.float32)
    b = np.array([f32(t[1]) for t in terms], np.float32)
    A = np.repeat(a, EDGE_I).reshape(len(terms), EDGE_I, 1)
    B = np.repeat(b, EDGE_J).reshape(len(terms), 1, EDGE_J)
    if dtype.kind == "c":
        assert name in COMPLEX_EDGES
        A = (A + 1j * A).astype(np.complex64)
    return [(0, 1)], [("s", "i", "k"), ("s", "k", "j")], [A.astype(dtype), B.astype(dtype)], ("i", "j"), ("s",)


def where_of(p, a):
    """The index of the block that assignment `a` of the plan `p` writes, into an array with the axes p.inds."""
    where = [slice(None)] * len(p.inds)
    for k, x in enumerate(p.slice_inds):
        if x in p.block_inds:
            where[p.inds.index(x)] = (a // math.prod(p.slice_dims[k + 1:])) % p.slice_dims[k]
    return tuple(where)


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_bytes(got, want) -> bool:
    """Byte for byte where `want` is finite or infinite, NaN at the same places (per part of a complex element)."""
    g = np.ascontiguousarray(got).reshape(-1).view(np.float32)
    w = np.ascontiguousarray(want).reshape(-1).view(np.float32)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])
