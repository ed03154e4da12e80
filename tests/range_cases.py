"""The case table and the fills of the number-range tests (tests/test_contraction_range_plan.py without a GPU,
tests/test_gpu_contract_range.py on one): the contraction kernels where their operands, products, sums or stored
results are subnormal, on a rounding tie, at the top of a type's range or not finite.  No device import.

Shapes are the smallest that reach each shape class: 64 x 64 x 33 (tiled / MFMA / split; the four operand layouts) and
65 x 127 x 48 (a k tail and tile edges), 4 x 5 x 512 (dot), 63 x 64 x 33 (stream).  `Case` is that of
tests/contract_cases.py; every case is one step A (i, k) B (k, j) -> (i, j) in some memory layout, so `mats` gives the
two operands as plain matrices for the host emulations.

Groups (the module docstring of tests/test_gpu_contract_range.py states each bound):
  A  storage=, unscaled: one operand, or both, wholly subnormal in the 16-bit type        fill_a
  B  compute="bf16x3": the lo of the split subnormal; the top of the admitted range       fill_b, fill_b_top
  C  the plain kernels: subnormal products and sums; subnormal operands                   fill_c
  D  the device's narrowing against round_to_storage, bit for bit                         narrow_table, scaled_table
  E  widening of every 16-bit pattern                                                     all_patterns
  F  an inf or a NaN part in the plain kernels and the unscaled MFMA kernel               fill_f
"""
from __future__ import annotations

import numpy as np

from tests.contract_cases import Case
from tnco_amd import contraction as ctr

STORAGES = ("float16", "bfloat16")
P_BITS = {"float16": 11, "bfloat16": 8}  # significand bits, the hidden one included
E_MIN = {"float16": -14, "bfloat16": -126}  # exponent of the smallest normal number
E_MAX = {"float16": 15, "bfloat16": 127}  # ... of the largest finite one


def _op(H, M, N, K, form_a, form_b):
    return dict(H=H, M=M, N=N, K=K, form_a=form_a, form_b=form_b, perms=0)


def _one_step(prefix, M, N, K, fa, fb, kernel=None):
    la = ("i", "k") if fa == 0 else ("k", "i")
    lb = ("k", "j") if fb == 0 else ("j", "k")
    tiled = "tiled_" + ("mk" if fa == 0 else "km") + "_" + ("kn" if fb == 0 else "nk")
    kernel = kernel or tiled
    tag = tiled[6:] + "-" if kernel == tiled else ""
    return Case(f"{prefix}-{tag}{M}x{N}x{K}", (la, lb), dict(i=M, j=N, k=K), None, (), _op(1, M, N, K, fa, fb),
                {kernel: 1}, K)


# the tiled class: the four layouts at the threshold shape, and a k tail with tile edges in one layout
TILED = [_one_step("tiled", 64, 64, 33, fa, fb) for fa in (0, 1) for fb in (0, 1)] + [_one_step("tiled", 65, 127, 48, 0, 0)]
DOT = _one_step("dot", 4, 5, 512, 0, 0, "dot")
STREAM = _one_step("stream", 63, 64, 33, 0, 0, "stream")
CASES = TILED + [DOT, STREAM]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
THRESHOLD = BY_NAME["tiled-mk_kn-64x64x33"]


def class_of(case) -> str:
    return case.name.split("-")[0]


def mats(case, arrays):
    """(A [M, K], B [K, N]) of a case's two arrays, whatever their memory layout."""
    a, b = arrays
    return (a if case.ops["form_a"] == 0 else a.T), (b if case.ops["form_b"] == 0 else b.T)


def pow2(rng, shape, lo, hi, cplx, dtype):
    """Every part +- 2^uniform(lo, hi), in the real or complex `dtype`."""
    part = lambda: rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(lo, hi, shape)  # noqa: E731
    a = part() + 1j * part() if cplx else part()
    return a.astype(dtype)


def parts(a):
    a = np.asarray(a)
    return np.stack([a.real, a.imag], -1) if np.iscomplexobj(a) else a


# --- A: 16-bit subnormal operands -------------------------------------------------------------------------------------
# (exponent range of the subnormal operand, of the normal one)
A_RANGES = {"float16": ((-24, -15), (-3, 3)), "bfloat16": ((-133, -127), (10, 16))}
A_ROLES = {"float16": ("A", "B", "both"), "bfloat16": ("A", "B")}  # which operand is subnormal


def is_storage_subnormal(a, storage):
    """Every part of `a` is a non-zero subnormal of the storage type."""
    x = np.abs(parts(a)).astype(np.float64)
    return bool(((x > 0) & (x < 2.0 ** E_MIN[storage])).all())


def fill_a(case, storage, cplx, role, seed=61):
    rng = np.random.RandomState(seed)
    sub, normal = A_RANGES[storage]
    dtype = np.complex64 if cplx else np.float32
    out = []
    for side, shape in zip("AB", case.shapes()):
        small = role in (side, "both")
        a = ctr.round_to_storage(pow2(rng, shape, *(sub if small else normal), cplx, dtype), storage)
        assert is_storage_subnormal(a, storage) == small
        out.append(a)
    return out


def flush_storage(a, storage):
    """`a` with the parts that are subnormal in the storage type set to zero: a matrix unit that flushes its inputs."""
    x = parts(a).copy()
    x[np.abs(x.astype(np.float64)) < 2.0 ** E_MIN[storage]] = 0
    return x[..., 0] + 1j * x[..., 1] if np.iscomplexobj(a) else x


# --- B: the split where lo is subnormal, and at the top of its range -------------------------------------------------
def fill_b(case, cplx, seed=62):
    rng = np.random.RandomState(seed)
    dtype = np.complex64 if cplx else np.float32
    sa, sb = case.shapes()
    return [pow2(rng, sa, -120, -118, cplx, dtype), pow2(rng, sb, 10, 16, cplx, dtype)]


TOP_FIRST, TOP_LAST = 0x7F7E8001, 0x7F7F7FFF  # the float32 patterns whose hi is the largest finite bfloat16


def fill_b_top(case, cplx, seed=63):
    rng = np.random.RandomState(seed)
    dtype = np.complex64 if cplx else np.float32
    sa, sb = case.shapes()
    n = 2 if cplx else 1

    def part():
        u = rng.randint(TOP_FIRST, TOP_LAST + 1, sa).astype(np.uint32)
        u.reshape(-1)[0] = TOP_LAST  # the last float32 below 2^128 - 2^119
        return u.view(np.float32) * rng.choice([-1.0, 1.0], sa).astype(np.float32)

    ps = [part() for _ in range(n)]
    a = (ps[0] + 1j * ps[1]).astype(np.complex64) if cplx else ps[0]
    return [a, pow2(rng, sb, -12, -6, cplx, dtype)]


def split_emulation(A, B, flush_lo=False):
    """a_lo b_hi + a_hi b_lo + a_hi b_hi of two matrices in float64 / complex128, hi and lo from
    contraction.split_bf16; flush_lo: the parts of a lo that are bfloat16 subnormals read as zero."""
    wide = np.complex128 if np.iscomplexobj(A) or np.iscomplexobj(B) else np.float64
    (a_hi, a_lo), (b_hi, b_lo) = ctr.split_bf16(A), ctr.split_bf16(B)
    if flush_lo:
        a_lo, b_lo = flush_storage(a_lo, "bfloat16"), flush_storage(b_lo, "bfloat16")
    a_hi, a_lo, b_hi, b_lo = (np.asarray(x, wide) for x in (a_hi, a_lo, b_hi, b_lo))
    return a_lo @ b_hi + a_hi @ b_lo + a_hi @ b_hi


# --- C: the plain kernels ---------------------------------------------------------------------------------------------
# kind -> (exponent range of A, of B) for the single and for the double types
C_RANGES = {"sums": {4: ((-68, -65), (-68, -65)), 8: ((-530, -527), (-530, -527))},
            "operands": {4: ((-140, -130), (20, 26)), 8: ((-1065, -1030), (60, 66))}}
C_KINDS = tuple(C_RANGES)
ETA = {4: 2.0 ** -150, 8: np.ldexp(np.longdouble(1), -1075)}  # half the spacing of the type's subnormals
UNIT = {4: 2.0 ** -24, 8: 2.0 ** -53}


def real_size(dtype) -> int:
    return np.dtype(dtype).itemsize // (2 if np.dtype(dtype).kind == "c" else 1)


# (the seeds of fill_a and fill_c are ones at which no element's sum cancels to below its bound, so that a flushed
# operand or sum shows in every element; tests/test_contraction_range_plan.py asserts that)
def fill_c(case, dtype, kind, seed=68):
    rng = np.random.RandomState(seed)
    cplx = np.dtype(dtype).kind == "c"
    ra, rb = C_RANGES[kind][real_size(dtype)]
    sa, sb = case.shapes()
    return [pow2(rng, sa, *ra, cplx, dtype), pow2(rng, sb, *rb, cplx, dtype)]


def wide_of(dtype):
    """The type reference and bound of group C are computed in."""
    if real_size(dtype) == 4:
        return np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    return np.clongdouble if np.dtype(dtype).kind == "c" else np.longdouble


def reference_c(case, arrays):
    """(A @ B, |A| @ |B|) in wide_of the arrays' dtype."""
    wide = wide_of(arrays[0].dtype)
    A, B = (np.asarray(x, wide) for x in mats(case, arrays))
    return A @ B, np.abs(A) @ np.abs(B)


def bound_c(mag, kt, dtype):
    size = real_size(dtype)
    return ((2 if np.dtype(dtype).kind == "c" else 1) * kt + 2) * (UNIT[size] * mag + ETA[size])


# --- host chains: a kernel's sum emulated term by term in a given real type ------------------------------------------
def chain(A, B, real, flush=False, terms=None):
    """sum_k A[:, k] B[k, :] in the real type `real`, one term after the other, every product rounded and every add
    rounded (two roundings per term); a complex product is its four real ones in the order of the kernels.  `terms`:
    a list of (A, B) pairs whose products are summed per k in that order instead (the split's three).  flush: every
    product and every sum that is subnormal in `real` becomes zero, as would a kernel built to flush."""
    terms = terms or [(A, B)]
    cplx = any(np.iscomplexobj(x) for t in terms for x in t)
    tiny = np.finfo(real).tiny

    def fl(x):
        x = np.asarray(x, real)
        return np.where(np.abs(x) < tiny, real(0), x) if flush else x

    M, N = terms[0][0].shape[0], terms[0][1].shape[1]
    re, im = np.zeros((M, N), real), np.zeros((M, N), real)
    with np.errstate(under="ignore"):
        for k in range(terms[0][0].shape[1]):
            for X, Y in terms:
                x, y = X[:, k:k + 1], Y[k:k + 1, :]
                xr, yr = np.asarray(x.real, real), np.asarray(y.real, real)
                re = fl(re + fl(xr * yr))
                if cplx:
                    xi, yi = np.asarray(x.imag, real), np.asarray(y.imag, real)
                    re = fl(re + fl(-xi * yi))
                    im = fl(im + fl(xr * yi))
                    im = fl(im + fl(xi * yr))
    return re + 1j * im if cplx else re


# --- D: the narrowing table -------------------------------------------------------------------------------------------
CATEGORIES = ("tie_down", "tie_up", "above_tie", "below_tie", "subnormal", "underflow_tie", "above_underflow_tie", "largest")
D_SHAPES = {"tiled": (64, 33), "dot": (8, 512), "stream": (63, 33)}  # class -> (M, K) of step 1; N = 64
D_N = 64


def round_model(P, E, storage):
    """The integers P 2^E (P > 0) rounded to the storage type, in integer arithmetic: (nearest-even value, truncated
    value, flags per category), the values as float64 (beyond the largest finite: inf)."""
    p, emin, emax = P_BITS[storage], E_MIN[storage], E_MAX[storage]
    P, E = np.asarray(P, np.int64), np.asarray(E, np.int64)
    n = np.floor(np.log2(P.astype(np.float64))).astype(np.int64) + 1  # bit length (P < 2^53)
    qe = np.maximum(n - 1 + E, emin) - (p - 1)  # exponent of the spacing of the storage type at the value
    shift = qe - E  # product bits below that spacing
    sh = np.clip(shift, 0, 62)
    keep, low, half = P >> sh, P & ((np.int64(1) << sh) - 1), (np.int64(1) << sh) >> 1
    tie = (shift >= 1) & (low == half)
    up = (shift >= 1) & ((low > half) | (tie & (keep & 1 == 1)))
    scale = lambda q: np.ldexp(q.astype(np.float64), np.where(shift > 0, qe, E).astype(np.int64))  # noqa: E731
    top = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    nearest, cut = scale(keep + up), scale(keep)
    nearest = np.where(nearest > top, np.inf, nearest)
    flags = dict(tie_down=tie & (keep & 1 == 0) & (keep > 0), tie_up=tie & (keep & 1 == 1),
                 above_tie=(shift >= 2) & (low == half + 1) & (keep > 0), below_tie=(shift >= 2) & (low == half - 1) & (keep > 0),
                 subnormal=(nearest > 0) & (nearest < 2.0 ** emin), underflow_tie=tie & (keep == 0),
                 above_underflow_tie=(keep == 0) & (low > half) & (low - half <= half >> (p - 1)), largest=nearest == top)
    return nearest, cut, flags


def _pair_sets(storage):
    """For every significand ma: the significands mb by what rounding their product to p bits (a normal result) meets:
    the four tie categories, and a result whose significand is all ones."""
    p = P_BITS[storage]
    m = np.arange(1 << (p - 1), 1 << p, dtype=np.int64)
    P = m[:, None] * m[None, :]
    _, _, f = round_model(P, np.zeros_like(P), "bfloat16" if storage == "bfloat16" else "float16")
    n = np.floor(np.log2(P.astype(np.float64))).astype(np.int64) + 1
    sh = n - p
    keep, low, half = P >> sh, P & ((np.int64(1) << sh) - 1), (np.int64(1) << sh) >> 1
    ones = (keep + ((low > half) | ((low == half) & (keep & 1 == 1)))) == (1 << p) - 1
    sets = dict(tie_down=f["tie_down"], tie_up=f["tie_up"], above_tie=f["above_tie"], below_tie=f["below_tie"], largest=ones)
    return m, {c: [m[row] for row in mask] for c, mask in sets.items()}


_PAIRS = {}


def _draw_b(storage, MA, XA, rng):
    """One real plane of B for the row significands MA and exponents XA: (MB, XB, SB) [K, N], b = SB MB 2^(XB - p + 1).
    Row k is of type k % 5: ties in the normal range; the neighbours of ties (no significand has both a tie and a
    neighbour among its products); results in the subnormal range; the underflow tie and its neighbours; the largest
    finite value."""
    if storage not in _PAIRS:
        _PAIRS[storage] = _pair_sets(storage)
    m, sets = _PAIRS[storage]
    p, emin, emax = P_BITS[storage], E_MIN[storage], E_MAX[storage]
    K = len(MA)
    MB, X = np.zeros((K, D_N), np.int64), np.zeros((K, D_N), np.int64)  # X: exponent of the product's leading bit
    for k in range(K):
        at = int(MA[k]) - (1 << (p - 1))
        for j in range(D_N):
            t = k % 5
            if t < 2:
                MB[k, j] = rng.choice(sets[(("tie_down", "tie_up"), ("above_tie", "below_tie"))[t][j % 2]][at])
                X[k, j] = rng.randint(-6, 7)
            elif t == 2:
                MB[k, j] = rng.choice(m)
                X[k, j] = rng.randint(emin - p, emin)
            elif t == 3:
                MB[k, j] = ((1 << (p - 1)), (1 << (p - 1)) + 1, (1 << (p - 1)), (1 << p) - 1)[j % 4]
                X[k, j] = emin - p - (j % 4 == 3)
            else:
                MB[k, j] = rng.choice(sets["largest"][at])
                X[k, j] = emax
    n = np.floor(np.log2((MA[:, None] * MB).astype(np.float64))).astype(np.int64) + 1
    XB = X - (n - 1) + 2 * (p - 1) - XA[:, None]
    assert (XB >= emin).all() and (XB <= emax).all()
    return MB, XB, rng.choice([-1, 1], (K, D_N))


def _row_significands(storage, K, rng):
    """Per row k of B the significand and exponent of the a that multiplies it, by the row's type."""
    if storage not in _PAIRS:
        _PAIRS[storage] = _pair_sets(storage)
    m, sets = _PAIRS[storage]
    p = P_BITS[storage]
    ties, nbrs = _rich(storage)
    tops = [int(v) for k, v in enumerate(m) if len(sets["largest"][k]) and v != 1 << (p - 1)]
    low, high = (-12, 7) if storage == "float16" else (-64, 63)
    MA, XA = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for k in range(K):
        t = k % 5
        MA[k] = rng.choice(ties) if t in (0, 2) else rng.choice(nbrs) if t == 1 else 1 << (p - 1) if t == 3 or k % 10 == 4 \
            else rng.choice(tops)
        XA[k] = rng.randint(-3, 4) if t < 2 else low if t < 4 else high
    return MA, XA


def _rich(storage):
    """(the significands that have a tie of either kind among their products, those that have both neighbours)."""
    if storage not in _PAIRS:
        _PAIRS[storage] = _pair_sets(storage)
    m, sets = _PAIRS[storage]
    both = lambda c, d: [int(v) for k, v in enumerate(m) if len(sets[c][k]) and len(sets[d][k])]  # noqa: E731
    return both("tie_down", "tie_up"), both("above_tie", "below_tie")


def narrow_table(storage, cls, cplx, seed=65):
    """The two leaves of step 1 and what its stored result must be.  Returns a dict: A [M, K], B [K, 64] (float32 /
    complex64, exact in storage and normal there), Z the exact products (float64 / complex128), P, E the integers
    with |part of Z| = P 2^E, [M, 64] or [M, 64, 2].  Row i of A holds a_i at column i % K: real, or for a complex
    table real in the even rows and imaginary in the odd ones, so that every part of Z is one product."""
    M, K = D_SHAPES[cls]
    rng = np.random.RandomState(seed + 7 * STORAGES.index(storage) + 3 * list(D_SHAPES).index(cls))
    p = P_BITS[storage]
    rows = min(M, K)
    MAk, XAk = _row_significands(storage, rows, rng)
    planes = [_draw_b(storage, MAk, XAk, rng) for _ in range(2 if cplx else 1)]
    i = np.arange(M)
    k = i % K
    MA, XA = MAk[k], XAk[k] - (i >= K)  # a row that shares its row of B: one binade down, the other sign
    SA = np.where(i >= K, -1, rng.choice([-1, 1], M))
    a = SA * np.ldexp(MA.astype(np.float64), XA - (p - 1))
    b = [np.zeros((K, D_N)) for _ in planes]
    for q, (MB, XB, SB) in enumerate(planes):
        b[q][:rows] = SB * np.ldexp(MB.astype(np.float64), XB - (p - 1))
    A = np.zeros((M, K), np.complex128 if cplx else np.float64)
    A[i, k] = a * np.where(i % 2 == 1, 1j, 1) if cplx else a
    B = b[0] + 1j * b[1] if cplx else b[0]
    E = [XA[:, None] + XB[k] - 2 * (p - 1) for _, XB, _ in planes]
    P = [MA[:, None] * MB[k] for MB, _, _ in planes]
    if cplx:  # even rows: (a br, a bi); odd rows, a = i alpha: (-alpha bi, alpha br)
        odd = (i % 2 == 1)[:, None]
        P = np.stack([np.where(odd, P[1], P[0]), np.where(odd, P[0], P[1])], -1)
        E = np.stack([np.where(odd, E[1], E[0]), np.where(odd, E[0], E[1])], -1)
    else:
        P, E = P[0], E[0]
    Z = A[i, k][:, None] * B[k]
    assert np.array_equal(np.abs(parts(Z)), np.ldexp(P.astype(np.float64), E))
    single = np.complex64 if cplx else np.float32
    A32, B32 = A.astype(single), B.astype(single)
    assert np.array_equal(A32, A) and np.array_equal(B32, B) and np.array_equal(Z.astype(single), Z)
    for x in (A32, B32):
        assert np.array_equal(ctr.round_to_storage(x, storage), x)
        nz = np.abs(parts(x))[parts(x) != 0]
        assert nz.min() >= 2.0 ** E_MIN[storage]
    return dict(A=A32, B=B32, Z=Z, P=P, E=E, M=M, K=K)


def stored(z, storage):
    """float32 / complex64 `z` as a step stores it: rounded to storage, what lies beyond the range becoming inf."""
    with np.errstate(over="ignore"):
        return ctr._from_storage_bits(ctr._storage_bits(z, storage, check=False), storage, z)


# significand pairs whose product is the tie between the largest finite value and the next binade (it rounds to inf),
# and pairs whose product lies between that tie and the next binade (float32 still holds it, bfloat16 storage too)
OVER_TIE = {"float16": (1365, 1536), "bfloat16": (146, 224)}
OVER_BEYOND = {"float16": (1448, 1448), "bfloat16": (181, 181)}
for _s in STORAGES:
    _tie = ((1 << (P_BITS[_s] + 1)) - 1) << (P_BITS[_s] - 2)
    assert OVER_TIE[_s][0] * OVER_TIE[_s][1] == _tie < OVER_BEYOND[_s][0] * OVER_BEYOND[_s][1] < 1 << (2 * P_BITS[_s] - 1)
# rows planted in the overflow call: rows of ties and neighbours in the normal range, |b| < 2^10 there.  The planted a
# is below 2^(OVER_XA + 1), so the rest of its row stays finite (inf x 0 in step 2 would turn the planted element
# itself into a NaN), and so does the row that shares the planted b
OVER_ROWS = (0, 1, 5, 6)
OVER_XA = {"float16": 4, "bfloat16": 63}


def overflow_table(storage, cls, cplx, seed=65):
    """narrow_table with four rows replanted: (A, B, planted) -- planted: (row, column, part, sign) of a product at
    the tie that rounds to infinity (both signs) and between it and 2^(emax + 1) (both signs): finite in float32."""
    t = narrow_table(storage, cls, cplx, seed)
    A, B, K = t["A"].copy(), t["B"].copy(), t["K"]
    p, emax = P_BITS[storage], E_MAX[storage]
    ma, mb = OVER_TIE[storage]
    half = OVER_XA[storage]
    planted = []
    for q, row in enumerate(OVER_ROWS):
        col, sign = 3 + row, (1, -1, -1, 1)[q]
        ma_q, mb_q = (ma, mb) if q < 2 else OVER_BEYOND[storage]
        # ma mb has 2 p - 1 bits: a b = ma mb 2^(emax - 2 p + 2) has its leading bit at 2^emax
        a = np.ldexp(float(ma_q), half - (p - 1))
        b = sign * np.ldexp(float(mb_q), emax - half - (p - 1))
        part = q % 2 if cplx else 0
        A[row, row % K] = a  # (real, in an odd row of a complex table too: part c of Z is then a times part c of b)
        old = B[row % K, col]
        B[row % K, col] = (b + 1j * old.imag if part == 0 else old.real + 1j * b) if cplx else b
        planted.append((row, col, part, sign))
    return A, B, planted


def scaled_table(storage, cls, cplx, seed=66):
    """Leaves for the chain under scaling="tensor": the normal-range ties and neighbours of narrow_table, the rows of A
    spread over 2^-22 ... 1 and the parts of B over 2^-23 ... 1, and one planted product that is the largest.  Both
    leaves are exact in scaled storage.  Returns (A, B, Z exact in float64 / complex128)."""
    if storage not in _PAIRS:
        _PAIRS[storage] = _pair_sets(storage)
    m, sets = _PAIRS[storage]
    M, K = D_SHAPES[cls]
    rng = np.random.RandomState(seed + 7 * STORAGES.index(storage) + 3 * list(D_SHAPES).index(cls))
    p = P_BITS[storage]
    rows = min(M, K)
    ties, nbrs = _rich(storage)
    MAk = np.array([rng.choice(nbrs if k % 2 else ties) for k in range(rows)], np.int64)
    XAk = -rng.randint(1, 23, rows)
    planes = []
    for _ in range(2 if cplx else 1):
        kinds = (("tie_down", "tie_up"), ("above_tie", "below_tie"))
        MB = np.array([[rng.choice(sets[kinds[k % 2][j % 2]][int(MAk[k]) - (1 << (p - 1))]) for j in range(D_N)]
                       for k in range(rows)], np.int64)
        planes.append(rng.choice([-1, 1], MB.shape) * np.ldexp(MB.astype(np.float64), -rng.randint(1, 24, MB.shape) - (p - 1)))
    i = np.arange(M)
    k = i % K
    a = np.where(i >= K, -0.5, 1.0) * rng.choice([-1, 1], M) * np.ldexp(MAk[k].astype(np.float64), XAk[k] - (p - 1))
    a[0] = np.ldexp(float((1 << p) - 1), -(p - 1))  # the planted maximum: a_0 b_00, both significands all ones
    b = [np.zeros((K, D_N)) for _ in planes]
    for q, plane in enumerate(planes):
        b[q][:rows] = plane
        b[q][0, 0] = np.ldexp(float((1 << p) - 1), -(p - 1))
    A = np.zeros((M, K), np.complex128 if cplx else np.float64)
    A[i, k] = a * np.where((i % 2 == 1) & (i > 0), 1j, 1) if cplx else a
    B = b[0] + 1j * b[1] if cplx else b[0]
    Z = A[i, k][:, None] * B[k]
    single = np.complex64 if cplx else np.float32
    A32, B32 = A.astype(single), B.astype(single)
    assert np.array_equal(A32, A) and np.array_equal(B32, B) and np.array_equal(Z.astype(single), Z)
    for x in (A32, B32):
        assert np.array_equal(ctr.scale_to_storage(x, storage)[0], x)
    assert np.abs(parts(Z)).max() == np.abs(parts(Z))[0, 0].max()
    return A32, B32, Z


def expected_scaled(Z, storage):
    """(what the scaled chain must return for the exact products Z, the exponent of the stored Z)."""
    z = Z.astype(np.complex64 if np.iscomplexobj(Z) else np.float32)
    return ctr.scale_to_storage(z, storage)


# the two-step chain A (i, k) B (k, j) -> Z (i, j); I (j, l) Z (i, j) -> (l, i): the result is the stored Z transposed
CHAIN_TS, CHAIN_PATH = [("i", "k"), ("k", "j"), ("j", "l")], [(0, 1), (0, 1)]
IDENTITY = np.eye(D_N, dtype=np.float32)


def step2_class(cls) -> str:
    """Z [M, 64] times the 64 x 64 identity: tiled when step 1 is (M = 64), else M < 64 and K = 64 < 512: stream."""
    return "tiled" if D_SHAPES[cls][0] >= 64 else "stream"


# --- E: every 16-bit pattern ------------------------------------------------------------------------------------------
def all_patterns(storage):
    """Every 16-bit pattern of the type that is not a NaN, as uint16, in ascending order."""
    u = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    mant, expo = ((0x03FF, 0x7C00) if storage == "float16" else (0x007F, 0x7F80))
    return u[~(((u & expo) == expo) & ((u & mant) != 0))]


def widen(bits, storage):
    """The float32 values of 16-bit patterns, by the host."""
    return ctr._from_storage_bits(np.ascontiguousarray(bits, np.uint16), storage, np.empty(np.shape(bits), np.float32))


# --- F: non-finite operands -------------------------------------------------------------------------------------------
F_AT = {"tiled": (37, 20), "dot": (2, 300), "stream": (37, 20)}  # (row of A, k) of the planted part


def fill_f(case, cplx, seed=67, storage=None):
    rng = np.random.RandomState(seed)
    dtype = np.complex64 if cplx else np.float32
    out = [pow2(rng, shape, -3, 3, cplx, dtype) for shape in case.shapes()]
    return [ctr.round_to_storage(a, storage) for a in out] if storage else out
