"""The case table of the matrix kernel's edge tests (tests/test_gpu_contract_matrix.py): one-step networks for
`contraction.contract(..., compute="matrix")`, patterned on tests/split_cases.py and with the `Case` of
tests/contract_cases.py -- `kernels` are the launches of the whole call per kernel path (contraction.KERNEL_PATHS), every
path not named being zero; `kt` the products summed into one result element.  Under `compute="matrix"` the four tiled
slots count ct_matrix_tiled_kernel (csrc/contract_matrix.h) and `ContractionResult.matrix_launches` counts the same
launches once more: `matrix_launches(case)`.

The kernel's geometry: 16 x 16 MFMA tiles; a wavefront takes 64 x 64 (complex128: 32 x 32), a block of 2 x 2 wavefronts
128 x 128 (complex128: 64 x 64); k in blocks of 16, read from LDS in groups of 4.  The shapes are the smallest at which
each thing can go wrong; every case runs in the four dtypes.
"""
from __future__ import annotations

from tests.contract_cases import Case


def _op(H, M, N, K, form_a, form_b, perms=0):
    return dict(H=H, M=M, N=N, K=K, form_a=form_a, form_b=form_b, perms=perms)


def _tiled(form_a, form_b):
    return "tiled_" + ("mk" if form_a == 0 else "km") + "_" + ("kn" if form_b == 0 else "nk")


def matrix_launches(case) -> int:
    """Launches of the matrix kernel that the whole call of `case` makes: those of its tiled slots."""
    return sum(v for name, v in case.kernels.items() if name.startswith("tiled"))


def _layouts(fa, fb):
    return (("i", "k") if fa == 0 else ("k", "i")), (("k", "j") if fb == 0 else ("j", "k"))


LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
MS = NS = (64, 65, 127, 129)
KS = (33, 48, 63, 64, 65, 97)


def _cases():
    out = []
    # M, N in {64, 65, 127, 129}: 64 is a whole wavefront tile (complex128: a whole block), 65 one row past it (a second
    # wavefront, or block, with one row), 127 one short of and 129 one past the 128 of a block (complex128: of two
    # blocks); the class starts at 64, so there is nothing below.  K in {33, 48, 63, 64, 65, 97}: two to seven k
    # blocks of 16; one short of, at and one past a multiple of the k block (63, 64, 65) and of the read group of 4 (the
    # same three), a whole number of k blocks (48, 64) and tails of 1 (33, 65, 97) and 15 (63).  H in {1, 3}, the four
    # layouts.  Every layout meets every K; along K the (M, N) pairs and H rotate so that every layout also meets every
    # M, every N and both H.
    for L, (fa, fb) in enumerate(LAYOUTS):
        for q, K in enumerate(KS):
            M, N, H = MS[(q + L) % 4], NS[(q + 2 * L + 1 + q // 4) % 4], 1 + 2 * ((q + L) % 2)
            la, lb = _layouts(fa, fb)
            if H > 1:
                la, lb, output = ("h",) + la, ("h",) + lb, ("h", "i", "j")
            else:
                output = None
            out.append(Case(f"matrix_{_tiled(fa, fb)[6:]}-{H}x{M}x{N}x{K}", (la, lb), dict(h=H, i=M, j=N, k=K), output, (),
                            _op(H, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # the exact sums: one row past a wavefront tile in m (complex128: past a block), one column past a block in n
    # (complex128: past two), six k blocks and a tail of 1
    for fa, fb in LAYOUTS:
        la, lb = _layouts(fa, fb)
        out.append(Case(f"matrix_exact_{_tiled(fa, fb)[6:]}-65x129x97", (la, lb), dict(h=1, i=65, j=129, k=97), None, (),
                        _op(1, 65, 129, 97, fa, fb), {_tiled(fa, fb): 1}, 97))
    # the 16-byte loads of the stage: taken per operand when its leading stride is a multiple of 16 bytes -- 4 float32,
    # 2 float64 or complex64 elements, any number of complex128 ones.  The shapes of the split kernel's table:
    # (136, 72, 40): both operands on them in every layout and type, with a block edge in m and in n whose last group of
    # 4 is whole, and a last k block of which two groups are whole and two are beyond K; (136, 72, 41) and (135, 71, 40):
    # the leading stride of the operands contiguous in k / in m, n is odd, so one operand or both fall back to element
    # loads beside a neighbour on the vector path (complex128 stays on it); (136, 72, 42) and (134, 70, 40): the same
    # strides at 2 mod 4, where float32 falls back and the other types do not
    for fa, fb in LAYOUTS:
        la, lb = _layouts(fa, fb)
        for M, N, K in ((136, 72, 40), (136, 72, 41), (135, 71, 40), (136, 72, 42), (134, 70, 40)):
            out.append(Case(f"matrix_vec_{_tiled(fa, fb)[6:]}-{M}x{N}x{K}", (la, lb), dict(h=1, i=M, j=N, k=K), None, (),
                            _op(1, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # beta = 1 on a matrix step: a sliced index of dimension 2 that is summed ...
    out.append(Case("matrix_beta-summed", (("s", "i", "k"), ("s", "k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 80))
    # ... and one the result holds: each assignment writes its own block once
    out.append(Case("matrix_beta-block", (("s", "i", "k"), ("k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 40))
    # the dispatch thresholds from both sides: below them the plain kernels run, as without the keyword
    out.append(Case("matrix-64x64x33", (("i", "k"), ("k", "j")), dict(i=64, j=64, k=33), None, (),
                    _op(1, 64, 64, 33, 0, 0), {"tiled_mk_kn": 1}, 33))
    out.append(Case("stream-63x64x33", (("i", "k"), ("k", "j")), dict(i=63, j=64, k=33), None, (),
                    _op(1, 63, 64, 33, 0, 0), {"stream": 1}, 33))
    out.append(Case("stream-64x63x33", (("i", "k"), ("k", "j")), dict(i=64, j=63, k=33), None, (),
                    _op(1, 64, 63, 33, 0, 0), {"stream": 1}, 33))
    out.append(Case("stream-64x64x32", (("k", "i"), ("j", "k")), dict(i=64, j=64, k=32), None, (),
                    _op(1, 64, 64, 32, 1, 1), {"stream": 1}, 32))
    out.append(Case("dot-K512", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=512), None, (),
                    _op(1, 4, 5, 512, 0, 0), {"dot": 1}, 512))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
MATRIX = [c for c in CASES if matrix_launches(c)]
PLAIN = [c for c in CASES if not matrix_launches(c)]  # no tiled-class step: the bytes of compute=None
EDGES = [c for c in CASES if c.name.startswith("matrix_") and c.name.split("_")[1] in ("mk", "km")]
EXACT = [c for c in CASES if c.name.startswith("matrix_exact_")]
VEC = [c for c in CASES if c.name.startswith("matrix_vec_")]
assert len(EDGES) == 24 and len(EXACT) == 4 and len(VEC) == 20
assert {c.dims[x] for c in EDGES for x in "ij"} == set(MS) and {c.dims["h"] for c in EDGES} == {1, 3}
for _layout in ("mk_kn", "mk_nk", "km_kn", "km_nk"):  # every layout meets every K, M, N and H
    _mine = [c for c in EDGES if c.name.startswith(f"matrix_{_layout}-")]
    assert {c.dims["k"] for c in _mine} == set(KS)
    assert {c.dims["i"] for c in _mine} == {c.dims["j"] for c in _mine} == set(MS)
    assert {c.dims["h"] for c in _mine} == {1, 3}
