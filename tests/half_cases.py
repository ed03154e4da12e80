"""The case table of the storage-mode kernels' edge tests (tests/test_gpu_contract_half.py): one-step networks for
`contraction.contract(..., storage=...)`, patterned on tests/contract_cases.py and with its `Case` -- `kernels` are the
launches of the whole call per kernel path (contraction.KERNEL_PATHS), every path not named being zero; `kt` the
products summed into one result element.  Under `storage` the four tiled slots count ct_mfma_tiled_kernel
(csrc/contract_half.h: 128 x 128 block tiles, 64 x 64 per wavefront, 16 x 16 MFMA tiles, k blocks of 32).

The shapes are the smallest at which each thing can go wrong; every case runs for both storage types, real and complex.
"""
from __future__ import annotations

from tests.contract_cases import Case

STORAGES = ("float16", "bfloat16")


def _op(H, M, N, K, form_a, form_b, perms=0):
    return dict(H=H, M=M, N=N, K=K, form_a=form_a, form_b=form_b, perms=perms)


def _tiled(form_a, form_b):
    return "tiled_" + ("mk" if form_a == 0 else "km") + "_" + ("kn" if form_b == 0 else "nk")


def _cases():
    out = []
    # MFMA tiles: M, N in {64, 65, 127, 129} (one 16-row MFMA tile short of / past a wavefront's 64, one short of / past
    # the block's 128), K in {33, 48, 63, 64, 65, 97} (one and several k blocks, every tail class of a 32-wide block),
    # H in {1, 3}, the four layouts.  Every layout meets every K; along K the (M, N) pairs and H rotate so that every
    # layout also meets every M, every N and both H.
    Ms = Ns = (64, 65, 127, 129)
    Ks = (33, 48, 63, 64, 65, 97)
    for L, (fa, fb) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for q, K in enumerate(Ks):
            M, N, H = Ms[(q + L) % 4], Ns[(q + 2 * L + 1 + q // 4) % 4], 1 + 2 * ((q + L) % 2)
            la = ("i", "k") if fa == 0 else ("k", "i")
            lb = ("k", "j") if fb == 0 else ("j", "k")
            if H > 1:
                la, lb, output = ("h",) + la, ("h",) + lb, ("h", "i", "j")
            else:
                output = None
            out.append(Case(f"mfma_{_tiled(fa, fb)[6:]}-{H}x{M}x{N}x{K}", (la, lb), dict(h=H, i=M, j=N, k=K), output, (),
                            _op(H, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # the 16-byte loads of the stage: taken per operand when its leading stride is a multiple of 8 elements (the rotation
    # above has them at K in {48, 64} and M, N = 64 only).  (136, 72, 40): both operands on them in every layout, with a
    # block edge in m and in n whose last run of 8 is whole, and a k block of which one quarter is whole and three are
    # beyond K; (136, 72, 41) and (135, 71, 40): the leading stride of the operands contiguous in k / in m, n is odd, so
    # one operand or both fall back to 2-byte loads beside a neighbour on the vector path
    for fa, fb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        la = ("i", "k") if fa == 0 else ("k", "i")
        lb = ("k", "j") if fb == 0 else ("j", "k")
        for M, N, K in ((136, 72, 40), (136, 72, 41), (135, 71, 40)):
            out.append(Case(f"mfma_vec_{_tiled(fa, fb)[6:]}-{M}x{N}x{K}", (la, lb), dict(h=1, i=M, j=N, k=K), None, (),
                            _op(1, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # (a misaligned base under an aligned leading stride does not arise from plan(): leaves and arena blocks start at
    # multiples of 64 elements, and the slice and batch offsets of an operand read in place are multiples of M K or
    # K N, which the leading stride divides; the pointer test of the launch guards callers of the C ABI)
    # beta = 1 on an MFMA-class step: a sliced index of dimension 2 that is summed ...
    out.append(Case("mfma_beta-summed", (("s", "i", "k"), ("s", "k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 80))
    # ... and one the result holds: each assignment writes its own block once
    out.append(Case("mfma_beta-block", (("s", "i", "k"), ("k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 40))
    # the dispatch thresholds from both sides
    out.append(Case("mfma-64x64x33", (("i", "k"), ("k", "j")), dict(i=64, j=64, k=33), None, (),
                    _op(1, 64, 64, 33, 0, 0), {"tiled_mk_kn": 1}, 33))
    out.append(Case("stream-63x64x33", (("i", "k"), ("k", "j")), dict(i=63, j=64, k=33), None, (),
                    _op(1, 63, 64, 33, 0, 0), {"stream": 1}, 33))
    out.append(Case("stream-64x64x32", (("k", "i"), ("j", "k")), dict(i=64, j=64, k=32), None, (),
                    _op(1, 64, 64, 32, 1, 1), {"stream": 1}, 32))
    out.append(Case("dot-K512", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=512), None, (),
                    _op(1, 4, 5, 512, 0, 0), {"dot": 1}, 512))
    out.append(Case("stream-K511", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=511), None, (),
                    _op(1, 4, 5, 511, 0, 0), {"stream": 1}, 511))
    # dot: one element past two trips of the 256-stride loop
    out.append(Case("dot-K513", (("i", "k"), ("j", "k")), dict(i=3, j=2, k=513), None, (),
                    _op(1, 3, 2, 513, 0, 1), {"dot": 1}, 513))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
MFMA = [c for c in CASES if c.name.startswith("mfma_") and "beta" not in c.name and "vec" not in c.name]
assert {c.dims[x] for c in MFMA for x in "ij"} == {64, 65, 127, 129} and {c.dims["h"] for c in MFMA} == {1, 3}
for _layout in ("mk_kn", "mk_nk", "km_kn", "km_nk"):  # every layout meets every K, M, N and H
    _mine = [c for c in MFMA if c.name.startswith(f"mfma_{_layout}-")]
    assert {c.dims["k"] for c in _mine} == {33, 48, 63, 64, 65, 97}
    assert {c.dims["i"] for c in _mine} == {c.dims["j"] for c in _mine} == {64, 65, 127, 129}
    assert {c.dims["h"] for c in _mine} == {1, 3}
