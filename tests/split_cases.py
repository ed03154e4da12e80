"""The case table of the split kernel's edge tests (tests/test_gpu_contract_split.py): one-step networks for
`contraction.contract(..., compute="bf16x3")`, patterned on tests/half_cases.py and with the `Case` of
tests/contract_cases.py -- `kernels` are the launches of the whole call per kernel path (contraction.KERNEL_PATHS), every
path not named being zero; `kt` the products summed into one result element.  Under `compute` the four tiled slots count
ct_split_tiled_kernel (csrc/contract_split.h: 128 x 128 block tiles, 64 x 64 per wavefront, 16 x 16 MFMA tiles, k blocks
of 32), and `ContractionResult.split_launches` counts the same launches once more: `split_launches(case)`.

The shapes are the smallest at which each thing can go wrong; every case runs real and complex.
"""
from __future__ import annotations

from tests.contract_cases import Case


def _op(H, M, N, K, form_a, form_b, perms=0):
    return dict(H=H, M=M, N=N, K=K, form_a=form_a, form_b=form_b, perms=perms)


def _tiled(form_a, form_b):
    return "tiled_" + ("mk" if form_a == 0 else "km") + "_" + ("kn" if form_b == 0 else "nk")


def split_launches(case) -> int:
    """Launches of the split kernel that the whole call of `case` makes: those of its tiled slots."""
    return sum(v for name, v in case.kernels.items() if name.startswith("tiled"))


def _layouts(fa, fb):
    return (("i", "k") if fa == 0 else ("k", "i")), (("k", "j") if fb == 0 else ("j", "k"))


def _cases():
    out = []
    # MFMA tiles: M, N in {64, 65, 127, 129} (one 16-row MFMA tile short of / past a wavefront's 64, one short of / past
    # the block's 128), K in {33, 48, 63, 64, 65, 97} (one and several k blocks, every tail class of a 32-wide block and
    # of the groups of 4 the stage reads), H in {1, 3}, the four layouts.  Every layout meets every K; along K the (M, N)
    # pairs and H rotate so that every layout also meets every M, every N and both H.
    Ms = Ns = (64, 65, 127, 129)
    Ks = (33, 48, 63, 64, 65, 97)
    for L, (fa, fb) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for q, K in enumerate(Ks):
            M, N, H = Ms[(q + L) % 4], Ns[(q + 2 * L + 1 + q // 4) % 4], 1 + 2 * ((q + L) % 2)
            la, lb = _layouts(fa, fb)
            if H > 1:
                la, lb, output = ("h",) + la, ("h",) + lb, ("h", "i", "j")
            else:
                output = None
            out.append(Case(f"split_{_tiled(fa, fb)[6:]}-{H}x{M}x{N}x{K}", (la, lb), dict(h=H, i=M, j=N, k=K), output, (),
                            _op(H, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # the 16-byte loads of the stage: taken per operand when its leading stride is a multiple of 16 bytes, 4 float32 or 2
    # complex64 elements.  (136, 72, 40): both operands on them in every layout, real and complex, with a block edge in
    # m and in n whose last group of 4 is whole, and a k block of which two groups are whole and six are beyond K;
    # (136, 72, 41) and (135, 71, 40): the leading stride of the operands contiguous in k / in m, n is odd, so one operand
    # or both fall back to element loads beside a neighbour on the vector path; (136, 72, 42) and (134, 70, 40): the
    # same strides at 2 mod 4, where the real operands fall back and the complex ones do not
    for fa, fb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        la, lb = _layouts(fa, fb)
        for M, N, K in ((136, 72, 40), (136, 72, 41), (135, 71, 40), (136, 72, 42), (134, 70, 40)):
            out.append(Case(f"split_vec_{_tiled(fa, fb)[6:]}-{M}x{N}x{K}", (la, lb), dict(h=1, i=M, j=N, k=K), None, (),
                            _op(1, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))
    # beta = 1 on a split step: a sliced index of dimension 2 that is summed ...
    out.append(Case("split_beta-summed", (("s", "i", "k"), ("s", "k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 80))
    # ... and one the result holds: each assignment writes its own block once
    out.append(Case("split_beta-block", (("s", "i", "k"), ("k", "j")), dict(s=2, i=65, j=64, k=40), None, ("s",),
                    _op(1, 65, 64, 40, 0, 0), {"tiled_mk_kn": 2}, 40))
    # the dispatch thresholds from both sides: below them the float32 kernels run, as without the keyword
    out.append(Case("split-64x64x33", (("i", "k"), ("k", "j")), dict(i=64, j=64, k=33), None, (),
                    _op(1, 64, 64, 33, 0, 0), {"tiled_mk_kn": 1}, 33))
    out.append(Case("stream-63x64x33", (("i", "k"), ("k", "j")), dict(i=63, j=64, k=33), None, (),
                    _op(1, 63, 64, 33, 0, 0), {"stream": 1}, 33))
    out.append(Case("stream-64x64x32", (("k", "i"), ("j", "k")), dict(i=64, j=64, k=32), None, (),
                    _op(1, 64, 64, 32, 1, 1), {"stream": 1}, 32))
    out.append(Case("dot-K512", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=512), None, (),
                    _op(1, 4, 5, 512, 0, 0), {"dot": 1}, 512))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SPLIT = [c for c in CASES if split_launches(c)]
PLAIN = [c for c in CASES if not split_launches(c)]  # no tiled-class step: the bytes of compute=None
EDGES = [c for c in CASES if c.name.startswith("split_") and "beta" not in c.name and "vec" not in c.name]
assert {c.dims[x] for c in EDGES for x in "ij"} == {64, 65, 127, 129} and {c.dims["h"] for c in EDGES} == {1, 3}
for _layout in ("mk_kn", "mk_nk", "km_kn", "km_nk"):  # every layout meets every K, M, N and H
    _mine = [c for c in EDGES if c.name.startswith(f"split_{_layout}-")]
    assert {c.dims["k"] for c in _mine} == {33, 48, 63, 64, 65, 97}
    assert {c.dims["i"] for c in _mine} == {c.dims["j"] for c in _mine} == {64, 65, 127, 129}
    assert {c.dims["h"] for c in _mine} == {1, 3}
