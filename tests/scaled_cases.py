"""The case table of the scaled storage-mode tests (tests/test_gpu_contract_scaled.py): one-step networks for
`contraction.contract(..., storage=..., scaling="tensor")`, patterned on tests/half_cases.py and with the same `Case`.

ONE_STEP: the step writes the output, one case per shape class of the dispatch in csrc/contract.hip --
  the MFMA kernel at M, N in {64, 65, 129} (a wavefront's 64 rows, one past them, one past the block's 128) and
  K in {33, 64, 97} (one k block and a tail, two whole ones, three and a tail), and all four operand layouts at one shape;
  the dot kernel (K >= 512, few outputs), with a tail past two trips of its loop; the stream kernel.
FIRST_STEPS: (I, K, J) of a first step A (i, k) B (k, j) in each class, whose result Z (i, j) is stored and then
multiplied with a vector over j (a stream-class step).
"""
from __future__ import annotations

from tests.contract_cases import Case
from tests.half_cases import STORAGES, _op, _tiled  # noqa: F401

FACTORS = (2.0 ** 40, 2.0 ** -70)  # of the two leaves of a one-step case


def _cases():
    out = []

    def mfma(M, N, K, fa, fb):
        la = ("i", "k") if fa == 0 else ("k", "i")
        lb = ("k", "j") if fb == 0 else ("j", "k")
        out.append(Case(f"mfma_{_tiled(fa, fb)[6:]}-{M}x{N}x{K}", (la, lb), dict(i=M, j=N, k=K), None, (),
                        _op(1, M, N, K, fa, fb), {_tiled(fa, fb): 1}, K))

    for M, N, K in ((64, 65, 33), (65, 129, 64), (129, 64, 97)):
        mfma(M, N, K, 0, 0)
    for fa, fb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        mfma(129, 65, 97, fa, fb)
    out.append(Case("dot-K512", (("i", "k"), ("k", "j")), dict(i=4, j=5, k=512), None, (),
                    _op(1, 4, 5, 512, 0, 0), {"dot": 1}, 512))
    out.append(Case("dot-K513", (("i", "k"), ("j", "k")), dict(i=3, j=2, k=513), None, (),
                    _op(1, 3, 2, 513, 0, 1), {"dot": 1}, 513))
    out.append(Case("stream-63x64x33", (("i", "k"), ("k", "j")), dict(i=63, j=64, k=33), None, (),
                    _op(1, 63, 64, 33, 0, 0), {"stream": 1}, 33))
    out.append(Case("stream-64x64x32", (("k", "i"), ("j", "k")), dict(i=64, j=64, k=32), None, (),
                    _op(1, 64, 64, 32, 1, 1), {"stream": 1}, 32))
    return out


ONE_STEP = _cases()
BY_NAME = {c.name: c for c in ONE_STEP}
assert len(BY_NAME) == len(ONE_STEP)
_M = [c for c in ONE_STEP if c.name.startswith("mfma_")]
assert {c.dims["i"] for c in _M} == {c.dims["j"] for c in _M} == {64, 65, 129} and {c.dims["k"] for c in _M} == {33, 64, 97}
assert {c.name.split("-")[0] for c in _M if c.name.endswith("-129x65x97")} == {"mfma_mk_kn", "mfma_mk_nk", "mfma_km_kn", "mfma_km_nk"}

# class of the first step -> (I, K, J): Z is I x J
FIRST_STEPS = {"tiled_mk_kn": (65, 48, 70), "dot": (4, 512, 5), "stream": (63, 33, 64)}
