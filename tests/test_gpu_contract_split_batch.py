"""Slice batches under the compute mode (`contract(..., compute="bf16x3", slice_batch=B)`): the split kernel has the
member axis of every GEMM kernel of the slice loop (csrc/contract.hip MemberArgs), so a batched run must be bit for bit
the unbatched one.

The three-tensor chains of tests/batch_cases.py with one tiled-class step -- as the stored step, whose operands are a
leaf read in place at the member's slice offset and a gathered copy in the member's arena, and as the output step, which
writes the members' blocks to the batch staging -- run unbatched and with B in (1, 5, 64): the bytes of the result, the
multiply-adds and the launch counts (ceil(12 / B) per path where the unbatched run makes 12, `split_launches` among them)
are compared.  Two equal wrong answers would pass that, so the result is also held to numpy's einsum of the whole sliced
sum in float64 / complex128:

    |got - ref| <= [2^-14 + (2 c 3 kt + 2) 2^-24] (|A| |B| |C|)      c = 1 real, c = 2 complex

the bound of tests/test_gpu_contract_split.py with one split step on the way of every term (2^-14, to first order: the
error of the stored step enters the output step's terms once) and kt the roundings an element goes through, counted as
in tests/test_gpu_contract_batch.py: K of the stored step, K of the output step and the assignments added into the
element; the float32 step is given the three roundings per product of the split one.
"""
import numpy as np
import pytest

from tests import batch_cases as bc
from tests.test_gpu_contract_batch import bits, by_class, einsum_reference, tiled

pytestmark = pytest.mark.gpu

N = bc.N_ASSIGNMENTS
BATCHES = (1, 5, 64)
CHAINS = [c for c in bc.PLAIN if c.classes.count("tiled") == 1]
assert [c.classes for c in CHAINS] == [("tiled", "stream"), ("stream", "tiled")]
COMPUTE = "bf16x3"


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def fill(chain, cplx, seed):
    """Full-precision float32 parts, magnitudes 2^uniform(-2, 2), random signs."""
    rng = np.random.RandomState(seed)
    part = lambda s: (rng.choice([-1.0, 1.0], s) * 2.0 ** rng.uniform(-2, 2, s)).astype(np.float32)  # noqa: E731
    return [(part(s) + 1j * part(s)).astype(np.complex64) if cplx else part(s) for s in chain.shapes()]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("chain", CHAINS, ids=[c.name for c in CHAINS])
def test_a_batched_run_is_the_unbatched_one_bit_for_bit(ctr, chain, cplx):
    arrays = fill(chain, cplx, seed=71)
    call = lambda **kw: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, compute=COMPUTE, **kw)  # noqa: E731
    base = call()
    want = dict(tiled=0, dot=0, stream=0)
    for k in chain.classes:
        want[k] += N
    assert by_class(ctr, base) == want and base.kernel_launches[0] == N
    assert base.split_launches == tiled(ctr, base) == N and base.batch_launches == 0 and base.slice_batch is None
    assert base.launches == sum(base.kernel_launches)
    for B in BATCHES:
        groups = -(-N // B)
        r = call(slice_batch=B)
        what = f"{chain.name} B = {B}"
        assert r.inds == base.inds and r.array.dtype == base.array.dtype, what
        assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the unbatched run"
        assert r.macs == base.macs and r.n_slices == base.n_slices == N, what
        assert r.kernel_launches == tuple(v // N * groups for v in base.kernel_launches), what
        assert r.split_launches == tiled(ctr, r) == groups, what
        assert r.batch_launches == groups and r.slice_batch == min(B, N) and r.compute == COMPUTE, what
        assert r.launches == sum(r.kernel_launches) + r.batch_launches, what
    # ... and the unbatched result against the einsum of the whole sliced sum
    ref, mag = einsum_reference(chain, arrays)
    got = base.array.transpose([base.inds.index(x) for x in chain.output])
    (_, _, k1), (_, _, k2) = chain.steps()
    kt = k1 + k2 + chain.summed
    bound = (2.0 ** -14 + (2 * (2 if cplx else 1) * 3 * kt + 2) * 2.0 ** -24) * mag
    err = np.abs(got.astype(ref.dtype) - ref)
    print(f"{chain.name}: largest error / bound {float((err / bound).max()):.4f} (kt {kt})")
    assert got.shape == ref.shape and (err <= bound).all()
    # the plain mode differs from it (the keyword does reach the batched launches)
    plain = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, slice_batch=5)
    assert plain.split_launches == 0 and not np.array_equal(bits(plain.array), bits(base.array))
