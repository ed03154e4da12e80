"""Slice batches and hoisting under the matrix mode (`contract(..., compute="matrix", slice_batch=B, hoist=True)`): the
matrix kernel has the member axis of every GEMM kernel of the slice loop (csrc/contract.hip MemberArgs) and runs a hoisted
step as a one-member launch, so a batched or hoisted run must be bit for bit the run without the keyword, in the four
dtypes.

The three-tensor chains of tests/batch_cases.py with one tiled-class step -- as the stored step, whose operands are a
leaf read in place at the member's slice offset and a gathered copy in the member's arena, and as the output step, which
writes the members' blocks to the batch staging -- run unbatched and with B in (1, 5, 64): the bytes of the result, the
multiply-adds and the launch counts (ceil(12 / B) per path where the unbatched run makes 12, `matrix_launches` among
them) are compared.  Two equal wrong answers would pass that, so the result is also held to numpy's einsum of the whole
sliced sum under the bound of the plain run (tests/test_gpu_contract_batch.py assert_einsum: the mode rounds nothing more
than the plain kernels do).

The tiled cases of tests/hoist_cases.py, where the kept tensor feeds a tiled-class step as its first or its second
operand: hoist=True alone and with slice_batch=5 against hoist=None, bytes and launch counts, and the einsum bound of the
plain run (tests/mode_cases.py plain_bound).
"""
import numpy as np
import pytest

from tests import batch_cases as bc
from tests import hoist_cases as hc
from tests import mode_cases as mc
from tests.test_gpu_contract_batch import assert_einsum, bits, by_class, fill, tiled

pytestmark = pytest.mark.gpu

N = bc.N_ASSIGNMENTS
BATCHES = (1, 5, 64)
CHAINS = [c for c in bc.PLAIN if c.classes.count("tiled") == 1]
assert [c.classes for c in CHAINS] == [("tiled", "stream"), ("stream", "tiled")]
COMPUTE = "matrix"


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=[np.dtype(d).name for d in bc.DTYPES])
@pytest.mark.parametrize("chain", CHAINS, ids=[c.name for c in CHAINS])
def test_a_batched_run_is_the_unbatched_one_bit_for_bit(ctr, chain, dtype):
    arrays = fill(chain, dtype, seed=91)
    call = lambda **kw: ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, compute=COMPUTE, **kw)  # noqa: E731
    base = call()
    want = dict(tiled=0, dot=0, stream=0)
    for k in chain.classes:
        want[k] += N
    assert by_class(ctr, base) == want and base.kernel_launches[0] == N
    assert base.matrix_launches == tiled(ctr, base) == N and base.batch_launches == 0 and base.slice_batch is None
    assert base.launches == sum(base.kernel_launches) and base.split_launches == 0
    assert base.array.dtype == np.dtype(dtype)
    for B in BATCHES:
        groups = -(-N // B)
        r = call(slice_batch=B)
        what = f"{chain.name} {np.dtype(dtype).name} B = {B}"
        assert r.inds == base.inds and r.array.dtype == base.array.dtype, what
        assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the unbatched run"
        assert r.macs == base.macs and r.n_slices == base.n_slices == N, what
        assert r.kernel_launches == tuple(v // N * groups for v in base.kernel_launches), what
        assert r.matrix_launches == tiled(ctr, r) == groups, what
        assert r.batch_launches == groups and r.slice_batch == min(B, N) and r.compute == COMPUTE, what
        assert r.launches == sum(r.kernel_launches) + r.batch_launches, what
    # ... and the unbatched result against the einsum of the whole sliced sum
    assert_einsum(chain, arrays, base, dtype, f"{chain.name} {np.dtype(dtype).name}")
    # the same launches as the plain mode, which does not count them as the matrix kernel's
    plain = ctr.contract(bc.PATH, chain.ts, arrays, chain.output, slices=bc.SLICES, slice_batch=5)
    assert plain.matrix_launches == 0 and plain.kernel_launches == call(slice_batch=5).kernel_launches


@pytest.mark.parametrize("dtype", ("float32", "float64", "complex64", "complex128"))
@pytest.mark.parametrize("name", hc.TILED)
def test_a_hoisted_run_is_the_run_without_hoist_bit_for_bit(ctr, name, dtype):
    case = hc.case(name, dtype)
    arrays = mc.fill(case, None)
    n = case.n_assignments()
    p = case.plan(hoist=True, compute=COMPUTE)
    assert p.hoisted == hc.TABLE[name][1] and p.compute == COMPUTE
    tiled_steps = [sig[0] == "tiled" for sig in mc.signature(p)]
    flags = [bool(f) for f in p.step_hoist]
    per = sum(t and not f for t, f in zip(tiled_steps, flags))  # tiled-class steps of an assignment
    once = sum(t and f for t, f in zip(tiled_steps, flags))  # ... of the hoisted phase
    assert per >= 1  # (the step that reads the kept tensor)

    def call(**kw):
        return ctr.contract(list(case.path), case.ts_inds, arrays, case.output_inds, slices=case.slices,
                            slice_range=case.slice_range, compute=COMPUTE, **kw)

    for B in (None, 5):
        kw = {} if B is None else dict(slice_batch=B)
        what = f"{name} {dtype} {kw}"
        base, r = call(**kw), call(hoist=True, **kw)
        G = n if B is None else -(-n // B)
        assert r.inds == base.inds and r.array.dtype == base.array.dtype == np.dtype(dtype), what
        assert np.array_equal(bits(r.array), bits(base.array)), f"{what}: the result differs from the run without hoist"
        assert r.hoisted == p.hoisted and base.hoisted is None, what
        assert base.matrix_launches == tiled(ctr, base) == (per + once) * G, what
        assert r.matrix_launches == tiled(ctr, r) == per * G + once, what
        assert r.macs == base.macs - (n - 1) * p.hoisted_macs, what
    got = call(hoist=True)
    ref, mag = mc.reference(case, case.plan(), arrays)
    err = np.abs(np.asarray(got.array).astype(ref.dtype) - ref)
    limit = mc.plain_bound(case, case.plan(), mag)
    print(f"{name} {dtype}: largest error / bound {float((err / limit).max()):.4f}")
    assert got.array.shape == ref.shape and not np.isnan(got.array).any() and (err <= limit).all(), (name, dtype)
