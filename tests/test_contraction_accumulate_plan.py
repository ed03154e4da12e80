"""`accumulate="float64"` (tnco_amd/contraction.py, "Wide accumulation") without a GPU: what the keyword refuses and in
which order, that it leaves every table of the plan alone, what it adds to `Plan.peak_device_bytes` term by term, and the
numpy model of the definition (tests/accumulate_cases.py `model`) against exact rational arithmetic on the designed sums.

The planted defect: a running sum in float32, which is what the engine does without the keyword
(`accumulate_cases.running_float32`).  The model must differ from it on exactly the sums designed to differ."""
import dataclasses
import math
import types
from fractions import Fraction

import numpy as np
import pytest

from tests import accumulate_cases as ac
from tests import batch_cases as bc
from tests import hoist_cases as hc
from tests import reuse_cases as rc
from tnco_amd import contraction as ctr

PATH = [(0, 1), (0, 1)]
TS = [("a", "b"), ("b", "c"), ("c", "a", "d")]
SHAPES = [(2, 3), (3, 2), (2, 2, 2)]
PROJS = [[0], [1]]
VALUE = (ValueError, "'accumulate' must be None or 'float64'.")
DTYPE = (TypeError, "with 'accumulate' the compute dtype must be float32 or complex64, not {}.")
NO_PROJS = (NotImplementedError, "projections are not supported with 'accumulate'.")


class Untouchable:
    def __getattribute__(self, name):
        raise AssertionError(f"the network was touched ({name})")


@pytest.fixture
def no_gpu(monkeypatch):
    from tnco_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", refuse)


def outcome(call):
    try:
        return call()
    except Exception as e:  # noqa: BLE001 (every type is compared)
        return type(e), str(e)


def three_ways(dtype, **kw):
    """The outcomes of plan, contract and contract_results for one set of keywords."""
    arrays = [np.ones(s, dtype) for s in SHAPES]
    net = Untouchable()
    more = dict(kw, sparse_inds=("d",)) if kw.get("projs") is not None else kw
    return (outcome(lambda: ctr.plan(PATH, TS, SHAPES, ("d",), slices=("a",), dtype=dtype, **more)),
            outcome(lambda: ctr.contract(PATH, TS, arrays, ("d",), slices=("a",), **more)),
            outcome(lambda: ctr.contract_results(net, arrays, net, net, **kw)))


@pytest.mark.parametrize("value", ["float32", "x", True, 64, np.float64, ("float64",)], ids=repr)
def test_a_value_other_than_none_and_float64_is_refused(no_gpu, value):
    assert three_ways(np.float32, accumulate=value) == (VALUE,) * 3
    # its own rules in order: the value before the dtype before the projections
    assert three_ways(np.float64, accumulate=value, projs=PROJS)[:2] == (VALUE,) * 2


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["float64", "complex128"])
def test_a_wide_compute_dtype_is_refused_before_the_projections(no_gpu, dtype):
    want = (DTYPE[0], DTYPE[1].format(np.dtype(dtype).name))
    plan, contract, results = three_ways(dtype, accumulate="float64")
    assert plan == contract == want
    # contract_results checks at float32 before it looks at the network, at the arrays' dtype after
    assert results[0] is AssertionError and "the network was touched" in results[1]
    dense = types.SimpleNamespace(sparse_inds=())
    arrays = [np.ones(s, dtype) for s in SHAPES]
    assert outcome(lambda: ctr.contract_results(dense, arrays, dense, Untouchable(), accumulate="float64")) == want
    assert three_ways(dtype, accumulate="float64", projs=PROJS)[:2] == (want,) * 2
    assert three_ways(dtype, accumulate="float64", projs=PROJS)[2] == NO_PROJS  # (first stage: float32)


def test_projections_are_refused(no_gpu):
    assert three_ways(np.float32, accumulate="float64", projs=PROJS) == (NO_PROJS,) * 3
    assert three_ways(np.complex64, accumulate="float64", projs=PROJS) == (NO_PROJS,) * 3


EARLIER = [
    (dict(compute="x"), ValueError, "'compute' must be None or 'bf16x3' or 'matrix'."),
    (dict(compute="bf16x3", storage="float16"), ValueError, "'compute' and 'storage' are exclusive."),
    (dict(storage="x"), ValueError, "'storage' must be None, 'float16' or 'bfloat16'."),
    (dict(scaling="tensor"), ValueError, "'scaling' needs 'storage'."),
    (dict(slice_batch=0), ValueError, "'slice_batch' must be None or an integer from 1 to 64."),
    (dict(path_kernel=2, slice_batch=4), ValueError, "'path_kernel' and 'slice_batch' are exclusive."),
    (dict(hoist=False), ValueError, "'hoist' must be None or True."),
    (dict(hoist=True, path_kernel=2), NotImplementedError, "'hoist' is not supported with 'path_kernel'."),
    (dict(indirect=True, storage="float16"), NotImplementedError, "'storage' is not supported with 'indirect'."),
    (dict(reuse=True, hoist=True), ValueError, "'reuse' includes 'hoist': give one of them."),
    (dict(slice_order="reuse"), ValueError, "slice_order='reuse' needs reuse=True."),
    (dict(slice_order="x"), ValueError, "'slice_order' must be None, 'reuse' or every sliced index once."),
    (dict(hoist=True, projs=PROJS), NotImplementedError, "projections are not supported with 'hoist'."),
    (dict(slice_order=("a",), projs=PROJS), NotImplementedError, "projections are not supported with 'slice_order'."),
]


@pytest.mark.parametrize("kw,exc,text", EARLIER, ids=[",".join(k[0]) for k in EARLIER])
@pytest.mark.parametrize("value", ["float64", "x"])
def test_the_refusal_of_an_earlier_keyword_wins(no_gpu, kw, exc, text, value):
    """`accumulate` is checked after every other keyword: valid or not, with it the call is refused as without it."""
    assert three_ways(np.float32, **kw) == ((exc, text),) * 3
    assert three_ways(np.float32, accumulate=value, **kw) == ((exc, text),) * 3


def test_the_dtype_refusal_of_an_earlier_keyword_wins(no_gpu):
    want = (TypeError, "with 'storage' the compute dtype must be float32 or complex64, not float64.")
    assert three_ways(np.float64, storage="float16", accumulate="float64")[:2] == (want,) * 2


def fields_equal(a, b, skip=()):
    assert [f.name for f in dataclasses.fields(a)] == [f.name for f in dataclasses.fields(b)]
    for f in dataclasses.fields(a):
        if f.name in skip:
            continue
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f.name
        elif f.name == "ops":
            assert repr(x) == repr(y)
        else:
            assert type(x) is type(y) and x == y, f.name


def chain_plan(chain, dtype=np.float32, **kw):
    return ctr.plan(bc.PATH, chain.ts, chain.shapes(), chain.output, slices=bc.SLICES, dtype=dtype, **kw)


MODES = [dict(), dict(slice_batch=5), dict(path_kernel=5), dict(slice_range=(1, 11)), dict(storage="bfloat16"),
         dict(storage="float16", scaling="tensor", slice_batch=5), dict(compute="bf16x3"), dict(compute="matrix"),
         dict(indirect=True), dict(hoist=True), dict(reuse=True, slice_order="reuse")]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: ",".join(m) or "plain")
def test_none_is_the_plan_without_the_keyword_and_float64_changes_no_table(mode):
    for chain in (bc.PLAIN[0], bc.SUMMED, bc.PLACED):
        for dtype in (np.float32, np.complex64):
            base = chain_plan(chain, dtype, **mode)
            fields_equal(chain_plan(chain, dtype, accumulate=None, **mode), base)
            wide = chain_plan(chain, dtype, accumulate="float64", **mode)
            assert wide.accumulate == "float64" and base.accumulate is None
            fields_equal(wide, base, skip=("accumulate",))
            assert wide.macs == base.macs and wide.n_slices == base.n_slices
    for table, name in ((hc, "kept-first-stream-7-9-11"), (rc, "nested")):
        c = table.case(name)
        kw = {k: v for k, v in mode.items() if k in ("hoist", "reuse", "slice_order", "indirect")}
        if table is hc and "reuse" in kw:
            continue
        fields_equal(c.plan(accumulate="float64", **kw), c.plan(**kw), skip=("accumulate",))


def test_the_field_is_the_last_of_the_plan_and_the_result_has_none():
    assert dataclasses.fields(ctr.Plan)[-1].name == "accumulate" and dataclasses.fields(ctr.Plan)[-1].default is None
    assert "accumulate" not in {f.name for f in dataclasses.fields(ctr.ContractionResult)}
    assert ctr.ACCUMULATES == ("float64",) and "ACCUMULATES" in ctr.__all__


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["float32", "complex64"])
@pytest.mark.parametrize("chain", [bc.PLAIN[4], bc.SUMMED, bc.PLACED, bc.HALF[0]], ids=lambda c: c.name)
def test_peak_device_bytes_term_by_term(chain, dtype):
    item = np.dtype(dtype).itemsize
    for mode in (dict(), dict(storage="float16", scaling="tensor"), dict(hoist=True)):
        base = chain_plan(chain, dtype, **mode)
        out, block = base.out_numel, base.out_numel // chain.n_blocks
        assert out == math.prod(base.shape)
        # unbatched: the accumulator and a staging block
        assert chain_plan(chain, dtype, accumulate="float64", **mode).peak_device_bytes == \
            base.peak_device_bytes + 2 * item * out + item * block
        # a slice batch and the path kernel stage in their own buffers: the accumulator alone
        for kw in (dict(slice_batch=5), dict(slice_batch=1), dict(path_kernel=5), dict(path_kernel=1024)):
            if "path_kernel" in kw and mode.keys() & {"storage", "hoist"}:
                continue
            grouped = chain_plan(chain, dtype, **mode, **kw)
            assert chain_plan(chain, dtype, accumulate="float64", **mode, **kw).peak_device_bytes == \
                grouped.peak_device_bytes + 2 * item * out
    free = 10 ** 9
    p = chain_plan(chain, dtype, accumulate="float64")
    ctr.check_memory(p, p.peak_device_bytes)
    with pytest.raises(RuntimeError, match=f"needs {p.peak_device_bytes} bytes"):
        ctr.check_memory(p, p.peak_device_bytes - 1)
    ctr.check_memory(p, free)


def test_a_plan_without_steps_sums_nothing_and_reserves_nothing():
    kw = dict(slices=("s",), dtype=np.complex64)
    base = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], **kw)
    wide = ctr.plan([], [("i", "s", "j")], [(5, 3, 7)], accumulate="float64", **kw)
    fields_equal(wide, base, skip=("accumulate",))
    assert wide.peak_device_bytes == base.peak_device_bytes and len(wide.steps) == 0


# --- the model --------------------------------------------------------------------------------------------------------
def one_block(terms):
    return [((), np.float32(t)) for t in terms]


@pytest.mark.parametrize("name", ac.EDGES)
def test_the_model_is_the_exact_sum_rounded_once_where_the_float64_sum_is_exact(name):
    terms = ac.edge_terms(name)
    got = ac.model(one_block(terms), (), np.float32)
    assert got.dtype == np.float32 and got.shape == ()
    if not all(np.isfinite(t) for t in terms):
        assert np.isnan(got) and np.isnan(math.fsum([float(terms[0])]) - math.fsum([float(-terms[1])]))
        return
    exact = sum((Fraction(float(t)) for t in terms), Fraction(0))
    # the float64 running sum, step by step in rational arithmetic: exact, except where the case is the float64 tie
    run, inexact = 0.0, False
    for k, t in enumerate(terms):
        nxt = run + float(t)
        inexact |= Fraction(nxt) != Fraction(run) + Fraction(float(t))
        run = nxt
    assert inexact == (name == "float64-tie")
    assert run == math.fsum(float(t) for t in terms) or inexact
    want = ac.round_to_float32_bits(Fraction(run))
    if Fraction(run) == 0:  # a rational has no sign: the zero is -0.0 iff every term is
        want = 0x80000000 if all(np.signbit(t) for t in terms) else 0
    assert int(got.view(np.uint32)) == want, (name, got, hex(want))
    if not inexact:
        assert ac.round_to_float32_bits(exact) == (want & 0x7FFFFFFF if exact == 0 else want)


EXPECTED = {"ones-after-2^24": ac.TWO24 + 64, "tie-to-even-down": ac.TWO24, "tie-to-even-up": ac.TWO24 + 4, "overflow": np.inf,
            "overflow-taken-back": ac.BIG, "minus-zero-alone": -0.0, "minus-zero-then-zero": 0.0,
            "subnormal-after-cancellation": ac.TINY, "subnormal-odd-multiple": 3 * ac.TINY, "float64-tie": 2.0 ** -96,
            "two-half-ulps": 1.0 + 2.0 ** -23}


@pytest.mark.parametrize("name", ac.EDGES)
def test_the_designed_sums_are_what_they_are_named_after(name):
    got = ac.model(one_block(ac.edge_terms(name)), (), np.float32)
    if name == "inf-minus-inf":
        assert np.isnan(got)
    else:
        assert ac.bits(got).tobytes() == ac.bits(np.float32(EXPECTED[name])).tobytes(), (name, got)
    if name.startswith("minus-zero"):
        assert ac.bits(ac.edge_terms(name)[0]).tobytes() == ac.bits(np.float32(-0.0)).tobytes()  # the product underflows


@pytest.mark.parametrize("name", ac.EDGES)
def test_the_model_differs_from_a_float32_running_sum_exactly_where_it_is_meant_to(name):
    parts = one_block(ac.edge_terms(name))
    wide, narrow = ac.model(parts, (), np.float32), ac.running_float32(parts, (), np.float32)
    assert ac.same_bytes(wide, narrow) != EDGES_DIFFER[name], (name, wide, narrow)
    if name == "ones-after-2^24":
        assert narrow == ac.TWO24 and wide == ac.TWO24 + 64


EDGES_DIFFER = {n: d for n, (_, d) in ac.EDGES.items()}


def test_the_model_places_the_first_block_adds_the_later_ones_and_leaves_the_rest_zero():
    """Blocks in assignment order over an output of three blocks, complex: each part on its own."""
    z = lambda re, im: np.full(2, re + 1j * im, np.complex64)  # noqa: E731
    parts = [((0, slice(None)), z(ac.TWO24, -0.0)), ((2, slice(None)), z(1, ac.TWO24)), ((0, slice(None)), z(1, 0.0)),
             ((2, slice(None)), z(1, 3)), ((0, slice(None)), z(2, -0.0))]
    got = ac.model(parts, (3, 2), np.complex64)
    want = np.array([[ac.TWO24 + 4 + 0j] * 2, [0j] * 2, [2 + 1j * (ac.TWO24 + 4)] * 2], np.complex64)
    assert ac.same_bytes(got, want)
    narrow = ac.running_float32(parts, (3, 2), np.complex64)
    assert narrow[0, 0].real == ac.TWO24 + 2 and narrow[2, 0].imag == ac.TWO24 + 4
    # a -0.0 block alone stays -0.0; a block that no assignment reaches is +0.0
    alone = ac.model([((1,), np.float32(-0.0))], (2,), np.float32)
    assert ac.bits(alone).tobytes() == ac.bits(np.array([0.0, -0.0], np.float32)).tobytes()


def test_where_of_follows_the_order_of_the_sliced_indices():
    p = chain_plan(bc.PLAIN[4])
    assert p.slice_inds == ("p", "u", "t") and p.block_inds == ("p",)
    assert [ac.where_of(p, a)[p.inds.index("p")] for a in range(12)] == [0] * 4 + [1] * 4 + [2] * 4
    q = chain_plan(bc.PLAIN[4], slice_order=("t", "p", "u"))
    assert [ac.where_of(q, a)[q.inds.index("p")] for a in range(12)] == [0, 0, 1, 1, 2, 2] * 2
