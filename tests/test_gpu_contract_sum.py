"""A path that leaves several tensors (`contract`, tnco_amd/contraction.py) on the device: its result is the sum, field
by field (`_sum_results`), of the calls on its parts.  The merging is host code, so the shapes are the smallest that
launch a kernel: two products of two matrices and a leaf that the path does not touch."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the path multiplies leaves 0 and 1, then (of what is left: leaf 2, leaf 3, leaf 4, the product) leaves 3 and 4
TS = [("a", "b"), ("b", "c"), ("u",), ("d", "e"), ("e", "f")]
SHAPES = [(2, 3), (3, 2), (5,), (3, 3), (3, 2)]
PATH = [(0, 1), (1, 2)]
OUT = ("a", "c", "u", "d", "f")


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.mark.parametrize("mode", [dict(), dict(hoist=True, indirect=True)], ids=["plain", "hoist-indirect"])
def test_a_path_that_leaves_three_tensors_is_the_sum_of_its_parts(ctr, mode):
    rng = np.random.default_rng(7)
    arrays = [rng.uniform(0.5, 1.5, s).astype(np.float32) for s in SHAPES]
    got = ctr.contract(PATH, TS, arrays, OUT, **mode)
    # the untouched leaf is made on the host: no launch, and of every keyword given the count of a call with nothing to do
    none = {k: v for k, v in dict(hoisted=(0, 0), indirect=0).items() if mode}
    parts = [ctr.ContractionResult(TS[2], arrays[2], 0, 1, 0, **none),
             ctr.contract([(0, 1)], TS[0:2], arrays[0:2], ("a", "c"), **mode),
             ctr.contract([(0, 1)], TS[3:5], arrays[3:5], ("d", "f"), **mode)]
    want = ctr._sum_results(parts, inds=[r.inds for r in parts], array=[r.array for r in parts], n_slices=1, exponents=None)
    assert [f.name for f in dataclasses.fields(got)][:2] == ["inds", "array"]
    assert got.inds == want.inds == [("u",), ("a", "c"), ("d", "f")]
    assert len(got.array) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got.array, want.array))
    assert np.array_equal(got.array[0], arrays[2])
    assert np.allclose(got.array[1], arrays[0] @ arrays[1], rtol=1e-6) and np.allclose(got.array[2], arrays[3] @ arrays[4], rtol=1e-6)
    for f in dataclasses.fields(got)[2:]:
        if f.name != "device_s":  # (wall clock)
            assert getattr(got, f.name) == getattr(want, f.name), f.name
    assert got.device_s > 0 and all(r.device_s > 0 for r in parts[1:])
    assert got.launches >= 2 and got.macs == 2 * 3 * 2 + 3 * 3 * 2 and got.n_slices == 1
    assert (got.hoisted, got.indirect) == (((0, 0), 0) if mode else (None, None))
