"""How several calls become one `ContractionResult` (tnco_amd/contraction.py `_sum_results`), without a GPU: every
field of the sum of hand-made parts against the rule for that field, the counters distinct primes so that no two fields
and no two parts can be mistaken for each other."""
import dataclasses
import itertools

import numpy as np
import pytest

from tnco_amd import contraction as ctr

SUMS = ("macs", "launches", "device_s", "narrow_launches", "batch_launches", "split_launches", "matrix_launches")
TUPLE_SUMS = ("kernel_launches", "row_kernel_launches", "path_launches", "indirect_launches")
GIVEN = ("inds", "array", "n_slices", "exponents", "fuse_macs")


def primes():
    return (n for n in itertools.count(2) if all(n % d for d in range(2, int(n ** 0.5) + 1)))


def part(p, **optional):
    """A result with the next primes of `p` in every counter; `optional`: the fields that a call may leave None."""
    nxt = lambda: next(p)  # noqa: E731
    return ctr.ContractionResult(
        inds=("i", nxt()), array=np.full(2, nxt()), macs=nxt(), n_slices=nxt(), peak_device_bytes=nxt(), launches=nxt(),
        device_s=float(nxt()), fuse_macs=nxt(), kernel_launches=tuple(nxt() for _ in ctr.KERNEL_PATHS),
        row_kernel_launches=tuple(nxt() for _ in ctr.ROW_KERNEL_PATHS), scaling="tensor", exponents=(nxt(), nxt()),
        narrow_launches=nxt(), batch_launches=nxt(), compute="matrix", split_launches=nxt(), path_launches=(nxt(), nxt()),
        indirect_launches=tuple(nxt() for _ in ctr.INDIRECT_KERNEL_PATHS), matrix_launches=nxt(), **optional)


def test_every_field_of_a_sum_follows_its_rule():
    assert {f.name for f in dataclasses.fields(ctr.ContractionResult)} == \
        set(SUMS) | set(TUPLE_SUMS) | set(GIVEN) | {"peak_device_bytes", "slice_batch", "path_kernel", "hoisted", "reused",
                                                    "indirect", "scaling", "compute"}
    p = primes()
    nxt = lambda: next(p)  # noqa: E731
    parts = [part(p),
             part(p, slice_batch=nxt(), path_kernel=nxt(), hoisted=(nxt(), nxt()), reused=(nxt(), nxt()), indirect=nxt()),
             part(p, slice_batch=nxt(), hoisted=(nxt(), nxt()), indirect=nxt()),
             part(p, path_kernel=nxt(), reused=(nxt(), nxt()))]
    counters = [v for r in parts for f in dataclasses.fields(r) if f.name not in ("inds", "array", "scaling", "compute")
                for v in np.ravel(getattr(r, f.name)) if v is not None]
    assert len(set(counters)) == len(counters)  # (no value stands in two places)
    array, exponents = object(), object()
    got = ctr._sum_results(parts, inds=("z",), array=array, n_slices=1009, exponents=exponents, fuse_macs=1013)
    assert type(got) is ctr.ContractionResult
    for name in SUMS:
        assert getattr(got, name) == sum(getattr(r, name) for r in parts), name
        assert type(getattr(got, name)) is type(getattr(parts[0], name)), name
    for name in TUPLE_SUMS:
        assert getattr(got, name) == tuple(sum(c) for c in zip(*(getattr(r, name) for r in parts))), name
    assert got.peak_device_bytes == max(r.peak_device_bytes for r in parts) == parts[3].peak_device_bytes
    assert got.slice_batch == parts[2].slice_batch and got.path_kernel == parts[3].path_kernel  # the largest of those set
    assert got.hoisted == tuple(a + b for a, b in zip(parts[1].hoisted, parts[2].hoisted))
    assert got.reused == tuple(a + b for a, b in zip(parts[1].reused, parts[3].reused))
    assert got.indirect == parts[1].indirect + parts[2].indirect
    assert got.scaling == "tensor" and got.compute == "matrix"
    assert got.inds == ("z",) and got.array is array and got.n_slices == 1009 and got.exponents is exponents
    assert got.fuse_macs == 1013
    # what no part has stays None; what the caller does not give is the field's default
    bare = ctr._sum_results(parts[:1], inds=(), array=None, n_slices=1, exponents=None)
    assert (bare.slice_batch, bare.path_kernel, bare.hoisted, bare.reused, bare.indirect) == (None,) * 5
    assert bare.fuse_macs == 0 and bare.macs == parts[0].macs and bare.kernel_launches == parts[0].kernel_launches
    zeros = ctr._sum_results([dataclasses.replace(parts[0], hoisted=(0, 0), reused=(0, 0), indirect=0, slice_batch=1)] * 2,
                             inds=(), array=None, n_slices=1, exponents=None)
    assert (zeros.hoisted, zeros.reused, zeros.indirect, zeros.slice_batch) == ((0, 0), (0, 0), 0, 1)  # (0 is not None)
    plain = ctr._sum_results([ctr.ContractionResult((), None, 3, 1, 5)] * 2, inds=(), array=None, n_slices=1, exponents=None)
    assert plain == ctr.ContractionResult((), None, 6, 1, 5)
    with pytest.raises(ValueError):  # the parts of one call run in one mode
        ctr._sum_results([parts[0], dataclasses.replace(parts[1], compute=None)], inds=(), array=None, n_slices=1,
                         exponents=None)


def test_replacing_fuse_macs_leaves_every_other_field():
    p = primes()
    r = part(p, slice_batch=next(p), path_kernel=next(p), hoisted=(next(p), next(p)), reused=(next(p), next(p)),
             indirect=next(p))
    q = dataclasses.replace(r, fuse_macs=4)
    assert q.fuse_macs == 4 and type(q) is type(r)
    for f in dataclasses.fields(r):
        if f.name != "fuse_macs":
            assert getattr(q, f.name) is getattr(r, f.name), f.name
