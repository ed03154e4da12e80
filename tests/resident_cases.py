"""The case table of the resident contraction tests (`contraction.Contractor`, csrc/contract_io.h), no GPU:
tests/test_contraction_resident_plan.py checks the table against the numpy models below, tests/test_gpu_contract_resident.py
runs it on the device against `contract()`.

A `View` is a base array and the operations that make the operand from it; `apply` performs them on a numpy array or on a
torch tensor alike, so the tensor a device test passes has exactly the dims, strides and storage offset the table states.
The model of the ingest kernel is `np.ascontiguousarray(view, dtype)`; the model of the emit kernel is the transpose of
`contraction._host_layout`.

Every view is run as a one-tensor network (a plan without steps: the leaf is the result) and as the first operand of a
step whose second operand B holds the view's last axis and a new one of 6 (a 0-d view: an outer product with B (6,));
"plain-4x5" makes that the 4 x 5 x 6 step.

The sizes: 1, 2, 3, 4, 5 and 7 elements cover every remainder of the 16-byte path in each dtype (4 floats, 2 doubles or
complex64, 1 complex128 per 16 bytes); `t[1:]` of a longer tensor moves the base off a 16-byte boundary (by 4 or 8 bytes;
a complex128 base stays aligned); 7 x 101 x 3 x 251 = 532 371 elements is the first odd-sized shape past one trip of the
grid, TRIP = 2048 blocks x 256 lanes = 524 288 (on the vector path a lane moves 16 bytes, so only the float32 -> float32
copy of that shape stays within one trip; the strided and the widening paths move one element per lane).

Unmergeable axes: an axis of dimension d >= 2 that does not merge with its neighbour multiplies the element count by d, so
32 of them need 2^32 elements, 16 GiB of float32 in the handle alone.  The device case is therefore 16 axes of dimension 2
in reversed order (65 536 elements, none of them merges); the 32 / 33-axis edge of `merge_axes` is tested on dims and
strides alone (MANY_AXES), with no storage of that size.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

TRIP = 2048 * 256  # elements one launch of ct_ingest_kernel / ct_emit_kernel reaches before its grid stride
DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
WIDENINGS = ((np.float32, np.float64), (np.float32, np.complex64), (np.float32, np.complex128),
             (np.float64, np.complex128), (np.complex64, np.complex128))
SMALL_SIZES = (1, 2, 3, 4, 5, 7)
EVERY = slice(None)


@dataclass(frozen=True)
class View:
    name: str
    base: tuple  # shape of the base array
    ops: tuple = ()  # ("index", key) / ("permute", axes) / ("expand", shape), in order
    merged: tuple = None  # what merge_axes makes of the view: (dims, strides in elements)
    offset: int = 0  # storage offset of the view, in elements

    @property
    def shape(self):
        return apply(self, np.zeros(self.base, np.int8)).shape

    @property
    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))


def apply(view, a):
    """The view of the base array `a`: numpy array or torch tensor."""
    for op, arg in view.ops:
        if op == "index":
            a = a[arg]
        elif op == "permute":
            a = a.permute(*arg) if hasattr(a, "permute") else a.transpose(arg)
        elif op == "expand":
            a = a.expand(*arg) if hasattr(a, "expand") else np.broadcast_to(a, arg)
        else:
            raise ValueError(op)
    return a


def fill(shape, dtype, seed):
    """Values that are exact in every dtype and distinct enough to tell a wrong element: small integers, both parts."""
    rng = np.random.RandomState(seed)
    a = rng.randint(-99, 100, size=shape).astype(np.float64)
    if np.dtype(dtype).kind == "c":
        a = a + 1j * rng.randint(-99, 100, size=shape)
    return a.astype(dtype)


def ingest_model(view, base, dtype):
    """What ct_ingest_kernel leaves in the leaf buffer: the view, C-contiguous, in the plan's dtype."""
    a = apply(view, base)
    return np.ascontiguousarray(a, dtype).reshape(a.shape)  # (ascontiguousarray alone gives a 0-d array one axis)


def emit_model(p, staging):
    """What ct_emit_kernel leaves in the caller's buffer: the output buffer, [block axes][the other axes], in the result's
    own axis order (contraction._host_layout without projections)."""
    rest = tuple(x for x in p.inds if x not in set(p.slice_inds))
    held = p.block_inds + rest
    array = np.asarray(staging).reshape(tuple(p.shape[p.inds.index(x)] for x in held))
    return array.transpose([held.index(x) for x in p.inds]).copy(order="C")  # (0-d stays 0-d)


def numpy_strides(a):
    return tuple(s // a.itemsize for s in a.strides)


CONTIGUOUS = tuple(View(f"contiguous-{n}", (n,), merged=(((n,), (1,)) if n > 1 else ((), ()))) for n in SMALL_SIZES)
UNALIGNED = tuple(View(f"unaligned-{n}", (n + 1,), (("index", slice(1, None)),),
                       merged=(((n,), (1,)) if n > 1 else ((), ())), offset=1) for n in SMALL_SIZES)
BIG = View("past-one-trip", (7, 101, 3, 251), merged=((7 * 101 * 3 * 251,), (1,)))
BIG_UNALIGNED = View("past-one-trip-unaligned", (7 * 101 * 3 * 251 + 1,), (("index", slice(1, None)),),
                     merged=((7 * 101 * 3 * 251,), (1,)), offset=1)
BIG_STRIDED = View("past-one-trip-permuted", (251, 7, 101, 3), (("permute", (1, 2, 3, 0)),),
                   merged=((7 * 101 * 3, 251), (1, 7 * 101 * 3)))
STRIDED = (
    View("scalar", (), merged=((), ())),
    View("plain-4x5", (4, 5), merged=((20,), (1,))),
    View("permuted", (5, 3, 4), (("permute", (2, 0, 1)),), merged=((4, 15), (1, 4))),
    View("stepped", (6, 11), (("index", (EVERY, slice(None, None, 2))),), merged=((6, 6), (11, 2))),
    View("stepped-merging", (6, 10), (("index", (EVERY, slice(None, None, 2))),), merged=((30,), (2,))),
    View("expanded", (4, 1, 5), (("expand", (4, 3, 5)),), merged=((4, 3, 5), (5, 0, 1))),
    View("expanded-twice", (1, 1, 5), (("expand", (2, 3, 5)),), merged=((6, 5), (0, 1))),
    View("offset", (6, 7), (("index", (slice(2, None), slice(3, None))),), merged=((4, 4), (7, 1)), offset=2 * 7 + 3),
    View("offset-row", (6, 7), (("index", 5),), merged=((7,), (1,)), offset=35),
    View("16-axes", (2,) * 16, (("permute", tuple(reversed(range(16)))),),
         merged=((2,) * 16, tuple(2 ** k for k in range(16)))),
)
assert BIG.numel == 532371 > TRIP and BIG.numel % 2 == 1
assert STRIDED[-1].numel == 65536
VIEWS = CONTIGUOUS + UNALIGNED + (BIG, BIG_UNALIGNED, BIG_STRIDED) + STRIDED


def networks(view):
    """The two networks of a view as (name, ts_inds, shapes, path, output): the leaf alone, and the leaf times B."""
    axes = tuple(f"a{k}" for k in range(len(view.shape)))
    shape = tuple(view.shape)
    alone = ("alone", [axes], [shape], [], axes)
    if axes:
        step = ("step", [axes, (axes[-1], "n")], [shape, (shape[-1], 6)], [(0, 1)], axes[:-1] + ("n",))
    else:
        step = ("step", [axes, ("n",)], [shape, (6,)], [(0, 1)], ("n",))
    return alone, step


# merge_axes on dims and strides alone: (name, shape, strides, merged or the exception)
def _many(n):  # n axes of dimension 2, reversed: none merges
    return (2,) * n, tuple(2 ** k for k in range(n))


MANY_AXES = (
    ("32-axes", *_many(32), _many(32)),
    ("33-axes", *_many(33), NotImplementedError),
    # 33 axes of which the last two merge: 32 are left
    ("33-axes-two-merge", (2,) * 33, tuple(2 ** k for k in range(2, 33)) + (2, 1),
     ((2,) * 31 + (4,), tuple(2 ** k for k in range(2, 33)) + (1,))),
    # 40 axes of which 8 have dimension 1: 32 are left
    ("40-axes-8-ones", (2, 1) * 8 + (2,) * 24, tuple(2 ** k for k in range(40)),
     ((2,) * 32, tuple(2 ** k for k in range(0, 16, 2)) + tuple(2 ** k for k in range(16, 40)))),
    ("negative", (3, 4), (4, -1), ValueError),
    ("negative-on-a-one", (3, 1), (1, -1), ((3,), (1,))),
)
# emit: (name, ts_inds, dims, path, output_inds, slices): the result's kept sliced index is not its leading axis
EMIT_SCALAR = ("scalar", [("i",), ("i",)], dict(i=7), [(0, 1)], (), ())
EMIT_PERMUTE = ("permute", [("i", "p", "k"), ("k", "j")], dict(i=3, p=4, k=5, j=6), [(0, 1)], ("i", "p", "j"), ("p",))
