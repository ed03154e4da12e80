"""The case table of the mode tests (tests/test_contraction_modes_plan.py, tests/test_gpu_contract_modes.py,
tools/fuzz_contract.py): small random networks, and a few written by hand, that every way of running a plan -- plain,
`slice_batch=`, `path_kernel=`, `compute="bf16x3"`, `storage=`, `storage=` with `scaling="tensor"` -- is run on.  No GPU
and no device import.

The chains of tests/batch_cases.py, tests/path_cases.py and tests/split_cases.py hold the GEMM edges; what they do not
vary is the *plan*: which operand is a leaf read in place and which lives in the arena, the memory order of either, a
batch axis, how many permutes run between two steps, what stays live in the arena while another branch is contracted.
`signature(plan)` names that per step, `coverage(case, plan)` turns it into the list of REQUIRED items, and the table
below reaches every one of them in a real and in a complex dtype (tests/test_contraction_modes_plan.py asserts it item
by item).

A case is cheap by construction (`caps`): 4 to 10 leaves of at most 2^18 elements, 2 to 64 slice assignments, at most
5 10^7 multiply-adds over all of them, an arena of at most 2^22 elements, every step within MAX_PATH_STEP_MACS, so that
it is legal in every mode.

Two fills, alternating over the table: "uniform", both parts uniform in (0.5, 1.5) (no zeros, no cancellation: the fill
of tests/path_cases.py), and "normal", standard normal times 1 / sqrt(numel) (signed: the `_arrays` of
tests/test_contraction_plan.py).
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import numpy as np

from tests.test_contraction_plan import _arrays, _greedy_path, _random_path
from tnco_amd import contraction as ctr
from tnco_amd import synthetic as syn

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
SINGLES = (np.dtype(np.float32), np.dtype(np.complex64))  # the dtypes the bf16x3 and the storage modes take
FILLS = ("uniform", "normal")
BATCHES = (3, 64)  # slice_batch= of the device test
GROUPS = (3, 1024)  # path_kernel= of the device test
HALF_BATCH = 3  # slice_batch= beside compute= and storage=
STORAGE_MODES = (dict(storage="bfloat16"), dict(storage="float16", scaling="tensor"))
U_STORAGE = dict(bfloat16=2.0 ** -8, float16=2.0 ** -11)  # unit roundoff of the storage types

MAX_LEAF = 1 << 18
MAX_ARENA = 1 << 22
MAX_MACS = 5 * 10 ** 7
MAX_OUT = 1 << 18  # (the generator's own: keeps the double-precision einsum of a case well under a second)
CLASSES = ("tiled", "dot", "stream")


@dataclass(frozen=True)
class Case:
    name: str
    ts_inds: tuple
    dims: tuple  # ((index, dimension), ...)
    output_inds: tuple
    path: tuple
    slices: tuple
    dtype: str
    fill: str
    slice_range: tuple = None

    @property
    def dim(self):
        return dict(self.dims)

    def shapes(self):
        d = self.dim
        return [tuple(d[x] for x in xs) for xs in self.ts_inds]

    def n_assignments(self):
        lo, hi = self.slice_range or (0, math.prod(self.dim[x] for x in self.slices))
        return hi - lo

    def plan(self, **mode):
        return ctr.plan(list(self.path), self.ts_inds, self.shapes(), self.output_inds, slices=self.slices,
                        slice_range=self.slice_range, dtype=np.dtype(self.dtype), **mode)

    def with_(self, **kw):
        return Case(**{**self.__dict__, **kw})

    def paste(self):
        """The case as a line of Python for the table."""
        return (f"Case({self.name!r}, {self.ts_inds!r}, {self.dims!r}, {self.output_inds!r}, {self.path!r}, "
                f"{self.slices!r}, {self.dtype!r}, {self.fill!r}, {self.slice_range!r})")


def klass(H, M, N, K):
    """The shape class of a step: the dispatch of csrc/contract.hip launch_gemm (the dot class counts H in its outputs)."""
    if M >= 64 and N >= 64 and K > 32:
        return "tiled"
    return "dot" if K >= 512 and H * M * N <= 8192 else "stream"


def signature(p):
    """Per step of the plan: (class, form_a, form_b, H > 1, kind of A, kind of B), kinds "leaf" (read in place) or
    "arena"."""
    kind = {ctr.LEAF: "leaf", ctr.ARENA: "arena"}
    return tuple((klass(op["H"], op["M"], op["N"], op["K"]), op["form_a"], op["form_b"], op["H"] > 1,
                  kind[int(st[0])], kind[int(st[4])]) for st, op in zip(p.steps, p.ops))


def kernel_slot(sig):
    """The name in contraction.KERNEL_PATHS that a step of this signature is counted under."""
    cls, form_a, form_b = sig[:3]
    if cls != "tiled":
        return cls
    return ctr.KERNEL_PATHS[1 + 2 * (form_a == 0) + (form_b == 0)]


def launches_per_assignment(p):
    """kernel_launches of one slice assignment of an unbatched run, in KERNEL_PATHS order: a gather launch per permute
    group that has rows, and every step in the slot of its class."""
    count = dict.fromkeys(ctr.KERNEL_PATHS, 0)
    count["gather"] = len(set(p.perms[:, 6].tolist()))
    for sig in signature(p):
        count[kernel_slot(sig)] += 1
    return tuple(count[name] for name in ctr.KERNEL_PATHS)


def _sliced_by(p, leaf):
    row = p.leaf_sl[leaf]
    return frozenset(int(v) for v in row[1:1 + int(row[0])])


def arena_permutes(p):
    return int(((p.perms[:, 0] == ctr.ARENA) & (p.perms[:, 2] == ctr.ARENA)).sum())


REQUIRED = tuple(
    [f"{c}:arena-arena" for c in CLASSES] + [f"{c}:leaf" for c in CLASSES] + ["stream:two-sliced-leaves"] +
    [f"{c}:H>1" for c in CLASSES] +
    [f"{c}:form{a}{b}" for c in ("tiled", "stream") for a in (0, 1) for b in (0, 1)] +
    [f"dot:form{a}{b}" for a, b in ((0, 0), (0, 1), (1, 0))] +
    ["permutes>=3", "sliced-index-on-3-tensors", "block-revisited", "dimension-1", "ragged-count", "range-off-zero"])
# the items that the bf16x3 and the storage modes must see too: in float32 or complex64
REQUIRED_SINGLE = tuple(r for r in REQUIRED if r.startswith(("tiled:", "dot:")))


def coverage(case, p):
    """The items of REQUIRED (and more of their kind) that the case reaches."""
    got = set()
    for st, (cls, form_a, form_b, batch, ka, kb) in zip(p.steps, signature(p)):
        if ka == kb == "arena":
            got.add(f"{cls}:arena-arena")
        if "leaf" in (ka, kb):
            got.add(f"{cls}:leaf")
        if cls == "stream" and ka == kb == "leaf":
            sa, sb = _sliced_by(p, int(st[1])), _sliced_by(p, int(st[5]))
            if sa and sb and sa != sb:
                got.add("stream:two-sliced-leaves")
        if batch:
            got.add(f"{cls}:H>1")
        got.add(f"{cls}:form{form_a}{form_b}")
    if arena_permutes(p) >= 3:
        got.add("permutes>=3")
    if any(sum(x in xs for xs in case.ts_inds) >= 3 for x in case.slices):
        got.add("sliced-index-on-3-tensors")
    if p.block_inds and len(p.block_inds) < len(p.slice_inds):
        lo, hi = p.slice_range
        n_blocks = math.prod(case.dim[x] for x in p.block_inds)
        if hi - lo > n_blocks or _blocks_of(p, lo, hi) < hi - lo:
            got.add("block-revisited")
    if any(d == 1 for x, d in case.dims if any(x in xs for xs in case.ts_inds)):
        got.add("dimension-1")
    n = case.n_assignments()
    if all(n % q for q in set(BATCHES + GROUPS + (HALF_BATCH,))):
        got.add("ragged-count")
    if p.slice_range[0] > 0:
        got.add("range-off-zero")
    return got


def _block_of(p, sid):
    blk = 0
    for x in p.block_inds:
        s = p.slice_inds.index(x)
        blk = blk * p.slice_dims[s] + (sid // math.prod(p.slice_dims[s + 1:])) % p.slice_dims[s]
    return blk


def _blocks_of(p, lo, hi):
    return len({_block_of(p, sid) for sid in range(lo, hi)})


def summed_assignments(p):
    """The largest number of assignments of the plan's range that are added into one element of the result."""
    seen = {}
    for sid in range(*p.slice_range):
        seen[_block_of(p, sid)] = seen.get(_block_of(p, sid), 0) + 1
    return max(seen.values())


def kt(p):
    """The roundings an element of the result goes through: K of every step, and the assignments added into it."""
    return sum(op["K"] for op in p.ops) + summed_assignments(p)


def tiled_depth(case, p):
    """The number of tiled-class steps on the longest chain of steps that feeds the output."""
    live = [0] * len(case.ts_inds)
    for (a, b), sig in zip(case.path, signature(p)):
        a, b = sorted((a, b))
        db, da = live.pop(b), live.pop(a)
        live.append(max(da, db) + (sig[0] == "tiled"))
    return live[0]


def caps(case):
    """The limits of a case that are broken, as strings; empty: the case is within all of them."""
    bad = []
    if not 4 <= len(case.ts_inds) <= 10:
        bad.append("leaves")
    if any(math.prod(s) > MAX_LEAF for s in case.shapes()):
        bad.append("leaf size")
    if not 2 <= case.n_assignments() <= 64:
        bad.append("assignments")
    try:
        p = case.plan(path_kernel=8)
    except ValueError as e:  # (a step beyond MAX_PATH_STEP_MACS)
        return bad + [str(e)]
    if p.macs > MAX_MACS:
        bad.append("multiply-adds")
    if p.arena_elems > MAX_ARENA:
        bad.append("arena")
    if p.out_numel > MAX_OUT:
        bad.append("output size")
    return bad


DIM_SETS = ((2,), (2, 3), (1, 2, 3, 5), (2, 4, 8), (2, 3, 4, 16), (4, 8, 16, 32), (1, 2, 32), (2, 6, 24), (3, 8, 64),
            (2, 2, 2, 600), (2, 2, 3, 520), (8, 9, 40))


def generate(seed, dtype=None, fill=None):
    """The case of a seed, or None when the network the seed gives is beyond the caps.  Deterministic: numpy's frozen
    RandomState stream and the project's own generators."""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(4, 11))
    choices = DIM_SETS[int(rng.randint(len(DIM_SETS)))]
    if rng.randint(2):
        n += n % 2
        ts, _, _ = syn.random_regular_tn(n, seed=seed)
        n_inds = 1 + max(x for xs in ts for x in xs)
        dims = [int(choices[int(rng.randint(len(choices)))]) for _ in range(n_inds)]
        output = tuple(sorted(int(x) for x in rng.choice(n_inds, size=int(rng.randint(0, 3)), replace=False)))
    else:
        ts, dims, output = syn.random_hyper_tn(n, n + int(rng.randint(0, n // 2 + 1)), k=3, n_output=int(rng.randint(0, 3)),
                                               seed=seed, dims_choices=choices)
    ts = tuple(tuple(int(x) for x in xs) for xs in ts)
    held = sorted({x for xs in ts for x in xs})
    path = _random_path(len(ts), seed) if rng.randint(2) else _greedy_path(ts)
    slices = tuple(sorted(int(x) for x in rng.choice(held, size=min(len(held), int(rng.randint(1, 4))), replace=False)))
    total = math.prod(dims[x] for x in slices)
    slice_range = None
    if total > 3 and rng.randint(4) == 0:
        slice_range = (1 + int(rng.randint(2)), total - int(rng.randint(2)))
    case = Case(f"seed-{seed}", ts, tuple((x, int(dims[x])) for x in held), tuple(output),
                tuple((int(a), int(b)) for a, b in path), slices,
                np.dtype(dtype if dtype is not None else DTYPES[seed % 4]).name, fill or FILLS[(seed // 4) % 2], slice_range)
    return None if caps(case) else case


def two_branches(name, form, sizes, H, dtype, fill, inner=2, stored=False):
    """A network written by hand for a step with both operands in the arena: two branches, Z1 = T0 T1 with axes
    ([h], i0, i1) and Z2 = T2 T3 with axes ([h], j0, j1), and the step Z1 Z2 in the memory order `form` = (form_a, form_b)
    with sizes (M, N, K) and a batch axis h of dimension H (1: none).  Sliced over u (3, held by T0 and T2, summed), w (2,
    held by T1 and T3, summed) and p (2, an axis of T0 and of the output: blocks that are revisited).  `stored`: a fifth
    tensor takes the step's result from the output to the arena."""
    M, N, K = sizes
    fa, fb = form
    i0, i1 = ("k", "m") if fa else ("m", "k")
    j0, j1 = ("n", "k") if fb else ("k", "n")
    h = ("h",) if H > 1 else ()
    ts = [("p", "u") + h + (i0, "c"), ("w", "c", i1), ("u",) + h + (j0, "e"), ("w", "e", j1)]
    dims = dict(p=2, u=3, w=2, h=H, m=M, n=N, k=K, c=inner, e=inner)
    path = [(0, 1), (0, 1), (0, 1)]
    output = ("p",) + h + ("m", "n")
    if stored:
        ts.append(("n", "z"))
        dims["z"] = 3
        path = [(0, 1), (0, 1), (1, 2), (0, 1)]  # (T4 stays first: it is the first operand of the last step)
        output = ("p",) + h + ("m", "z")
    if H == 1:
        del dims["h"]
    return Case(name, tuple(ts), tuple(dims.items()), output, tuple(path), ("p", "u", "w"), np.dtype(dtype).name, fill)


def fill(case, storage=None):
    """The leaves of a case in its dtype; with `storage` every part rounded to that type (`contraction.round_to_storage`):
    device and reference then start from equal values."""
    dtype, seed = np.dtype(case.dtype), zlib.crc32(case.name.encode()) % (1 << 31)
    if case.fill == "normal":
        out = _arrays(case.ts_inds, case.dim, dtype, seed)
    else:
        rng = np.random.RandomState(seed)
        out = []
        for shape in case.shapes():
            a = rng.uniform(0.5, 1.5, shape)
            if dtype.kind == "c":
                a = a + 1j * rng.uniform(0.5, 1.5, shape)
            out.append(a.astype(dtype))
    return out if storage is None else [ctr.round_to_storage(a, storage) for a in out]


def reference(case, p, arrays):
    """(the sum over the plan's assignments, the same of the moduli), float64 / complex128, axes in p.inds order:
    numpy's einsum over the whole network, unsliced; with a slice_range that is not the whole, over each assignment of
    it."""
    sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in case.ts_inds for x in xs))}
    wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in arrays]
    out = []
    whole = p.slice_range == (0, p.n_slices)
    # (pairwise in the order of the case's own path: numpy's own choice of an order can cost far more than the network)
    order = ["einsum_path"] + [tuple(sorted(step)) for step in case.path]
    for ws in (wide, [np.abs(w) for w in wide]):
        if whole:
            args = [q for w, xs in zip(ws, case.ts_inds) for q in (w, [sym[x] for x in xs])]
            out.append(np.einsum(*args, [sym[x] for x in p.inds], optimize=order))
            continue
        total = np.zeros(p.shape, ws[0].dtype)
        rest = [x for x in p.inds if x not in p.slice_inds]
        for sid in range(*p.slice_range):
            at = {x: (sid // math.prod(p.slice_dims[s + 1:])) % p.slice_dims[s] for s, x in enumerate(p.slice_inds)}
            args = [q for w, xs in zip(ws, case.ts_inds)
                    for q in (w[tuple(at.get(x, slice(None)) for x in xs)], [sym[x] for x in xs if x not in at])]
            total[tuple(at.get(x, slice(None)) for x in p.inds)] += np.einsum(*args, [sym[x] for x in rest], optimize=order)
        out.append(total)
    return tuple(out)


def plain_bound(case, p, mag):
    """(c kt + 2) u mag: the first-order bound of tests/test_gpu_contract_path.py over all the steps of the plan."""
    dtype = np.dtype(case.dtype)
    return ((2 if dtype.kind == "c" else 1) * kt(p) + 2) * (float(np.finfo(dtype).eps) / 2) * mag


def split_bound(case, p, mag):
    """compute="bf16x3": the one-step bound of tests/test_gpu_contract_split.py, its 2^-14 once per tiled step of the
    longest chain that feeds the output."""
    c = 2 if np.dtype(case.dtype).kind == "c" else 1
    return (tiled_depth(case, p) * 2.0 ** -14 + (2 * c * 3 * kt(p) + 2) * 2.0 ** -24) * mag


def storage_bound(case, p, mag, storage):
    """storage=: a rounding to the storage type per stored intermediate (every step but the last; a permuted copy does
    not round again), and the float32 accumulation bound of tests/test_gpu_contract_half.py."""
    c = 2 if np.dtype(case.dtype).kind == "c" else 1
    return ((len(p.steps) - 1) * U_STORAGE[storage] + (2 * c * kt(p) + 2) * 2.0 ** -24) * mag


# networks written by hand (two_branches): what the generator does not find under the caps -- the tiled class with a
# batch axis, and in the memory order (1, 1), from two arena operands -- and such a step stored to the arena
HAND = {
    "hand-tiled-11-h2": dict(form=(1, 1), sizes=(64, 65, 33), H=2),
    "hand-tiled-01-h2-stored": dict(form=(0, 1), sizes=(65, 64, 40), H=2, stored=True),
    "hand-tiled-11-h3-stored": dict(form=(1, 1), sizes=(64, 64, 48), H=3, stored=True),
    "hand-dot-10-h3-stored": dict(form=(1, 0), sizes=(4, 5, 520), H=3, stored=True),
    "hand-stream-11-h2-stored": dict(form=(1, 1), sizes=(7, 9, 11), H=2, stored=True),
}
# (a seed of `generate` or a name of HAND, dtype, fill): the dtypes rotate so that every item of REQUIRED is reached in a
# real and in a complex type, the tiled and dot items in a single-precision type too; the fills alternate
TABLE = (
    (520, "float32", "uniform"),
    ("hand-tiled-11-h2", "complex64", "normal"),
    (2793, "complex128", "uniform"),
    ("hand-tiled-01-h2-stored", "float32", "normal"),
    (959, "float32", "uniform"),
    (259, "complex128", "normal"),
    (1376, "float64", "uniform"),
    (2416, "complex128", "normal"),
    (747, "complex64", "uniform"),
    (62, "complex128", "normal"),
    (673, "float64", "uniform"),
    ("hand-tiled-11-h3-stored", "float64", "normal"),
    (1025, "complex64", "uniform"),
    (369, "float32", "normal"),
    (358, "float64", "uniform"),
    (1889, "complex128", "normal"),
    (1309, "float32", "uniform"),
    (235, "float64", "normal"),
    (1079, "complex64", "uniform"),
    (556, "complex128", "normal"),
    (2268, "float32", "uniform"),
    (2036, "float64", "normal"),
    (1302, "complex64", "uniform"),
    (256, "complex128", "normal"),
    ("hand-stream-11-h2-stored", "float32", "uniform"),
    (1318, "float64", "normal"),
    (2610, "complex64", "uniform"),
    ("hand-dot-10-h3-stored", "float32", "normal"),
)


def make(key, dtype, fill):
    if isinstance(key, str):
        return two_branches(key, dtype=dtype, fill=fill, **HAND[key])
    return generate(key, dtype, fill)


CASES = tuple(make(*row) for row in TABLE)
IDS = tuple(f"{c.name}-{c.dtype}" for c in CASES)
