"""The case table of the mode tests (tests/mode_cases.py) on the CPU: every case plans in every mode the device test
runs it in, stays within the caps, and the table reaches every item of `mode_cases.REQUIRED` -- asserted item by item, so
that an edit of the table cannot lose one silently.

The bounds of tests/test_gpu_contract_modes.py are shown here to be bounds that a correct contraction meets on these
inputs, without a device: the plan's tables are replayed by the numpy interpreter of tests/test_contraction_plan.py in
the case's own dtype and held to the plain bound against numpy's einsum of the whole network in float64 / complex128; and
a host contraction that rounds every intermediate to the storage type (`host_contract` of
tests/test_gpu_contract_half_network.py) is held to the storage bounds, with every stored tensor inside the range in which
the storage type is a normal number."""
import math

import numpy as np
import pytest

from tests import mode_cases as mc
from tests.test_contraction_plan import _interpret
from tests.test_gpu_contract_half_network import host_contract
from tnco_amd import contraction as ctr

SINGLE_CASES = [c for c in mc.CASES if np.dtype(c.dtype) in mc.SINGLES]
SINGLE_IDS = [f"{c.name}-{c.dtype}" for c in SINGLE_CASES]


def tables(p):
    return [np.asarray(a).tobytes() for a in (p.perms, p.leaf_sl, p.leaf_numel)] + [p.steps[:, :14].tobytes()]


def modes_of(case):
    """The keyword sets the device test runs the case with."""
    out = [dict()] + [dict(slice_batch=b) for b in mc.BATCHES] + [dict(path_kernel=g) for g in mc.GROUPS]
    if np.dtype(case.dtype) in mc.SINGLES:
        halves = [dict(compute="bf16x3")] + [dict(m) for m in mc.STORAGE_MODES]
        out += halves + [dict(m, slice_batch=mc.HALF_BATCH) for m in halves]
    return out


def test_the_table_is_a_fixed_list_of_distinct_cases():
    assert 24 <= len(mc.CASES) <= 32 and len(set(mc.IDS)) == len(mc.IDS)
    assert len({(c.ts_inds, c.dims, c.path, c.slices) for c in mc.CASES}) == len(mc.CASES)
    per_dtype = {np.dtype(d).name: sum(c.dtype == np.dtype(d).name for c in mc.CASES) for d in mc.DTYPES}
    assert min(per_dtype.values()) >= len(mc.CASES) // 4 - 1, per_dtype
    assert [c.fill for c in mc.CASES] == [mc.FILLS[k % 2] for k in range(len(mc.CASES))]
    for (key, dtype, fill), case in zip(mc.TABLE, mc.CASES):  # the generator is deterministic
        assert mc.make(key, dtype, fill) == case
    assert mc.generate(520) == mc.generate(520) and mc.generate(520).dtype == np.dtype(mc.DTYPES[0]).name


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_a_case_is_within_the_caps(case):
    assert mc.caps(case) == []
    p = case.plan()
    assert 4 <= len(case.ts_inds) <= 10 and int(p.leaf_numel.max()) <= 1 << 18
    assert 2 <= p.slice_range[1] - p.slice_range[0] <= 64
    assert p.macs <= 5 * 10 ** 7 and p.arena_elems <= 1 << 22
    for op in p.ops:
        assert op["H"] * op["M"] * op["N"] * op["K"] <= ctr.MAX_PATH_STEP_MACS
    assert len(p.steps) == len(case.ts_inds) - 1  # (the path leaves one tensor)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_a_case_plans_in_every_mode_it_is_run_in(case):
    base = case.plan()
    n = case.n_assignments()
    assert base.slice_range[1] - base.slice_range[0] == n
    for mode in modes_of(case):
        p = case.plan(**mode)
        assert tables(p) == tables(base) and p.inds == base.inds and p.macs == base.macs, mode
        assert p.slice_batch == (min(mode["slice_batch"], n) if "slice_batch" in mode else None), mode
        assert p.path_kernel == (min(mode["path_kernel"], n) if "path_kernel" in mode else None), mode
        if "scaling" in mode:  # a staging buffer for every stored step, none for the last
            assert (p.stage_refs[:-1] >= 0).all() and p.stage_refs[-1] == -1, mode
    assert sum(mc.launches_per_assignment(base)) == len(base.steps) + len(set(base.perms[:, 6].tolist()))


def _reached(cases):
    got = {}
    for c in cases:
        for item in mc.coverage(c, c.plan()):
            got.setdefault(item, []).append(f"{c.name}-{c.dtype}")
    return got


@pytest.mark.parametrize("item", mc.REQUIRED)
def test_the_table_reaches(item):
    real = _reached(c for c in mc.CASES if np.dtype(c.dtype).kind == "f")
    cplx = _reached(c for c in mc.CASES if np.dtype(c.dtype).kind == "c")
    assert item in real, f"no case of a real dtype reaches '{item}'"
    assert item in cplx, f"no case of a complex dtype reaches '{item}'"
    if item in mc.REQUIRED_SINGLE:
        assert item in _reached(SINGLE_CASES), f"no float32 / complex64 case reaches '{item}' (bf16x3, storage modes)"


def test_the_table_goes_beyond_the_chains():
    """More step signatures than the three-tensor chains of tests/path_cases.py reach, dims other than 2, more than one
    arena-to-arena permute, and an intermediate that waits in the arena while another branch is contracted."""
    from tests import path_cases as pc
    chains = set()
    for chain in pc.CASES:
        chains |= set(mc.signature(ctr.plan(pc.PATH, chain.ts, chain.shapes(), chain.output, slices=pc.SLICES)))
    ours = set().union(*(mc.signature(c.plan()) for c in mc.CASES))
    assert len(ours) >= 26 > len(chains), (len(ours), len(chains))
    assert {d for c in mc.CASES for _, d in c.dims} >= {1, 2, 3, 4, 5, 8, 16, 32}
    assert max(mc.arena_permutes(c.plan()) for c in mc.CASES) >= 3
    waits = 0
    for c in mc.CASES:  # a step whose result is not an operand of the next step
        st = c.plan().steps
        waits += any(int(st[k, 9]) not in (int(st[k + 1, 1]), int(st[k + 1, 5])) and st[k, 8] == ctr.ARENA
                     for k in range(len(st) - 1))
    assert waits >= 5


_REFERENCE = {}


def reference_of(case, storage=None):
    """(plan, leaves, reference, magnitude) of a case, computed once."""
    key = (mc.CASES.index(case), storage)
    if key not in _REFERENCE:
        p, arrays = case.plan(), mc.fill(case, storage)
        _REFERENCE[key] = (p, arrays) + mc.reference(case, p, arrays)
    return _REFERENCE[key]


@pytest.mark.parametrize("case", mc.CASES, ids=mc.IDS)
def test_the_replay_in_the_case_dtype_is_inside_the_plain_bound(case):
    p, arrays, ref, mag = reference_of(case)
    got = _interpret(p, arrays)
    assert got.dtype == np.dtype(case.dtype) and got.shape == ref.shape == p.shape
    err, bound = np.abs(got.astype(ref.dtype) - ref), mc.plain_bound(case, p, mag)
    print(f"{case.name} {case.dtype}: replay, largest error / bound {float((err / bound).max()):.4f} (kt {mc.kt(p)})")
    assert np.isfinite(got).all() and (bound > 0).all() and (err <= bound).all()


def _emulate(case, p, arrays, store):
    """The sliced run on the host in complex128, every intermediate passed through `store`; every assignment's result
    added, or placed for a sliced index that the result holds, unrounded."""
    total = np.zeros(p.shape, np.complex128)
    for sid in range(*p.slice_range):
        at = {x: (sid // math.prod(p.slice_dims[s + 1:])) % p.slice_dims[s] for s, x in enumerate(p.slice_inds)}
        part = [a[tuple(at.get(x, slice(None)) for x in xs)] for xs, a in zip(case.ts_inds, arrays)]
        part_inds = [tuple(x for x in xs if x not in at) for xs in case.ts_inds]
        z, r = host_contract(case.path, part_inds, part, [x for x in case.output_inds if x not in at], store)
        rest = [x for x in p.inds if x not in at]
        total[tuple(at.get(x, slice(None)) for x in p.inds)] += r.transpose([z.index(x) for x in rest])
    return total


def _nonzero_parts(a):
    a = np.asarray(a)
    x = np.abs(np.concatenate([a.real.ravel(), a.imag.ravel()])) if np.iscomplexobj(a) else np.abs(a.ravel())
    return x[x > 0]


@pytest.mark.parametrize("mode", mc.STORAGE_MODES, ids=lambda m: m["storage"] + ("-scaled" if "scaling" in m else ""))
@pytest.mark.parametrize("case", SINGLE_CASES, ids=SINGLE_IDS)
def test_a_host_contraction_that_rounds_as_the_storage_mode_is_inside_its_bound(case, mode):
    storage, dtype = mode["storage"], np.dtype(case.dtype)
    p, arrays, ref, mag = reference_of(case, storage)
    stored = []

    def store(a):
        narrow = (a if dtype.kind == "c" else a.real).astype(dtype)
        with np.errstate(over="ignore"):
            kept = ctr.scale_to_storage(narrow, storage)[0] if "scaling" in mode else \
                ctr._from_storage_bits(ctr._storage_bits(narrow, storage, check=False), storage, narrow)
        stored.append(kept)
        return kept.astype(np.complex128)

    got = _emulate(case, p, arrays, store)
    got = got if dtype.kind == "c" else got.real
    err, bound = np.abs(got - ref), mc.storage_bound(case, p, mag, storage)
    print(f"{case.name} {case.dtype} {mode}: host emulation, largest error / bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    assert len(stored) == (len(p.steps) - 1) * case.n_assignments()
    every = [x for x in (_nonzero_parts(a) for a in list(arrays) + stored) if x.size]
    if "scaling" in mode:
        # no part more than 2^24 below its tensor's largest: scaled, every part is a normal float16
        for x in every:
            assert x.min() * 2.0 ** 24 >= x.max(), (float(x.min()), float(x.max()))
    elif case.fill == "uniform":
        tiny, huge = float(np.finfo(np.float32).tiny), 2.0 ** 127
        assert all(tiny <= x.min() and x.max() < huge for x in every)
