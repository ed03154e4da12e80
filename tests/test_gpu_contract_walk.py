"""The walkers on the device (csrc/contract_walk.h): `Contractor.bind_versions`, `run_walkers`, `choose`, `Walkers`.

Indexed leaves.  The oracle is `run_many` of the explicit stacks on the same Contractor -- stack[i] = versions[bits[i, q]]
(tests/walk_cases.py, select) -- and the outputs that `run_walkers` left on the device must be byte for byte its array.
The chains are those of tests/path_cases.py and tests/batch_cases.py; the leaves that are not indexed are those of set 0,
bound; a leaf's two versions are those of sets 0 and 1.

Choice.  The plan is out[m] = sum X[m, b1 .. b10] e1[b1] .. e10[b10] with ten indexed one-hot leaves: walker i, whose ten
bits spell i, meets the pair (X[0, i], X[1, i]), and a product with a one-hot vector is exact, so the test designs the
1024 pairs.  Bits and dead flags must be those of the model (tests/walk_cases.py) bit for bit.  A part that is not finite
cannot be confined to one pair: it meets the 0 of the other walkers' one-hot vectors and 0 x inf is NaN, so the runs with
an inf part and with a NaN part are runs of their own in which the model, too, has every walker dead.

Permute and the ABI's refusals: against the model, and text by text with the objects unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as bc
from tests import many_cases as mc
from tests import path_cases as pc
from tests import walk_cases as wc

pytestmark = pytest.mark.gpu

DTYPE_IDS = [np.dtype(d).name for d in mc.DTYPES]
N_QUBITS = 4
INDEXED = ({1: 2}, {0: 3, 2: 0}, {0: 1, 1: 3, 2: 0})  # {leaf: qubit}: one, two and all leaves indexed, by different qubits


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits_of(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def contractor(ctr, chain, dtype, **kw):
    kw.setdefault("slices", mc.SLICES)
    kw.setdefault("path_kernel", 5)
    return ctr.Contractor(mc.PATH, chain.ts, chain.shapes(), chain.output, dtype=dtype, **kw)


def random_bits(R, seed, n_qubits=N_QUBITS):
    return np.random.RandomState(seed).randint(0, 2, (R, n_qubits)).astype(np.uint8)


def check_walk(c, w, versions, leaf_qubit, bits, group, what):
    """run_walkers over `bits` against run_many of the explicit stacks; returns the outputs."""
    p = c.plan
    R, A = len(bits), p.slice_range[1] - p.slice_range[0]
    r = c.run_walkers(w, leaf_qubit, group=group)
    got = c.walker_outputs(w)
    launches = -(-R * A // min(group, R * A))
    assert r.array is None and r.inds == ("set",) + tuple(p.inds) and r.sets == R and r.group == min(group, R * A), what
    assert r.path_launches == (launches, launches) and r.launches == 2 * launches and r.macs == R * p.macs, what
    assert r.peak_device_bytes < mc.MEMORY_CAP, what
    assert (w.bits == bits).all(), what  # (a run does not touch the bits)
    want = c.run_many({t: wc.select(versions[t], bits, q) for t, q in leaf_qubit.items()}, group=group)
    assert got.shape == want.array.shape and got.dtype == p.dtype and np.isfinite(got).all(), what
    assert np.array_equal(bits_of(got), bits_of(want.array)), f"{what}: differs from run_many of the explicit stacks"
    assert (r.macs, r.launches, r.path_launches) == (want.macs, want.launches, want.path_launches), what
    # the memory, term by term: the versions and the walkers' table are part of many_bytes, and of the library's count
    from tnco_amd import _lib
    stats = np.zeros(4, np.int64)
    L, h = c._handle()
    _lib.check(L.tnco_hip_contract_stats(h, stats.ctypes.data_as(C.c_void_p)))
    assert want.peak_device_bytes == c.many_bytes(R, group=group) == int(stats[2]) >= r.peak_device_bytes, what
    return got


# ---- indexed leaves ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DTYPE_IDS)
def test_indexed_leaves_against_run_many_of_the_explicit_stacks(ctr, dtype):
    chain = pc.SMALL
    sets = mc.fill_sets(chain, dtype, 2, seed=91)
    versions = {t: mc.stack(sets, t) for t in range(3)}
    with contractor(ctr, chain, dtype) as c:
        c.bind({t: sets[0][t] for t in range(3)})
        c.bind_versions(versions)
        for R in (1, 5, 13):
            bits = random_bits(R, seed=R)
            with ctr.Walkers(R, N_QUBITS) as w:
                assert not w.bits.any() and not w.dead.any() and w.bits.shape == (R, N_QUBITS) and w.bits.dtype == np.uint8
                w.write(bits)
                for leaf_qubit in INDEXED:
                    for group in (1, 5, 1024):
                        what = f"{np.dtype(dtype).name} R = {R} {leaf_qubit} group = {group}"
                        first = check_walk(c, w, versions, leaf_qubit, bits, group, what)
                        # again, the versions not loaded anew (a run_many lay between): the same bytes
                        c.run_walkers(w, leaf_qubit, group=group)
                        assert np.array_equal(bits_of(c.walker_outputs(w)), bits_of(first)), f"{what}: a second run"
                # other bits: the result follows them
                flipped = 1 - bits
                w.write(flipped)
                got = check_walk(c, w, versions, INDEXED[2], flipped, 5, f"{np.dtype(dtype).name} R = {R} flipped")
                assert not np.array_equal(bits_of(got), bits_of(first))
                w.reset()
                assert not w.bits.any()
                check_walk(c, w, versions, INDEXED[2], np.zeros_like(bits), 1024, f"{np.dtype(dtype).name} R = {R} reset")
        # many qubits: the first, the last and one between index the leaves (a bit lies qubit x walkers bytes into the table)
        with ctr.Walkers(13, 70) as w:
            bits = random_bits(13, seed=70, n_qubits=70)
            w.write(bits)
            assert len({tuple(row) for row in bits[:, [69, 0, 63]]}) > 4
            check_walk(c, w, versions, {0: 69, 1: 0, 2: 63}, bits, 5, f"{np.dtype(dtype).name} 70 qubits")
        # every walker with all bits 0 reads version 0 of every leaf: the bound set
        one = c.run()
        with ctr.Walkers(3, N_QUBITS) as w:
            c.run_walkers(w, INDEXED[2])
            got = c.walker_outputs(w)
            assert all(np.array_equal(bits_of(got[i]), bits_of(one.array)) for i in range(3))
            # no leaf indexed: no output depends on the walker, one set is run and serves them all
            w.write(random_bits(3, seed=1))
            r = c.run_walkers(w, {}, group=5)
            assert (r.sets, r.group, r.macs, r.path_launches) == (1, 5, one.macs, (3, 3))
            got = c.walker_outputs(w)
            assert got.shape == (3,) + one.array.shape and all(np.array_equal(bits_of(got[i]), bits_of(one.array)) for i in range(3))


@pytest.mark.parametrize("slice_range", [None, (1, 11)], ids=["whole", "range-1-11"])
@pytest.mark.parametrize("variant", ["base", "summed", "placed"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_three_blocks_one_block_and_twelve_blocks(ctr, dtype, variant, slice_range):
    chain = bc.Chain(f"small-{variant}", bc.SMALL.sizes, bc.SMALL.classes, variant)
    R = 5
    sets = mc.fill_sets(chain, dtype, 2, seed=92)
    versions = {t: mc.stack(sets, t) for t in range(3)}
    bits = random_bits(R, seed=7)
    with contractor(ctr, chain, dtype, slice_range=slice_range) as c, ctr.Walkers(R, N_QUBITS) as w:
        c.bind({t: sets[0][t] for t in range(3)})
        c.bind_versions({1: versions[1], 2: versions[2]})
        w.write(bits)
        for group in (4, 5, 1024):
            got = check_walk(c, w, versions, {1: 0, 2: 3}, bits, group, f"{chain.name} {np.dtype(dtype).name} {slice_range} group = {group}")
        if slice_range is not None and variant == "placed":  # assignments 0 and 11 are not run: their blocks stay zero
            p = c.plan
            a = got.transpose([0] + [1 + p.inds.index(x) for x in chain.output]).reshape(R, 12, -1)
            assert not a[:, 0].any() and not a[:, 11].any() and (a[:, 1:11] != 0).all()


def assert_walkers_equal_runs(c, got, versions, leaf_qubit, bits, what):
    """Output i of a run_walkers with every leaf indexed against run() over the versions that walker i's bits select (the
    leaves are bound no longer afterwards)."""
    assert sorted(leaf_qubit) == [0, 1, 2]
    for i in range(len(bits)):
        one = c.run([versions[t][bits[i, leaf_qubit[t]]] for t in range(3)])
        assert np.array_equal(bits_of(got[i]), bits_of(one.array)), f"{what}: walker {i} differs from run()"


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
@pytest.mark.parametrize("chain", [pc.DOT_TAIL, pc.STREAM_TRIPS], ids=[pc.DOT_TAIL.name, pc.STREAM_TRIPS.name])
def test_a_dot_step_with_a_k_tail_and_a_second_trip_of_the_element_loop(ctr, chain, dtype):
    """The paths of ct_path_step that the small chain does not reach: the dot class with 5 outputs (a second trip with one
    quarter of the block at work) and K = 515 (a k tail), and 1200 outputs of one lane each (the 1024 lanes go round twice)."""
    R, group = 3, 5
    sets = mc.fill_sets(chain, dtype, 2, seed=94)
    versions = {t: mc.stack(sets, t) for t in range(3)}
    bits = random_bits(R, seed=12)
    assert len({tuple(row[[1, 3, 0]]) for row in bits}) == R  # (the walkers read different leaves)
    what = f"{chain.name} {np.dtype(dtype).name}"
    with contractor(ctr, chain, dtype) as c, ctr.Walkers(R, N_QUBITS) as w:
        c.bind({t: sets[0][t] for t in range(3)})
        c.bind_versions(versions)
        w.write(bits)
        got = check_walk(c, w, versions, INDEXED[2], bits, group, what)
        assert_walkers_equal_runs(c, got, versions, INDEXED[2], bits, what)


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_three_walkers_of_three_assignments_in_groups_of_two_and_four(ctr, dtype):
    """Every launch but the first starts inside a walker, and both groups end inside one."""
    chain, R = pc.SMALL, 3
    sets = mc.fill_sets(chain, dtype, 2, seed=95)
    versions = {t: mc.stack(sets, t) for t in range(3)}
    bits = random_bits(R, seed=12)
    with contractor(ctr, chain, dtype, slice_range=(3, 6)) as c, ctr.Walkers(R, N_QUBITS) as w:
        c.bind({t: sets[0][t] for t in range(3)})
        c.bind_versions(versions)
        w.write(bits)
        got = {}
        for group in (2, 4):
            what = f"{np.dtype(dtype).name} A = 3 R = 3 group = {group}"
            got[group] = check_walk(c, w, versions, INDEXED[2], bits, group, what)
            assert c.run_walkers(w, INDEXED[2], group=group).path_launches == ((5, 5) if group == 2 else (3, 3)), what
        for group in (2, 4):
            assert_walkers_equal_runs(c, got[group], versions, INDEXED[2], bits, f"group = {group}")


# ---- the choice ------------------------------------------------------------------------------------------------------------

N_PAIRS, N_INDEX = 1024, 10
CHOICE_TS = [(f"b{j}",) for j in range(N_INDEX)] + [("m",) + tuple(f"b{j}" for j in range(N_INDEX))]
CHOICE_PATH = [(0, j) for j in range(N_INDEX, 0, -1)]  # X with e1, the result with e2, ...
FLAG = N_INDEX  # the qubit that the choice writes: none of the ten that index the leaves


def designed_pairs(dtype, seed, step):
    """X [2, 1024] of `dtype`: the pairs that walker i = 0 .. 1023 meets (module docstring)."""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    rng = np.random.RandomState(5)
    X = rng.normal(size=(2, N_PAIRS)).astype(dtype)
    if dtype.kind == "c":
        X = (X + 1j * rng.normal(size=(2, N_PAIRS))).astype(dtype)
    tiny = float(np.finfo(real).tiny)
    special = [(1, 0), (0, 1), (0, 0), (tiny / 4, tiny / 2), (tiny / 2, tiny / 4), (1e30, 1e30), (3e30, 1e29), (3e-30, 4e-30), (-0.0, 0.0),
               (1e30, 1e-30)]
    for k, (x, y) in enumerate(special):
        X[0, k], X[1, k] = x, y
    if dtype.kind == "c":  # the same in the imaginary parts, and mixed
        for k, (x, y) in enumerate(special):
            X[0, 16 + k], X[1, 16 + k] = 1j * x, 1j * y
            X[0, 32 + k], X[1, 32 + k] = x * (1 + 1j), y * (1 - 1j)
    # pairs just either side of u s = p1 for the walker's own u: a0 = 1 and two neighbouring values of a1, the lower with
    # the bit 0 (even walkers), the upper with the bit 1 (odd walkers), bisected by the model over the bit patterns of the
    # positive numbers (s = 1 + p1 is rounded too, so the bit need not be monotonic an ulp at a time: the bisection keeps a
    # 0 below and a 1 above until they are neighbours)
    walkers = np.arange(N_PAIRS // 2, N_PAIRS)
    u = wc.uniforms(seed, walkers, step)
    word = np.int32 if real is np.float32 else np.int64
    bit_of = lambda pattern: wc.choose(np.ones(len(u), real), pattern.view(real), u)[0]  # noqa: E731
    lo, hi = np.zeros(len(u), real).view(word), np.full(len(u), 1e10, real).view(word)
    assert not bit_of(lo).any() and bit_of(hi).all()
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        up = bit_of(mid) == 1
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    assert (hi - lo == 1).all() and not bit_of(lo).any() and bit_of(hi).all()
    a1 = np.where(walkers % 2 == 1, hi, lo).view(real)
    X[0, walkers] = 1
    X[1, walkers] = a1 * (1j if dtype.kind == "c" else 1) ** (walkers % 4 // 2)  # (complex: every other pair in the imaginary part)
    return X


def index_bits():
    """Walker i's ten bits spell i, the first qubit the most significant; the flag qubit is 0."""
    i = np.arange(N_PAIRS)
    bits = np.zeros((N_PAIRS, N_INDEX + 1), np.uint8)
    for j in range(N_INDEX):
        bits[:, j] = (i >> (N_INDEX - 1 - j)) & 1
    return bits


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128, np.float32], ids=["complex64", "complex128", "float32"])
def test_the_choice_against_the_model_bit_for_bit(ctr, dtype):
    seed, walkers = 0x1234_5678_9ABC_DEF0, np.arange(N_PAIRS)
    shapes = [(2,)] * N_INDEX + [(2,) * (N_INDEX + 1)]
    leaf_qubit = {j: j for j in range(N_INDEX)}
    one_hot = np.eye(2, dtype=dtype)
    with ctr.Contractor(CHOICE_PATH, CHOICE_TS, shapes, ("m",), dtype=dtype, path_kernel=1024) as c:
        c.bind_versions({j: one_hot for j in range(N_INDEX)})

        def run(w, X, step):
            c.bind({N_INDEX: X.reshape(shapes[-1])})
            w.reset()
            w.write(index_bits())
            c.run_walkers(w, leaf_qubit)
            out = c.walker_outputs(w)
            c.run_walkers(w, leaf_qubit)
            c.choose(w, FLAG, step)
            return out, w.bits, w.dead

        drawn = {}
        for this_seed, step in ((seed, 0), (seed, 5), (seed + 1, 0), (seed + (1 << 32), 0)):
            X = designed_pairs(dtype, this_seed, step)
            finite = np.isfinite(X).all()
            assert finite
            with ctr.Walkers(N_PAIRS, N_INDEX + 1, seed=this_seed) as w:
                out, bits, dead = run(w, X, step)
                # the walker meets its pair, unchanged: subnormal parts too
                assert np.array_equal(bits_of(out + 0), bits_of(X.T + 0)), "a product with a one-hot vector is exact"
                want_bits, want_dead = wc.choose(X[0], X[1], wc.uniforms(this_seed, walkers, step))
                assert np.array_equal(bits[:, FLAG], want_bits) and np.array_equal(dead, want_dead), (this_seed, step)
                assert np.array_equal(bits[:, :N_INDEX], index_bits()[:, :N_INDEX])  # (only the flag qubit is written)
                assert want_dead.sum() >= 1 and want_dead[2] and 300 < want_bits.sum() < 724
                half = walkers[N_PAIRS // 2:]
                assert (want_bits[half] == half % 2).all()  # (the pairs either side of the threshold)
                drawn[(this_seed, step)] = wc.choose(designed_pairs(dtype, seed, 0)[0], designed_pairs(dtype, seed, 0)[1],
                                                     wc.uniforms(this_seed, walkers, step))[0]
                # dead flags stay until reset; a second choice of live pairs does not clear them
                c.bind({N_INDEX: np.ones(shapes[-1], dtype)})
                c.run_walkers(w, leaf_qubit)
                c.choose(w, FLAG, step)
                assert np.array_equal(w.dead, want_dead)
                if (this_seed, step) == (seed, 0):  # an inf part, a NaN part: 0 x inf is NaN in every other walker's sum
                    for bad in (np.inf, np.nan):
                        Y = X.copy()
                        Y[1, 700] = bad
                        _, bits, dead = run(w, Y, step)
                        assert dead.all() and not bits[:, FLAG].any(), bad
        # the same pairs under another step or seed: other draws, as the model has them
        base = drawn[(seed, 0)]
        assert all((drawn[k] != base).sum() > 100 for k in drawn if k != (seed, 0))


# ---- permute ---------------------------------------------------------------------------------------------------------------

def test_permute_cnot_swap_and_a_cycle(ctr):
    R, n = 1000, 5
    bits = np.random.RandomState(3).randint(0, 2, (R, n)).astype(np.uint8)
    cycle = [(v << 1 | v >> 2) & 7 for v in range(8)]
    with ctr.Walkers(R, n) as w:
        w.write(bits)
        for qubits, table in (((3, 1), (0, 1, 3, 2)), ((0, 4), (0, 2, 1, 3)), ((2, 0, 3), cycle), ((4,), (1, 0))):
            w.permute(qubits, table)
            bits = wc.permute(bits, qubits, table)
            assert np.array_equal(w.bits, bits), qubits
        assert not w.dead.any()
        full = np.random.RandomState(4).permutation(32).tolist()
        w.permute((0, 1, 2, 3, 4), full)
        assert np.array_equal(w.bits, wc.permute(bits, (0, 1, 2, 3, 4), full))
    with ctr.Walkers(70, 8) as w:  # k = 8: the whole table of 256 entries
        bits = np.random.RandomState(5).randint(0, 2, (70, 8)).astype(np.uint8)
        table = np.random.RandomState(6).permutation(256).tolist()
        w.write(bits)
        w.permute(tuple(range(8)), table)
        assert np.array_equal(w.bits, wc.permute(bits, tuple(range(8)), table))


# ---- the ABI's refusals ----------------------------------------------------------------------------------------------------

def test_abi_refusals_leave_the_objects_unchanged(ctr):
    from tnco_amd import _lib
    chain, dtype, R = pc.SMALL, np.float32, 5
    sets = mc.fill_sets(chain, dtype, 2, seed=93)
    versions = {t: mc.stack(sets, t) for t in range(3)}
    bits = random_bits(R, seed=9)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731

    def refused(rc, text, code=_lib.EINVAL):
        assert rc == code and L.tnco_hip_last_error().decode() == text, (rc, L.tnco_hip_last_error().decode())

    with contractor(ctr, chain, dtype) as c, ctr.Walkers(R, N_QUBITS) as w, contractor(ctr, chain, dtype, path_kernel=None) as plain:
        c.bind({0: sets[0][0], 1: sets[0][1]})
        c.bind_versions({1: versions[1]})
        w.write(bits)
        L, h = c._handle()
        wh = w._handle()
        two, n2 = np.ascontiguousarray(versions[2]), i64(versions[2].size)
        # load_leaf_versions
        refused(L.tnco_hip_contract_load_leaf_versions(None, 2, 2, ptr(two), 0, 0, 1, ptr(n2), None), "null argument.")
        refused(L.tnco_hip_contract_load_leaf_versions(h, 3, 2, ptr(two), 0, 0, 1, ptr(n2), None), "'leaf' is not a leaf of the plan.")
        for n in (1, 3, 0):
            refused(L.tnco_hip_contract_load_leaf_versions(h, 2, n, ptr(two), 0, 0, 1, ptr(n2), None), "'n_versions' must be 2.")
        refused(L.tnco_hip_contract_load_leaf_versions(plain._handle()[1], 2, 2, ptr(two), 0, 0, 1, ptr(n2), None),
                "leaf sets need a path kernel: call tnco_hip_contract_set_path_kernel first.")
        refused(L.tnco_hip_contract_load_leaf_versions(h, 2, 2, ptr(two), 2, 0, 1, ptr(n2), None), "'where' must be 0 (host) or 1 (device).")
        refused(L.tnco_hip_contract_load_leaf_versions(h, 2, 2, ptr(two), 0, 0, 1, ptr(i64(7)), None),
                "dims do not multiply to the versions' elements.")
        refused(L.tnco_hip_contract_load_leaf_versions(h, 2, 2, ptr(two), 0, 1, 1, ptr(n2), None), "a host stack must have the plan's dtype.")
        # run_walkers
        q = i64(-1, 2, -1)
        refused(L.tnco_hip_contract_run_walkers(h, None, ptr(q), 5), "null argument.")
        refused(L.tnco_hip_contract_run_walkers(h, wh, None, 5), "null argument.")
        for g in (0, 1025):
            refused(L.tnco_hip_contract_run_walkers(h, wh, ptr(q), g), "'group' must be from 1 to 1024.")
        refused(L.tnco_hip_contract_run_walkers(plain._handle()[1], wh, ptr(q), 5),
                "leaf sets need a path kernel: call tnco_hip_contract_set_path_kernel first.")
        refused(L.tnco_hip_contract_run_walkers(h, wh, ptr(i64(-1, 4, -1)), 5),
                "the qubit 4 of leaf 1 is not -1 or a qubit of the walkers (0 to 3).")
        refused(L.tnco_hip_contract_run_walkers(h, wh, ptr(i64(-2, 2, -1)), 5),
                "the qubit -2 of leaf 0 is not -1 or a qubit of the walkers (0 to 3).")
        refused(L.tnco_hip_contract_run_walkers(h, wh, ptr(i64(0, 2, -1)), 5), "leaf 0 has no versions loaded.")
        refused(L.tnco_hip_contract_run_walkers(h, wh, ptr(q), 5), "leaf 2 was never loaded.")
        c.bind({2: sets[0][2]})
        # choose, walkers_output: before any run_walkers
        out = np.zeros((R, c.plan.out_numel), dtype)
        not_walked = "the handle's last run was not a tnco_hip_contract_run_walkers over these walkers."
        refused(L.tnco_hip_walkers_choose(wh, h, 0, 0), not_walked)
        refused(L.tnco_hip_contract_walkers_output(h, wh, ptr(out)), not_walked)
        first = check_walk(c, w, versions, {1: 2}, bits, 5, "before the refusals")
        c.run_walkers(w, {1: 2}, group=5)
        refused(L.tnco_hip_walkers_choose(wh, h, 0, 0), f"the output of the handle holds {c.plan.out_numel} elements, not the 2 amplitudes of a choice.")
        refused(L.tnco_hip_walkers_choose(None, h, 0, 0), "null argument.")
        with ctr.Walkers(R, N_QUBITS) as other:
            refused(L.tnco_hip_walkers_choose(other._handle(), h, 0, 0), not_walked)
            refused(L.tnco_hip_contract_walkers_output(h, other._handle(), ptr(out)), not_walked)
        # the walkers
        new = C.c_void_p()
        refused(L.tnco_hip_walkers_create(0, 0, 3, 0, C.byref(new)), "'n_walkers' must be at least 1.")
        refused(L.tnco_hip_walkers_create(0, 3, 0, 0, C.byref(new)), "'n_qubits' must be at least 1.")
        refused(L.tnco_hip_walkers_create(0, 1 << 30, 1 << 11, 0, C.byref(new)), "the table of bits is too large (2^40 at the most).")
        refused(L.tnco_hip_walkers_create(-1, 3, 3, 0, C.byref(new)), "'device' is not valid.")
        refused(L.tnco_hip_walkers_create(0, 3, 3, 0, None), "null argument.")
        rc = L.tnco_hip_walkers_create(0, 1 << 39, 2, 0, C.byref(new))  # 2^40 bytes of bits: more than the device has
        text = L.tnco_hip_last_error().decode()
        assert rc == _lib.ERUNTIME and text.startswith(f"the walkers need {(1 << 40) + (1 << 39) + 320} bytes of device memory, ") \
            and text.endswith(" are free."), (rc, text)
        assert new.value is None
        if L.tnco_hip_device_count() > 1:
            with ctr.Walkers(R, N_QUBITS, device=1) as far:
                refused(L.tnco_hip_contract_run_walkers(h, far._handle(), ptr(q), 5), "the walkers are on device 1, the handle on device 0.")
        bad = np.ascontiguousarray(bits.T).copy()
        bad[1, 2] = 2
        refused(L.tnco_hip_walkers_write(wh, ptr(bad)), "a bit is neither 0 nor 1.")
        refused(L.tnco_hip_walkers_write(wh, None), "null argument.")
        refused(L.tnco_hip_walkers_read(wh, None, None), "null argument.")
        tb = np.array([0, 1, 3, 2], np.uint8)
        for k in (0, 9):
            refused(L.tnco_hip_walkers_permute(wh, k, ptr(i64(0, 1)), ptr(tb)), "'k' must be from 1 to 8.")
        refused(L.tnco_hip_walkers_permute(wh, 2, ptr(i64(0, 4)), ptr(tb)), "a qubit is not a qubit of the walkers (0 to 3).")
        refused(L.tnco_hip_walkers_permute(wh, 2, ptr(i64(1, 1)), ptr(tb)), "a qubit is named twice.")
        for table in ((0, 1, 2, 2), (0, 1, 2, 4)):
            refused(L.tnco_hip_walkers_permute(wh, 2, ptr(i64(0, 1)), ptr(np.array(table, np.uint8))), "'table' is not a permutation of 0 to 2^k - 1.")
        # nothing changed: the bits, the flags, the versions, the outputs of the last run and of the next one
        assert np.array_equal(w.bits, bits) and not w.dead.any()
        assert np.array_equal(bits_of(c.walker_outputs(w)), bits_of(first))
        assert np.array_equal(bits_of(check_walk(c, w, versions, {1: 2}, bits, 5, "after the refusals")), bits_of(first))
    with ctr.Contractor([(0, 1)], [("a", "x"), ("a",)], [(2, 2), (2,)], ("x",), dtype=np.complex64, path_kernel=4) as c, ctr.Walkers(3, 2) as w:
        c.bind({0: np.eye(2, dtype=np.complex64), 1: np.array([1, 0], np.complex64)})
        c.bind_versions({1: np.eye(2, dtype=np.complex64)})
        c.run_walkers(w, {1: 0})
        L, h = c._handle()
        for qubit in (-1, 2):
            refused(L.tnco_hip_walkers_choose(w._handle(), h, qubit, 0), "'qubit' is not a qubit of the walkers (0 to 1).")
        for step in (-1, 1 << 32):
            refused(L.tnco_hip_walkers_choose(w._handle(), h, 0, step), "'step' must be from 0 to 2^32 - 1.")
        c.choose(w, 1, 0)  # amplitudes (1, 0): the bit stays 0, nobody dies
        assert not w.bits.any() and not w.dead.any()
        c.run()
        refused(L.tnco_hip_walkers_choose(w._handle(), h, 0, 0), not_walked)
