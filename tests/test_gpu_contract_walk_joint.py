"""The joint draw on the device (csrc/contract_walk.h, ct_walk_choose_joint_kernel): `Contractor.choose_joint` and
tnco_hip_walkers_choose_joint, per element against the model (tests/walk_joint_cases.py).

The network.  One bound leaf A with axes (o1 .. ok, x1, x2, x3), all of dimension 2, and an indexed one-hot leaf on each of
x1, x2, x3; the output is (o1 .. ok).  A product with a one-hot vector is exact, so walker i meets A[..., its three bits]: 8
amplitude vectors, picked by `Walkers.write`.  Five of them are set by hand: all zero (a dead walker); one non-zero entry,
at v = 0 and at v = N - 1; zero entries between non-zero ones; parts near 1e-30, whose squares are subnormal or zero in
float32 and normal in float64.  A part that is not finite cannot be confined to one vector (0 x inf is NaN in every other
walker's sum): the runs with an inf part and with a NaN part are runs of their own in which every walker is dead.

The reference is the model applied to the outputs that the device holds (`walker_outputs`) with the uniforms of
tests/walk_cases.py: the k rows of the table and the dead flags must be its bits, for every walker.

Sizes.  k = 1 .. 6; 1, 300 and 70 000 walkers.  70 000 walkers are 274 blocks of 256 lanes: more than one block.  A second
trip of the grid-stride loop is not reached: the grid is capped at 65 536 blocks, 2^24 walkers."""
import ctypes as C

import numpy as np
import pytest

from tests import walk_cases as wc
from tests import walk_joint_cases as wj

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
DTYPE_IDS = [np.dtype(d).name for d in DTYPES]
N_QUBITS = 11
X_QUBITS = (9, 0, 5)  # the qubits that index the three closing leaves
TARGETS = (3, 7, 1, 10, 2, 6)  # the qubits drawn, the first k of them; 4 and 8 are never named
SEED = 0x0FED_CBA9_8765_4321
PATH = [(0, 3), (0, 2), (0, 1)]  # A with the leaf of x1, the result with that of x2, then x3


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def outputs_of(k):
    return tuple(f"o{j}" for j in range(1, k + 1))


def network(k):
    ts = [("x1",), ("x2",), ("x3",), outputs_of(k) + ("x1", "x2", "x3")]
    return ts, [(2,)] * 3 + [(2,) * (k + 3)]


def amplitudes(dtype, k, seed=1):
    """A [N, 8] of `dtype`: column x is the amplitude vector of the walkers whose three bits spell x (module docstring)."""
    dtype, N = np.dtype(dtype), 1 << k
    rng = np.random.RandomState(seed + k)
    A = rng.normal(size=(N, 8)).astype(dtype)
    if dtype.kind == "c":
        A = (A + 1j * rng.normal(size=(N, 8))).astype(dtype)
    A[:, 0] = 0
    A[:, 1], A[:, 2] = 0, 0
    A[0, 1], A[N - 1, 2] = 1.5, -0.75
    if N >= 4:
        A[1, 3], A[N - 2, 3] = 0, 0
    if N >= 8:
        A[3:5, 3] = 0
    A[:, 4] = A[:, 4] * 1e-30
    return A


def make(ctr, dtype, k, A=None, path=PATH):
    ts, shapes = network(k)
    c = ctr.Contractor(path, ts, shapes, outputs_of(k), dtype=dtype, path_kernel=1024)
    c.bind({3: (amplitudes(dtype, k) if A is None else A).reshape(shapes[3])})
    c.bind_versions({t: np.eye(2, dtype=dtype) for t in range(3)})
    return c


LEAF_QUBIT = {t: q for t, q in enumerate(X_QUBITS)}


def random_bits(R, seed):
    return np.random.RandomState(seed).randint(0, 2, (R, N_QUBITS)).astype(np.uint8)


def met(c, out, inds):
    """[walkers, N]: the outputs with the axes in the order `inds`, an outcome's bits spelling its column."""
    p = c.plan
    return out.transpose([0] + [1 + p.inds.index(x) for x in inds]).reshape(len(out), -1)


def draw_and_check(c, w, qubits, step, seed, leaf_qubit=LEAF_QUBIT, inds=None, what=""):
    """run_walkers, choose_joint, and the table against the model on the device's own outputs; returns (amplitudes met,
    outcomes, dead of this draw)."""
    k = len(qubits)
    before, dead_before = w.bits, w.dead
    c.run_walkers(w, leaf_qubit)
    a = met(c, c.walker_outputs(w), c.plan.inds if inds is None else inds)
    c.choose_joint(w, qubits, step, inds=inds)
    want, want_dead = wj.choose_joint(a, wc.uniforms(seed, np.arange(len(before)), step))
    after, dead = w.bits, w.dead
    assert np.array_equal(after[:, list(qubits)], wj.outcome_bits(want, k)), what
    assert np.array_equal(dead, dead_before | want_dead), what
    others = [q for q in range(after.shape[1]) if q not in qubits]
    assert np.array_equal(after[:, others], before[:, others]), f"{what}: a row of a qubit not named was written"
    return a, want, want_dead


def x_of(bits):
    return bits[:, X_QUBITS[0]] * 4 + bits[:, X_QUBITS[1]] * 2 + bits[:, X_QUBITS[2]]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_joint_choice_against_the_model_bit_for_bit(ctr, dtype):
    for k in range(1, 7):
        A, qubits = amplitudes(dtype, k), TARGETS[:k]
        with make(ctr, dtype, k, A) as c:
            for R in (1, 300, 70_000):
                what = f"{np.dtype(dtype).name} k = {k} R = {R}"
                bits = random_bits(R, seed=R + k)
                with ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
                    w.write(bits)
                    a, want, want_dead = draw_and_check(c, w, qubits, 7, SEED, what=what)
                    # the walker met its own vector, unchanged: subnormal parts too
                    assert np.array_equal((a + 0).view(np.uint8), (A.T[x_of(bits)] + 0).view(np.uint8)), what
                    p = wc.probability(a)
                    assert np.array_equal(want_dead, x_of(bits) == 0), what  # (dead: the all-zero vector, nobody else)
                    assert (p[np.arange(R), want] > 0)[~want_dead].all(), what  # (an outcome with p = 0 is not drawn)
                    assert (want[x_of(bits) == 1] == 0).all() and (want[x_of(bits) == 2] == (1 << k) - 1).all(), what
                    if R > 1:
                        assert len(set(x_of(bits).tolist())) == 8 and len(set(want.tolist())) > (1 << k) // 2, what
                        # parts near 1e-30: float32 squares would be 0, the squares are taken in float64 and the walkers live
                        assert (x_of(bits) == 4).any() and not want_dead[x_of(bits) == 4].any(), what
                    # a second draw at another step, from the bits that the first left: other uniforms, dead flags stay
                    draw_and_check(c, w, qubits, 8, SEED, what=what + " second draw")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_qubit_leaves_the_table_of_choose(ctr, dtype):
    R = 300
    bits = random_bits(R, seed=5)
    tables = []
    with make(ctr, dtype, 1) as c:
        for joint in (False, True):
            with ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
                w.write(bits)
                c.run_walkers(w, LEAF_QUBIT)
                if joint:
                    c.choose_joint(w, (TARGETS[0],), 3)
                else:
                    c.choose(w, TARGETS[0], 3)
                tables.append((w.bits, w.dead))
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
    assert tables[0][1].any() and not tables[0][1].all() and 50 < tables[0][0][:, TARGETS[0]].sum() < 250


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=["float32", "complex128"])
def test_a_part_that_is_not_finite_kills_every_walker(ctr, dtype, bad):
    k, R = 3, 300
    A = amplitudes(dtype, k)
    A[5, 6] = bad * (1j if np.dtype(dtype).kind == "c" else 1)
    bits = random_bits(R, seed=6)
    with make(ctr, dtype, k, A) as c, ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
        w.write(bits)
        a, want, want_dead = draw_and_check(c, w, TARGETS[:k], 0, SEED)
        # (inf in the walkers whose bits select the vector, 0 x inf = NaN in all the others)
        assert not np.isfinite(wc.probability(a)[:, 5]).any() and want_dead.all() and not want.any()
        assert w.dead.all() and not w.bits[:, list(TARGETS[:k])].any()


def test_inds_in_another_order_permute_the_bits_of_the_outcome(ctr):
    """The stride path of the kernel: the amplitude of outcome v lies at the sum of the strides of v's set bits."""
    k, R, dtype = 3, 300, np.complex64
    qubits = TARGETS[:k]
    bits = random_bits(R, seed=8)
    drawn = {}
    with make(ctr, dtype, k) as c:
        assert c.plan.inds == ("o1", "o2", "o3")
        for inds in (None, ("o1", "o2", "o3"), ("o3", "o1", "o2"), ("o2", "o3", "o1"), ("o3", "o2", "o1"), ("o1", "o3", "o2")):
            with ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
                w.write(bits)
                # (the model reads the outputs with their axes in the order `inds`: outcome v of the qubits is a[inds = v])
                draw_and_check(c, w, qubits, 2, SEED, inds=inds, what=str(inds))
                drawn[inds] = w.bits
    assert np.array_equal(drawn[None], drawn[("o1", "o2", "o3")])
    # the outcomes are numbered in another order, so the tails are other sums and the same u falls elsewhere: other tables
    assert all(not np.array_equal(drawn[None], drawn[inds]) for inds in drawn if inds not in (None, ("o1", "o2", "o3")))


def test_two_paths_of_one_network_give_the_same_table(ctr):
    """Layout independence.  With one leaf that holds every output axis no path changes their order, so here A is two
    leaves, (o1, x1, y) and (y, o2 .. ok, x2, x3), of small integers: every product and sum is exact, whatever the order.
    The first path ends with (o1, o2 .. ok) on the device, the second with (o2 .. ok, o1)."""
    R, dtype = 300, np.complex64
    for k in (2, 3, 6):
        outs = outputs_of(k)
        ts = [("x1",), ("x2",), ("x3",), ("o1", "x1", "y"), ("y",) + outs[1:] + ("x2", "x3")]
        shapes = [(2,)] * 3 + [(2, 2, 2), (2,) * (k + 2)]
        rng = np.random.RandomState(40 + k)
        A1 = (rng.randint(-3, 4, shapes[3]) + 1j * rng.randint(-3, 4, shapes[3])).astype(dtype)
        A2 = (rng.randint(-3, 4, shapes[4]) + 1j * rng.randint(-3, 4, shapes[4])).astype(dtype)
        bits = random_bits(R, seed=k)
        tables, held = [], []
        for path in ([(0, 3), (0, 2), (0, 2), (0, 1)], [(1, 4), (1, 3), (0, 1), (0, 1)]):
            with ctr.Contractor(path, ts, shapes, outs, dtype=dtype, path_kernel=1024) as c, ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
                held.append(ctr._held_axes(c.plan))
                c.bind({3: A1, 4: A2})
                c.bind_versions({t: np.eye(2, dtype=dtype) for t in range(3)})
                w.write(bits)
                a, _, _ = draw_and_check(c, w, TARGETS[:k], 1, SEED, inds=outs, what=f"k = {k} {path}")
                tables.append((w.bits, w.dead, a))
        assert held[0] == outs and held[1] == outs[1:] + outs[:1], held  # the layouts differ
        assert np.array_equal(tables[0][2], tables[1][2])  # (exact arithmetic: the same amplitudes)
        assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
        assert len({tuple(row) for row in tables[0][0][:, list(TARGETS[:k])]}) > 2


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["float32", "complex64"])
def test_one_output_serves_every_walker(ctr, dtype):
    """No indexed leaf: one set is run, `each` is 0, every walker reads the same amplitudes and differs only by u."""
    R = 70_000
    for k in (1, 2, 5):
        bits = random_bits(R, seed=9)
        with make(ctr, dtype, k) as c, ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
            c.bind({0: np.array([0, 1], dtype), 1: np.array([0, 1], dtype), 2: np.array([1, 0], dtype)})  # x = 6: a random vector
            w.write(bits)
            r = c.run_walkers(w, {})
            assert r.sets == 1
            a, want, want_dead = draw_and_check(c, w, TARGETS[:k], 4, SEED, leaf_qubit={}, what=f"k = {k}")
            assert (a == a[0]).all() and np.array_equal((a[0] + 0).view(np.uint8), (amplitudes(dtype, k)[:, 6] + 0).view(np.uint8))
            assert not want_dead.any()
            p = wc.probability(a[0])
            counts = np.bincount(want, minlength=1 << k)
            sigma = np.sqrt(R * (p / p.sum()) * (1 - p / p.sum()))
            assert (np.abs(counts - R * p / p.sum()) <= 5 * sigma).all(), (k, counts)


def test_abi_refusals_in_their_order_leave_the_objects_unchanged(ctr):
    from tnco_amd import _lib
    k, R, dtype = 2, 5, np.complex64
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    bits = random_bits(R, seed=10)
    not_walked = "the handle's last run was not a tnco_hip_contract_run_walkers over these walkers."
    not_qubit = f"a qubit is not a qubit of the walkers (0 to {N_QUBITS - 1})."
    not_strides = "'strides' is not a permutation of 1, 2, ..., 2^(k - 1)."
    with make(ctr, dtype, k) as c, ctr.Walkers(R, N_QUBITS, seed=SEED) as w:
        w.write(bits)
        L, h = c._handle()
        wh = w._handle()

        def refused(rc, text):
            assert rc == _lib.EINVAL and L.tnco_hip_last_error().decode() == text, (rc, L.tnco_hip_last_error().decode())

        qs, st = i64(3, 7), i64(2, 1)
        # before any run_walkers: a null argument comes first, then the run, then everything else
        refused(L.tnco_hip_walkers_choose_joint(None, h, 9, ptr(qs), ptr(st), -1), "null argument.")
        refused(L.tnco_hip_walkers_choose_joint(wh, None, 9, ptr(qs), ptr(st), -1), "null argument.")
        refused(L.tnco_hip_walkers_choose_joint(wh, h, 9, None, ptr(st), -1), "null argument.")
        refused(L.tnco_hip_walkers_choose_joint(wh, h, 9, ptr(qs), None, -1), "null argument.")
        refused(L.tnco_hip_walkers_choose_joint(wh, h, 9, ptr(i64(3, 3)), ptr(i64(1, 1)), -1), not_walked)
        c.run_walkers(w, LEAF_QUBIT)
        first = c.walker_outputs(w)
        with ctr.Walkers(R, N_QUBITS) as other:
            refused(L.tnco_hip_walkers_choose_joint(other._handle(), h, 9, ptr(qs), ptr(st), -1), not_walked)
        # k, with everything after it wrong too
        for bad in (0, 7, -1):
            refused(L.tnco_hip_walkers_choose_joint(wh, h, bad, ptr(i64(3, 3)), ptr(i64(1, 1)), -1), "'k' must be from 1 to 6.")
        # the size of the output
        for bad in (1, 3, 6):
            refused(L.tnco_hip_walkers_choose_joint(wh, h, bad, ptr(i64(3, 3, 3, 3, 3, 3)), ptr(i64(1, 1, 1, 1, 1, 1)), -1),
                    f"the output of the handle holds 4 elements, not the {1 << bad} amplitudes of a joint choice of {bad} qubits.")
        # the qubits
        for bad in (-1, N_QUBITS):
            refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(i64(3, bad)), ptr(i64(1, 1)), -1), not_qubit)
            refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(i64(bad, 3)), ptr(i64(1, 1)), -1), not_qubit)
        refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(i64(3, 3)), ptr(i64(1, 1)), -1), "a qubit is named twice.")
        # the strides
        for bad in ((1, 1), (2, 2), (0, 1), (1, 3), (4, 1), (-2, 1), (1, 1 << 40)):
            refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(qs), ptr(i64(*bad)), -1), not_strides)
        # the step
        for bad in (-1, 1 << 32):
            refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(qs), ptr(st), bad), "'step' must be from 0 to 2^32 - 1.")
        # nothing changed: the bits, the flags, the outputs; and the draw is still there to make
        assert np.array_equal(w.bits, bits) and not w.dead.any()
        assert np.array_equal(c.walker_outputs(w).view(np.uint8), first.view(np.uint8))
        assert L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(qs), ptr(i64(1, 2)), (1 << 32) - 1) == 0
        a = met(c, first, ("o2", "o1"))  # strides (1, 2): qubit 3 is given the last axis
        want, want_dead = wj.choose_joint(a, wc.uniforms(SEED, np.arange(R), (1 << 32) - 1))
        assert np.array_equal(w.bits[:, [3, 7]], wj.outcome_bits(want, 2)) and np.array_equal(w.dead, want_dead)
        c.bind({t: np.array([1, 0], dtype) for t in range(3)})
        c.run()  # (a run of another kind: the outputs of the walkers are gone)
        refused(L.tnco_hip_walkers_choose_joint(wh, h, 2, ptr(qs), ptr(st), 0), not_walked)
    # six qubits: every stride of 1 .. 32 must be there
    with make(ctr, np.float32, 6) as c, ctr.Walkers(3, N_QUBITS) as w:
        c.run_walkers(w, LEAF_QUBIT)
        L, h = c._handle()
        six = i64(*TARGETS)
        refused(L.tnco_hip_walkers_choose_joint(w._handle(), h, 6, ptr(six), ptr(i64(32, 16, 8, 4, 2, 64)), 0), not_strides)
        refused(L.tnco_hip_walkers_choose_joint(w._handle(), h, 6, ptr(six), ptr(i64(32, 16, 8, 4, 2, 2)), 0), not_strides)
        assert L.tnco_hip_walkers_choose_joint(w._handle(), h, 6, ptr(six), ptr(i64(1, 2, 4, 8, 16, 32)), 0) == 0
