"""The joint draw without a device: the model (tests/walk_joint_cases.py), `sampling.partial_network` and `connected_to`
for gates of several qubits, and every refusal of `Contractor.choose_joint` and `Sampler(max_gate_qubits=)` that the
Python side makes, in their order.

    the model at k = 1   walk_joint_cases.choose_joint on pairs is walk_cases.choose: 10^4 random pairs in the four
                         dtypes, and the edge rows (zeros, inf, NaN, subnormal parts);
    the distribution     fixed probability vectors of 4 and 8 outcomes, one of them with zero entries, 2 x 10^5 uniforms of
                         walk_cases.uniforms: every frequency within 5 sigma of p_v / s (sigma from the binomial law), and
                         an outcome v >= 1 with p_v = 0 never;
    the two consequences of the rule that the model's docstring states, on designed rows."""
import itertools

import numpy as np
import pytest

from tests import walk_cases as wc
from tests import walk_joint_cases as wj


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


@pytest.fixture(scope="module")
def smp():
    from tnco_amd import sampling
    return sampling


@pytest.fixture
def no_gpu(monkeypatch):
    from tnco_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", refuse)


def refusal(call, error, text):
    with pytest.raises(error) as e:
        call()
    assert type(e.value) is error and str(e.value) == text, (type(e.value), str(e.value))


def unitary(rng, n=2):
    q, r = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


CZ = np.diag([1, 1, 1, -1]).astype(complex)


# ---- the model -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_the_model_at_one_qubit_is_the_choice_of_walk_cases(dtype):
    rng = np.random.RandomState(31)
    n = 10 ** 4
    a = rng.normal(size=(n, 2)).astype(dtype)
    if np.dtype(dtype).kind == "c":
        a = (a + 1j * rng.normal(size=(n, 2))).astype(dtype)
    real = a.real.dtype.type
    tiny = float(np.finfo(real).tiny)
    edges = [(0, 0), (1, 0), (0, 1), (np.inf, 1), (1, np.inf), (np.nan, 1), (1, np.nan), (np.inf, np.inf), (tiny / 4, tiny / 2),
             (tiny / 2, tiny / 4), (tiny / 4, 0), (0, tiny / 4), (3e-30, 4e-30), (1e30, 1e-30), (-0.0, 0.0)]
    a[:len(edges)] = np.array(edges, real)
    if np.dtype(dtype).kind == "c":
        a[len(edges):2 * len(edges)] = 0
        a[len(edges):2 * len(edges)].imag = np.array(edges, real)  # (the same in the imaginary parts)
    u = wc.uniforms(77, np.arange(n), 4)
    u[:2 * len(edges):2] = 0.0  # (the smallest uniform on every other edge row)
    bits, dead = wc.choose(a[:, 0], a[:, 1], u)
    outcomes, dead_joint = wj.choose_joint(a, u)
    assert np.array_equal(outcomes, bits) and np.array_equal(dead_joint, dead)
    assert dead[0] and dead[3] and dead[5] and not dead[1] and 0.3 * n < bits.sum() < 0.7 * n
    assert np.array_equal(wj.outcome_bits(outcomes, 1)[:, 0], bits)


VECTORS = {  # probabilities, not normalised: the rule divides by nothing
    "4-outcomes": [0.1, 0.2, 0.3, 0.4],
    "4-outcomes-zeros": [0.5, 0.0, 1.5, 0.0],
    "8-outcomes": [0.05, 0.3, 0.02, 0.13, 0.2, 0.1, 0.15, 0.05],
    "8-outcomes-zeros": [0.0, 0.7, 0.0, 0.0, 1.1, 0.4, 0.0, 0.8],
}


@pytest.mark.parametrize("name", list(VECTORS))
def test_the_model_draws_every_outcome_with_its_probability(name):
    p = np.array(VECTORS[name])
    R = 2 * 10 ** 5
    u = wc.uniforms(0xABCDEF0123, np.arange(R), 9)
    outcomes, dead = wj.choose_joint(np.broadcast_to(np.sqrt(p), (R, len(p))), u)
    assert not dead.any()
    counts = np.bincount(outcomes, minlength=len(p))
    want = p / p.sum()
    sigma = np.sqrt(R * want * (1 - want))
    off = np.abs(counts - R * want)
    print(f"{name}: counts {counts.tolist()}, largest deviation {float((off[sigma > 0] / sigma[sigma > 0]).max()):.2f} sigma")
    assert (off[sigma > 0] <= 5 * sigma[sigma > 0]).all()
    assert not counts[1:][p[1:] == 0].any()  # an outcome v >= 1 with p_v = 0 never occurs
    if p[0] == 0:
        assert counts[0] == 0  # (no u s of these rounds up to s)


def test_the_two_consequences_of_the_rule():
    # an outcome v >= 1 with p_v = 0 is never drawn, whatever u is: tail(v) = tail(v + 1)
    a = np.array([[1, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]], np.float64)
    for u in (0.0, 0.25, 0.5, 0.75, 1 - 2.0 ** -53):
        outcomes, dead = wj.choose_joint(a, np.full(4, u))
        assert not dead.any() and all(a[i, v] != 0 for i, v in enumerate(outcomes)), u
    # outcome 0 with p_0 = 0 only where u s rounds up to s: a normal s never does (u <= 1 - 2^-53 moves it by more than
    # half an ulp), the smallest subnormal does
    top = 1 - 2.0 ** -53
    a = np.array([[0, 1, 2, 0], [0, 2.0 ** -537, 0, 0], [0, 2.0 ** -537, 0, 0]], np.float64)  # p = (0, 1, 4, 0), (0, 2^-1074, 0, 0)
    outcomes, dead = wj.choose_joint(a, np.array([top, top, 0.25]))
    s = wj.tails(a)[:, 0]
    assert s.tolist() == [5.0, 2.0 ** -1074, 2.0 ** -1074] and top * s[0] < s[0] and top * s[1] == s[1] and 0.25 * s[2] == 0
    assert outcomes.tolist() == [1, 0, 1] and not dead.any()
    # the tails are summed from the top: their order of additions is part of the rule
    a = np.array([[2.0 ** -27, 2.0 ** -27, 2.0 ** -27, 1.0]])  # p = 2^-54 three times, then 1
    assert wj.tails(a)[0].tolist() == [1.0, 1.0, 1.0, 1.0] and (2.0 ** -54 * 3) + 1.0 == 1 + 2.0 ** -52  # (the sum from the bottom)
    assert wj.outcome_bits([5, 2], 3).tolist() == [[1, 0, 1], [0, 1, 0]]


def test_the_model_walk_with_joint_draws_samples_the_exact_distribution(smp):
    rng = np.random.RandomState(12)
    u1 = lambda q: (unitary(rng), (q,))  # noqa: E731
    circuit = [u1(0), u1(1), u1(2), (unitary(rng, 4), (2, 0)), (CZ, (0, 1)), (unitary(rng, 8), (1, 2, 0)), u1(1), (unitary(rng, 4), (0, 1))]
    n, R = 3, 1 << 16
    exact = wc.exact_distribution(circuit, n)
    is_classical = lambda m, qs: None if len(qs) == 1 else smp.classical_table(m)  # noqa: E731
    bits, records = wj.model_walk_joint(circuit, n, R, 2025, is_classical)
    assert [r["qubits"] for r in records] == [(0,), (1,), (2,), (2, 0), (1, 2, 0), (1,), (0, 1)]
    assert all(r["a"].shape == r["mag"].shape == (R, 1 << len(r["qubits"])) and not r["dead"].any() for r in records)
    counts = np.zeros((2,) * n)
    np.add.at(counts, tuple(bits.T.astype(int)), 1)
    sigma = np.sqrt(R * exact * (1 - exact))
    worst = float((np.abs(counts - R * exact) / sigma).max())
    print(f"largest deviation {worst:.2f} sigma")
    assert worst <= 5
    # on a circuit of 1-qubit and classical gates it is walk_cases.model_walk
    plain = [g for g in circuit if len(g[1]) == 1 or smp.classical_table(g[0]) is not None]
    b0, r0 = wc.model_walk(plain, n, 512, 7, is_classical)
    b1, r1 = wj.model_walk_joint(plain, n, 512, 7, is_classical)
    assert np.array_equal(b0, b1) and all(np.array_equal(x["a0"], y["a"][:, 0]) and np.array_equal(x["mag1"], y["mag"][:, 1])
                                          for x, y in zip(r0, r1))


# ---- partial networks ----------------------------------------------------------------------------------------------------

def test_the_partial_network_of_a_one_qubit_gate_is_unchanged(smp):
    u, v = np.arange(4).reshape(2, 2), np.arange(4, 8).reshape(2, 2)
    cz = CZ.reshape(2, 2, 2, 2)
    gates = [(u, (0,)), (cz, (0, 2)), (v, (2,))]
    ts_inds, arrays, output, closing = smp.partial_network(gates, 2, 3)
    assert ts_inds == [("q0_0",), ("q1_0",), ("q2_0",), ("q0_1", "q0_0"), ("q0_2", "q2_2", "q0_1", "q2_0"), ("q2_3", "q2_2"), ("q0_2",),
                       ("q1_0",)]
    assert output == ("q2_3",) and closing == {6: 0, 7: 1}
    assert [None if a is None else np.asarray(a).tolist() for a in arrays] == [[1, 0], [1, 0], [1, 0], u.tolist(), cz.tolist(), v.tolist(), None,
                                                                              None]
    assert smp.connected_to(ts_inds, "q2_3") == [0, 2, 3, 4, 5, 6]  # (qubit 1 is a component of its own)
    assert smp.connected_to(ts_inds, "q1_0") == [1, 7]


def test_the_partial_network_of_a_drawing_gate_of_two_qubits(smp):
    rng = np.random.RandomState(3)
    u, w = unitary(rng), unitary(rng, 4).reshape(2, 2, 2, 2)
    gates = [(u, (0,)), (u, (3,)), (CZ.reshape(2, 2, 2, 2), (3, 1)), (w, (2, 0))]
    ts_inds, arrays, output, closing = smp.partial_network(gates, 3, 4)
    assert ts_inds[:4] == [(f"q{x}_0",) for x in range(4)]
    assert ts_inds[4:8] == [("q0_1", "q0_0"), ("q3_2", "q3_0"), ("q3_3", "q1_3", "q3_2", "q1_0"), ("q2_4", "q0_4", "q2_0", "q0_1")]
    assert output == ("q2_4", "q0_4") and closing == {8: 1, 9: 3} and ts_inds[8:] == [("q1_3",), ("q3_3",)]
    assert [a is None for a in arrays] == [False] * 8 + [True] * 2 and arrays[7] is w
    # the two open indices lie on the gate's tensor: one component holds them, the CZ's component is a factor that cancels
    both = smp.connected_to(ts_inds, output)
    assert both == [0, 2, 4, 7] == smp.connected_to(ts_inds, list(output)) == smp.connected_to(ts_inds, "q2_4")
    # the amplitudes, against the dense product
    psi = np.zeros((2,) * 4, complex)
    psi[0, 0, 0, 0] = 1
    for m, qs in gates:
        psi = wc.apply_gate(psi, m, qs, 4)
    sym = {x: chr(ord("a") + k) for k, x in enumerate(dict.fromkeys(x for xs in ts_inds for x in xs))}
    expr = ",".join("".join(sym[x] for x in xs) for xs in ts_inds) + "->" + "".join(sym[x] for x in output)
    for b1, b3 in itertools.product((0, 1), repeat=2):
        leaves = [np.eye(2)[{1: b1, 3: b3}[closing[t]]] if a is None else np.asarray(a, complex) for t, a in enumerate(arrays)]
        got = np.einsum(expr, *leaves)
        assert np.allclose(got, psi[:, b1, :, b3].T, atol=1e-14)  # (axes (qubit 2, qubit 0): the gate's order)


def test_connected_to_keeps_the_union_of_the_components(smp):
    ts_inds = [("a", "b"), ("b",), ("c", "d"), ("d",), ("e",), ("e", "f")]
    assert smp.connected_to(ts_inds, "a") == [0, 1] and smp.connected_to(ts_inds, "c") == [2, 3]
    assert smp.connected_to(ts_inds, ("a", "c")) == [0, 1, 2, 3] and smp.connected_to(ts_inds, ["c", "f"]) == [2, 3, 4, 5]
    assert smp.connected_to(ts_inds, ("a", "b")) == [0, 1]


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_sampler_refusals_of_the_new_keyword(smp, ctr, no_gpu):
    rng = np.random.RandomState(0)
    u = unitary(rng)
    good = [(u, ("a",)), (CZ, ("a", "b"))]
    assert ctr.MAX_CHOOSE_QUBITS == 6 and "MAX_CHOOSE_QUBITS" in ctr.__all__
    for bad in (0, 7, -1, 2.0, "2", None, True):
        refusal(lambda: smp.Sampler(good, max_gate_qubits=bad), ValueError, "'max_gate_qubits' must be an integer from 1 to 6.")
    # ... which comes before anything about the circuit
    refusal(lambda: smp.Sampler([(np.kron(u, u), (0, 1))], max_gate_qubits=7), ValueError, "'max_gate_qubits' must be an integer from 1 to 6.")
    # a gate that is not classical on more qubits than the keyword allows
    u8 = unitary(rng, 8)
    for most in (1, 2):
        refusal(lambda: smp.Sampler([(u, (0,)), (u8, (0, 1, 2))], max_gate_qubits=most), ValueError, smp.GATES_ERROR)
    refusal(lambda: smp.Sampler([(u, (0,)), (np.kron(u, u), (0, 1))]), ValueError, smp.GATES_ERROR)  # the default, as before
    refusal(lambda: smp.Sampler([(u, (0,)), (np.kron(u, u), (0, 1))], max_gate_qubits=1), ValueError, smp.GATES_ERROR)
    # what was refused before stays refused under the keyword: a 1-qubit matrix of another shape, a classical table of the wrong size
    for bad in ([(np.ones((2, 3)), (0,))], [(CZ, (0, 1, 2))], [(np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]], (0, 1))]):
        refusal(lambda: smp.Sampler(bad, max_gate_qubits=3), ValueError, smp.GATES_ERROR)
    # a drawing gate's matrix of the wrong size
    refusal(lambda: smp.Sampler([(u8, (0, 1))], max_gate_qubits=2), ValueError,
            "the matrix of a gate on 2 qubits must be 4 x 4, not of shape (8, 8).")
    refusal(lambda: smp.Sampler([(u, (0, 1, 2))], max_gate_qubits=3), ValueError,
            "the matrix of a gate on 3 qubits must be 8 x 8, not of shape (2, 2).")
    refusal(lambda: smp.Sampler([(np.ones((4, 3)), (0, 1))], max_gate_qubits=2), ValueError,
            "the matrix of a gate on 2 qubits must be 4 x 4, not of shape (4, 3).")
    # the size comes before the order of the qubits, and the other refusals after both, as before
    refusal(lambda: smp.Sampler([(u8, (0, 1))], max_gate_qubits=2, qubit_order=(0, 2)), ValueError,
            "the matrix of a gate on 2 qubits must be 4 x 4, not of shape (8, 8).")
    u4 = unitary(rng, 4)
    refusal(lambda: smp.Sampler([(u4, (0, 1))], max_gate_qubits=2, qubit_order=(0, 2)), ValueError, smp.ORDER_ERROR)
    refusal(lambda: smp.Sampler([(u4, (0, 0))], max_gate_qubits=2), ValueError, "a gate names a qubit twice.")
    refusal(lambda: smp.Sampler([(u4, (0, 1))], max_gate_qubits=2, max_width=10), NotImplementedError,
            "Sampling with finite width is not yet implemented.")


JOINT_TS = [("o1", "o2", "x"), ("x",)]


def test_choose_joint_refusals(ctr, no_gpu):
    w = ctr.Walkers(4, 3, device=0)
    make = lambda **kw: ctr.Contractor([(0, 1)], JOINT_TS, [(2, 2, 2), (2,)], ("o1", "o2"), dtype=np.complex64, device=0,  # noqa: E731
                                       **{"path_kernel": 4, **kw})
    c = make()
    c.close()
    refusal(lambda: c.choose_joint(w, (0, 1), 0), ValueError, "the Contractor is closed.")
    with make(path_kernel=None) as c:
        refusal(lambda: c.choose_joint(w, (0, 1), 0), NotImplementedError, "'choose_joint' needs a Contractor with 'path_kernel'.")
    with make(accumulate="float64") as c:
        refusal(lambda: c.choose_joint(w, (0, 1), 0), NotImplementedError, "'accumulate' is not supported with 'choose_joint'.")
    with ctr.Contractor([], [("i", "j")], [(2, 2)], dtype=np.float32, path_kernel=2) as c:
        refusal(lambda: c.choose_joint(w, (0, 1), 0), NotImplementedError, "'choose_joint' needs a plan with steps.")
    with make() as c:
        refusal(lambda: c.choose_joint(None, (0, 1), 0), TypeError, "'walkers' must be a Walkers object, not NoneType.")
        refusal(lambda: c.choose_joint(ctr.Walkers(4, 3, device=1), (0, 1), 0), ValueError,
                "the walkers are on device 1, the Contractor on device 0.")
        for bad in ((), tuple(range(7))):
            refusal(lambda: c.choose_joint(ctr.Walkers(4, 9, device=0), bad, 0), ValueError, "'qubits' must name 1 to 6 qubits.")
        for bad in (3, -1, 1.0, True):
            refusal(lambda: c.choose_joint(w, (0, bad), 0), ValueError, f"{bad!r} is not a qubit of the walkers (0 to 2).")
        refusal(lambda: c.choose_joint(w, (1, 1), 0), ValueError, "'qubits' names a qubit twice.")
        for bad in ((0,), (0, 1, 2)):
            refusal(lambda: c.choose_joint(w, bad, 0), ValueError,
                    f"the output of the plan holds 4 elements, not the {1 << len(bad)} amplitudes of a choice of {len(bad)} qubits.")
        for bad in (("o1",), ("o1", "o1"), ("o1", "x"), ("o1", "o2", "o2")):
            refusal(lambda: c.choose_joint(w, (0, 1), 0, inds=bad), ValueError,
                    "'inds' must name every index of the output ('o1', 'o2') once, one per qubit.")
        for bad in (-1, 1 << 32, 1.0, True):
            refusal(lambda: c.choose_joint(w, (0, 1), bad), ValueError, "'step' must be an integer from 0 to 2^32 - 1.")
            refusal(lambda: c.choose_joint(w, (0, 1), bad, inds=("o2", "o1")), ValueError, "'step' must be an integer from 0 to 2^32 - 1.")
        refusal(lambda: c.choose_joint(w, (0, 1), 0), ValueError, "the last run of the Contractor was not a 'run_walkers' over these walkers.")
    # an output axis of another dimension than 2 (4 elements all the same)
    with ctr.Contractor([(0, 1)], [("o", "x"), ("x",)], [(4, 2), (2,)], ("o",), dtype=np.float32, path_kernel=4, device=0) as c:
        refusal(lambda: c.choose_joint(w, (0, 1), 0), ValueError, "every axis of the output must have dimension 2, not (4,).")
    # an output that a sliced index selects block by block
    with make(slices=("o1",)) as c:
        assert c.plan.block_inds == ("o1",)
        refusal(lambda: c.choose_joint(w, (0, 1), 0), NotImplementedError,
                "'choose_joint' needs an output whose axes are all held at once: this plan's is a block that a sliced index selects.")
    w.close()
    with make() as c:
        refusal(lambda: c.choose_joint(w, (0, 1), 0), ValueError, "the Walkers are closed.")
