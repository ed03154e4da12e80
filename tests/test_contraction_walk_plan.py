"""The walkers without a GPU: the model of tests/walk_cases.py against what is known of it, and what `Walkers`,
`Contractor.bind_versions`, `run_walkers`, `choose` and `sampling.Sampler` refuse, with which type and words and in which
order, before the device is touched (`_lib.load` is made to raise).

    Philox4x32-10      the restatement from the constants gives Random123's known-answer vectors;
    partial networks   `sampling.partial_network` of a 3-qubit circuit, at every drawing gate and for every bitstring of
                       the other qubits, against the dense product of the gates in numpy;
    the model's walk   2^16 walkers over a 3-qubit circuit: the frequency of every bitstring within 5 sigma of the exact
                       distribution, sigma from the binomial law.  (This holds the model to account, not the kernels.)"""
import itertools

import numpy as np
import pytest

from tests import path_cases as pc
from tests import walk_cases as wc

CHAIN = pc.SMALL
ARGS = (pc.PATH, CHAIN.ts, CHAIN.shapes(), CHAIN.output)


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


def contractor(ctr, **kw):
    kw.setdefault("dtype", np.float32)
    kw.setdefault("slices", pc.SLICES)
    kw.setdefault("path_kernel", 5)
    return ctr.Contractor(*ARGS, **kw)


def unitary(rng):
    q, r = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


CZ = np.diag([1, 1, 1, -1]).astype(complex)
CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], complex)
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], complex)
ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], complex)


def circuit3(seed=11):
    rng = np.random.RandomState(seed)
    u = lambda q: (unitary(rng), (q,))  # noqa: E731
    return [u(0), u(1), u(2), (CNOT, (0, 1)), u(1), (CZ, (1, 2)), u(2), u(0), (SWAP, (2, 0)), u(1), (ISWAP, (0, 1)), u(0)]


# ---- the model -----------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter and key all zeros, and all ones."""
    zeros = wc.philox4x32_10(np.zeros(4, np.uint64), (0, 0))
    assert [f"{int(x):08x}" for x in zeros] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = wc.philox4x32_10(np.full(4, 0xFFFFFFFF, np.uint64), (0xFFFFFFFF, 0xFFFFFFFF))
    assert [f"{int(x):08x}" for x in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_uniforms_are_53_bit_fractions_that_depend_on_seed_walker_and_step():
    u = wc.uniforms(7, np.arange(1000), 3)
    assert ((0 <= u) & (u < 1)).all() and (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()
    assert len(set(u.tolist())) == 1000
    for other in (wc.uniforms(8, np.arange(1000), 3), wc.uniforms(7, np.arange(1000), 4), wc.uniforms(7 + (1 << 32), np.arange(1000), 3)):
        assert not (other == u).any()
    assert wc.uniforms(7, np.array([5 + (1 << 32)]), 3)[0] != u[5]  # (the high word of the walker's number counts)
    x = wc.philox4x32_10(np.array([5, 0, 3, 0], np.uint64), (7, 0))
    assert u[5] == ((int(x[0]) >> 5) * 2 ** 26 + (int(x[1]) >> 6)) / 2 ** 53


def test_choice_and_dead_walkers():
    a0 = np.array([1, 0, 0, np.inf, np.nan, 3e-30, 1e30], np.float32)
    a1 = np.array([0, 1, 0, 1, 1, 4e-30, 1e30], np.float32)
    u = np.full(7, 0.5)
    bits, dead = wc.choose(a0, a1, u)
    assert bits.tolist() == [0, 1, 0, 0, 0, 1, 0] and dead.tolist() == [False, False, True, True, True, False, False]
    assert wc.probability(np.array([3 + 4j], np.complex64))[0] == 25.0 and wc.probability(np.float32(1e30)) == np.float64(np.float32(1e30)) ** 2


def test_permute_and_select():
    bits = np.array(list(itertools.product((0, 1), repeat=3)), np.uint8)
    cnot = wc.permute(bits, (0, 2), (0, 1, 3, 2))  # qubit 0 controls qubit 2
    assert (cnot[:, 0] == bits[:, 0]).all() and (cnot[:, 1] == bits[:, 1]).all() and (cnot[:, 2] == bits[:, 2] ^ bits[:, 0]).all()
    cycle = wc.permute(bits, (0, 1, 2), [(v << 1 | v >> 2) & 7 for v in range(8)])  # b0 b1 b2 -> b1 b2 b0
    assert (cycle == bits[:, [1, 2, 0]]).all()
    versions = np.arange(12).reshape(2, 2, 3)
    assert (wc.select(versions, bits, 1) == versions[bits[:, 1]]).all() and wc.select(versions, bits, 1).shape == (8, 2, 3)


def test_the_model_walk_samples_the_exact_distribution(smp):
    circuit, n, R = circuit3(), 3, 1 << 16
    exact = wc.exact_distribution(circuit, n)
    assert abs(exact.sum() - 1) < 1e-12
    bits, records = wc.model_walk(circuit, n, R, seed=2024, is_classical=lambda m, qs: None if len(qs) == 1 else smp.classical_table(m))
    assert len(records) == 8 and not any(r["dead"].any() for r in records)
    counts = np.zeros((2,) * n)
    np.add.at(counts, tuple(bits.T.astype(int)), 1)
    sigma = np.sqrt(R * exact * (1 - exact))
    worst = float((np.abs(counts - R * exact) / sigma).max())
    print(f"largest deviation {worst:.2f} sigma")
    assert worst <= 5


# ---- partial networks ----------------------------------------------------------------------------------------------------

def test_partial_networks_against_the_dense_product(smp):
    circuit, n = circuit3(), 3
    gates = [(np.asarray(m).reshape((2,) * (2 * len(qs))), qs) for m, qs in circuit]
    psi = np.zeros((2,) * n, np.complex128)
    psi[(0,) * n] = 1
    drawn = 0
    for g, (m, qs) in enumerate(circuit):
        dense = np.asarray(m)
        psi = wc.apply_gate(psi, dense, qs, n)
        if len(qs) != 1:
            continue
        drawn += 1
        ts_inds, arrays, output, closing = smp.partial_network(gates, g, n)
        assert len(ts_inds) == len(arrays) == n + (g + 1) + (n - 1) and sorted(closing.values()) == [x for x in range(n) if x != qs[0]]
        assert [a is None for a in arrays] == [t in closing for t in range(len(arrays))]
        sym = {x: k for k, x in enumerate(dict.fromkeys(x for xs in ts_inds for x in xs))}
        for others in itertools.product((0, 1), repeat=n - 1):
            b = dict(zip(sorted(closing.values()), others))
            leaves = [np.eye(2)[b[closing[t]]] if a is None else np.asarray(a, np.complex128) for t, a in enumerate(arrays)]
            got = np.einsum(*[x for a, xs in zip(leaves, ts_inds) for x in (a, [sym[i] for i in xs])], [sym[i] for i in output])
            want = psi[tuple(slice(None) if x == qs[0] else b[x] for x in range(n))]
            assert np.allclose(got, want, rtol=0, atol=1e-13), (g, others)
    assert drawn == 8


def test_classical_gates(smp):
    assert smp.classical_table(CZ) == (0, 1, 2, 3) and smp.classical_table(CNOT) == (0, 1, 3, 2)
    assert smp.classical_table(SWAP) == (0, 2, 1, 3) == smp.classical_table(ISWAP)
    for bad in (np.ones((4, 4)), CZ * 0.5, np.eye(3), np.zeros((4, 4)), np.eye(4)[:, :2], np.array([[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]])):
        assert smp.classical_table(bad) is None
    bits = np.array([[0, 1], [1, 0], [1, 1]], np.uint8)
    assert smp.tally(bits[[0, 1, 1, 2, 2, 2]]) == {"11": 0.5, "10": 2 / 6, "01": 1 / 6}
    assert list(smp.tally(bits[[0, 1, 1, 2, 2, 2]], normalize=False).items()) == [("11", 3), ("10", 2), ("01", 1)]


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_walkers_refusals(ctr, no_gpu):
    for bad in (0, -1, 1.0, "3", True, None):
        refusal(lambda: ctr.Walkers(bad, 3), ValueError, "'n_walkers' must be a positive integer.")
        refusal(lambda: ctr.Walkers(3, bad), ValueError, "'n_qubits' must be a positive integer.")
    refusal(lambda: ctr.Walkers(1 << 30, 1 << 11), ValueError, "'n_walkers' x 'n_qubits' must be 2^40 at the most.")
    for bad in (-1, 1 << 64, 0.5, "1", True, None):
        refusal(lambda: ctr.Walkers(3, 2, seed=bad), ValueError, "'seed' must be an integer from 0 to 2^64 - 1.")
    w = ctr.Walkers(3, 2, seed=(1 << 64) - 1, device=0)
    assert (w.n_walkers, w.n_qubits, w.seed, w.device) == (3, 2, (1 << 64) - 1, 0)
    for bad in (np.zeros((2, 3), np.uint8), np.zeros((3, 2), np.float32), np.zeros(6, np.uint8)):
        refusal(lambda: w.write(bad), ValueError, "'bits' must be an integer array of shape (3, 2).")
    refusal(lambda: w.write(np.full((3, 2), 2)), ValueError, "'bits' must hold zeros and ones only.")
    refusal(lambda: w.write(np.full((3, 2), -1)), ValueError, "'bits' must hold zeros and ones only.")
    for bad in ((), tuple(range(9))):
        refusal(lambda: w.permute(bad, (0, 1)), ValueError, "'qubits' must name 1 to 8 qubits.")
    for bad in (2, -1, 1.0, True):
        refusal(lambda: w.permute((0, bad), (0, 1, 2, 3)), ValueError, f"{bad!r} is not a qubit of the walkers (0 to 1).")
    refusal(lambda: w.permute((1, 1), (0, 1, 2, 3)), ValueError, "'qubits' names a qubit twice.")
    for bad in ((0, 1, 2), (0, 1, 2, 2), (0, 1, 2, 4), (0, 1, 2, 3, 4), (0, 1, 2, 3.0)):
        refusal(lambda: w.permute((0, 1), bad), ValueError, "'table' must be a permutation of 0 to 3.")
    w.close()
    w.close()
    for call in (lambda: w.bits, lambda: w.dead, w.reset, lambda: w.write(np.zeros((3, 2), np.uint8)), lambda: w.permute((0,), (1, 0))):
        refusal(call, ValueError, "the Walkers are closed.")


def test_contractor_refusals(ctr, no_gpu):
    import torch
    w = ctr.Walkers(4, 3, device=0)
    two = {1: np.zeros((2,) + CHAIN.shapes()[1], np.float32)}
    c = contractor(ctr)
    c.close()
    for call in (lambda: c.bind_versions(two), lambda: c.run_walkers(w, {1: 0}), lambda: c.choose(w, 0, 0), lambda: c.walker_outputs(w)):
        refusal(call, ValueError, "the Contractor is closed.")
    for name, call in (("bind_versions", lambda c: c.bind_versions(two)), ("run_walkers", lambda c: c.run_walkers(w, {1: 0})),
                       ("choose", lambda c: c.choose(w, 0, 0))):
        with contractor(ctr, path_kernel=None) as c:
            refusal(lambda: call(c), NotImplementedError, f"'{name}' needs a Contractor with 'path_kernel'.")
        with contractor(ctr, accumulate="float64") as c:
            refusal(lambda: call(c), NotImplementedError, f"'accumulate' is not supported with '{name}'.")
        with ctr.Contractor([], [("i", "s", "j")], [(5, 3, 7)], dtype=np.float32, slices=("s",), path_kernel=2) as c:
            refusal(lambda: call(c), NotImplementedError, f"'{name}' needs a plan with steps.")
    with contractor(ctr, device=0) as c:
        # bind_versions
        for bad in ({}, None, [two[1]]):
            refusal(lambda: c.bind_versions(bad), ValueError, "'versions' must be a dict {leaf number: array} with at least one leaf.")
        refusal(lambda: c.bind_versions({3: two[1]}), ValueError, "3 is not a leaf of the plan (0 to 2).")
        refusal(lambda: c.bind_versions({1: two[1][0]}), ValueError,
                "the versions of leaf 1 have the shape (7, 2, 6), not (2,) + the leaf's (7, 2, 6).")
        refusal(lambda: c.bind_versions({1: np.zeros((3,) + CHAIN.shapes()[1], np.float32)}), ValueError,
                "the versions of leaf 1 have the shape (3, 7, 2, 6), not (2,) + the leaf's (7, 2, 6).")
        refusal(lambda: c.bind_versions({1: two[1].astype(np.float64)}), TypeError, "an array of dtype float64 does not cast safely to float32.")
        refusal(lambda: c.bind_versions({1: torch.from_numpy(two[1])}), ValueError, "a tensor is on cpu, not on cuda:0.")
        # run_walkers
        for bad in (0, 1025, 2.0, True):
            refusal(lambda: c.run_walkers(w, {1: 0}, group=bad), ValueError, "'group' must be None or an integer from 1 to 1024.")
        refusal(lambda: c.run_walkers(None, {1: 0}), TypeError, "'walkers' must be a Walkers object, not NoneType.")
        refusal(lambda: c.run_walkers(ctr.Walkers(4, 3, device=1), {1: 0}), ValueError, "the walkers are on device 1, the Contractor on device 0.")
        refusal(lambda: c.run_walkers(w, [0]), ValueError, "'leaf_qubit' must be a dict {leaf number: qubit}.")
        refusal(lambda: c.run_walkers(w, {3: 0}), ValueError, "3 is not a leaf of the plan (0 to 2).")
        for bad in (3, -1, 1.0, True):
            refusal(lambda: c.run_walkers(w, {1: bad}), ValueError, f"{bad!r} is not a qubit of the walkers (0 to 2).")
        refusal(lambda: c.run_walkers(w, {1: 0}), ValueError, "leaf 1 has no versions: call bind_versions first.")
        c._versions = {1}  # (as after bind_versions)
        refusal(lambda: c.run_walkers(w, {1: 0}), ValueError, "leaf 0 is neither bound nor indexed by a qubit.")
        # choose: the plan's output holds 3 x 5 x 3 elements
        refusal(lambda: c.choose(None, 0, 0), TypeError, "'walkers' must be a Walkers object, not NoneType.")
        refusal(lambda: c.choose(w, 0, 0), ValueError, f"the output of the plan holds {c.plan.out_numel} elements, not the 2 amplitudes of a choice.")
        refusal(lambda: c.walker_outputs(w), ValueError, "the last run of the Contractor was not a 'run_walkers' over these walkers.")
    with ctr.Contractor([(0, 1)], [("a", "x"), ("a",)], [(2, 2), (2,)], ("x",), dtype=np.complex64, path_kernel=4, device=0) as c:
        for bad in (3, -1, 1.0, True):
            refusal(lambda: c.choose(w, bad, 0), ValueError, f"{bad!r} is not a qubit of the walkers (0 to 2).")
        for bad in (-1, 1 << 32, 1.0, True):
            refusal(lambda: c.choose(w, 0, bad), ValueError, "'step' must be an integer from 0 to 2^32 - 1.")
        refusal(lambda: c.choose(w, 0, 0), ValueError, "the last run of the Contractor was not a 'run_walkers' over these walkers.")
        w.close()
        refusal(lambda: c.choose(w, 0, 0), ValueError, "the Walkers are closed.")
        refusal(lambda: c.run_walkers(w, {1: 0}), ValueError, "the Walkers are closed.")


def test_sampler_refusals(smp, no_gpu):
    rng = np.random.RandomState(0)
    u = unitary(rng)
    toffoli_like = np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]]
    for bad in ([(np.ones((4, 4)) / 2, (0, 1))], [(u, (0,)), (CZ * 0.5, (0, 1))], [(np.kron(u, u), (0, 1))], [(CZ, (0, 1, 2))],
                [(np.ones((2, 3)), (0,))], [(toffoli_like, (0, 1))]):
        refusal(lambda: smp.Sampler(bad), ValueError, smp.GATES_ERROR)
    assert smp.GATES_ERROR == "Only 1-qubit operations and linear transformations (with or without phase change) are allowed."
    assert smp.ORDER_ERROR == "'qubit_order' is not consistent with qubits in 'circuit'."
    good = [(u, ("a",)), (CZ, ("a", "b"))]
    for bad in (("a",), ("a", "b", "c"), ("a", "c"), ("a", "b", "b")):
        refusal(lambda: smp.Sampler(good, qubit_order=bad), ValueError, smp.ORDER_ERROR)
    refusal(lambda: smp.Sampler([(CZ, ("a", "a"))]), ValueError, "a gate names a qubit twice.")
    refusal(lambda: smp.Sampler(good, max_width=10), NotImplementedError, "Sampling with finite width is not yet implemented.")
    refusal(lambda: smp.Sampler(good, slices=("x",)), NotImplementedError, "Sampling with finite width is not yet implemented.")
    refusal(lambda: smp.Sampler(good, dtype=np.float16), TypeError, "'dtype' must be one of float32, float64, complex64, complex128.")
    for bad in (0, 1025, 2.0, True):
        refusal(lambda: smp.Sampler(good, group=bad), ValueError, "'group' must be an integer from 1 to 1024.")
    refusal(lambda: smp.Sampler(good, seed=0.5), ValueError, "'seed' must be None or an integer.")
