"""`sampling.Sampler` on the device against the float64 model walk with the same draws (tests/walk_cases.py).

Two circuits of random 1-qubit unitaries (rounded to complex64, so that model and device multiply the same numbers), CZ
and CNOT: 4 qubits with 12 gates, 6 qubits with 20; 4096 samples, complex64, fixed seeds.

A device amplitude differs from the model's by at most the engine's bound for its contraction,

    e = (c kt + 2) u (|A| |B| ...)       u = eps / 2 of float32, c = 2 (complex), kt = the sum of K over the plan's steps,

the product of moduli being the same walk over the moduli of the gates (walk_cases.model_walk, mag0 / mag1; the model sums
the whole partial network, the Sampler only the component of the measured qubit: the bound taken is the larger).  With
p = |a|^2 that moves p by at most 2 |a| e + e^2 and the threshold t = p1 / (p0 + p1) by at most

    delta = (p0 dp1 + p1 dp0) / (s (s - dp0 - dp1)) + 2^-50      (the last term: the float64 roundings of the choice)

A walker is undecided when one of its draws has |u - t| <= delta; every other walker's bitstring must be the model's.
The undecided are at most 1 % of the walkers: a condition on the seeds, not a measurement."""
import numpy as np
import pytest

from tests import walk_cases as wc

pytestmark = pytest.mark.gpu

N_SAMPLES = 4096
CZ = np.diag([1, 1, 1, -1]).astype(np.complex64)
CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], np.complex64)
CASES = {"4-qubits-12-gates": (4, 12, 21), "6-qubits-20-gates": (6, 20, 22)}  # qubits, gates, seed of the circuit


def random_circuit(n, n_gates, seed):
    rng = np.random.RandomState(seed)
    gates = []
    for q in range(n):  # a unitary on every qubit first: no bit is certain
        gates.append((unitary(rng), (q,)))
    while len(gates) < n_gates:
        kind = rng.randint(0, 4)
        if kind < 2:
            gates.append((unitary(rng), (int(rng.randint(0, n)),)))
        else:
            a, b = rng.choice(n, 2, replace=False)
            gates.append((CZ if kind == 2 else CNOT, (int(a), int(b))))
    return gates


def unitary(rng):
    q, r = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))
    return (q * (np.diag(r) / np.abs(np.diag(r)))).astype(np.complex64)


@pytest.fixture(scope="module")
def smp():
    from tnco_amd import sampling
    return sampling


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def sampled(request, smp):
    n, n_gates, seed = CASES[request.param]
    circuit = random_circuit(n, n_gates, seed)
    with smp.Sampler(circuit, seed=seed, n_steps=50, n_runs=4) as s:
        hits, qubits = s.sample(N_SAMPLES)
        yield dict(n=n, circuit=circuit, seed=seed, sampler=s, hits=hits, qubits=qubits, bits=s.last_bits, walk_seed=s.last_walk_seed)


def undecided(sampler, records):
    """[walkers] bool: a draw of the walker lies within delta of its threshold."""
    u32 = float(np.finfo(np.float32).eps) / 2
    out = np.zeros(len(records[0]["u"]), bool)
    for r in records:
        c, _closing = sampler.contractors[r["g"]]
        kt = int(np.asarray(c.plan.steps)[:, 13].sum())
        e0, e1 = ((2 * kt + 2) * u32 * r[k] for k in ("mag0", "mag1"))
        p0, p1 = np.abs(r["a0"]) ** 2, np.abs(r["a1"]) ** 2
        dp0, dp1 = 2 * np.abs(r["a0"]) * e0 + e0 ** 2, 2 * np.abs(r["a1"]) * e1 + e1 ** 2
        s = p0 + p1
        delta = (p0 * dp1 + p1 * dp0) / (s * np.maximum(s - dp0 - dp1, 1e-300)) + 2.0 ** -50
        out |= np.abs(r["u"] - p1 / s) <= delta
    return out


def test_decided_walkers_follow_the_model(sampled, smp):
    is_classical = lambda m, qs: None if len(qs) == 1 else smp.classical_table(m)  # noqa: E731
    want, records = wc.model_walk(sampled["circuit"], sampled["n"], N_SAMPLES, sampled["walk_seed"], is_classical)
    assert len(records) == sum(len(qs) == 1 for _, qs in sampled["circuit"]) == len(sampled["sampler"].contractors)
    assert not any(r["dead"].any() for r in records)
    open_ = undecided(sampled["sampler"], records)
    share = float(open_.mean())
    differ = (sampled["bits"] != want).any(axis=1)
    print(f"undecided walkers: {share:.4%}; walkers that differ from the model: {int(differ.sum())}, decided ones among them "
          f"{int((differ & ~open_).sum())}")
    assert share <= 0.01
    assert not (differ & ~open_).any()
    assert sampled["bits"].shape == (N_SAMPLES, sampled["n"]) and len(set(wc.bitstrings(sampled["bits"]))) > 2


def test_the_dict_is_the_tally_of_the_devices_bits(sampled, smp):
    hits, s = sampled["hits"], sampled["sampler"]
    assert sampled["qubits"] == tuple(range(sampled["n"]))
    strings = wc.bitstrings(sampled["bits"])
    counts = {}
    for b in strings:
        counts[b] = counts.get(b, 0) + 1
    assert hits == {b: k / N_SAMPLES for b, k in counts.items()} and abs(sum(hits.values()) - 1) < 1e-12
    assert list(hits.values()) == sorted(hits.values(), reverse=True)
    assert list(hits) == [b for b, _ in sorted(counts.items(), key=lambda kv: kv[1], reverse=True)]  # (ties: first seen first)
    raw, _ = s.sample(N_SAMPLES, normalize=False)
    assert raw == smp.tally(s.last_bits, normalize=False) and sum(raw.values()) == N_SAMPLES
    assert all(isinstance(k, int) for k in raw.values()) and list(raw.values()) == sorted(raw.values(), reverse=True)


def test_the_same_seed_gives_the_same_dict(smp):
    circuit = random_circuit(3, 7, 23)
    runs = []
    for seed in (5, 5, 6):
        with smp.Sampler(circuit, seed=seed, n_steps=50, n_runs=4) as s:
            runs.append((s.sample(512), s.last_walk_seed))
    assert runs[0] == runs[1] and list(runs[0][0][0]) == list(runs[1][0][0])
    assert runs[2][1] != runs[0][1] and runs[2][0][0] != runs[0][0][0]  # (another seed: other draws)


def test_a_dead_walker_raises_and_names_the_gate(smp):
    """A singular 1-qubit matrix that sends |0> to 0: both amplitudes of every walker are 0 at that gate."""
    rng = np.random.RandomState(2)
    kills_zero = np.array([[0, 1], [0, 0]], np.complex64)
    circuit = [(unitary(rng), ("a",)), (unitary(rng), ("b",)), (CZ, ("a", "b")), (unitary(rng), ("a",)), (kills_zero, ("c",)),
               (unitary(rng), ("b",))]
    with smp.Sampler(circuit, seed=4, n_steps=50, n_runs=4) as s:
        with pytest.raises(FloatingPointError) as e:
            s.sample(64)
        assert str(e.value) == ("64 of 64 walkers met probabilities that sum to 0 or are not finite, the first at gate 4 "
                                "(a 1-qubit gate on qubit 'c').")


def test_the_two_value_errors(smp):
    u = unitary(np.random.RandomState(1))
    with pytest.raises(ValueError) as e:
        smp.Sampler([(u, (0,)), (np.kron(u, u), (0, 1))])
    assert str(e.value) == "Only 1-qubit operations and linear transformations (with or without phase change) are allowed."
    with pytest.raises(ValueError) as e:
        smp.Sampler([(u, (0,)), (CZ, (0, 1))], qubit_order=(0, 2))
    assert str(e.value) == "'qubit_order' is not consistent with qubits in 'circuit'."


def test_classical_gates_only_give_the_one_permuted_bitstring(smp):
    X = np.array([[0, 1], [1, 0]], np.complex64)
    swap = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.complex64)
    x2 = np.kron(X, np.eye(2)).astype(np.complex64)  # X on the first qubit of a pair, as a classical 2-qubit gate
    circuit = [(x2, ("a", "b")), (CNOT, ("a", "c")), (swap, ("b", "d")), (CZ, ("c", "d")), (x2, ("d", "a"))]
    with smp.Sampler(circuit, qubit_order=("d", "c", "b", "a"), seed=3) as s:
        assert not s.contractors
        hits, qubits = s.sample(100, normalize=False)
    # a = 1; c ^= a -> 1; b <-> d: nothing; d = 1 at the end
    assert qubits == ("d", "c", "b", "a") and hits == {"1101": 100}
