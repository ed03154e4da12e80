"""`sampling.Sampler(max_gate_qubits=3)` on the device against the float64 model walk with the same draws
(tests/walk_joint_cases.py, model_walk_joint); the method is that of tests/test_gpu_sampler.py.

Two circuits of random unitaries (rounded to complex64, so that model and device multiply the same numbers) on 1, 2 and 3
qubits and CZ: 3 qubits with 7 gates (4 x 4, 4 x 4, 1-qubit, CZ after the first layer), 5 qubits with 14, one of them
a random 8 x 8 unitary on 3 qubits early in the circuit, where the moduli sums are still small; 4096 samples, complex64,
fixed seeds.

A device amplitude differs from the model's by at most the engine's bound for its contraction,

    e_v = (c kt + 2) u mag_v             u = eps / 2 of float32, c = 2 (complex), kt = the sum of K over the plan's steps,

mag_v being the same walk over the moduli of the gates.  With p = |a|^2 that moves p_v by at most dp_v = 2 |a_v| e_v + e_v^2.
Outcome v >= 1 is decided by the threshold T_v = tail(v) / s.  With H = tail(v), L = s - H, and dH, dL the sums of dp over
the outcomes of the tail and over the others, T_v moves by at most

    delta_v = (L dH + H dL) / (s (s - dH - dL)) + 2^-50          (the last term: the float64 roundings of the draw)

which at k = 1 is the delta of tests/test_gpu_sampler.py.  A walker is undecided when one of its draws has
|u - T_v| <= delta_v for some v >= 1; every other walker's bitstring must be the model's.  The undecided are at most 1 % of
the walkers: a condition on the seeds, not a measurement.  The seeds were chosen with the model alone and a stand-in for
kt that is far too large, 64 x the tensors of the gate's partial network: the share of undecided walkers was then 0.2686 %
(3 qubits) and 0.3906 % (5 qubits), below 0.5 %."""
from random import Random

import numpy as np
import pytest

from tests import walk_cases as wc
from tests import walk_joint_cases as wj

pytestmark = pytest.mark.gpu

N_SAMPLES = 4096
CZ = np.diag([1, 1, 1, -1]).astype(np.complex64)
CASES = {"3-qubits-7-gates": (3, 7, 22, None), "5-qubits-14-gates": (5, 14, 29, 6)}  # qubits, gates, seed, where the 8 x 8 stands


def unitary(rng, n=2):
    q, r = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return (q * (np.diag(r) / np.abs(np.diag(r)))).astype(np.complex64)


def random_circuit(n, n_gates, seed, three_at=None):
    rng = np.random.RandomState(seed)
    gates = [(unitary(rng), (q,)) for q in range(n)]  # a unitary on every qubit first: no bit is certain
    while len(gates) < n_gates:
        if len(gates) == three_at:
            gates.append((unitary(rng, 8), tuple(int(q) for q in rng.choice(n, 3, replace=False))))
            continue
        kind = rng.randint(0, 4)
        if kind == 0:
            gates.append((unitary(rng), (int(rng.randint(0, n)),)))
        else:
            pair = tuple(int(q) for q in rng.choice(n, 2, replace=False))
            gates.append((CZ, pair) if kind >= 2 else (unitary(rng, 4), pair))
    return gates


def walk_seed_of(circuit, seed, is_classical):
    """The seed of the walkers of a fresh Sampler's first sample(): its generator gives a seed to every gate that draws,
    then this one."""
    rng = Random(seed)
    for m, qs in circuit:
        if is_classical(m, qs) is None:
            rng.randrange(2 ** 32)
    return rng.randrange(2 ** 64)


def undecided(records, kt_of):
    """[walkers] bool: a draw of the walker lies within delta_v of a threshold T_v (module docstring); kt_of(record)."""
    u32 = float(np.finfo(np.float32).eps) / 2
    out = np.zeros(len(records[0]["u"]), bool)
    for r in records:
        e = (2 * kt_of(r) + 2) * u32 * r["mag"]
        size = np.abs(r["a"])
        p, dp = size ** 2, 2 * size * e + e ** 2
        s, ds = p.sum(axis=1), dp.sum(axis=1)
        for v in range(1, p.shape[1]):
            H, dH = p[:, v:].sum(axis=1), dp[:, v:].sum(axis=1)
            delta = ((s - H) * dH + H * (ds - dH)) / (s * np.maximum(s - ds, 1e-300)) + 2.0 ** -50
            out |= np.abs(r["u"] - H / s) <= delta
    return out


@pytest.fixture(scope="module")
def smp():
    from tnco_amd import sampling
    return sampling


def classical(smp):
    return lambda m, qs: None if len(qs) == 1 else smp.classical_table(m)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def sampled(request, smp):
    n, n_gates, seed, three_at = CASES[request.param]
    circuit = random_circuit(n, n_gates, seed, three_at)
    with smp.Sampler(circuit, seed=seed, n_steps=50, n_runs=4, max_gate_qubits=3) as s:
        hits, qubits = s.sample(N_SAMPLES)
        yield dict(n=n, circuit=circuit, seed=seed, sampler=s, hits=hits, qubits=qubits, bits=s.last_bits, walk_seed=s.last_walk_seed)


def test_the_circuits_hold_what_they_should():
    for n, n_gates, seed, three_at in CASES.values():
        circuit = random_circuit(n, n_gates, seed, three_at)
        sizes = [np.asarray(m).shape[0] for m, _ in circuit]
        assert len(circuit) == n_gates and sizes.count(8) == (three_at is not None)
        kinds = {"cz" if m is CZ else f"u{m.shape[0]}" for m, _ in circuit[n:]}
        assert {"cz", "u2", "u4"} <= kinds, kinds


def test_decided_walkers_follow_the_model(sampled, smp):
    s, circuit = sampled["sampler"], sampled["circuit"]
    assert sampled["walk_seed"] == walk_seed_of(circuit, sampled["seed"], classical(smp))
    want, records = wj.model_walk_joint(circuit, sampled["n"], N_SAMPLES, sampled["walk_seed"], classical(smp))
    assert len(records) == sum(m is not CZ for m, _ in circuit) == len(s.contractors)
    assert sorted({len(r["qubits"]) for r in records}) == ([1, 2, 3] if sampled["n"] == 5 else [1, 2])
    assert not any(r["dead"].any() for r in records)
    for r in records:  # a gate of several qubits is one run_walkers and one joint draw: its plan's output holds 2^k elements
        assert s.contractors[r["g"]][0].plan.out_numel == 1 << len(r["qubits"])
    open_ = undecided(records, lambda r: int(np.asarray(s.contractors[r["g"]][0].plan.steps)[:, 13].sum()))
    share = float(open_.mean())
    differ = (sampled["bits"] != want).any(axis=1)
    print(f"undecided walkers: {share:.4%}; walkers that differ from the model: {int(differ.sum())}, decided ones among them "
          f"{int((differ & ~open_).sum())}")
    assert share <= 0.01
    assert not (differ & ~open_).any()
    assert sampled["bits"].shape == (N_SAMPLES, sampled["n"]) and len(set(wc.bitstrings(sampled["bits"]))) > 2


def test_the_dict_is_the_tally_of_the_devices_bits(sampled, smp):
    hits = sampled["hits"]
    assert sampled["qubits"] == tuple(range(sampled["n"]))
    counts = {}
    for b in wc.bitstrings(sampled["bits"]):
        counts[b] = counts.get(b, 0) + 1
    assert hits == {b: k / N_SAMPLES for b, k in counts.items()} and abs(sum(hits.values()) - 1) < 1e-12
    assert list(hits) == [b for b, _ in sorted(counts.items(), key=lambda kv: kv[1], reverse=True)]  # (ties: first seen first)
    assert hits == smp.tally(sampled["bits"])


def test_the_same_seed_gives_the_same_dict(smp):
    circuit = random_circuit(3, 7, 22)
    runs = []
    for seed in (5, 5, 6):
        with smp.Sampler(circuit, seed=seed, n_steps=50, n_runs=4, max_gate_qubits=2) as s:
            runs.append((s.sample(512), s.last_walk_seed))
    assert runs[0] == runs[1] and list(runs[0][0][0]) == list(runs[1][0][0])
    assert runs[2][1] != runs[0][1] and runs[2][0][0] != runs[0][0][0]  # (another seed: other draws)


def test_a_dead_walker_raises_and_names_the_gate_of_two_qubits(smp):
    """A singular 4 x 4 matrix that sends |00> to 0, on two fresh qubits: all four amplitudes of every walker are 0 there."""
    rng = np.random.RandomState(2)
    kills_zero = np.zeros((4, 4), np.complex64)
    kills_zero[0, 1] = kills_zero[1, 2] = kills_zero[2, 3] = 1
    circuit = [(unitary(rng), ("a",)), (unitary(rng), ("b",)), (unitary(rng, 4), ("a", "b")), (unitary(rng), ("a",)),
               (kills_zero, ("c", "d")), (unitary(rng), ("b",))]
    with smp.Sampler(circuit, seed=4, n_steps=50, n_runs=4, max_gate_qubits=2) as s:
        with pytest.raises(FloatingPointError) as e:
            s.sample(64)
        assert str(e.value) == ("64 of 64 walkers met probabilities that sum to 0 or are not finite, the first at gate 4 "
                                "(a 2-qubit gate on qubits ('c', 'd')).")
    with pytest.raises(ValueError) as e:  # the default refuses the circuit as it did
        smp.Sampler(circuit, seed=4, n_steps=50, n_runs=4)
    assert str(e.value) == smp.GATES_ERROR


def test_one_qubit_and_classical_gates_give_the_bits_of_the_default(smp):
    rng = np.random.RandomState(7)
    cnot = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], np.complex64)
    circuit = [(unitary(rng), (q,)) for q in range(3)] + [(CZ, (0, 1)), (unitary(rng), (1,)), (cnot, (2, 0)), (unitary(rng), (0,)),
                                                          (unitary(rng), (2,))]
    got = []
    for kw in ({}, {"max_gate_qubits": 2}):
        with smp.Sampler(circuit, seed=9, n_steps=50, n_runs=4, **kw) as s:
            hits, _ = s.sample(1024)
            got.append((s.last_bits, s.last_walk_seed, hits))
    assert got[0][1] == got[1][1] and np.array_equal(got[0][0], got[1][0]) and got[0][0].dtype == got[1][0].dtype
    assert got[0][2] == got[1][2] and len(got[0][2]) > 2
