"""The model of the joint draw (csrc/contract_walk.h, ct_walk_choose_joint_kernel), restated in numpy for
tests/test_contraction_walk_joint_plan.py, tests/test_gpu_contract_walk_joint.py and tests/test_gpu_sampler_joint.py (no
GPU here); the generator, the uniforms, |a|^2 and the classical gates are those of tests/walk_cases.py:

    tails             tail(v) = p_v + ... + p_{N-1}, summed from the top in float64, one rounding per addition;
    choose_joint      the outcome of every walker: the largest v >= 1 with u tail(0) < tail(v), or 0; dead where tail(0) is 0
                      or not finite;
    outcome_bits      the k bits of an outcome, the first qubit the most significant;
    model_walk_joint  walk_cases.model_walk with drawing gates of k qubits: all N amplitudes and moduli sums per record.

Two consequences of the rule: an outcome v >= 1 with p_v = 0 is never drawn, because tail(v) = tail(v + 1) and v + 1 (or
nothing) is then the largest; outcome 0 with p_0 = 0 is drawn only where u s rounds up to s = tail(1), as bit 0 is at k = 1
(u <= 1 - 2^-53 moves a normal s by more than half an ulp: only a subnormal s is reached).
"""
from __future__ import annotations

import numpy as np

from tests import walk_cases as wc


def tails(amplitudes):
    """[walkers, N] float64: tail(N - 1) = p_{N-1}, tail(v) = tail(v + 1) + p_v."""
    p = wc.probability(np.asarray(amplitudes))
    out = np.empty(p.shape, np.float64)
    out[:, -1] = p[:, -1]
    for v in range(p.shape[1] - 2, -1, -1):
        out[:, v] = out[:, v + 1] + p[:, v]
    return out


def choose_joint(amplitudes, u):
    """(outcomes int64, dead bool) of the walkers with amplitudes [walkers, N], N = 2^k, and uniforms u."""
    with np.errstate(all="ignore"):
        tail = tails(amplitudes)
        s = tail[:, 0]
        alive = (s > 0) & (s < np.inf)
        t = u * s
        outcome = np.zeros(len(s), np.int64)
        for v in range(1, tail.shape[1]):  # ascending: the last hit is the largest
            outcome = np.where(t < tail[:, v], v, outcome)
    return np.where(alive, outcome, 0), ~alive


def outcome_bits(outcomes, k):
    """uint8 [walkers, k]: bit j of an outcome is (v >> (k - 1 - j)) & 1."""
    v = np.asarray(outcomes, np.int64)
    return np.stack([(v >> (k - 1 - j)) & 1 for j in range(k)], axis=1).astype(np.uint8)


def model_walk_joint(circuit, n_qubits, n_walkers, seed, is_classical):
    """walk_cases.model_walk where a gate that draws may act on k qubits.  Returns (bits [walkers, qubits], records): a
    record per drawing gate, dict(g, qubits, u, a, mag, dead); a[walker, v] is the amplitude of outcome v of the gate's
    qubits (the first the most significant bit) with the walker's other bits, mag the same sum over the moduli of every
    tensor."""
    walkers = np.arange(n_walkers)
    bits = np.zeros((n_walkers, n_qubits), np.uint8)
    psi = np.zeros((2,) * n_qubits, np.complex128)
    psi[(0,) * n_qubits] = 1
    mag = np.abs(psi)
    records = []
    for g, (m, qs) in enumerate(circuit):
        psi, mag = wc.apply_gate(psi, m, qs, n_qubits), wc.apply_gate(mag, m, qs, n_qubits, absolute=True).real
        table = is_classical(m, qs)
        if table is not None:
            bits = wc.permute(bits, qs, table)
            continue
        k = len(qs)
        a, size = np.empty((n_walkers, 1 << k), np.complex128), np.empty((n_walkers, 1 << k), np.float64)
        for v in range(1 << k):
            at = bits.copy()
            at[:, list(qs)] = outcome_bits(np.full(n_walkers, v), k)
            a[:, v], size[:, v] = psi[tuple(at.T)], mag[tuple(at.T)]
        u = wc.uniforms(seed, walkers, g)
        outcomes, dead = choose_joint(a, u)
        bits[:, list(qs)] = outcome_bits(outcomes, k)
        records.append(dict(g=g, qubits=tuple(qs), u=u, a=a, mag=size, dead=dead))
    return bits, records
