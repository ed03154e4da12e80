"""The model of the walkers' kernels (csrc/contract_walk.h), restated in numpy for tests/test_contraction_walk_plan.py,
tests/test_gpu_contract_walk.py and tests/test_gpu_sampler.py (no GPU here):

    philox4x32_10   the generator, from its published constants;
    uniforms        u of walker i at a step: 53 bits of the block's first two words;
    probability     |a|^2 in float64, parts widened exactly, one rounding per operation;
    choose          bit = (u (p0 + p1) < p1), dead where p0 + p1 is 0 or not finite;
    permute         a classical gate on a table of bits;
    select          the leaf that a walker's bit picks of two versions;
    model_walk      a float64 state-vector walk of a circuit with the same draws, and what every draw met.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the multipliers of Philox4x32
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key increments (golden ratio, sqrt(3) - 1)
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: uint array [..., 4]; key: (k0, k1).  Returns the block, uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(counter, np.uint64)[..., j] & np.uint64(MASK) for j in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: exact in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1)


def uniforms(seed, walkers, step):
    """u in [0, 1) of the walkers numbered `walkers` at draw `step`: key (seed lo, seed hi), counter (i lo, i hi, step, 0)."""
    i = np.asarray(walkers, np.uint64)
    counter = np.stack([i & np.uint64(MASK), i >> np.uint64(32), np.full_like(i, step), np.zeros_like(i)], axis=-1)
    x = philox4x32_10(counter, (seed & MASK, (seed >> 32) & MASK))
    hi, lo = (x[..., 0] >> np.uint64(5)).astype(np.float64), (x[..., 1] >> np.uint64(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) * 2.0 ** -53


def probability(a):
    """|a|^2 in float64 as the kernel rounds it: re re + im im, every product and the sum rounded once."""
    a = np.asarray(a)
    if a.dtype.kind == "c":
        re, im = a.real.astype(np.float64), a.imag.astype(np.float64)
        return re * re + im * im
    wide = a.astype(np.float64)
    return wide * wide


def choose(a0, a1, u):
    """(bits uint8, dead bool) of the walkers with amplitudes a0, a1 and uniforms u."""
    with np.errstate(all="ignore"):
        p0, p1 = probability(a0), probability(a1)
        s = p0 + p1
        alive = (s > 0) & (s < np.inf)
        bits = alive & (u * s < p1)
    return bits.astype(np.uint8), ~alive


def permute(bits, qubits, table):
    """The table of bits [walkers, qubits] after the classical gate: the first qubit is the most significant bit."""
    bits = np.array(bits, np.uint8)
    k = len(qubits)
    value = np.zeros(len(bits), np.int64)
    for q in qubits:
        value = 2 * value + bits[:, q]
    nxt = np.asarray(table, np.int64)[value]
    for j, q in enumerate(qubits):
        bits[:, q] = (nxt >> (k - 1 - j)) & 1
    return bits


def select(versions, bits, qubit):
    """The explicit stack of an indexed leaf: versions[bits[i, qubit]] for every walker i."""
    return np.asarray(versions)[np.asarray(bits)[:, qubit]]


def apply_gate(psi, matrix, qubits, n_qubits, absolute=False):
    """The state [2] * n_qubits after the gate (qubit 0 is axis 0); absolute: with the moduli of the matrix."""
    k = len(qubits)
    m = np.asarray(matrix, np.complex128).reshape((2,) * (2 * k))
    if absolute:
        m = np.abs(m).astype(np.float64)
    out = np.tensordot(m, psi, axes=(list(range(k, 2 * k)), list(qubits)))
    return np.moveaxis(out, list(range(k)), list(qubits))


def exact_distribution(circuit, n_qubits):
    """|<b|circuit|0>|^2 for every bitstring b, an array [2] * n_qubits."""
    psi = np.zeros((2,) * n_qubits, np.complex128)
    psi[(0,) * n_qubits] = 1
    for m, qs in circuit:
        psi = apply_gate(psi, m, qs, n_qubits)
    return np.abs(psi) ** 2


def model_walk(circuit, n_qubits, n_walkers, seed, is_classical):
    """The walk of n_walkers walkers over `circuit`, [(matrix, positions of its qubits)], in float64 with the draws of the
    kernel.  is_classical(matrix, qubits): the gate's table, or None for a gate that draws.  Returns (bits
    [walkers, qubits], records): a record per drawing gate, dict(g, qubit, u, a0, a1, mag0, mag1, dead) with the
    amplitudes that each walker met and the same sums over the moduli of every tensor (the magnitude that a rounding
    error bound of the contraction scales with)."""
    walkers = np.arange(n_walkers)
    bits = np.zeros((n_walkers, n_qubits), np.uint8)
    psi = np.zeros((2,) * n_qubits, np.complex128)
    psi[(0,) * n_qubits] = 1
    mag = np.abs(psi)
    records = []
    for g, (m, qs) in enumerate(circuit):
        psi, mag = apply_gate(psi, m, qs, n_qubits), apply_gate(mag, m, qs, n_qubits, absolute=True).real
        table = is_classical(m, qs)
        if table is not None:
            bits = permute(bits, qs, table)
            continue
        (q,) = qs
        at0, at1 = bits.copy(), bits.copy()
        at0[:, q], at1[:, q] = 0, 1
        a0, a1 = psi[tuple(at0.T)], psi[tuple(at1.T)]
        u = uniforms(seed, walkers, g)
        bits[:, q], dead = choose(a0, a1, u)
        records.append(dict(g=g, qubit=q, u=u, a0=a0, a1=a1, mag0=mag[tuple(at0.T)], mag1=mag[tuple(at1.T)], dead=dead))
    return bits, records


def bitstrings(bits):
    return ["".join(map(str, row.tolist())) for row in bits]
