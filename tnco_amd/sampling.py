"""Gate-by-gate sampling of bitstrings from a circuit on the device (S. Bravyi, D. Gosset, Y. Liu: "How to simulate
quantum measurement without computing marginals", Phys. Rev. Lett. 128, 220503 (2022)).

    sampler = Sampler(circuit, seed=0)              # circuit: an iterable of (matrix, qubits)
    hits, qubits = sampler.sample(4096)             # {bitstring: fraction of the samples}, the order of its qubits

Every sample is a walker: a bitstring that starts at 0...0 and follows the circuit gate by gate.  A classical gate -- the
non-zero entries of its matrix form a permutation and have modulus 1: CZ, CNOT, SWAP, iSWAP -- maps a bitstring to a
bitstring.  After a 1-qubit gate g on qubit q the walker draws q's bit anew, from the two amplitudes
<b with q = x | circuit[:g + 1] | 0...0>, x = 0, 1, of its own bitstring b.  Both come from one contraction of the partial
network of the gate (`partial_network`), whose only open index is q's last one.

The walkers are `contraction.Walkers`: their bits stay on the device from the first gate to the last.  Every 1-qubit gate
has a `contraction.Contractor` of its own, made and optimised once when the Sampler is made and held until close(), with
the gate tensors bound and every closing one-hot leaf bound as its two versions (1, 0), (0, 1).  A walk is then one
`Walkers.permute` per classical gate and one `Contractor.run_walkers` plus one `Contractor.choose` per 1-qubit gate, and a
single read of the bits at its end.

A part of that network that is not connected to q's index is a scalar factor of both amplitudes and cancels in the
choice: the Sampler contracts the component that holds q's index only.

With `max_gate_qubits=k` (2 to `contraction.MAX_CHOOSE_QUBITS`) a gate on at most k qubits that is not classical -- fSim, a
CPHASE with a generic angle, a fused pair of gates -- is a drawing gate too: after it the walker redraws the gate's bits
jointly, from the 2^k amplitudes of its bitstring with those bits open (`Contractor.choose_joint`).  Its partial network
keeps the last index of each of its qubits open; all of them are axes of the gate's tensor, so one component holds them.

Limits: one handle per gate that draws, all of them held at once; two versions per leaf, so qubits only; nothing is reused
between the networks of consecutive gates, each is contracted from the |0> vectors on; no slicing (`max_width`, `slices`).
"""
from __future__ import annotations

from random import Random

import numpy as np

from . import contraction
from .app import tn as tnmod

__all__ = ["Sampler", "classical_table", "partial_network", "connected_to", "tally", "GATES_ERROR", "ORDER_ERROR"]

GATES_ERROR = "Only 1-qubit operations and linear transformations (with or without phase change) are allowed."
ORDER_ERROR = "'qubit_order' is not consistent with qubits in 'circuit'."
ONE_HOT = ((1, 0), (0, 1))  # the two versions of a closing leaf


def classical_table(matrix):
    """The table of a classical gate, or None when `matrix` is not one: the matrix is 2^k x 2^k, every column and every
    row holds exactly one non-zero entry, and each of them has modulus 1; table[v] is the row of column v's entry, the
    basis state that the gate sends v to (a phase aside).  The first qubit of the gate is the most significant bit."""
    m = np.asarray(matrix)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2 or m.shape[0] & (m.shape[0] - 1):
        return None
    rows, cols = np.nonzero(m)
    n = m.shape[0]
    if len(rows) != n or sorted(rows) != list(range(n)) or sorted(cols) != list(range(n)):
        return None
    if not (np.abs(m[rows, cols]) == 1).all():
        return None
    table = [0] * n
    for r, c in zip(rows, cols):
        table[int(c)] = int(r)
    return tuple(table)


def partial_network(gates, g, n_qubits):
    """The network whose contraction gives a walker's 2^k amplitudes after gate g, a gate that draws on its k qubits qs
    (k = 1: the two amplitudes of a 1-qubit gate).

    gates: [(array of shape (2,) * 2k, positions of its k qubits)], axes (out_1 .. out_k, in_1 .. in_k).  Returns
    (ts_inds, arrays, output_inds, closing): the tensors are a |0> vector per qubit, the gates 0 .. g, and a closing leaf
    on the last index of every qubit but those of qs, in that order; `arrays` holds None for a closing leaf, which is
    (1, 0) or (0, 1) as the walker's bit says; `closing` is {leaf number: qubit}; output_inds are the last indices of qs,
    in the order of qs: all of them axes of gate g's tensor."""
    qs = tuple(gates[g][1])
    last = [f"q{x}_0" for x in range(n_qubits)]
    ts_inds = [(x,) for x in last]
    arrays = [np.array([1, 0]) for _ in range(n_qubits)]
    for pos in range(g + 1):
        array, at = gates[pos]
        new = [f"q{x}_{pos + 1}" for x in at]
        ts_inds.append(tuple(new) + tuple(last[x] for x in at))
        arrays.append(array)
        for x, name in zip(at, new):
            last[x] = name
    closing = {}
    for x in range(n_qubits):
        if x not in qs:
            closing[len(ts_inds)] = x
            ts_inds.append((last[x],))
            arrays.append(None)
    return ts_inds, arrays, tuple(last[x] for x in qs), closing


def connected_to(ts_inds, index) -> list:
    """The tensors of the connected component that holds `index`, in their order; for a tuple or list of indices, of the
    union of their components."""
    reached, found = set(index) if isinstance(index, (tuple, list)) else {index}, set()
    grown = True
    while grown:
        grown = False
        for t, xs in enumerate(ts_inds):
            if t not in found and reached & set(xs):
                found.add(t)
                reached |= set(xs)
                grown = True
    return sorted(found)


class Sampler:
    """Samples bitstrings from `circuit`, an iterable of (matrix, qubits): 1-qubit gates and classical gates (module
    docstring); anything else is a ValueError.  qubit_order: the qubits of the circuit in the order of the bitstrings
    (None: sorted by str).  dtype: of the contractions.  seed: of the optimisations and of the draws (None: from the
    system).  group: members per launch of the walkers' path kernel.  max_gate_qubits: with 2 to 6, a gate that is not
    classical on at most that many qubits is taken too and its bits are drawn jointly (its matrix must be 2^k x 2^k); the
    default, 1, refuses it as before.  optimize_params go to `Optimizer.optimize` for
    every partial network (betas, n_steps, n_runs default to (0, 100), 100, 8); a finite `max_width` or `slices` is
    not implemented.  The handles live until close(); the object is a context manager."""

    def __init__(self, circuit, *, qubit_order=None, dtype=np.complex64, seed=None, device=None, group=1024, max_gate_qubits=1,
                 **optimize_params):
        most = contraction.MAX_CHOOSE_QUBITS
        if isinstance(max_gate_qubits, bool) or not isinstance(max_gate_qubits, (int, np.integer)) or not 1 <= max_gate_qubits <= most:
            raise ValueError(f"'max_gate_qubits' must be an integer from 1 to {most}.")
        circuit = [(np.asarray(m), tuple(qs)) for m, qs in circuit]
        tables = [None if len(qs) == 1 else classical_table(m) for m, qs in circuit]
        for (m, qs), table in zip(circuit, tables):
            if len(qs) > 1 and table is None and len(qs) <= max_gate_qubits:  # a drawing gate of several qubits
                if m.shape != (1 << len(qs),) * 2:
                    raise ValueError(f"the matrix of a gate on {len(qs)} qubits must be {1 << len(qs)} x {1 << len(qs)}, not of shape "
                                     f"{m.shape}.")
                continue
            ok = m.shape == (2, 2) if len(qs) == 1 else (table is not None and len(table) == 1 << len(qs))
            if not ok:
                raise ValueError(GATES_ERROR)
        qubits = {x for _, qs in circuit for x in qs}
        if qubit_order is None:
            qubit_order = sorted(qubits, key=str)
        self.qubits = tuple(qubit_order)
        if set(self.qubits) != qubits or len(self.qubits) != len(qubits):
            raise ValueError(ORDER_ERROR)
        if any(len(set(qs)) != len(qs) for _, qs in circuit):
            raise ValueError("a gate names a qubit twice.")
        if any(len(qs) > contraction.MAX_PERMUTE_QUBITS for _, qs in circuit):
            raise NotImplementedError(f"a classical gate acts on {contraction.MAX_PERMUTE_QUBITS} qubits at the most.")
        if not self.qubits:
            raise ValueError("the circuit has no gates.")
        width = optimize_params.get("max_width")
        if (width is not None and width < float("inf")) or optimize_params.get("slices"):
            raise NotImplementedError("Sampling with finite width is not yet implemented.")
        optimize_params = {k: v for k, v in optimize_params.items() if k not in ("max_width", "slices")}
        self.dtype = np.dtype(dtype)
        if self.dtype not in contraction.DTYPES:
            raise TypeError(f"'dtype' must be one of {', '.join(d.name for d in contraction.DTYPES)}.")
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or not 1 <= group <= contraction.MAX_PATH_KERNEL:
            raise ValueError(f"'group' must be an integer from 1 to {contraction.MAX_PATH_KERNEL}.")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
            raise ValueError("'seed' must be None or an integer.")
        from . import parallel
        self.device = parallel.local_device() if device is None else int(device)
        self.group = int(group)
        self._rng = Random(None if seed is None else int(seed))
        at = {x: k for k, x in enumerate(self.qubits)}
        self.gates = [(m.reshape((2,) * (2 * len(qs))), tuple(at[x] for x in qs)) for m, qs in circuit]
        self.tables = tables
        self.contractors = {}  # {gate position: (Contractor, {leaf: qubit})} for the gates that draw
        self.open_inds = {}  # {gate position: the open index of each of the gate's qubits}
        self.last_walk_seed = None  # the seed of the walkers of the last sample()
        self._closed = False
        params = dict(dict(betas=(0, 100), n_steps=100, n_runs=8), **optimize_params)
        try:
            for g, table in enumerate(tables):
                if table is None:
                    self.contractors[g] = self._contractor(g, params)
        except Exception:
            self.close()
            raise

    def _contractor(self, g, params):
        from .app import Optimizer
        ts_inds, arrays, output, closing = partial_network(self.gates, g, len(self.qubits))
        # the components that do not hold an open index are scalars, factors of all amplitudes alike: they cancel in
        # p_v / s and are left out (the open indices are all axes of the gate's tensor: one component holds them)
        kept = connected_to(ts_inds, output[0] if len(output) == 1 else output)
        self.open_inds[g] = output
        closing = {k: closing[t] for k, t in enumerate(kept) if t in closing}
        ts_inds, arrays = [ts_inds[t] for t in kept], [arrays[t] for t in kept]
        seed = self._rng.randrange(2 ** 32)
        if len(ts_inds) > 2:
            tn0 = tnmod.TensorNetwork([tnmod.Tensor(xs, [2] * len(xs)) for xs in ts_inds], output_inds=output)
            tn, res = Optimizer(method="sa", seed=seed).optimize(tn0, fuse=None, decompose_hyper_inds=False, device=self.device, **params)
            if [tuple(xs) for xs in tn.ts_inds] != [tuple(xs) for xs in ts_inds]:
                raise RuntimeError("the optimizer changed the network.")
            path = min(res, key=lambda r: r.cost).path
        else:  # (|0> and the gate: nothing to optimise)
            path = [(0, 1)]
        c = contraction.Contractor(path, ts_inds, [(2,) * len(xs) for xs in ts_inds], output, dtype=self.dtype,
                                   path_kernel=self.group, device=self.device)
        try:
            c.bind({t: np.asarray(a).astype(self.dtype) for t, a in enumerate(arrays) if a is not None})
            if closing:
                c.bind_versions({t: np.array(ONE_HOT, self.dtype) for t in closing})
        except Exception:
            c.close()
            raise
        return c, closing

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        """Destroys every handle; closing twice is fine."""
        for c, _ in self.contractors.values():
            c.close()
        self._closed = True

    def _walk(self, walkers, stop_at_dead=False):
        """Walks the circuit; stop_at_dead: the position of the first gate that leaves a dead walker, or None."""
        for g, ((_, qs), table) in enumerate(zip(self.gates, self.tables)):
            if table is not None:
                walkers.permute(qs, table)
                continue
            c, closing = self.contractors[g]
            c.run_walkers(walkers, closing, group=self.group)
            if len(qs) == 1:
                c.choose(walkers, qs[0], g)
            else:
                c.choose_joint(walkers, qs, g, inds=self.open_inds[g])
            if stop_at_dead and walkers.dead.any():
                return g
        return None

    def sample(self, n_samples, normalize=True):
        """({bitstring: fraction of the samples, or their number with normalize=False}, sorted by hits, the most first;
        the qubits in the order of a bitstring's characters).  FloatingPointError when a walker met two amplitudes whose
        probabilities sum to 0 or to no finite number."""
        if self._closed:
            raise ValueError("the Sampler is closed.")
        if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
            raise ValueError("'n_samples' must be a positive integer.")
        seed = self.last_walk_seed = self._rng.randrange(2 ** 64)
        with contraction.Walkers(int(n_samples), len(self.qubits), seed=seed, device=self.device) as w:
            self._walk(w)
            bits, dead = w.bits, w.dead
            if dead.any():
                w.reset()
                g = self._walk(w, stop_at_dead=True)  # (the same seed, the same walk: which gate it was)
                names = tuple(self.qubits[x] for x in self.gates[g][1])
                gate = f"a 1-qubit gate on qubit {names[0]!r}" if len(names) == 1 else f"a {len(names)}-qubit gate on qubits {names!r}"
                raise FloatingPointError(f"{int(dead.sum())} of {n_samples} walkers met probabilities that sum to 0 or are not "
                                         f"finite, the first at gate {g} ({gate}).")
        self.last_bits = bits
        return tally(bits, normalize), self.qubits


def tally(bits, normalize=True) -> dict:
    """{bitstring: hits} of a table of bits [samples, qubits], the most hits first (ties in order of first appearance);
    normalize: hits as fractions of the samples."""
    hits = {}
    for row in bits:
        key = "".join(map(str, row.tolist()))
        hits[key] = hits.get(key, 0) + 1
    if normalize:
        hits = {k: v / len(bits) for k, v in hits.items()}
    return dict(sorted(hits.items(), key=lambda kv: kv[1], reverse=True))
