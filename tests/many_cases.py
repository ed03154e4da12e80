"""The cases of the leaf-set tests (tests/test_contraction_many_plan.py, tests/test_gpu_contract_many.py):
`Contractor.run_many` over the three-tensor chains of tests/path_cases.py and tests/batch_cases.py,

    A (p, u, i, k)   B (k, t, j)   C (t, u, j, l)   ->   (p, i, l)         sliced over p (3), u (2), t (2): 12 assignments

B is the leaf a permute row gathers at a slice offset, A and C are step operands read in place at one.

A member of a launch is a pair (set, assignment), numbered set-major: with slice_range = (lo, hi) and A = hi - lo,
member m = i A + (a - lo).  `schedule` is the numpy model of the launches: consecutive members, `group` per launch, the
last one partial.  With A = 12 the groups of GROUPS cut the sets everywhere: 1 (every member alone), 5 (a launch ends
inside a set), 12 (exactly at its end), 13 (one member into the next set), 1024 (all members in one launch).
"""
from __future__ import annotations

import numpy as np

from tests import path_cases as pc

PATH, SLICES, N_ASSIGNMENTS, DTYPES = pc.PATH, pc.SLICES, pc.N_ASSIGNMENTS, pc.DTYPES
GROUPS = (1, 5, 12, 13, 1024)
SETS = (1, 2, 5)
STACKED = ((0,), (1,), (2,), (0, 1, 2))  # the leaves given as stacks: A, B, C alone, all three
MEMORY_CAP = 70 * 10 ** 6  # device bytes a run of these tests may hold (the cards are shared)


def member(m: int, lo: int, hi: int) -> tuple:
    """(set, assignment) of member m."""
    return m // (hi - lo), lo + m % (hi - lo)


def schedule(R: int, lo: int, hi: int, group: int) -> list:
    """[(first member, count)] of the launches of R sets over the assignments [lo, hi)."""
    members = R * (hi - lo)
    g = min(group, members)
    return [(m0, min(g, members - m0)) for m0 in range(0, members, g)]


def fill_sets(chain, dtype, R: int, seed: int) -> list:
    """R leaf sets of the chain, path_cases.fill with a different seed per set: [set][leaf]."""
    return [pc.fill(chain, dtype, seed + 1000 * i) for i in range(R)]


def stack(sets, t: int) -> np.ndarray:
    """Leaf t of every set along a leading axis."""
    return np.stack([leaves[t] for leaves in sets])


assert schedule(2, 0, 12, 5) == [(0, 5), (5, 5), (10, 5), (15, 5), (20, 4)]
assert schedule(2, 0, 12, 13) == [(0, 13), (13, 11)] and schedule(5, 0, 12, 1024) == [(0, 60)]
assert [member(m, 1, 11) for m in (0, 9, 10, 19)] == [(0, 1), (0, 10), (1, 1), (1, 10)]
