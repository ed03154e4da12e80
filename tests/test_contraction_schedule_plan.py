"""The case table of the schedule tests (tests/schedule_cases.py) on the CPU: the table reaches every item of
`schedule_cases.REQUIRED_SCHEDULE` in a real and in a complex dtype -- asserted item by item, so that an edit of the table
cannot lose one silently -- every EXTRA case is within the caps of tests/mode_cases.py, distinct, and needed: without it
an item is lost.

The bound of tests/test_gpu_contract_schedules.py is `mode_cases.plain_bound`; that a correct contraction meets it on the
EXTRA cases too is shown here without a device, as tests/test_contraction_modes_plan.py shows it for `mode_cases.CASES`:
the plan's tables are replayed by the numpy interpreter of tests/test_contraction_plan.py in the case's own dtype and
held to it against numpy's einsum in float64 / complex128 -- and, for every case with a tiled-class step, in each of the
four dtypes that the device test runs `compute="matrix"` in.  (The EXTRA plans under `hoist=True`, `reuse=True` and
`indirect=True` are replayed on a NaN-poisoned arena by the interpreters of those features' own plan tests, whose lists
hold the EXTRA cases.)"""
import numpy as np
import pytest

from tests import mode_cases as mc
from tests import schedule_cases as sc
from tests.test_contraction_plan import _interpret

EXTRA_IDS = [f"{c.name}-{c.dtype}" for c in sc.EXTRA]
TILED = [c for c in sc.CASES if sc.tiled_steps(c.plan())]


def _reached(cases):
    got = {}
    for c in cases:
        for item in sc.coverage(c):
            got.setdefault(item, []).append(f"{c.name}-{c.dtype}")
    return got


def _by_kind(cases):
    return {kind: _reached(c for c in cases if np.dtype(c.dtype).kind == kind) for kind in "fc"}


REACHED = _by_kind(sc.CASES)


@pytest.mark.parametrize("item", sc.REQUIRED_SCHEDULE)
def test_the_table_reaches(item):
    assert item in REACHED["f"], f"no case of a real dtype reaches '{item}'"
    assert item in REACHED["c"], f"no case of a complex dtype reaches '{item}'"


def test_the_items_are_distinct_and_the_old_table_leaves_some_open():
    assert len(set(sc.REQUIRED_SCHEDULE)) == len(sc.REQUIRED_SCHEDULE)
    old = _by_kind(mc.CASES)
    missing = [(item, kind) for item in sc.REQUIRED_SCHEDULE for kind in "fc" if item not in old[kind]]
    assert missing, "mode_cases.CASES reaches everything: EXTRA is not needed"
    print(f"mode_cases.CASES leaves open: {missing}")


def test_the_extra_cases_are_few_distinct_and_within_the_caps():
    assert sc.CASES == mc.CASES + sc.EXTRA and 0 < len(sc.EXTRA) <= sc.MAX_EXTRA
    assert len(set(sc.IDS)) == len(sc.IDS)
    assert len({(c.ts_inds, c.dims, c.path, c.slices) for c in sc.CASES}) == len(sc.CASES)
    for row, c in zip(sc.EXTRA_TABLE, sc.EXTRA):
        assert c is not None and mc.caps(c) == [], (c.name, mc.caps(c))
        assert len(c.slices) <= sc.MAX_SLICED, c.name
        assert sc.make(*row) == c  # (the generator is deterministic)


@pytest.mark.parametrize("case", sc.EXTRA, ids=EXTRA_IDS)
def test_an_extra_case_is_needed(case):
    """Without the case, some item is no longer reached in some kind of dtype."""
    rest = _by_kind([c for c in sc.CASES if c != case])
    lost = [(item, kind) for item in sc.REQUIRED_SCHEDULE for kind in "fc" if item not in rest[kind]]
    assert lost, f"{case.name}: every item is reached without it"
    print(f"{case.name} {case.dtype}: alone in reaching {lost}")


def test_every_order_plans_and_the_device_test_skips_nothing_it_needs():
    """What tests/test_gpu_contract_schedules.py decides from the plan: the orders of the sliced indices are at most
    three per case, and the table has cases on both sides of each decision."""
    for c in sc.CASES:
        P = sc.Plans(c)
        orders = {p.slice_inds for p in P.reuse.values()}
        assert 1 <= len(orders) <= 3 and P.reuse[None].slice_inds == P.plain.slice_inds
        assert set(P.reuse["reversed"].slice_inds) == set(P.plain.slice_inds)
    assert TILED and len(TILED) < len(sc.CASES)
    assert any(sc.Plans(c).indirect.indirect == 0 for c in sc.CASES) and any(sc.Plans(c).indirect.indirect for c in sc.CASES)
    assert any(sc.Plans(c).hoist.hoisted == (0, 0) for c in sc.CASES)


def _replay_inside_the_bound(case):
    p, arrays = case.plan(), mc.fill(case)
    ref, mag = mc.reference(case, p, arrays)
    got = _interpret(p, arrays)
    assert got.dtype == np.dtype(case.dtype) and got.shape == ref.shape == p.shape
    err, bound = np.abs(got.astype(ref.dtype) - ref), mc.plain_bound(case, p, mag)
    print(f"{case.name} {case.dtype}: replay, largest error / bound {float((err / bound).max()):.4f} (kt {mc.kt(p)})")
    assert np.isfinite(got).all() and (bound > 0).all() and (err <= bound).all()


@pytest.mark.parametrize("case", sc.EXTRA, ids=EXTRA_IDS)
def test_the_replay_in_the_case_dtype_is_inside_the_plain_bound(case):
    _replay_inside_the_bound(case)


# (a case's own dtype is held above or in tests/test_contraction_modes_plan.py)
OTHER_DTYPES = [pytest.param(c, d, id=f"{c.name}-{d}") for c in TILED for d in sc.DTYPES if d != c.dtype]


@pytest.mark.parametrize("case,dtype", OTHER_DTYPES)
def test_the_replay_of_a_case_with_a_tiled_step_is_inside_the_plain_bound_in_every_dtype(case, dtype):
    _replay_inside_the_bound(case.with_(dtype=dtype))
