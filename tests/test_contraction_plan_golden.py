"""The plans of every tabled case under every keyword setting against tests/golden/plans.json (written by
tests/golden/make_plan_golden.py): a change to `contraction.plan()` that means to leave the plans alone leaves every byte
of every table, every offset and every keyword field of the `Plan` as it was, and the refusals with their texts.

The tabled cases are those of tests/schedule_cases.py (which include tests/mode_cases.py), tests/projs_cases.py with
their projections, tests/reuse_cases.py, tests/hoist_cases.py, tests/indirect_cases.py (the chains and the one-step
table) and tests/path_cases.py.  No GPU."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests import hoist_cases as hc
from tests import indirect_cases as ic
from tests import path_cases as pc
from tests import projs_cases as jc
from tests import reuse_cases as rc
from tests import schedule_cases as sc
from tnco_amd import contraction as ctr

GOLDEN = Path(__file__).parent / "golden" / "plans.json"
SETTINGS = (
    dict(),
    dict(slice_batch=64),
    dict(path_kernel=1024),
    dict(hoist=True),
    dict(hoist=True, slice_batch=3),
    dict(reuse=True),
    dict(reuse=True, slice_order="reuse"),
    dict(indirect=True),
    dict(indirect=True, hoist=True),
    dict(indirect=True, reuse=True, slice_order="reuse"),
    dict(storage="bfloat16"),
    dict(storage="float16", scaling="tensor"),
    dict(storage="float16", scaling="tensor", hoist=True),
    dict(compute="bf16x3"),
    dict(compute="matrix"),
    dict(accumulate="float64"),
)
REFUSALS = (ValueError, TypeError, NotImplementedError)


def setting_id(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items()) or "none"


def _mode_case(c):
    return dict(path=list(c.path), ts_inds=c.ts_inds, shapes=c.shapes(), output_inds=c.output_inds, slices=c.slices,
                slice_range=c.slice_range, dtype=np.dtype(c.dtype))


def _projs_case(c):
    return dict(_mode_case(c), sparse_inds=c.sparse, projs=c.projs())


def _chain(c):
    return dict(path=list(pc.PATH), ts_inds=c.ts, shapes=c.shapes(), output_inds=c.output, slices=pc.SLICES,
                dtype=np.dtype(np.float32))


def cases():
    """{id: the arguments of plan() without the setting's keywords}, in the order of the tables."""
    out = {}
    for c, i in zip(sc.CASES, sc.IDS):
        out["schedule:" + i] = _mode_case(c)
    for c, i in zip(jc.CASES, jc.IDS):
        out["projs:" + i] = _projs_case(c)
    for name in rc.NAMES:
        out["reuse:" + name] = _mode_case(rc.case(name))
    for name in hc.NAMES:
        out["hoist:" + name] = _mode_case(hc.case(name))
    for name in ic.CHAINS:
        out["indirect:" + name] = _mode_case(ic.case(name))
    for name, fold in ic.ONE_STEP:
        out[f"indirect:{name}-{fold}"] = _mode_case(ic.case(name, fold))
    for c in pc.CASES:
        out["path:" + c.name] = _chain(c)
    return out


def digest(p):
    """sha256 over the sorted vars(plan): arrays by dtype, shape and bytes, everything else by its repr."""
    h = hashlib.sha256()
    for k, v in sorted(vars(p).items()):
        h.update(k.encode())
        if isinstance(v, np.ndarray):
            h.update(str(v.dtype).encode() + str(v.shape).encode() + v.tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()[:16]


def record(args, kw):
    """The 16 hex digits of the plan's digest, or "Type: text" of the refusal."""
    a = dict(args)
    try:
        return digest(ctr.plan(a.pop("path"), a.pop("ts_inds"), a.pop("shapes"), a.pop("output_inds"), **a, **kw))
    except REFUSALS as e:
        return f"{type(e).__name__}: {e}"


def records():
    """({case id: one record per setting, joined by blanks}, the refusal texts): a refusal is stored as "#k", the k-th text."""
    out, texts = {}, []
    for i, args in cases().items():
        row = [record(args, kw) for kw in SETTINGS]
        texts += [r for r in dict.fromkeys(row) if len(r) > 16 and r not in texts]
        out[i] = " ".join(f"#{texts.index(r)}" if len(r) > 16 else r for r in row)
    return out, texts


def _golden():
    g = json.loads(GOLDEN.read_text())
    plans = {i: [g["refusals"][int(r[1:])] if r[0] == "#" else r for r in row.split()] for i, row in g["plans"].items()}
    return g["settings"], plans


def test_the_golden_has_the_settings_and_the_cases_of_the_tables():
    settings, plans = _golden()
    assert settings == [setting_id(kw) for kw in SETTINGS]
    assert list(plans) == list(cases())
    assert all(len(row) == len(SETTINGS) for row in plans.values())


def test_every_plan_is_the_golden_plan():
    ids, plans = _golden()
    every = cases()
    differ = [f"{i} [{ids[k]}]: {now} != {then}" for i, row in plans.items() for k, then in enumerate(row)
              for now in [record(every[i], SETTINGS[k])] if now != then]
    assert not differ, "\n".join(differ[:40])


@pytest.mark.parametrize("kw", SETTINGS, ids=setting_id)
def test_every_setting_is_accepted_by_some_case_and_every_digest_is_16_hex_digits(kw):
    _, plans = _golden()
    column = [row[SETTINGS.index(kw)] for row in plans.values()]
    assert any(len(r) == 16 for r in column)
    assert all(len(r) == 16 and int(r, 16) >= 0 or r.startswith(("ValueError: ", "TypeError: ", "NotImplementedError: ")) for r in column)
