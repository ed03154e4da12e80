"""A digest of the `Plan` of every tabled case under every keyword setting of tests/test_contraction_plan_golden.py,
recorded as tests/golden/plans.json: 16 hex digits of sha256 over the sorted vars(plan) per (case, setting), or "#k" for
the k-th entry of "refusals", the type and text of the exception.  Data only -- the cases come from the tables of
tests/*_cases.py.  Run it at a commit whose plans are the ones to keep, before contraction.plan() is touched:

    python tests/golden/make_plan_golden.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import test_contraction_plan_golden as pg  # noqa: E402

plans, refusals = pg.records()
out = {"settings": [pg.setting_id(kw) for kw in pg.SETTINGS], "refusals": refusals, "plans": plans}
text = json.dumps(out, separators=(",", ":")).replace('","', '",\n"') + "\n"
assert len(text) < 50_000, len(text)
pg.GOLDEN.write_text(text)
print(f"{len(out['plans'])} cases x {len(pg.SETTINGS)} settings, {len(text)} bytes")
