"""The real reference Tree's verdict (constructed and is_valid) on every tree of tests/tree_check_cases.py::families,
recorded as tests/golden/tree_check.json, so that tests/test_tree_check_model.py also runs where
oracle/_ref/libref_tree.so cannot be built (no reference checkout).  Per family: how many trees it has and the
indices of those the reference accepts -- data only, the trees come from the seeds and rules of tree_check_cases.py.
Run where the library can be built:

    python tests/golden/make_tree_check_golden.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import oracle as orc  # noqa: E402
from tests import tree_check_cases as tc  # noqa: E402
from tests.test_tree_check_model import real_reference_verdicts  # noqa: E402

orc.build()
ref = orc.ref_tree()
if ref is None:
    sys.exit("oracle/_ref/libref_tree.so is not built: the reference checkout is needed")
out = {}
for name, trees in tc.families().items():
    ok = real_reference_verdicts(ref, trees)
    out[name] = {"trees": len(trees), "accepted": [int(k) for k in ok.nonzero()[0]]}
Path(__file__).with_name("tree_check.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")
