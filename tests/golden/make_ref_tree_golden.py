"""The real reference Tree's swap_with_nn / is_valid over the fixed sequence of
tests/test_oracle.py::test_rotation_and_validity_against_reference_tree, recorded as
tests/golden/ref_tree.json, so that the test also runs where oracle/_ref/libref_tree.so cannot be
built (no reference checkout).  Run where it can:

    python tests/golden/make_ref_tree_golden.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import oracle as orc  # noqa: E402
from tests.test_oracle import reference_tree_run  # noqa: E402

orc.build()
ref = orc.ref_tree()
if ref is None:
    sys.exit("oracle/_ref/libref_tree.so is not built: the reference checkout is needed")
out = reference_tree_run(ref.ref_tree_swap_with_nn, lambda *a: ref.ref_tree_is_valid(*a) == 1)
Path(__file__).with_name("ref_tree.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")
