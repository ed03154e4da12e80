"""Writes profiles/contract_range.txt on one GPU: what the number-range tests (tests/test_gpu_contract_range.py) measure.

    python tools/range_profile.py [--out profiles/contract_range.txt] [--matrix]

Per group, type and shape class the largest error / bound of one device run (every bound is stated in the module
docstring of the test file; the tests assert a ratio of at most 1), for group D the parts that differ from the host's
rounding per category, and the sentence on what the matrix cores do with subnormal 16-bit inputs: group A's ratios in
the tiled class decide it, since an MFMA that read them as zero would leave the bound in every element.  Section G does
the same for compute="matrix" (tests/test_gpu_contract_matrix_range.py): the float32 and float64 matrix instructions on
subnormal operands, products and sums; `--matrix` appends that section alone to the file.  Nothing is asserted here
beyond the kernel paths: a ratio above 1 is written down as it is.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's HIP runtime first: tnco_amd/_lib.py)

from tests import range_cases as rc  # noqa: E402
from tests import test_gpu_contract_matrix_range as matrix_tests  # noqa: E402
from tests import test_gpu_contract_range as tests  # noqa: E402
from tnco_amd import contraction as ctr  # noqa: E402

CLASSES = ("tiled", "dot", "stream")


def per_class(runs):
    """{class: largest ratio} of (case, ratio) pairs, as three columns."""
    worst = {}
    for case, ratio in runs:
        worst[rc.class_of(case)] = max(worst.get(rc.class_of(case), 0.0), ratio)
    return " ".join(f"{worst[c]:10.4f}" if c in worst else f"{'-':>10}" for c in CLASSES), worst


def matrix_section():
    """Section G: compute="matrix" on the fills of group C, the tiled cases, per dtype and kind; and per instruction the
    sentence on what it does with subnormal numbers."""
    matrix_tests.MEASURE_ONLY = True
    lines = ["", "## G: compute=\"matrix\", subnormal sums / subnormal operands, the tiled cases; bound (c kt + 2) (u |A| @ |B| + eta)",
             f"{'dtype':>10} {'kind':>9} {'tiled':>10}"]
    worst = {4: 0.0, 8: 0.0}
    for dtype in matrix_tests.DTYPES:
        for kind in rc.C_KINDS:
            ratio = max(matrix_tests.run(ctr, c, dtype, kind) for c in rc.TILED)
            worst[rc.real_size(dtype)] = max(worst[rc.real_size(dtype)], ratio)
            lines.append(f"{np.dtype(dtype).name:>10} {kind:>9} {ratio:10.4f}")
    for size, mnemonic in ((4, "v_mfma_f32_16x16x4_f32"), (8, "v_mfma_f64_16x16x4_f64")):
        lines.append(f"subnormal numbers, {mnemonic}: " + (
            "takes subnormal operands at their value and keeps subnormal products and sums: inside the bound of the plain "
            "kernels, which a flushed operand or result leaves in every element" if worst[size] <= 1 else
            f"does NOT meet the bound of the plain kernels (largest error / bound {worst[size]:.3g}): subnormal numbers are lost"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contract_range.txt"))
    ap.add_argument("--matrix", action="store_true", help="only section G, appended to --out")
    a = ap.parse_args()
    if a.matrix:
        lines = [f"(the section below: {torch.cuda.get_device_name(0)}; torch {torch.__version__})"] + matrix_section()[1:]
        with open(a.out, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    tests.MEASURE_ONLY = True
    kinds = (("real", False), ("complex", True))
    head = f"{'tiled':>10} {'dot':>10} {'stream':>10}"
    lines = [f"# tools/range_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "# largest error / bound of one run per group, type and shape class; the tests assert <= 1", "",
             "## A: storage=, unscaled, operands wholly subnormal in the 16-bit type; bound (2 c kt + 2) 2^-24 |A| @ |B|",
             f"{'storage':>9} {'subnormal':>9} {'type':>8} {head}"]
    mfma = {}
    for storage in rc.STORAGES:
        for role in rc.A_ROLES[storage]:
            for name, cplx in kinds:
                cols, worst = per_class((c, tests.run_a(ctr, c, storage, role, cplx)) for c in rc.CASES)
                mfma[storage] = max(mfma.get(storage, 0.0), worst["tiled"])
                lines.append(f"{storage:>9} {role:>9} {name:>8} {cols}")
    for storage in rc.STORAGES:
        mnemonic = "v_mfma_f32_16x16x32_" + ("f16" if storage == "float16" else "bf16")
        lines.append(f"subnormal inputs, {storage}: {mnemonic} " + (
            "takes subnormal inputs at their value: the tiled class is inside the bound of the float32 sums, which a "
            "flushed operand leaves in every element" if mfma[storage] <= 1 else
            f"does NOT meet the strict bound (largest error / bound {mfma[storage]:.3g}): subnormal inputs are lost"))
    lines += ["", "## B: compute=\"bf16x3\", lo subnormal, against the three-product emulation; "
              "bound (2 c 3 kt + 2) 2^-24 |A| @ |B|",
              f"{'type':>8} {'tiled':>10}   top of the range, against the float64 einsum (the mode's bound)"]
    for name, cplx in kinds:
        _, worst = per_class((c, tests.run_b(ctr, c, cplx)) for c in rc.TILED)
        lines.append(f"{name:>8} {worst['tiled']:10.4f}   {tests.run_b_top(ctr, cplx):10.4f}")
    lines += ["", "## C: plain kernels, subnormal sums / subnormal operands; bound (c kt + 2) (u |A| @ |B| + eta)",
              f"{'dtype':>10} {'kind':>9} {head}"]
    for dtype in tests.SINGLES + tests.DOUBLES:
        for kind in rc.C_KINDS:
            cols, _ = per_class((c, tests.run_c(ctr, c, dtype, kind)[0]) for c in tests.CLASS_CASES)
            lines.append(f"{np.dtype(dtype).name:>10} {kind:>9} {cols}")
    lines += ["", "## D: stored products against round_to_storage, bit for bit: parts that differ / parts, per category",
              f"{'storage':>9} {'step 1':>7} {'type':>8}   " + " ".join(rc.CATEGORIES)
              + "   | scaled: parts that differ, exponent - host's"]
    for storage in rc.STORAGES:
        for cls in rc.D_SHAPES:
            for name, cplx in kinds:
                counts = tests.run_d(ctr, storage, cls, cplx)
                differ, de = tests.run_d_scaled(ctr, storage, cls, cplx)
                lines.append(f"{storage:>9} {cls:>7} {name:>8}   "
                             + " ".join(f"{counts[k][1]}/{counts[k][0]}" for k in rc.CATEGORIES) + f"   | {differ} {de:+d}")
    lines += ["", "## E: every 16-bit pattern widened: patterns whose float32 is not the host's"]
    for storage in rc.STORAGES:
        for name, cplx in kinds:
            tests.run_e(ctr, storage, cplx)  # (asserts: a difference is an error of the widening, not a figure)
            lines.append(f"{storage:>9} {name:>8} 0 of {len(rc.all_patterns(storage))}")
    lines += matrix_section()
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
