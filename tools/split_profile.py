"""Writes profiles/contract_split.txt on one GPU: the accuracy figures of the compute mode that its tests assert on.

    python tools/split_profile.py [--out profiles/contract_split.txt]

Real and complex: the largest err / (2^-16 |A| @ |B|) over the one-step cases of tests/split_cases.py that run the
split kernel (tests/test_gpu_contract_split.py asserts err <= [2^-14 + (2 c 3 kt + 2) 2^-24] |A| @ |B|, that is a ratio of
at most 4 + (2 c 3 kt + 2) 2^-8), with leaf factors 1 and 2^40, 2^-70.  For the network of
tests/test_gpu_contract_split_network.py: e_dev, e_emul, e_f32 (asserted: e_dev <= 2 e_emul + e_f32) and the error of
storage="bfloat16" (asserted: above e_dev).
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (torch's HIP runtime first: tnco_amd/_lib.py)

from tests import split_cases as sc  # noqa: E402
from tests import test_gpu_contract_split as kernels  # noqa: E402
from tests import test_gpu_contract_split_network as network  # noqa: E402
from tnco_amd import contraction as ctr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contract_split.txt"))
    a = ap.parse_args()
    lines = [f"# tools/split_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}", "",
             "## one-step cases (tests/split_cases.py): largest err / (2^-16 |A| @ |B|) over the cases of the split kernel",
             f"{'type':>8} {'leaf factors':>14} {'ratio':>8}   worst case"]
    for cplx in (False, True):
        for label, scales in (("1, 1", (1.0, 1.0)), ("2^40, 2^-70", (2.0 ** 40, 2.0 ** -70))):
            worst = max((kernels.run_case(ctr, case, cplx, scales=scales), case.name) for case in sc.SPLIT)
            lines.append(f"{'complex' if cplx else 'real':>8} {label:>14} {worst[0]:8.4f}   {worst[1]}")
    e_dev, e_emul, e_f32, e_bf16, split, _ = network.measure(ctr)
    res, tiled, p = network.optimized(ctr)[3], network.optimized(ctr)[5], network.optimized(ctr)[6]
    lines += ["", "## network (tests/test_gpu_contract_split_network.py): relative distances to the complex128 host "
              "contraction, by norm", f"{'network':>8} {'e_dev':>10} {'e_emul':>10} {'e_f32':>10} {'storage bfloat16':>17} "
              f"{'slices':>7} {'split steps':>12}",
              f"{'chain':>8} {e_dev:10.3e} {e_emul:10.3e} {e_f32:10.3e} {e_bf16:17.3e} {len(res.slices):7d} "
              f"{len(tiled):7d} of {len(p.ops)}"]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
