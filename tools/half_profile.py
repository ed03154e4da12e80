"""Writes profiles/contract_half.txt on one GPU: the accuracy figures of the storage mode that its tests assert on.

    python tools/half_profile.py [--out profiles/contract_half.txt]

Per storage type, real and complex: the largest err / (2^-24 kt |A| @ |B|) over the one-step cases of
tests/half_cases.py (tests/test_gpu_contract_half.py asserts err <= (2 c kt + 2) 2^-24 |A| @ |B|, that is a ratio of
at most about 2 real, 4 complex).  Per network and storage type: e_dev, e_emul, e_f32 of
tests/test_gpu_contract_half_network.py (asserted: e_dev <= 2 e_emul + e_f32).  With `scaling="tensor"`: the same three
per network and storage type on the arrays of tests/test_gpu_contract_scaled_network.py (a further 2^-F each), e_emul
from its emulation of the scaling rule, and the ratio unscaled bfloat16 / scaled float16 that test asserts to be > 1.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402  (torch's HIP runtime first: tnco_amd/_lib.py)

from tests import half_cases as hc  # noqa: E402
from tests import test_gpu_contract_half as kernels  # noqa: E402
from tests import test_gpu_contract_half_network as networks  # noqa: E402
from tests import test_gpu_contract_scaled_network as scaled  # noqa: E402
from tnco_amd import contraction as ctr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contract_half.txt"))
    a = ap.parse_args()
    lines = [f"# tools/half_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}", "",
             "## one-step cases (tests/half_cases.py): largest err / (2^-24 kt |A| @ |B|) per kernel class",
             f"{'storage':>9} {'type':>8} {'mfma':>8} {'dot':>8} {'stream':>8}   worst case"]
    for storage in hc.STORAGES:
        for cplx in (False, True):
            worst = {}
            for case in hc.CASES:
                ratio = kernels.run_case(ctr, case, storage, cplx)
                cls = "mfma" if case.name.startswith("mfma") else case.name.split("-")[0]
                if ratio > worst.get(cls, (0.0, ""))[0]:
                    worst[cls] = (ratio, case.name)
            top = max(worst.values())
            lines.append(f"{storage:>9} {'complex' if cplx else 'real':>8} {worst['mfma'][0]:8.4f} {worst['dot'][0]:8.4f} "
                         f"{worst['stream'][0]:8.4f}   {top[1]} ({top[0]:.4f})")
    lines += ["", "## networks (tests/test_gpu_contract_half_network.py): relative distances to the complex128 host "
              "contraction, by norm", f"{'network':>8} {'storage':>9} {'e_dev':>10} {'e_emul':>10} {'e_f32':>10} {'slices':>7}"]
    for kind in networks.NETWORKS:
        for storage in hc.STORAGES:
            e_dev, e_emul, e_f32, *_ = networks.measure(ctr, kind, storage)
            lines.append(f"{kind:>8} {storage:>9} {e_dev:10.3e} {e_emul:10.3e} {e_f32:10.3e} "
                         f"{len(networks.optimized(kind)[3].slices):7d}")
    lines += ["", f"## networks with scaling=\"tensor\" (tests/test_gpu_contract_scaled_network.py): every array times 2^-{scaled.F}",
              f"{'network':>8} {'storage':>9} {'e_dev':>10} {'e_emul':>10} {'e_f32':>10} {'unscaled e_dev':>15}"]
    for kind in networks.NETWORKS:
        tn0, arrays, tn, res, ref = scaled.scaled_down(kind)
        plain = ctr.contract_results(tn0, arrays, tn, res)
        ref = ref.transpose([networks._ref_inds(tn, res).index(x) for x in plain.inds]) if plain.inds else ref
        args = (res.path, tn.ts_inds, arrays, tn.output_inds, res.slices, tn0.dims, plain.inds)
        e_dev = {}
        for storage in hc.STORAGES:
            r = ctr.contract_results(tn0, arrays, tn, res, storage=storage, scaling="tensor")
            un = ctr.contract_results(tn0, arrays, tn, res, storage=storage)
            e_dev[storage, True], e_dev[storage, False] = networks._rel(r.array, ref), networks._rel(un.array, ref)
            lines.append(f"{kind:>8} {storage:>9} {e_dev[storage, True]:10.3e} "
                         f"{networks._rel(scaled.emulate_scaled(ctr, *args, storage), ref):10.3e} "
                         f"{networks._rel(plain.array, ref):10.3e} {e_dev[storage, False]:15.3e}")
        lines.append(f"{kind:>8}: unscaled bfloat16 e_dev / scaled float16 e_dev = "
                     f"{e_dev['bfloat16', False] / e_dev['float16', True]:.2f}")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
