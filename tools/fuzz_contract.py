#!/usr/bin/env python3
"""Every way of running a plan of the contraction engine, on random networks beyond the table of the tests.

    python tools/fuzz_contract.py --seeds 3000:3400

For every seed of the range the generator of tests/mode_cases.py gives a network (or none, when the seed's network is
beyond the caps of a case); it is replayed by the numpy interpreter in its own dtype against the plain bound, its plans
under `hoist=True`, `reuse=True` (three orders of the sliced indices) and `indirect=True` are replayed on a NaN-poisoned
arena by the interpreters of those features' plan tests, and then it is run on the device in every mode with the checks of
tests/test_gpu_contract_modes.py and in every schedule with those of tests/test_gpu_contract_schedules.py (the two
`check_case`).  One process.  The run stops at the first mismatch or exception and prints the case as a line that can be
pasted into `mode_cases`; at the end it prints the largest error / bound per mode.  Not part of the suite.

    python tools/fuzz_contract.py --projs --seeds 3000:3100

With `--projs` the networks are those of the generator of tests/projs_cases.py, contracted at projections of sparse
indices: the row tables are replayed by the numpy interpreter in the case's own dtype against the bound
(`replay_case` of tests/test_contraction_projs_cases_plan.py; `--cpu-only`: that alone), then run on the device with the
checks of tests/test_gpu_contract_projs_cases.py (`check_case`); at the end the launches per row-mapped kernel.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seeds", default="3000:3100", help="A:B, the seeds A .. B - 1")
    ap.add_argument("--cpu-only", action="store_true", help="the replay of the tables alone, no device")
    ap.add_argument("--projs", action="store_true", help="projections of sparse indices: the networks of tests/projs_cases.py")
    args = ap.parse_args()
    lo, hi = (int(v) for v in args.seeds.split(":"))
    if args.projs:
        return fuzz_projs(lo, hi, args.cpu_only)
    from tests import mode_cases as mc
    from tests.test_contraction_plan import _interpret
    from tests import indirect_cases as ic
    from tests import schedule_cases as sc
    from tests.test_contraction_reuse_plan import interpret as interpret_reuse
    ctr = check_case = check_schedules = None
    if not args.cpu_only:
        from tests.test_gpu_contract_modes import check_case
        from tests.test_gpu_contract_schedules import check_case as check_schedules
        from tnco_amd import contraction as ctr

    def schedules_replayed(case):
        """The plans of the schedule tests on one flat arena that is NaN wherever nothing valid lies, in double precision."""
        P = sc.Plans(case)
        wide = [np.asarray(a, np.complex128 if np.iscomplexobj(a) else np.float64) for a in mc.fill(case)]
        runs = [(q, ic.interpret(q, wide)) for q in (P.hoist, P.indirect, P.indirect_hoist)]
        runs += [(q, interpret_reuse(case, q, wide)) for q in list(P.reuse.values()) + list(P.indirect_reuse.values())]
        for q, got in runs:
            ref, mag = mc.reference(case, q, wide)
            assert not np.isnan(got).any(), "a schedule reads a buffer that nothing valid is in"
            assert (np.abs(got - ref) <= 1e-12 * mc.kt(q) * mag).all(), "the replay of a schedule is not the einsum"
    worst, ran = {}, 0
    for seed in range(lo, hi):
        case = mc.generate(seed)
        if case is None:
            continue
        ran += 1
        try:
            p, arrays = case.plan(), mc.fill(case)
            ref, mag = mc.reference(case, p, arrays)
            err = np.abs(_interpret(p, arrays).astype(ref.dtype) - ref)
            bound = mc.plain_bound(case, p, mag)
            assert (err <= bound).all(), "the replay of the tables leaves the plain bound"
            ratios = {"replay": float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())}
            schedules_replayed(case)
            if check_case is not None:
                ratios.update(check_case(ctr, case, out=lambda line: None))
                ratios.update({f"schedules {k}": v for k, v in check_schedules(ctr, case, out=lambda line: None).items()})
        except Exception as e:  # noqa: BLE001 -- whatever it is, the case is what is wanted
            print(f"seed {seed}: {type(e).__name__}: {e}\n{case.paste()}")
            return 1
        for mode, ratio in ratios.items():
            if ratio > worst.get(mode, (0.0, None))[0] or mode not in worst:
                worst[mode] = (ratio, seed)
    print(f"{ran} networks of seeds {lo}:{hi}, every check passed")
    for mode, (ratio, seed) in worst.items():
        print(f"  {mode:18s} largest error / bound {ratio:.4f} (seed {seed})")
    return 0


def fuzz_projs(lo, hi, cpu_only):
    from tests import projs_cases as pc
    from tests.test_contraction_projs_cases_plan import replay_case
    ctr = check_case = None
    if not cpu_only:
        from tests.test_gpu_contract_projs_cases import check_case
        from tnco_amd import contraction as ctr
    worst, ran, slots = {}, 0, [0] * 3
    for seed in range(lo, hi):
        case = pc.generate(seed)
        if case is None:
            continue
        ran += 1
        try:
            ratios = {"replay": replay_case(case)}
            if check_case is not None:
                ratios["device"], rows = check_case(ctr, case, out=lambda line: None)
                slots = [a + b for a, b in zip(slots, rows)]
        except Exception as e:  # noqa: BLE001 -- whatever it is, the case is what is wanted
            print(f"seed {seed}: {type(e).__name__}: {e}\n{case.paste()}")
            return 1
        for mode, ratio in ratios.items():
            key = f"{mode} {case.dtype}"
            if ratio > worst.get(key, (0.0, None))[0] or key not in worst:
                worst[key] = (ratio, seed)
    print(f"{ran} networks with projections of seeds {lo}:{hi}, every check passed")
    for key, (ratio, seed) in sorted(worst.items()):
        print(f"  {key:18s} largest error / bound {ratio:.4f} (seed {seed})")
    if check_case is not None:
        print("  launches per row-mapped kernel: " + ", ".join(f"{n} {v}" for n, v in zip(ctr.ROW_KERNEL_PATHS, slots)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
