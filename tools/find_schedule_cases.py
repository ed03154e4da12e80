#!/usr/bin/env python3
"""Seeds of tests/mode_cases.py `generate` for the items of tests/schedule_cases.py REQUIRED_SCHEDULE.

    python tools/find_schedule_cases.py --seeds 0:6000 --jobs 8

Plans every seed's network in the modes of the schedule tests (no device), prints which items the present table
(`schedule_cases.CASES`) lacks in a real or in a complex dtype, and a greedy choice of seeds, with a dtype and a fill each,
that closes those the generator reaches.  What stays open needs a network written by hand.  Not part of the suite.
"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def scan(seed):
    from tests import mode_cases as mc
    from tests import schedule_cases as sc
    try:
        case = mc.generate(seed)
        if case is None or len(case.slices) > sc.MAX_SLICED:
            return seed, None
        by_kind = {}
        for kind, dtype in (("f", "float32"), ("c", "complex64")):  # (folding depends on the item size: the smaller of each kind)
            got = sc.coverage(case.with_(dtype=dtype))
            by_kind[kind] = {g for g in got if not g.startswith("fill:")}
        return seed, by_kind
    except Exception as e:  # noqa: BLE001
        return seed, repr(e)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seeds", default="0:3000")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    lo, hi = (int(v) for v in args.seeds.split(":"))
    from tests import mode_cases as mc
    from tests import schedule_cases as sc
    have = {"f": set(), "c": set()}
    for c in sc.CASES:
        have[np.dtype(c.dtype).kind] |= sc.coverage(c)
    need = {(item, kind) for item in sc.REQUIRED_SCHEDULE for kind in "fc" if item not in have[kind]}
    print(f"{len(sc.CASES)} cases; open: {sorted(need)}")
    in_table = {c.name for c in sc.CASES}
    with Pool(args.jobs) as pool:
        found = [(s, g) for s, g in pool.imap_unordered(scan, range(lo, hi), chunksize=16) if g is not None]
    for s, g in found:
        if isinstance(g, str):
            print(f"seed {s}: {g}")
    found = {s: g for s, g in found if isinstance(g, dict) and f"seed-{s}" not in in_table}
    need = {(i, k) for i, k in need if not i.startswith("fill:")}
    reach = {i for g in found.values() for i in g["f"] | g["c"]}
    print(f"{len(found)} networks; never reached: {sorted({i for i, _ in need} - reach)}")
    while need:
        best = max(((len({(i, k) for i in g[k]} & need), -s, s, k) for s, g in found.items() for k in "fc"), default=None)
        if best is None or best[0] == 0:
            break
        _, _, s, k = best
        closed = sorted(i for i in found[s][k] if (i, k) in need)
        print(f"seed {s} as a {'real' if k == 'f' else 'complex'} dtype closes {closed}")
        need -= {(i, k) for i in closed}
        del found[s]
    print(f"left open: {sorted(need)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
