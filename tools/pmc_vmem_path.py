"""Is the vector-memory path of a CU backed up under the headline sweep kernel?  Busy and stall counters of the texture
addresser (TA) and the L1 (TCP) and the vector-memory instruction counts of the SQ, under `rocprofv3 --pmc` with
`--kernel-trace` and no other tracing, one pass per small counter group, for the kernels whose name contains KERNEL
(profiles/r09_node_access.md).  The names are taken from `rocprofv3 --list-avail`: a candidate this machine does not
offer is left out and said so.

    python tools/pmc_vmem_path.py OUTDIR [--lib build_variants/lib_x.so] [--kernel sa_run_kernel]

A pass that ends by a signal or at its time limit ends the run: nothing more is started on the GPU after it.
"""
import argparse
import csv
import glob
import os
import pathlib
import re
import shutil
import subprocess
import sys
from collections import defaultdict

ROOT = pathlib.Path(__file__).resolve().parents[1]

# (counters of one block share its few hardware slots: two per pass)
CANDIDATES = [
    ["SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_VALU", "SQ_WAVE_CYCLES"],
    ["SQ_BUSY_CYCLES", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_VMEM"],
    ["SQ_INST_CYCLES_VMEM", "SQ_INST_CYCLES_VMEM_RD", "SQ_INST_CYCLES_VMEM_WR", "SQ_WAVES"],
    ["TA_TA_BUSY_sum", "TA_BUSY_avr"],
    ["TA_ADDR_STALLED_BY_TC_CYCLES_sum", "TA_ADDR_STALLED_BY_TD_CYCLES_sum"],
    ["TA_DATA_STALLED_BY_TC_CYCLES_sum", "TA_FLAT_WAVEFRONTS_sum"],
    ["TA_FLAT_READ_WAVEFRONTS_sum", "TA_FLAT_WRITE_WAVEFRONTS_sum"],
    ["TCP_GATE_EN1_sum", "TCP_GATE_EN2_sum"],
    ["TCP_TA_TCP_STATE_READ_sum", "TCP_TCP_TA_DATA_STALL_CYCLES_sum"],
    ["TCP_TD_TCP_STALL_CYCLES_sum", "TCP_TCR_TCP_STALL_CYCLES_sum"],
    ["TCP_PENDING_STALL_CYCLES_sum", "TCP_READ_TAGCONFLICT_STALL_CYCLES_sum"],
    ["TCP_TOTAL_ACCESSES_sum", "TCP_TOTAL_CACHE_ACCESSES_sum"],
    ["TCP_TCC_READ_REQ_sum", "TCP_TCC_WRITE_REQ_sum"],
    ["GRBM_GUI_ACTIVE", "GRBM_COUNT"],
]
FATAL = {124, 137, 134, 139, -6, -9, -11}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--kernel", default="sa_run_kernel")
    ap.add_argument("--pass-timeout", type=int, default=150)
    a = ap.parse_args()
    out = pathlib.Path(a.out).resolve()
    out.mkdir(parents=True, exist_ok=True)
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    avail = subprocess.run([prof, "--list-avail"], capture_output=True, text=True, timeout=120)
    (out / "list_avail.txt").write_text(avail.stdout + avail.stderr)
    names = set(re.findall(r"[A-Za-z][A-Za-z0-9_]+", avail.stdout + avail.stderr))
    env = dict(os.environ)
    if a.lib:
        env["TNCO_HIP_LIB"] = str(pathlib.Path(a.lib).resolve())
    missing = []
    for grp in CANDIDATES:
        have = [c for c in grp if c in names]
        missing += [c for c in grp if c not in names]
        if not have:
            continue
        d = out / ("pmc_" + have[0])
        cmd = ["timeout", "-k", "10", str(a.pass_timeout), prof, "--pmc", *have, "--kernel-trace", "--output-format", "csv", "-d", str(d), "-o", "pmc",
               "--", sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "im"]
        with open(out / f"pmc_{have[0]}.log", "w") as log:
            rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, env=env, cwd="/tmp").returncode
        print(f"pass {' '.join(have)}: rc {rc}", flush=True)
        if rc in FATAL:
            print("that pass ended by a signal or at its time limit: stopping here")
            sys.exit(1)
    print("not offered here:", " ".join(missing) or "-")
    pmc, calls = defaultdict(list), {}
    for f in glob.glob(str(out / "pmc_*" / "**" / "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if a.kernel in name:
                pmc[(name.split("(")[0][-48:], r["Counter_Name"])].append(float(r["Counter_Value"]))
    with open(out / "summary.txt", "w") as fh:
        for k in sorted(pmc):
            v = pmc[k]
            line = f"{k[0]:48s} {k[1]:40s} {sum(v) / len(v):16.6g}  ({len(v)} launches)"
            print(line)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
