"""Did a change touch the code of a kernel it was not meant to touch?  One line per gfx950 kernel of a library: VGPRs, LDS,
scratch and a hash of its disassembly (mnemonics + operands; branch targets are relative and the pc-relative distance to
another symbol -- the literal added behind an `s_getpc_b64` -- is left out, so a kernel that only moved inside its code
object keeps its hash).  No GPU needed.

    python tools/code_hashes.py [lib.so] [name fragment, default sa_run] > before.txt     # ... build ... > after.txt; diff
"""
import hashlib
import pathlib
import re
import shutil
import subprocess
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import code_objects as co  # noqa: E402


def text(ins) -> str:
    out, since_getpc = [], 9
    for _a, op, args in ins:
        since_getpc = 0 if op == "s_getpc_b64" else since_getpc + 1
        if since_getpc in (1, 2) and op in ("s_add_u32", "s_addc_u32"):
            args = re.sub(r"0x[0-9a-f]+$", "REL", args)
        out.append(f"{op} {args}")
    return "\n".join(out)


def main():
    lib = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else co.LIB
    frag = sys.argv[2] if len(sys.argv) > 2 else "sa_run"
    rows = {}
    for elf in co.code_objects(lib):
        for name, meta in co.kernel_table(elf).items():
            if frag in name:
                h = hashlib.sha256(text(co.disassemble(elf, name)).encode()).hexdigest()[:16]
                rows[name] = (meta["vgpr_count"], meta["group_segment_fixed_size"], meta["private_segment_fixed_size"], h)
    filt = shutil.which("c++filt") or str(co.LLVM / "llvm-cxxfilt")
    names = sorted(rows)
    short = [co.short_kernel_name(ln) for ln in
             subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()]
    for name, s in sorted(zip(names, short), key=lambda x: x[1]):
        v, lds, scr, h = rows[name]
        print(f"{s:60s} VGPRs {v:3d}  LDS {lds:6d} B  scratch {scr:3d} B  {h}")


if __name__ == "__main__":
    main()
