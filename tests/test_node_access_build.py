"""What the compiler made of the node access of the child-partial sweep kernels (csrc/sa_sweep.h, TNCO_NODE_ACCESS), read
from the libtnco_hip.so of the tree through tools/code_objects.py (no GPU):

* the headline code object, sa_run_kernel<2, 3, false, false, false, false>: the vector-memory instructions of its loop, its
  registers, spills, scratch and LDS;
* every other sa_run* code object -- hyper-indices, the general cost models, finite width -- is the parent's, instruction
  for instruction: tests/golden/sa_run_code_hashes.txt, recorded from the parent commit with tools/code_hashes.py.

The loop's instructions, counted over the whole outer loop (the widest backward branch), rare paths included:

    loads    a MOVE iteration: header 1, legs 2 (one pair row, the single row), the 8 bytes of `xa` 1               =  4
             a refill round: mt[k .. k+3] 1, mt[k+4] 1, mt[k+397 ..] 1; the arm that straddles the wrap, mt[621 .. 623]
             and mt[0], 2 of its own                                                                                 =  5
             the full copy of a best tree (END, log overflowed): 4 leaf parents + 4 headers                          =  8
    stores   an accepted move: parent words 2, legs 2, B's record 1                                                 =  5
             journal 1, generator (state words, shadow words) 2                                                     =  3
             END's record ahead of a full copy 2 (32 bytes of lane 0), the copy's links 4                            =  6

The parent's loop held 20 loads and 16 stores by the same count."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

HEADLINE = "sa_run_kernelILi2ELi3ELb0ELb0ELb0ELb0E"
MAX_LOADS = 4 + 5 + 8
MAX_STORES = 5 + 3 + 6
GOLDEN = ROOT / "tests" / "golden" / "sa_run_code_hashes.txt"


@pytest.fixture(scope="module")
def code_objects():
    import code_objects as co
    if not co.LIB.exists():
        pytest.fail("tnco_amd/libtnco_hip.so is missing: run __graft_entry__.build()")
    if not (co.LLVM / "llvm-objdump").exists():
        pytest.skip("no ROCm LLVM tools on this machine")
    return co


@pytest.fixture(scope="module")
def headline(code_objects):
    co = code_objects
    for elf in co.code_objects():
        for name, meta in co.kernel_table(elf).items():
            if HEADLINE in name:
                return meta, co.disassemble(elf, name)
    pytest.fail("the headline kernel is not in the library")


def test_registers_spills_scratch_and_lds_of_the_headline_kernel(headline):
    meta, _ = headline
    assert meta["vgpr_count"] <= 168 and meta["agpr_count"] == 0, meta
    assert meta["vgpr_spill_count"] <= 2 and meta["private_segment_fixed_size"] <= 16, meta
    assert meta["group_segment_fixed_size"] == 22016, meta


def test_vector_memory_instructions_of_the_headline_loop(code_objects, headline):
    co = code_objects
    _, ins = headline
    head, tail = max(co.loops(ins), key=lambda x: x[1] - x[0])
    body = [i for i in ins if head <= i[0] <= tail]
    loads = [i for i in body if i[1].startswith(("global_load", "buffer_load", "flat_load"))]
    stores = [i for i in body if i[1].startswith(("global_store", "buffer_store", "flat_store"))]
    print(f"loop of {len(body)} instructions: {len(loads)} loads {sorted(i[1] for i in loads)}, "
          f"{len(stores)} stores {sorted(i[1] for i in stores)}")
    assert 4 <= len(loads) <= MAX_LOADS, [i[1] for i in loads]
    assert 5 <= len(stores) <= MAX_STORES, [i[1] for i in stores]
    # no access of fewer than 8 bytes to a node: the single dwords left are the generator's mt[k+4] (and the wrap arm's
    # mt[0]), the leaf parents of the full copy, and the two parent words of an accepted move
    assert sum(1 for i in loads if i[1] == "global_load_dword") <= 2 + 4, [i[1] for i in loads]
    assert sum(1 for i in stores if i[1] == "global_store_dword") <= 2, [i[1] for i in stores]
    rep = co.main_loop_report(ins)
    assert rep["fences"] == 1 and not rep["scratch_in_loop"], rep
    assert not [i for i in body if i[1].startswith("scratch_")]


def test_the_other_sweep_kernels_are_the_parents(code_objects):
    """Hyper-indices, general cost models, finite width, in both forms and all eight (lanes, words) pairs: 112 code objects."""
    import code_hashes
    co = code_objects
    want = {}
    for ln in GOLDEN.read_text().splitlines():
        if ln.strip() and not ln.startswith("#"):
            name, rest = ln.split(">", 1)[0] + ">", ln.rsplit(None, 1)
            want[name.strip()] = rest[1]
    assert len(want) == 112
    import hashlib
    import shutil
    import subprocess
    got = {}
    for elf in co.code_objects():
        for name in co.kernel_table(elf):
            if "sa_run" in name:
                got[name] = hashlib.sha256(code_hashes.text(co.disassemble(elf, name)).encode()).hexdigest()[:16]
    filt = shutil.which("c++filt") or str(co.LLVM / "llvm-cxxfilt")
    names = sorted(got)
    short = [co.short_kernel_name(ln) for ln in subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()]
    have = {s: got[n] for n, s in zip(names, short)}
    assert len(have) == 128
    changed = sorted(s for s in want if have.get(s) != want[s])
    assert not changed, f"code objects that differ from the parent's (or a new toolchain: record the list again): {changed}"
    # ... and the sixteen that are meant to differ are the child-partial ones
    assert sorted(set(have) - set(want)) == sorted(f"sa_run_kernel<{l}, {k}, false, false, false, {s}>" for l, k in
                                                   ((2, 1), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 3), (4, 4)) for s in ("false", "true"))
