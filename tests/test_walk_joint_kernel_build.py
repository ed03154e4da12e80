"""The code objects of the joint-draw kernel (csrc/contract_walk.h), read from the libtnco_hip.so of the tree through
tools/code_objects.py (no GPU): ct_walk_choose_joint_kernel exists for float, double, cplx<float> and cplx<double>; none of
the four uses scratch (the qubits and strides are kernel arguments indexed by a loop counter), spills or LDS; a block of 256
lanes is resident at once; the block is read with 16-byte loads; and the library exports the entry point."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

# the template argument as the Itanium ABI mangles it: f, d, and cplx<f>, cplx<d> of the anonymous namespace
ELEMENTS = {"float": "If", "double": "Id", "cplx<float>": "INS_4cplxIfE", "cplx<double>": "INS_4cplxIdE"}
KERNEL = "ct_walk_choose_joint_kernel"


@pytest.fixture(scope="module")
def objects():
    import code_objects
    if not code_objects.LIB.exists():
        pytest.fail("tnco_amd/libtnco_hip.so is missing: run __graft_entry__.build()")
    if not (code_objects.LLVM / "llvm-readelf").exists():
        pytest.skip("no ROCm LLVM tools on this machine")
    found = {}
    for elf in code_objects.code_objects():
        for name, meta in code_objects.kernel_table(elf).items():
            if f"{len(KERNEL)}{KERNEL}" in name:
                found[name] = (meta, elf)
    return found


@pytest.mark.parametrize("element", list(ELEMENTS))
def test_the_instantiation_exists_without_scratch_spills_or_lds(objects, element):
    import code_objects
    names = [name for name in objects if f"{len(KERNEL)}{KERNEL}{ELEMENTS[element]}E" in name]
    assert len(names) == 1, f"{KERNEL}<{element}>: {sorted(objects)}"
    meta, elf = objects[names[0]]
    print(f"{KERNEL}<{element}>: {meta}")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["group_segment_fixed_size"] == 0, meta
    assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) >= 256 // 64 // 4, meta
    ops = [op for _, op, _ in code_objects.disassemble(elf, names[0])]
    assert ops and not any(op.startswith(("scratch_", "ds_")) or "atomic" in op for op in ops)
    assert "global_load_dwordx4" in ops  # (the natural layout: a lane reads its block 16 bytes at a time)


def test_the_library_exports_the_entry_point():
    from tnco_amd import _lib
    assert "tnco_hip_walkers_choose_joint" in _lib.EXPORTS
    header = (ROOT / "include" / "tnco_hip.h").read_text()
    assert "int tnco_hip_walkers_choose_joint(tnco_hip_walkers w, tnco_hip_contract h, int64_t k, const int64_t* qubits," in header
