"""The matrix kernel's code objects (csrc/contract_matrix.h), read from the libtnco_hip.so of the tree through
tools/code_objects.py (no GPU): ct_matrix_tiled_kernel exists for float, double, cplx<float> and cplx<double> in the four
operand layouts, none of the 16 uses scratch or spills a register, each fits a compute unit with at least one wavefront
per SIMD, and its LDS images stay inside the 160 KiB of a compute unit."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

KERNEL = "ct_matrix_tiled_kernel"
# the template argument as the Itanium ABI mangles it: f, d, and cplx<f>, cplx<d> of the anonymous namespace
ELEMENTS = {"float": "If", "double": "Id", "cplx<float>": "INS_4cplxIfEE", "cplx<double>": "INS_4cplxIdEE"}
LAYOUTS = {(ak, bn): f"Lb{ak}ELb{bn}EEE" for ak in (0, 1) for bn in (0, 1)}
# LDS of a block, both operands: (rows of A + rows of B) x parts x row pitch in bytes (16 k + 16 bytes)
LDS = {"float": 256 * 80, "double": 256 * 144, "cplx<float>": 256 * 2 * 80, "cplx<double>": 128 * 2 * 144}


@pytest.fixture(scope="module")
def kernels():
    import code_objects
    if not code_objects.LIB.exists():
        pytest.fail("tnco_amd/libtnco_hip.so is missing: run __graft_entry__.build()")
    if not (code_objects.LLVM / "llvm-readelf").exists():
        pytest.fail("no ROCm LLVM tools on this machine: the code objects cannot be read")
    table = {}
    for elf in code_objects.code_objects():
        table.update(code_objects.kernel_table(elf))
    return table


@pytest.mark.parametrize("element", ELEMENTS)
def test_the_four_layouts_exist_use_no_scratch_and_fit_a_compute_unit(kernels, element):
    import code_objects
    for layout, tail in LAYOUTS.items():
        frag = f"{len(KERNEL)}{KERNEL}{ELEMENTS[element]}{tail}"
        found = {name: meta for name, meta in kernels.items() if frag in name}
        assert len(found) == 1, f"{KERNEL}<{element}, {layout}>: {sorted(found)}"
        (name, meta), = found.items()
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
        assert meta.get("sgpr_spill_count", 0) == 0, (name, meta)
        assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) >= 1, (name, meta)
        assert meta["group_segment_fixed_size"] == LDS[element] <= 160 * 1024, (name, meta)


def test_there_are_sixteen_of_them(kernels):
    assert len([name for name in kernels if f"{len(KERNEL)}{KERNEL}I" in name]) == 16
