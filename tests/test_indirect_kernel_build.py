"""The code objects of the kernels that read a folded operand in place (csrc/contract_indirect.h), read from the
libtnco_hip.so of the tree through tools/code_objects.py (no GPU): ct_ix_tiled_kernel, ct_ix_dot_kernel and
ct_ix_stream_kernel exist for float, double, cplx<float> and cplx<double>, none of the twelve uses scratch or spills a
register, each fits a compute unit, and the LDS of each is that of its plain twin."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

KERNELS = ("ct_ix_tiled_kernel", "ct_ix_dot_kernel", "ct_ix_stream_kernel")
# the template argument as the Itanium ABI mangles it: f, d, and cplx<f>, cplx<d> of the anonymous namespace
ELEMENTS = {"float": "IfEE", "double": "IdEE", "cplx<float>": "INS_4cplxIfEEEE", "cplx<double>": "INS_4cplxIdEEEE"}
SIZE = {"float": 4, "double": 8, "cplx<float>": 8, "cplx<double>": 16}
# tiled: two images of 16 x (64 + 1) elements; dot: 256 partials; stream: none
LDS = {"ct_ix_tiled_kernel": 2 * 16 * 65, "ct_ix_dot_kernel": 256, "ct_ix_stream_kernel": 0}


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
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_kernel_exists_uses_no_scratch_and_fits_a_compute_unit(kernels, kernel, element):
    import code_objects
    frag = f"{len(kernel)}{kernel}{ELEMENTS[element]}v"
    found = {name: meta for name, meta in kernels.items() if frag in name}
    assert len(found) == 1, f"{kernel}<{element}>: {sorted(found)}"
    (name, meta), = found.items()
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
    assert meta.get("sgpr_spill_count", 0) == 0, (name, meta)
    assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) >= 1, (name, meta)
    assert meta["group_segment_fixed_size"] == LDS[kernel] * SIZE[element] <= 160 * 1024, (name, meta)


def test_there_are_twelve_of_them(kernels):
    assert len([name for name in kernels if any(f"{len(k)}{k}I" in name for k in KERNELS)]) == 12
