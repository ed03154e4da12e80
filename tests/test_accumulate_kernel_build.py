"""The code objects of the wide accumulation (csrc/contract_accumulate.h), read from the libtnco_hip.so of the tree
through tools/code_objects.py (no GPU): the two folds and the narrowing kernel exist for float and cplx<float>, and for
nothing else; none of the six uses scratch or LDS or spills a register, and each leaves room for eight wavefronts per SIMD:
they are streaming kernels and live on memory requests in flight."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

KERNELS = ("ct_acc_reduce_kernel", "ct_acc_path_reduce_kernel", "ct_acc_narrow_kernel")
# the template argument as the Itanium ABI mangles it: f, and cplx<f> of the anonymous namespace
ELEMENTS = {"float": "IfEE", "cplx<float>": "INS_4cplxIfEEEE"}


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
def test_the_kernel_exists_and_uses_no_scratch_and_no_lds(kernels, kernel, element):
    import code_objects
    frag = f"{len(kernel)}{kernel}{ELEMENTS[element]}"
    found = {name: meta for name, meta in kernels.items() if frag in name}
    assert len(found) == 1, f"{kernel}<{element}>: {sorted(found)}"
    (name, meta), = found.items()
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
    assert meta.get("sgpr_spill_count", 0) == 0, (name, meta)
    assert meta["group_segment_fixed_size"] == 0, (name, meta)
    assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) == 8, (name, meta)


def test_there_are_six_of_them(kernels):
    for kernel in KERNELS:
        assert len([name for name in kernels if f"{len(kernel)}{kernel}I" in name]) == 2, kernel
