"""The path kernel's code objects (csrc/contract_path.h), read from the libtnco_hip.so of the tree through
tools/code_objects.py (no GPU): ct_path_kernel and ct_path_reduce_kernel exist for float, double, cplx<float> and
cplx<double>, and none of them uses scratch -- a block of the path kernel is 1024 lanes, 16 wavefronts, so a lane has 128
registers at most, and what does not fit would be spilled."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

# the template argument as the Itanium ABI mangles it: f, d, and cplx<f>, cplx<d> of the anonymous namespace
ELEMENTS = {"float": "If", "double": "Id", "cplx<float>": "INS_4cplxIfE", "cplx<double>": "INS_4cplxIdE"}


@pytest.fixture(scope="module")
def kernels():
    import code_objects
    if not code_objects.LIB.exists():
        pytest.fail("tnco_amd/libtnco_hip.so is missing: run __graft_entry__.build()")
    if not (code_objects.LLVM / "llvm-readelf").exists():
        pytest.skip("no ROCm LLVM tools on this machine")
    table = {}
    for elf in code_objects.code_objects():
        table.update(code_objects.kernel_table(elf))
    return table


@pytest.mark.parametrize("kernel,lanes", [("ct_path_kernel", 1024), ("ct_path_reduce_kernel", 256)])
def test_the_four_instantiations_exist_and_use_no_scratch(kernels, kernel, lanes):
    import code_objects
    for element, mangled in ELEMENTS.items():
        frag = f"{len(kernel)}{kernel}{mangled}"
        found = {name: meta for name, meta in kernels.items() if frag in name}
        assert len(found) == 1, f"{kernel}<{element}>: {sorted(found)}"
        (name, meta), = found.items()
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
        # the whole block is resident at once: lanes / 64 wavefronts over the 4 SIMDs of a compute unit
        assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) >= lanes // 64 // 4, (name, meta)
    # the dot class keeps 1024 partials in LDS, nothing else
    lds = sorted(meta["group_segment_fixed_size"] for name, meta in kernels.items() if "14ct_path_kernelI" in name)
    assert lds == [4096, 8192, 8192, 16384]
