"""The code objects of the walkers' kernels (csrc/contract_walk.h), read from the libtnco_hip.so of the tree through
tools/code_objects.py (no GPU): ct_walk_path_kernel and ct_walk_choose_kernel exist for float, double, cplx<float> and
cplx<double>, ct_walk_permute_kernel once; none of them uses scratch or spills; a block of the path kernel over walkers
(1024 lanes, 16 wavefronts) is resident at once, and its LDS is that of its ct_sets_path_kernel twin: the 1024 partials of
the dot class, nothing else; the other two use no LDS."""
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


def one(kernels, kernel, element=None):
    frag = f"{len(kernel)}{kernel}{ELEMENTS[element] if element else 'E'}"
    found = {name: meta for name, meta in kernels.items() if frag in name}
    assert len(found) == 1, f"{kernel}<{element}>: {sorted(found)}"
    (name, meta), = found.items()
    return name, meta


@pytest.mark.parametrize("kernel,lanes", [("ct_walk_path_kernel", 1024), ("ct_walk_choose_kernel", 256)])
def test_the_four_instantiations_exist_without_scratch_or_spills(kernels, kernel, lanes):
    import code_objects
    for element in ELEMENTS:
        name, meta = one(kernels, kernel, element)
        print(f"{kernel}<{element}>: {meta}")
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
        # the whole block is resident at once: lanes / 64 wavefronts over the 4 SIMDs of a compute unit
        assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) >= lanes // 64 // 4, (name, meta)


def test_the_permute_kernel_exists_without_scratch_spills_or_lds(kernels):
    name, meta = one(kernels, "ct_walk_permute_kernel")
    print(f"ct_walk_permute_kernel: {meta}")
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["group_segment_fixed_size"] == 0, (name, meta)


@pytest.mark.parametrize("element", list(ELEMENTS))
def test_the_lds_is_that_of_the_sets_kernel_twin(kernels, element):
    _, walk = one(kernels, "ct_walk_path_kernel", element)
    _, twin = one(kernels, "ct_sets_path_kernel", element)
    assert walk["group_segment_fixed_size"] == twin["group_segment_fixed_size"] > 0
    assert walk["vgpr_count"] <= twin["vgpr_count"]  # (the walker's bit lives in scalar registers)
    assert one(kernels, "ct_walk_choose_kernel", element)[1]["group_segment_fixed_size"] == 0
