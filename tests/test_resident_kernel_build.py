"""The code objects of the resident entry points (csrc/contract_io.h), read from the libtnco_hip.so of the tree through
tools/code_objects.py (no GPU): ct_ingest_kernel exists for the identity in the four dtypes and for the five exact
widenings, ct_emit_kernel for the four dtypes, and for nothing else; none of the thirteen uses scratch or LDS or spills a
register, and each leaves room for eight wavefronts per SIMD: they are copies and live on memory requests in flight."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

# the template arguments as the Itanium ABI mangles them: f, d, and cplx<f>, cplx<d> of the anonymous namespace (the second
# mention of a type is a substitution: S2_ the destination's cplx<...>, NS1_I...E the template cplx with another argument)
INGEST = {
    "float <- float": "IffEE", "double <- double": "IddEE", "double <- float": "IdfEE",
    "cplx<float> <- cplx<float>": "INS_4cplxIfEES2_EE", "cplx<double> <- cplx<double>": "INS_4cplxIdEES2_EE",
    "cplx<float> <- float": "INS_4cplxIfEEfEE", "cplx<double> <- float": "INS_4cplxIdEEfEE",
    "cplx<double> <- double": "INS_4cplxIdEEdEE", "cplx<double> <- cplx<float>": "INS_4cplxIdEENS1_IfEEEE",
}
EMIT = {"float": "IfEE", "double": "IdEE", "cplx<float>": "INS_4cplxIfEEEE", "cplx<double>": "INS_4cplxIdEEEE"}
CASES = [("ct_ingest_kernel", what, frag) for what, frag in INGEST.items()] + \
        [("ct_emit_kernel", what, frag) for what, frag in EMIT.items()]


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


@pytest.mark.parametrize("kernel, what, frag", CASES, ids=[f"{k}<{w}>" for k, w, _ in CASES])
def test_the_kernel_exists_and_uses_no_scratch_and_no_lds(kernels, kernel, what, frag):
    import code_objects
    found = {name: meta for name, meta in kernels.items() if f"{len(kernel)}{kernel}{frag}v" in name}
    assert len(found) == 1, f"{kernel}<{what}>: {sorted(found)}"
    (name, meta), = found.items()
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, (name, meta)
    assert meta.get("sgpr_spill_count", 0) == 0, (name, meta)
    assert meta["group_segment_fixed_size"] == 0, (name, meta)
    assert code_objects.waves_per_simd(meta["vgpr_count"] + meta["agpr_count"]) == 8, (name, meta)


def test_there_are_thirteen_of_them(kernels):
    assert len(CASES) == 13
    assert len([name for name in kernels if "16ct_ingest_kernelI" in name]) == 9
    assert len([name for name in kernels if "14ct_emit_kernelI" in name]) == 4
