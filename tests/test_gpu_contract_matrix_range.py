"""The matrix kernel (`compute="matrix"`) at the bottom of its number range, element by element, in the four dtypes: the
fills of group C of tests/range_cases.py (by import) on the tiled cases of that table -- the four layouts at 64 x 64 x 33
and 65 x 127 x 48.

    sums      A and B in 2^[-68, -65) (double: 2^[-530, -527)): every product and nearly every sum is subnormal in the type;
    operands  A in 2^[-140, -130) (double: 2^[-1065, -1030)), subnormal, B in 2^[20, 26) (2^[60, 66)), normal.

Held to the bound the plain kernels are held to (tests/test_gpu_contract_range.py, group C):

    |got - ref| <= (c kt + 2) (u |A| @ |B| + eta)      eta half the spacing of the type's subnormals (2^-150, 2^-1075)

with reference and bound in float64 for the single types and in numpy's longdouble for the double types.  A matrix unit
that read subnormal operands as zero, or flushed a subnormal result, would be beyond it in every element (the fills are
ones at which no sum cancels to below its bound: tests/test_contraction_range_plan.py).  tools/range_profile.py writes the
largest error / bound per type and kind into profiles/contract_range.txt.
"""
import numpy as np
import pytest

from tests import range_cases as rc
from tests.test_gpu_contract_half import assert_kernels, assert_within, result_inds

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
MEASURE_ONLY = False  # tools/range_profile.py: return the largest error / bound of a case without asserting on it


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def run(ctr, case, dtype, kind):
    """Returns the largest error / bound."""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy's longdouble has no more precision than float64 here"
    arrays = rc.fill_c(case, dtype, kind)
    r = ctr.contract([(0, 1)], case.ts, arrays, case.output, compute="matrix")
    what = f"{case.name} {np.dtype(dtype).name} subnormal {kind}"
    assert r.inds == result_inds(case.ts, case.output) == ("i", "j") and r.n_slices == 1, what
    assert_kernels(ctr, r, case.kernels, what)
    assert r.matrix_launches == 1 and r.compute == "matrix" and r.array.dtype == np.dtype(dtype), what
    ref, mag = rc.reference_c(case, arrays)
    bnd = rc.bound_c(mag, case.kt, dtype)
    if not MEASURE_ONLY:
        return assert_within(r.array, ref, bnd, what)
    err = np.abs(r.array.astype(ref.dtype) - ref)
    ratio = np.divide(err, bnd, out=np.zeros_like(bnd), where=bnd > 0)
    ratio[~(err <= bnd) & ~(ratio > 1)] = np.inf
    return float(ratio.max())


@pytest.mark.parametrize("kind", rc.C_KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", rc.TILED, ids=[c.name for c in rc.TILED])
def test_the_matrix_kernel_keeps_subnormal_operands_products_and_sums(ctr, case, dtype, kind):
    run(ctr, case, dtype, kind)
