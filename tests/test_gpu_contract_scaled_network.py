"""Whole networks through optimize(max_width=...) -> contract_results(storage="float16", scaling="tensor"): the networks,
the pattern and the helpers of tests/test_gpu_contract_half_network.py, with every array multiplied by a further 2^-F.

F = 2.  Checked on the host with that file's `emulate` before F was fixed:
    the float16 emulation WITHOUT scaling has relative error 1.000 on the closed and 1.000 on the open network (> 0.5:
        the sub-networks of more than a few tensors fall below float16's subnormals and the result is zero); with F = 1
        the open network still came through with 0.47, with F = 3 the closed network's reference, 2^-128.7, leaves
        float32's normal range;
    the complex128 reference is 2^-88.7 in modulus (closed) and 2^-76.3 ... 2^-74.4 (open), inside float32's normal range.
Both conditions are asserted again below.  (The emulations at F = 2: scaled float16 7.5e-3 / 1.8e-3, unscaled bfloat16
2.3e-2 / 1.4e-2, closed / open.)

Required, as in that file and for its reason (device and emulation differ by one-storage-ulp flips at each stored step):
    e_dev <= 2 e_emul + e_f32
with e_emul from an emulation that applies the scaling rule at every stored tensor, leaves included; and
    e_dev (float16, scaled) < e_dev (bfloat16, unscaled)
on the same data: 11 significant bits against 8.  tools/half_profile.py writes the measured ratio into
profiles/contract_half.txt.
"""
import itertools
import math

import numpy as np
import pytest

from tests import test_gpu_contract_half_network as hn

pytestmark = pytest.mark.gpu

F = 2


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def rule64(z) -> int:
    parts = np.abs(np.concatenate([np.ravel(z.real), np.ravel(z.imag)]))
    parts = parts[np.isfinite(parts)]
    m = float(parts.max()) if parts.size else 0.0
    return 0 if m == 0 else int(np.frexp(m)[1]) - 1 - 14


def store_scaled(ctr, z, storage):
    """A complex128 tensor as the engine holds it under scaling: the rule, round to storage at that scale, back."""
    e = rule64(z)
    scaled = (np.ldexp(z.real, -e) + 1j * np.ldexp(z.imag, -e)).astype(np.complex64)
    return ctr.round_to_storage(scaled, storage).astype(np.complex128) * 2.0 ** e


def emulate_scaled(ctr, path, ts_inds, arrays, output_inds, slices, dims, inds, storage):
    """`emulate` of tests/test_gpu_contract_half_network.py with the scaling rule at every stored tensor: a leaf has one
    exponent for the whole leaf, an intermediate one per slice assignment."""
    store = lambda a: store_scaled(ctr, a, storage)  # noqa: E731
    leaves = [store(np.asarray(a, np.complex128)) for a in arrays]
    cut = [x for x in dict.fromkeys(x for xs in ts_inds for x in xs) if x in set(slices)]
    total = np.zeros([dims[x] for x in inds], np.complex128)
    for values in itertools.product(*(range(dims[x]) for x in cut)):
        at = dict(zip(cut, values))
        part = [a[tuple(at.get(x, slice(None)) for x in xs)] for xs, a in zip(ts_inds, leaves)]
        part_inds = [tuple(x for x in xs if x not in at) for xs in ts_inds]
        z, r = hn.host_contract(path, part_inds, part, [x for x in output_inds if x not in at], store)
        rest = [x for x in inds if x not in at]
        total[tuple(at.get(x, slice(None)) for x in inds)] += r.transpose([z.index(x) for x in rest])
    return total


_CACHE = {}


def scaled_down(kind):
    """(tn0, arrays 2^-F, tn, result, reference of those arrays): the optimization of that file, shared with it."""
    if kind not in _CACHE:
        tn0, arrays, tn, res, _ = hn.optimized(kind)
        small = [(a * np.float32(2.0 ** -F)).astype(np.complex64) for a in arrays]
        _, ref = hn.host_contract(res.path, tn.ts_inds, small, tn.output_inds)
        _CACHE[kind] = (tn0, small, tn, res, ref)
    return _CACHE[kind]


@pytest.mark.parametrize("kind", hn.NETWORKS)
def test_scaled_float16_costs_its_roundings_where_float16_alone_is_lost(ctr, kind):
    tn0, arrays, tn, res, ref = scaled_down(kind)
    plain = ctr.contract_results(tn0, arrays, tn, res)
    r = ctr.contract_results(tn0, arrays, tn, res, storage="float16", scaling="tensor")
    bf = ctr.contract_results(tn0, arrays, tn, res, storage="bfloat16")
    assert r.inds == plain.inds and r.array.dtype == np.complex64 and r.scaling == "tensor"
    ref = ref.transpose([hn._ref_inds(tn, res).index(x) for x in r.inds]) if r.inds else ref
    # the two conditions F was chosen by
    args = (res.path, tn.ts_inds, arrays, tn.output_inds, res.slices, tn0.dims, r.inds)
    e_unscaled = hn._rel(hn.emulate(ctr, *args, "float16"), ref)
    moduli = np.abs(ref[ref != 0])
    print(f"{kind}: F {F}  unscaled float16 emulation {e_unscaled:.3e}  reference moduli {moduli.min():.3e} .. {moduli.max():.3e}")
    assert e_unscaled > 0.5
    assert moduli.min() > 2.0 ** -126 and moduli.max() < 2.0 ** 127
    e_dev, e_emul = hn._rel(r.array, ref), hn._rel(emulate_scaled(ctr, *args, "float16"), ref)
    e_f32, e_bf = hn._rel(plain.array, ref), hn._rel(bf.array, ref)
    print(f"{kind} float16 scaled: e_dev {e_dev:.3e}  e_emul {e_emul:.3e}  e_f32 {e_f32:.3e}  bfloat16 unscaled {e_bf:.3e}"
          f"  ratio {e_bf / e_dev:.2f}")
    assert e_dev <= 2 * e_emul + e_f32
    assert e_dev < e_bf
    assert r.macs == plain.macs and r.n_slices == plain.n_slices == math.prod(2 for _ in res.slices)
    assert r.peak_device_bytes < plain.peak_device_bytes
    assert r.narrow_launches > 0 and r.launches == sum(r.kernel_launches) + r.narrow_launches
    again = ctr.contract_results(tn0, arrays, tn, res, storage="float16", scaling="tensor")
    assert np.array_equal(again.array, r.array) and again.exponents == r.exponents
