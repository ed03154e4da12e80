"""The ways of running a plan that change when and from where a step runs, on the device, over the networks of
tests/schedule_cases.py (the random networks of tests/mode_cases.py and a few more): `hoist=True`, `reuse=True`,
`slice_order=`, `indirect=True` and `compute="matrix"`.  The hand-made tables of those features share one structure; here
the C++ that executes their tables -- the phase loop, the permute groups with rows of several periods, the hoisted phase
in a slice batch, folded leaves at a slice offset, the matrix kernel fed from kept buffers -- sees plans nobody drew.

Per case, in this order (every bound is `mode_cases.plain_bound`, (c kt + 2) u mag; no number is new):

    plain       once per order of the sliced indices that the case is run in (the default one, the default one back to
                front, the one `slice_order="reuse"` chooses), element by element against numpy's einsum of the network in
                float64 / complex128 over the assignments that the order puts in `slice_range`;
    hoist       unbatched and with slice_batch 3 and 64: the bytes of the plain run; `hoisted` and `macs` those of the
                plan, no more than the plain ones; every launch count from the plan (tests/indirect_cases.py
                launch_counts): the hoisted share once, the rest per group of assignments;
    reuse       in the three orders, each against the run without the keyword in the same order: equal bytes, every launch
                count and `macs` those of tests/reuse_cases.py predicted, the change of `peak_device_bytes` the plans';
                under another order than the default the result is also held to that order's reference (the assignments
                are summed in another order: only the bound ties it to the default); a second call gives the same bytes;
    indirect    alone, with slice_batch 3, with hoist, with both, with reuse and with reuse in the order "reuse" chooses:
                the bytes of the same call without the keyword, `indirect` the plan's, `kernel_launches` and
                `indirect_launches` those predicted; with nothing folded also equal launches and device memory;
    matrix      in each of the four dtypes: alone, with slice_batch 3, with hoist and with reuse byte-equal to each other;
                `matrix_launches` the tiled-class steps times the runs the schedule gives them; without a tiled-class step
                the bytes of the plain run of that dtype, with one the reference's bound.

What is skipped is decided from the plan (an order that equals one already run; the bound where no tiled-class step
changes the bytes), never from a result.  tests/test_contraction_schedule_plan.py shows without a device that the table
reaches every item of `schedule_cases.REQUIRED_SCHEDULE` and that a correct contraction meets the bound on these inputs.
`check_case` is also what tools/fuzz_contract.py runs over seeds beyond the table.
"""
import functools

import numpy as np
import pytest

from tests import indirect_cases as ic
from tests import mode_cases as mc
from tests import reuse_cases as rc
from tests import schedule_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctr():
    from tnco_amd import contraction
    return contraction


def bits(a):
    """The bytes of an array as unsigned integers: NaN patterns and signed zeros count."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


@functools.lru_cache(maxsize=8)
def leaves(case):
    arrays = mc.fill(case)
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=16)
def _reference(case, slice_inds):
    return mc.reference(case, case.plan(slice_order=slice_inds), leaves(case))


def reference(case, slice_inds):
    """(the einsum of the network in double precision, the same of the moduli) under an order of the sliced indices: the
    order decides which assignments a slice_range holds, and nothing else."""
    return _reference(case, tuple(slice_inds) if case.slice_range is not None else None)


def _ratio(r, ref, bound, what, out):
    got = np.asarray(r.array)
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    err = np.abs(got.astype(ref.dtype) - ref)
    ratio = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())
    out(f"{what}: largest error / bound {ratio:.4f}")
    assert (err <= bound).all(), what
    return ratio


def _total(counts, G):
    """(kernel_launches, indirect_launches) of a call from `indirect_cases.launch_counts`: once + G x per."""
    once, per = counts
    return tuple(tuple(a + G * b for a, b in zip(o, q)) for o, q in zip(once, per))


def check_case(ctr, case, out=print):
    """Run `case` in every schedule and assert the module docstring; returns the largest error / bound per mode."""
    what = f"{case.name} {case.dtype}"
    P = sc.Plans(case)
    n = case.n_assignments()
    default = P.plain.slice_inds
    ratios = {}

    def call(c=case, **kw):
        return ctr.contract(list(c.path), c.ts_inds, list(leaves(c)), c.output_inds, slices=c.slices,
                            slice_range=c.slice_range, **kw)

    ran = {}

    def run(**kw):
        """The result of the case's call with these keywords, run once (an order by its tuple, the default one by none)."""
        if kw.get("slice_order") == default:
            del kw["slice_order"]
        key = tuple(sorted(kw.items()))
        if key not in ran:
            ran[key] = call(**kw)
        return ran[key]

    def in_order(inds):
        return {} if inds == default else dict(slice_order=inds)

    # 1. plain, once per order, against the reference of that order
    orders = list(dict.fromkeys(P.reuse[o].slice_inds for o in sc.ORDERS))
    assert orders[0] == default and len(orders) <= 3, what
    for inds in orders:
        q = case.plan(**in_order(inds))
        r = run(**in_order(inds))
        ref, mag = reference(case, inds)
        assert r.inds == q.inds and r.array.dtype == np.dtype(case.dtype) and r.n_slices == n and r.macs == q.macs, what
        key = "plain" if inds == default else "order"
        ratios[key] = max(ratios.get(key, 0.0), _ratio(r, ref, mc.plain_bound(case, q, mag), f"{what} plain, order {inds} (kt {mc.kt(q)})", out))
    base = run()

    # 2. hoist=True, unbatched and in slice batches
    p = P.hoist
    assert p.macs <= P.plain.macs, what
    for B in (None,) + sc.BATCHES:
        kw = {} if B is None else dict(slice_batch=B)
        tag = f"{what} hoist {kw}"
        r, G = run(hoist=True, **kw), ic.groups(n, B)
        assert r.inds == base.inds and np.array_equal(bits(r.array), bits(base.array)), f"{tag}: differs from the plain run"
        assert r.hoisted == p.hoisted and r.macs == p.macs <= base.macs and r.n_slices == n, tag
        assert r.slice_batch == (None if B is None else min(B, n)), tag
        kernel, through = _total(ic.launch_counts(p), G)
        assert r.kernel_launches == kernel and r.indirect_launches == through == (0, 0, 0), (tag, r.kernel_launches, kernel)
        assert r.batch_launches == (0 if B is None else G) and r.launches == sum(kernel) + r.batch_launches, tag
        assert r.row_kernel_launches == (0, 0, 0) and r.path_launches == (0, 0) and r.matrix_launches == 0, tag

    # 3. reuse=True in the three orders
    done = set()
    for order in (None, "reuse", "reversed"):  # ("reuse" before the named order: where they agree the word is what is passed)
        p = P.reuse[order]
        if p.slice_inds in done:  # (from the plan: this order has been run)
            continue
        done.add(p.slice_inds)
        tag = f"{what} reuse, order {order} {p.slice_inds}"
        q = case.plan(**in_order(p.slice_inds))
        plain = run(**in_order(p.slice_inds))
        kw = rc.order_kw(case, order)
        r = ran[tuple(sorted(dict(reuse=True, **in_order(p.slice_inds)).items()))] = call(reuse=True, **kw)
        want = rc.predicted(p)
        assert r.inds == plain.inds and np.array_equal(bits(r.array), bits(plain.array)), f"{tag}: differs from the run without reuse"
        assert r.reused == p.reused and plain.reused is None and r.hoisted is None and r.n_slices == n, tag
        assert r.macs == p.macs == want["macs"] <= plain.macs == q.macs, tag
        # (fewer iff some step is not due at every assignment of the range: a period above 1 can still be, in a short range)
        assert (r.macs < plain.macs) == any(rc.runs(int(per), *p.slice_range) < n for per in p.step_period), tag
        assert r.kernel_launches == want["kernel"], (tag, r.kernel_launches, want["kernel"])
        assert plain.kernel_launches == rc.predicted(q)["kernel"], tag
        assert r.indirect_launches == want["indirect"] == (0, 0, 0) and r.narrow_launches == r.split_launches == r.matrix_launches == 0, tag
        assert r.launches == want["launches"] == sum(r.kernel_launches), tag
        assert r.batch_launches == 0 and r.row_kernel_launches == (0, 0, 0) and r.path_launches == (0, 0), tag
        assert r.peak_device_bytes - plain.peak_device_bytes == p.peak_device_bytes - q.peak_device_bytes, tag
        if p.slice_inds != default:
            ref, mag = reference(case, p.slice_inds)
            ratios["order"] = max(ratios.get("order", 0.0), _ratio(r, ref, mc.plain_bound(case, q, mag), tag, out))
        again = call(reuse=True, **kw)
        assert np.array_equal(bits(again.array), bits(r.array)), f"{tag}: a second call differs"

    # 4. indirect=True beside each of the others
    chosen = in_order(P.indirect_reuse["reuse"].slice_inds)
    assert P.indirect_reuse["reuse"].slice_inds == P.reuse["reuse"].slice_inds, what
    settings = [dict(), dict(slice_batch=sc.BATCH), dict(hoist=True), dict(hoist=True, slice_batch=sc.BATCH),
                dict(reuse=True)] + ([dict(reuse=True, **chosen)] if chosen else [])  # (from the plan: "reuse" moves the order)
    for kw in settings:
        tag = f"{what} indirect {kw}"
        p, p0 = case.plan(indirect=True, **kw), case.plan(**kw)
        asked = dict(kw, slice_order="reuse") if "slice_order" in kw else kw
        same, r = run(**kw), call(indirect=True, **asked)
        assert r.inds == same.inds and np.array_equal(bits(r.array), bits(same.array)), f"{tag}: differs from the run without indirect"
        assert r.indirect == p.indirect and same.indirect is None and r.macs == same.macs == p.macs and r.n_slices == n, tag
        if "reuse" in kw:
            want = rc.predicted(p)
            kernel, through = want["kernel"], want["indirect"]
            assert r.reused == p.reused and r.launches == want["launches"], tag
        else:
            kernel, through = _total(ic.launch_counts(p), ic.groups(n, kw.get("slice_batch")))
            assert r.hoisted == p.hoisted and r.slice_batch == same.slice_batch and r.batch_launches == same.batch_launches, tag
            assert r.launches == sum(kernel) + sum(through) + r.batch_launches, tag
        assert r.kernel_launches == kernel and r.indirect_launches == through, (tag, r.kernel_launches, kernel, r.indirect_launches, through)
        assert (sum(through) > 0) == (p.indirect > 0), tag
        if p.indirect == 0:
            assert r.launches == same.launches and r.kernel_launches == same.kernel_launches, tag
            assert r.peak_device_bytes == same.peak_device_bytes and p.peak_device_bytes == p0.peak_device_bytes, tag

    # 5. compute="matrix" in the four dtypes
    for dtype in sc.DTYPES:
        c = case.with_(dtype=dtype)
        tag = f"{case.name} {dtype} matrix"
        q = c.plan(compute="matrix")
        tiled = [k for k, s in enumerate(mc.signature(q)) if s[0] == "tiled"]
        plain = base if dtype == case.dtype else call(c)
        G = ic.groups(n, sc.BATCH)
        hp = c.plan(compute="matrix", hoist=True)
        runs = dict(alone=(dict(), len(tiled) * n), batch=(dict(slice_batch=sc.BATCH), len(tiled) * G),
                    hoist=(dict(hoist=True), sum(1 if hp.step_hoist[k] else n for k in tiled)),
                    reuse=(dict(reuse=True), rc.predicted(c.plan(compute="matrix", reuse=True))["matrix"]))
        first = None
        for name, (kw, launches) in runs.items():
            r = call(c, compute="matrix", **kw)
            assert r.array.dtype == np.dtype(dtype) and r.inds == plain.inds and r.n_slices == n, (tag, name)
            assert r.matrix_launches == launches, (tag, name, r.matrix_launches, launches)
            first = r if first is None else first
            assert np.array_equal(bits(r.array), bits(first.array)), f"{tag}: the run '{name}' differs from the run alone"
        if not tiled:  # (from the plan: matrix mode changes no step)
            assert np.array_equal(bits(first.array), bits(plain.array)), f"{tag}: no tiled step, yet not the plain bytes"
        else:
            ref, mag = reference(c, default)
            ratios["matrix"] = max(ratios.get("matrix", 0.0), _ratio(first, ref, mc.plain_bound(c, q, mag), f"{tag} ({len(tiled)} tiled)", out))
    return ratios


@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_every_schedule_on_a_random_network(ctr, case):
    check_case(ctr, case)
