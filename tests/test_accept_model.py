"""The Metropolis accept filter of the sweep kernels, without a GPU: is its margin sufficient, GIVEN the error bound it
assumes for the hardware log?  (tests/test_gpu_accept.py measures that bound on the card and tests the shipped code;
tests/accept_cases.py holds the reference and the input families of both.)

The model is the filter's arithmetic in numpy float32 -- its constants READ from csrc/sa_sweep.h and csrc/sa_small.h,
so a change of either copy is a change of the model -- with each log2f replaced by the true value plus or minus the
worst error `2e-7 + 1.2e-7 |result|` allows, in all four sign combinations.  A "sure yes" or "sure no" of the model
must never contradict the exact rule.  Also here: the reference side of the GPU test checked alone (how far the placed
inputs lie from p), and the oracle's glibc pow against the same reference.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import accept_cases as A

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "tnco_amd" / "csrc"
LOG_ABS, LOG_REL = 2e-7, 1.2e-7   # the bound on v_log_f32 the margin is derived from (sa_sweep.h)

MARGIN_RE = re.compile(r"const float margin = \(fabsf\(lp\) \+ fabsf\(lu\)\) \* ([0-9.e+-]+)f \+ fabsf\(bf\) \* ([0-9.e+-]+)f \+ ([0-9.e+-]+)f;")
GUARD_RE = re.compile(r"uf > ([0-9.e+-]+)f && xf < ([0-9.e+-]+)f && fabsf\(lp\) < ([0-9.e+-]+)f && beta >= 0\.0")


def filter_constants(header):
    src = (CSRC / header).read_text()
    m, g = MARGIN_RE.findall(src), GUARD_RE.findall(src)
    assert len(m) == 1 and len(g) == 1, f"{header}: the filter's margin / guard line is not where this test reads it"
    return tuple(float(v) for v in m[0]), tuple(float(v) for v in g[0])


def worst_log2(t32, sign):
    """A float that v_log_f32(t) may return under the assumed bound, as far on the `sign` side of log2 t as it allows."""
    with np.errstate(all="ignore"):
        true = np.log2(t32.astype(np.float64))
        bound = LOG_ABS + LOG_REL * np.abs(true)
        lo, hi = true - bound, true + bound
        v = (true + sign * bound).astype(np.float32)
        # (rounded to a float it may have left the interval: one step back)
        v = np.where(v.astype(np.float64) > hi, np.nextafter(v, np.float32(-np.inf)), v)
        v = np.where(v.astype(np.float64) < lo, np.nextafter(v, np.float32(np.inf)), v)
    return v.astype(np.float32)


def filter_model(c, su, sx, margin, guard):
    """(sure yes, sure no) of the filter for Metropolis cases with delta > 0, total != 0: float32 arithmetic, one rounding
    per operation, as the kernels are compiled (-ffp-contract=off)."""
    f32 = np.float32
    f = int(c["f32"][0])
    x = A.x_of(c["delta"], c["total"], f)
    with np.errstate(all="ignore"):
        uf, xf, bf = c["u"].astype(f32), x.astype(f32), c["beta"].astype(f32)
        lu, lx = worst_log2(uf, su), worst_log2(xf, sx)
        lp = -bf * lx
        m = (np.abs(lp) + np.abs(lu)) * f32(margin[0]) + np.abs(bf) * f32(margin[1]) + f32(margin[2])
        ok = (uf > f32(guard[0])) & (xf < f32(guard[1])) & (np.abs(lp) < f32(guard[2])) & (c["beta"] >= 0.0)
        assert m.dtype == np.float32 and lp.dtype == np.float32
        return ok & (lu < lp - m), ok & (lu > lp + m)


def contradictions(c, ref, margin, guard):
    live = (c["kind"] == 2) & (c["delta"] > 0) & (c["total"] != 0)
    c, ref = A.take(c, live), ref[live]
    bad = np.zeros(ref.size, bool)
    for su in (-1.0, 1.0):
        for sx in (-1.0, 1.0):
            yes, no = filter_model(c, su, sx, margin, guard)
            bad |= (yes & ~ref) | (no & ref)
    return c, bad


@pytest.fixture(scope="module")
def grids():
    return {f: A.grid(f) for f in (0, 1)}


@pytest.fixture(scope="module")
def families(grids):
    out = {}
    for f in (0, 1):
        out["margin bands", f] = A.margin_bands(f, grids[f])
        out["guard edges", f] = A.guard_edges(f)
    return out


def reference(c):
    return A.decide(A.prob_exact(c["kind"], c["f32"], c["beta"], c["delta"], c["total"]), c["u"])


def test_both_copies_of_the_filter_have_the_same_constants():
    assert filter_constants("sa_sweep.h") == filter_constants("sa_small.h")
    assert filter_constants("sa_sweep.h") == ((2e-6, 3e-7, 1e-5), (1e-30, 1e30, 1e30))


@pytest.mark.parametrize("header", ["sa_sweep.h", "sa_small.h"])
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("family", ["margin bands", "guard edges"])
def test_margin_is_sufficient_given_the_instruction_bound(families, family, f32, header):
    margin, guard = filter_constants(header)
    c = families[family, f32]
    cc, bad = contradictions(c, reference(c), margin, guard)
    assert cc["u"].size > 10_000
    i = np.flatnonzero(bad)
    assert i.size == 0, (f"{i.size} of {bad.size} filtered decisions contradict the exact rule, the first: "
                         + str({k: cc[k][i[0]] for k in ("beta", "delta", "total", "u")}))


@pytest.mark.parametrize("f32", [0, 1])
def test_the_model_needs_the_margin_it_has(families, f32):
    """The check above bites: with half the beta coefficient the model contradicts the exact rule in the margin-band family
    (k = 0.25, beta from a few hundred up).  In float32 mode x is a float already, the 8.6e-8 of its rounding is not
    spent, and it takes a quarter."""
    margin, guard = filter_constants("sa_sweep.h")
    c = families["margin bands", f32]
    cc, bad = contradictions(c, reference(c), (margin[0], margin[1] / (4 if f32 else 2), margin[2]), guard)
    assert bad.sum() >= 1000 and (cc["k"][bad] <= 0.5).all() and cc["beta"][bad].min() > 100


@pytest.mark.parametrize("f32", [0, 1])
def test_placed_inputs_lie_far_from_p(families, grids, f32):
    """The reference side of the GPU test alone: every u of the margin-band family is at least 0.25 * 1e-5 * ln 2 of p away
    from it -- 7.8e9 units in the last place of a double, 14.5 of a float -- so a last-place error of any pow cannot
    make one of them ambiguous, and the cap on excluded cases of that family is zero."""
    c = families["margin bands", f32]
    p = c["p_ref"]
    assert np.array_equal(p, A.prob_exact(c["kind"], c["f32"], c["beta"], c["delta"], c["total"]))
    dist = np.abs(c["u"] - p) / A.ulp_of(p, f32)
    print(f"margin bands, float32 mode {f32}: {c['u'].size} cases, least distance from p {dist.min():.4g} ulps")
    assert dist.min() >= (14.0 if f32 else 7.7e9)
    assert c["u"].size >= 200 * 200 * 4 and ((c["u"] > 0) & (c["u"] < 1)).all()
    b = A.rounding_boundary(f32, grids[f32])
    assert np.array_equal(A.ulps_apart(b["u"], b["p_ref"], f32), np.abs(b["ulps"]))
    assert np.array_equal(A.decide(b["p_ref"], b["u"]), b["ulps"] <= 0)


def test_pow_special_values_table():
    inf, nan = np.inf, np.nan
    for x, beta, want in [(nan, 0.0, 1.0), (nan, -0.0, 1.0), (inf, 0.0, 1.0), (1.0, nan, 1.0), (1.0, inf, 1.0), (nan, 1.0, nan),
                          (2.0, nan, nan), (inf, 1.0, 0.0), (inf, 1e-300, 0.0), (inf, -1.0, inf), (2.0, inf, 0.0), (2.0, -inf, inf),
                          (inf, inf, 0.0), (inf, -inf, inf), (2.0, 1.0, 0.5), (4.0, 0.5, 0.5), (2.0, 1074.0, 5e-324), (2.0, 1076.0, 0.0),
                          (2.0, -1024.0, inf)]:
        got = A.pow_exact(x, beta)
        assert (np.isnan(got) and np.isnan(want)) or got == want, (x, beta, got, want)


def test_numpy_pow_stays_inside_the_guard_of_decide_fast():
    """decide_fast lets numpy's pow decide the cases further than 64 ulps from it: numpy's pow against mpmath on a sample of
    the inputs it is used for."""
    c = A.kernel_draws(0, 20_000, seed=5)
    live = (c["kind"] == 2) & (c["delta"] > 0)
    x, beta = A.x_of(c["delta"], c["total"], 0)[live], c["beta"][live]
    p = A.pow_exact_array(x, beta)
    with np.errstate(all="ignore"):
        pn = np.power(x, -beta)
    sel = p > 1e-290
    assert sel.sum() > 5_000
    worst = int(A.ulps_apart(p[sel], pn[sel]).max())
    print(f"numpy pow against the correctly rounded value: at most {worst} ulps over {sel.sum()} inputs")
    assert worst <= 8
    for f in (0, 1):
        c = A.kernel_draws(f, 20_000, seed=6 + f)
        dec, _ = A.decide_fast(c)
        assert np.array_equal(dec, reference(c))


@pytest.mark.parametrize("cost_type", ["float64", "float32"])
def test_oracle_prob_against_the_exact_rule(oracle_lib, grids, cost_type):
    """oracle/tnco_oracle.c `prob` (glibc pow): its distance from the correctly rounded value over the grid of the margin-band
    and rounding-boundary families, the guard-edge family and the edges of the rule."""
    f = int(cost_type == "float32")
    g = grids[f]
    pts = [(2, b, d, 1.0) for b, d in zip(g["beta"], g["delta"])]
    for c in (A.guard_edges(f), A.edges(f)):
        pts += list({(int(k), b, d, t) for k, b, d, t in zip(c["kind"], c["beta"], c["delta"], c["total"])
                     if not (np.isnan(b) or np.isnan(d))})
    nan_pts = [(2, np.nan, 1.0, 1.0), (2, 1.0, np.nan, 1.0), (2, 0.0, np.nan, 1.0), (1, 1.0, np.nan, 1.0)]
    pts += nan_pts
    kind, beta, delta, total = (np.array(v) for v in zip(*pts))
    want = A.prob_exact(kind.astype(np.int32), np.full(kind.size, f, np.int32), beta, delta, total)
    got = np.array([oracle_lib.prob(int(k), b, d, t, cost_type) for k, b, d, t in pts])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    dist = A.ulps_apart(got[fin], want[fin], f)
    print(f"oracle prob ({cost_type}): at most {int(dist.max())} ulps from the correctly rounded value over {fin.sum()} points, "
          f"{int((dist > 0).sum())} of them differ")
    assert dist.max() <= 1   # glibc documents its pow to under one unit in the last place
