"""The Metropolis accept filter of the sweep kernels against the exact rule, on the card, at its margins -- and the two
reciprocal shortcuts next to it.  Every sweep kernel decides `u <= pow(1 + delta/total, -beta)` in the log2 domain from
two bare v_log_f32 and a hand-derived margin (csrc/sa_sweep.h accept_move, csrc/sa_small.h small_accept) and calls the
float64 pow only when u falls inside the margin; a wrong filter decision needs u within ~1e-7 (in log2) of the margin,
where no annealing run ever lands.  Here the shipped functions run through a test-only probe compiled from the product
headers (tests/csrc/accept_probe.hip, built by __graft_entry__.build()):

  (a) the bound on v_log_f32 that the margin is derived from, for EVERY float of the filter's domain [1e-30, 1e30];
  (b) both functions' decisions against a high-precision restatement of the rule (tests/accept_cases.py), on inputs
      placed at fractions and multiples of the margin around p, at p +- a few units in the last place, at the filter's
      guards, at the edges of the rule, and as the kernels draw them; plus the path each decision took;
  (c) small_mod (x % n through a double reciprocal) and fws_divmod (the shuffle's float-reciprocal quotient) against
      integer division over their whole domains.
tests/test_accept_model.py closes the chain without a GPU: the bound of (a) makes the margin sound.
Measured figures: profiles/accept_probe.md.
"""
import ctypes as C
from pathlib import Path

import mpmath
import numpy as np
import pytest

from tests import accept_cases as A

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "csrc" / "libaccept_probe.so"
LOG_ABS, LOG_REL = 2e-7, 1.2e-7   # |v_log_f32(t) - log2 t| <= LOG_ABS + LOG_REL |log2 t|: what sa_sweep.h derives its margin from


@pytest.fixture(scope="module")
def probe():
    if not LIB.exists():
        pytest.fail("tests/csrc/libaccept_probe.so is missing: run __graft_entry__.build()")
    L = C.CDLL(str(LIB))
    p = lambda t: np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS")  # noqa: E731
    L.probe_log2_scan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, p(np.float64)]
    L.probe_log2_at.argtypes = [C.c_int, C.c_int64, p(np.uint32), p(np.float32), p(np.float64)]
    L.probe_accept.argtypes = [C.c_int, C.c_int64, p(np.int32), p(np.int32)] + [p(np.float64)] * 4 + [p(np.uint8)] * 4
    L.probe_pow.argtypes = [C.c_int, C.c_int64, p(np.float64), p(np.float64), p(np.float64)]
    L.probe_small_mod.argtypes = [C.c_int, C.c_uint32, C.c_uint32, p(np.uint64)]
    L.probe_fws_divmod.argtypes = [C.c_int, p(np.uint64)]
    return L


def run_accept(L, c):
    n = c["u"].size
    out = [np.empty(n, np.uint8) for _ in range(4)]
    args = [np.ascontiguousarray(c[k]) for k in ("kind", "f32", "beta", "delta", "total", "u")]
    assert L.probe_accept(0, n, *args, *out) == 0
    move, small, path_move, path_small = out
    assert (path_move <= 4).all() and (path_small <= 4).all()
    return move.astype(bool), small.astype(bool), path_move, path_small


def mp_log2(bits):
    with mpmath.workprec(120):
        return np.array([float(mpmath.log(mpmath.mpf(float(t)), 2)) for t in np.asarray(bits, np.uint32).view(np.float32)])


# ---------------------------------------------------------------------------------------------------------------------
# (a) the instruction bound
# ---------------------------------------------------------------------------------------------------------------------
def test_v_log_f32_meets_the_bound_the_margin_assumes_on_every_float_of_the_domain(probe):
    lo, hi = (int(np.float32(v).view(np.uint32)) for v in (1e-30, 1e30))
    assert hi - lo + 1 > 1_600_000_000
    out = np.zeros(255 * 8)
    assert probe.probe_log2_scan(0, lo, hi, out) == 0
    out = out.reshape(255, 8)
    binades = np.arange(lo >> 23, (hi >> 23) + 1)
    r = out[binades]
    assert (r[:, 0] >= 0).all(), "a binade of the range came back empty"
    # the float64 log2 the device compared with, against mpmath: at every argmax, and at a random sample
    rng = np.random.default_rng(3)
    sample = rng.integers(lo, hi + 1, 100_000).astype(np.uint32)
    dev = np.empty(sample.size, np.float32)
    ref = np.empty(sample.size, np.float64)
    assert probe.probe_log2_at(0, sample.size, sample, dev, ref) == 0
    ref_err = max(np.abs(ref - mp_log2(sample)).max(), np.abs(r[:, 3] - mp_log2(r[:, 1].astype(np.uint32))).max(),
                  np.abs(r[:, 7] - mp_log2(r[:, 5].astype(np.uint32))).max())
    print(f"device float64 log2 against mpmath (120 bits): at most {ref_err:.3g} absolute over {sample.size} random inputs and "
          f"{2 * len(binades)} argmaxes")
    assert ref_err <= 1e-12
    # (the sample again, through the other entry point: the scan's reduction cannot have hidden a worse input among these)
    assert (np.abs(dev.astype(np.float64) - ref) <= LOG_ABS + LOG_REL * np.abs(ref)).all()
    f = lambda bits: float(np.uint32(bits).view(np.float32))  # noqa: E731
    near1 = (binades == 126) | (binades == 127)
    i, j, k = np.argmax(np.where(near1, r[:, 0], -1)), np.argmax(r[:, 0]), np.argmax(r[:, 4])
    rel = r[:, 0] / np.maximum(np.abs(r[:, 3]), 1e-300)
    m = np.argmax(np.where(near1, -1, rel))
    print(f"v_log_f32 over {hi - lo + 1} floats in [1e-30, 1e30]:")
    print(f"  near 1 (t in [0.5, 2)): max |err| = {r[i, 0]:.4g} at t = {f(r[i, 1])!r} (bits {int(r[i, 1]):#x})")
    print(f"  whole range: max |err| = {r[j, 0]:.4g} at t = {f(r[j, 1])!r}, log2 t = {r[j, 3]:.6g}")
    print(f"  relative to the result outside [0.5, 2): max |err| / |log2 t| = {rel[m]:.4g} at t = {f(r[m, 1])!r}")
    print(f"  max of |err| - {LOG_REL} |log2 t| = {r[k, 4]:.4g} (allowed: {LOG_ABS}) at t = {f(r[k, 5])!r}")
    bad = ~(r[:, 4] <= LOG_ABS)
    assert not bad.any(), [(int(b), r[n, 4], f(r[n, 5])) for n, b in enumerate(binades) if bad[n]]


# ---------------------------------------------------------------------------------------------------------------------
# (b) decisions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids():
    return {f: A.grid(f) for f in (0, 1)}


@pytest.fixture(scope="module")
def pow_E(probe, grids):
    """E: the largest distance, in units in the last place, between the device's pow and the correctly rounded value over
    the test's own (x, beta) grid -- float64's, and a float's after the conversion of float32 mode."""
    E = {}
    for f in (0, 1):
        g = grids[f]
        sel = (g["p64"] >= 1e-300) & np.isfinite(g["p64"])
        x, beta = np.ascontiguousarray(g["x"][sel]), np.ascontiguousarray(g["beta"][sel])
        got = np.empty(x.size)
        assert probe.probe_pow(0, x.size, x, beta, got) == 0
        d = A.ulps_apart(got, g["p64"][sel])
        E[f] = int(A.ulps_apart(got, g["p64"][sel], True).max()) if f else int(d.max())
        print(f"device pow against the correctly rounded value, float32 mode {f}: E = {E[f]} ulps over {x.size} grid points "
              f"({int((d > 0).sum())} differ in float64)")
    return E


def reference(c):
    return A.decide(A.prob_exact(c["kind"], c["f32"], c["beta"], c["delta"], c["total"]), c["u"])


def check(probe, name, c, ref, ambiguous=None):
    """Both functions against the reference on every case that is not ambiguous; small_accept (float64 only) also against
    accept_move on every case.  Returns the paths."""
    f32 = int(c["f32"][0])
    move, small, path_move, path_small = run_accept(probe, c)
    amb = np.zeros(ref.size, bool) if ambiguous is None else ambiguous
    print(f"{name}, float32 mode {f32}: {ref.size} cases, {int(amb.sum())} ambiguous, accept_move paths "
          f"{dict(zip(A.PATHS, np.bincount(path_move, minlength=5).tolist()))}")
    show = lambda i: {k: c[k][i] for k in ("kind", "beta", "delta", "total", "u")}  # noqa: E731
    bad = np.flatnonzero((move != ref) & ~amb)
    assert bad.size == 0, f"{name}: accept_move differs from the exact rule on {bad.size} cases, the first {show(bad[0])}, path {path_move[bad[0]]}"
    if f32 == 0:
        print(f"    small_accept paths {dict(zip(A.PATHS, np.bincount(path_small, minlength=5).tolist()))}")
        bad = np.flatnonzero((small != ref) & ~amb)
        assert bad.size == 0, f"{name}: small_accept differs from the exact rule on {bad.size} cases, the first {show(bad[0])}, path {path_small[bad[0]]}"
        bad = np.flatnonzero(small != move)
        assert bad.size == 0, f"{name}: small_accept != accept_move on {bad.size} cases, the first {show(bad[0])}"
    return path_move, path_small


@pytest.mark.parametrize("f32", [0, 1])
def test_edges_of_the_rule(probe, f32):
    c = A.edges(f32)
    assert c["u"].size == 3 * 8 * 5 * 10 * 5
    pm, ps = check(probe, "edges of the rule", c, reference(c))
    # the early paths of both functions: reached here, not in the families below (all Metropolis moves uphill)
    for path in (pm, ps):
        assert (np.bincount(path, minlength=5)[:2] >= 1000).all()


@pytest.mark.parametrize("f32", [0, 1])
def test_margin_bands(probe, grids, f32):
    """u = p 2^(+-k m) around every grid point: no case is excluded.  Path counts: the filter still decides (it has not
    degraded to "always exact") and the exact pow is still reached; k = 8 lies outside the margin, so those cases take the
    filter, on the reference's side -- unless the guard u > 1e-30 sends them to the pow.  (The two early paths cannot occur
    in this family -- delta > 0, total = 1 -- and are counted in test_edges_of_the_rule.)"""
    c = A.margin_bands(f32, grids[f32])
    ref = reference(c)
    pm, ps = check(probe, "margin bands", c, ref)
    far = (c["k"] == 8.0) & (c["u"].astype(np.float32) > np.float32(1e-30))
    assert far.sum() > 10_000
    for name, path in (("accept_move", pm),) + ((("small_accept", ps),) if f32 == 0 else ()):
        counts = np.bincount(path, minlength=5)
        assert (counts[2:] >= 1000).all(), (name, counts)
        assert np.array_equal(path[far], np.where(ref[far], 2, 3)), name


@pytest.mark.parametrize("f32", [0, 1])
def test_rounding_boundary(probe, grids, pow_E, f32):
    """u = p moved by 0, +-1, ... +-4096 units in the last place.  Ambiguous -- the device's pow and the correctly rounded
    one may differ in the last place -- is a case within E units of p, E measured above: nothing else
    is excluded, and E must stay below 256."""
    E = pow_E[f32]
    assert E < 256 and (f32 == 0 or E <= 1)
    c = A.rounding_boundary(f32, grids[f32])
    amb = np.abs(c["ulps"]) <= E if E else np.zeros(c["u"].size, bool)
    assert np.isin(np.abs(c["ulps"][amb]), [k for k in A.ULP_OFFSETS if abs(k) <= E]).all()
    check(probe, "rounding boundary", c, reference(c), amb)


@pytest.mark.parametrize("f32", [0, 1])
def test_guard_edges(probe, f32):
    c = A.guard_edges(f32)
    check(probe, "guard edges", c, reference(c))


@pytest.mark.parametrize("f32,n", [(0, 10_000_000), (1, 2_500_000)])
def test_as_the_kernels_draw_them(probe, f32, n):
    step, slow = 2_500_000, 0
    for i in range(n // step):
        c = A.kernel_draws(f32, step, seed=100 + 10 * i + f32)
        ref, k = A.decide_fast(c)
        slow += k
        check(probe, f"kernel draws {i}", c, ref)
    print(f"    mpmath decided {slow} of {n} cases")


# ---------------------------------------------------------------------------------------------------------------------
# (c) the reciprocal shortcuts
# ---------------------------------------------------------------------------------------------------------------------
def test_small_mod_is_the_remainder_for_every_leaf_count(probe):
    """small_mod(x, n, 1.0 / n) == x % n for x in {q n - 1, q n, q n + 1} of every quotient q, 0, 2^31 +- 1, 2^32 - 1 and every
    n = 2 ... 65535: what its comment claims (n < 2^16), a superset of what the LDS-resident kernels pass -- SmallStore
    up to 128 leaves, WideStore / LdsPlan at most 32 767 (2 n - 1 <= 65 534 nodes behind 16-bit links, tnco_hip.hip) and in
    practice what 160 KiB of LDS hold at >= 50 bytes per node."""
    out = np.zeros(3, np.uint64)
    assert probe.probe_small_mod(0, 2, 65535, out) == 0
    assert out[0] == 0, f"{out[0]} mismatches, one at x = {out[1]}, n = {out[2]}"


def test_fws_divmod_over_its_whole_domain(probe):
    """fw_wave.h fws_divmod: dv = 2 ... 129, every x < dv (dv - 1).  The call site: dv = i0 + 2, i0 = base + 2 lane with
    base <= 1 and lane <= 63, x = (raw * range) >> 32 < range = (i0 + 1)(i0 + 2)."""
    out = np.zeros(3, np.uint64)
    assert probe.probe_fws_divmod(0, out) == 0
    assert out[0] == 0, f"{out[0]} mismatches, one at x = {out[1]}, dv = {out[2]}"
