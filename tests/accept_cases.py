"""The Metropolis accept rule `u <= pow(1 + delta/total, -beta)` restated in high precision, and the input families
that aim at the margins of the kernels' log2-domain filter (csrc/sa_sweep.h accept_move, csrc/sa_small.h
small_accept).  Shared by tests/test_accept_model.py (no GPU: a float32 model of the filter, the oracle's `prob`) and
tests/test_gpu_accept.py (the shipped functions through tests/csrc/accept_probe.hip).

The reference: x = 1 + delta/total in IEEE float64 (numpy), each operation rounded to float in float32 mode as
rnd_cost does; p = mpmath.power(x, -beta) at 240 bits rounded ONCE to float64, then to float in float32 mode
(oracle/tnco_oracle.c `prob`: computed in double, converted on return); the decision is u <= p.  Special operands
follow C99 Annex F `pow` (F.9.4.4), written out in pow_special() below -- nothing here comes from the device.
"""
from __future__ import annotations

import itertools
import math

import mpmath
import numpy as np

PREC = 240
F32_TINY = float(np.float32(2.0 ** -149))   # smallest float denormal
F64_TINY = 5e-324                           # smallest double denormal
ONE_M = 1.0 - 2.0 ** -53                    # nextafter(1, 0): the largest u uniform01 returns
PATHS = ("early yes", "early zero", "filter yes", "filter no", "exact")
MARGIN_K = (0.25, 0.5, 0.9, 0.99, 1.01, 1.1, 2.0, 8.0)
ULP_OFFSETS = (0, 1, -1, 2, -2, 4, -4, 16, -16, 256, -256, 4096, -4096)


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def to_f32(a):
    with np.errstate(all="ignore"):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def x_of(delta, total, f32):
    """1 + delta/total as the rule computes it (mh.hpp:58): float64, or every operation rounded to float."""
    delta, total = np.asarray(delta, np.float64), np.asarray(total, np.float64)
    with np.errstate(all="ignore"):
        if f32:
            return to_f32(1.0 + to_f32(delta / total))
        return 1.0 + delta / total


def round_to_double(p) -> float:
    """A positive mpf rounded once, to nearest even, to float64 (gradual underflow and overflow included)."""
    if p == 0:
        return 0.0
    man, exp = int(p.man), int(p.exp)
    assert man > 0
    e = exp + man.bit_length()              # p in [2^(e-1), 2^e)
    if e > 1025:
        return math.inf
    if e < -1075:
        return 0.0
    lsb = max(e - 53, -1074)
    shift = lsb - exp
    if shift <= 0:
        m = man << -shift
    else:
        m, r = divmod(man, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and (m & 1)):
            m += 1
    try:
        return math.ldexp(m, lsb)
    except OverflowError:
        return math.inf


def pow_special(x: float, y: float):
    """C99 Annex F pow(x, y) where it is not an ordinary finite computation, for x >= 0 or NaN (the rule's x is
    1 + delta/total with delta > 0, total > 0: never negative); None otherwise."""
    if y == 0:
        return 1.0                              # pow(x, +-0) = 1 for any x, even a NaN
    if x == 1:
        return 1.0                              # pow(+1, y) = 1 for any y, even a NaN
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x < 0:
        raise ValueError("the rule never raises a negative base")
    if math.isinf(y):
        if x < 1:
            return math.inf if y < 0 else 0.0   # pow(|x| < 1, -inf) = +inf, pow(|x| < 1, +inf) = +0
        return 0.0 if y < 0 else math.inf       # pow(|x| > 1, -inf) = +0,   pow(|x| > 1, +inf) = +inf
    if math.isinf(x):
        return 0.0 if y < 0 else math.inf       # pow(+inf, y < 0) = +0, pow(+inf, y > 0) = +inf
    if x == 0:
        return math.inf if y < 0 else 0.0       # pow(+0, y < 0) = +inf, pow(+0, y > 0) = +0
    return None


_pow_cache: dict = {}


def pow_exact(x: float, beta: float) -> float:
    """pow(x, -beta) correctly rounded to float64."""
    x, y = float(x), -float(beta)
    key = (x, y)
    if key in _pow_cache:
        return _pow_cache[key]
    s = pow_special(x, y)
    if s is None:
        with mpmath.workprec(PREC):
            s = round_to_double(mpmath.power(mpmath.mpf(x), mpmath.mpf(y)))
    if len(_pow_cache) < 2_000_000:
        _pow_cache[key] = s
    return s


def pow_exact_array(x, beta):
    x, beta = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(beta, np.float64))
    out = np.empty(x.shape, np.float64)
    fo, fx, fb = out.reshape(-1), x.reshape(-1), beta.reshape(-1)
    for i in range(fx.size):
        fo[i] = pow_exact(fx[i], fb[i])
    return out


def prob_exact(kind, f32, beta, delta, total):
    """The acceptance probability of base.hpp / greedy.hpp / mh.hpp per element, as float64 (a float's value in float32
    mode)."""
    kind, f32 = np.asarray(kind), np.asarray(f32)
    beta, delta, total = (np.asarray(a, np.float64) for a in (beta, delta, total))
    p = np.empty(kind.shape, np.float64)
    for f in (0, 1):
        sel = f32 == f
        if not sel.any():
            continue
        x = x_of(delta[sel], total[sel], f)
        pp = np.zeros(x.shape, np.float64)
        k, d, t = kind[sel], delta[sel], total[sel]
        one = (k == 0) | (d <= 0)
        zero = ~one & ((k == 1) | (t == 0))
        mh = ~one & ~zero
        pp[one] = 1.0
        pp[mh] = pow_exact_array(x[mh], beta[sel][mh])
        p[sel] = to_f32(pp) if f else pp
    return p


def decide(p, u):
    with np.errstate(invalid="ignore"):
        return np.asarray(u, np.float64) <= p       # (False against a NaN)


def ulps_apart(a, b, f32=False):
    """Distance of two non-negative finite values in units in the last place (of float64, or of float)."""
    if f32:
        ia = np.asarray(a, np.float64).astype(np.float32).view(np.int32).astype(np.int64)
        ib = np.asarray(b, np.float64).astype(np.float32).view(np.int32).astype(np.int64)
    else:
        ia, ib = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def ulp_of(p, f32=False):
    p = np.asarray(p, np.float64)
    if f32:
        q = p.astype(np.float32)
        return (np.nextafter(q, np.float32(np.inf)) - q).astype(np.float64)
    return np.nextafter(p, np.inf) - p


def margin_of(beta, lp, lu):
    """The filter's margin formula.  It only PLACES inputs; nothing is asserted against it."""
    return (np.abs(lp) + np.abs(lu)) * 2e-6 + np.abs(beta) * 3e-7 + 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# input families: dicts of equally long arrays kind, f32 (int32), beta, delta, total, u (float64) + family-specific keys
# ---------------------------------------------------------------------------------------------------------------------
def _pack(f32, kind, beta, delta, total, u, **extra):
    beta, delta, total, u = np.broadcast_arrays(*(np.asarray(a, np.float64) for a in (beta, delta, total, u)))
    n = u.size
    c = {"kind": np.full(n, kind, np.int32) if np.isscalar(kind) else np.asarray(kind, np.int32).reshape(-1),
         "f32": np.full(n, int(f32), np.int32),
         "beta": beta.reshape(-1).copy(), "delta": delta.reshape(-1).copy(), "total": total.reshape(-1).copy(),
         "u": u.reshape(-1).copy()}
    if f32:  # a float32 optimizer holds its costs as floats
        c["delta"], c["total"] = to_f32(c["delta"]), to_f32(c["total"])
    for k, v in extra.items():
        c[k] = np.asarray(v).reshape(-1).copy()
    return c


def concat(cases):
    keys = set(cases[0])
    for c in cases:
        keys &= set(c)
    return {k: np.concatenate([c[k] for c in cases]) for k in keys}


def take(c, sel):
    return {k: v[sel] for k, v in c.items()}


def edges(f32):
    """The full product of the rule's edge operands (in float32 mode the denormal and the huge cost are a float's)."""
    tiny, huge = (F32_TINY, 1e30) if f32 else (F64_TINY, 1e300)
    kinds = (0, 1, 2)
    deltas = (-math.inf, -1.0, -0.0, 0.0, tiny, 1.0, math.inf, math.nan)
    totals = (0.0, tiny, 1.0, huge, math.inf)
    betas = (-1.0, -0.0, 0.0, 1e-300, 1.0, 100.0, 1e6, 1e300, math.inf, math.nan)
    us = (0.0, 2.0 ** -64, 2.0 ** -53, 0.5, ONE_M)
    rows = np.array(list(itertools.product(kinds, deltas, totals, betas, us)), np.float64)
    return _pack(f32, rows[:, 0].astype(np.int32), rows[:, 3], rows[:, 1], rows[:, 2], rows[:, 4])


def grid(f32, nb=200, nx=200):
    """beta log-spaced over [1e-3, 1e8] x (x - 1) log-spaced over [2^-52, 2^40]; total = 1.  The grid points and their
    correctly rounded p (a float's value in float32 mode)."""
    beta = np.logspace(-3, 8, nb)
    d = 2.0 ** np.linspace(-52, 40, nx)
    B, D = (a.reshape(-1) for a in np.meshgrid(beta, d, indexing="ij"))
    if f32:
        D = to_f32(D)
    x = x_of(D, np.ones_like(D), f32)
    p64 = pow_exact_array(x, B)
    return {"beta": B, "delta": D, "x": x, "p64": p64, "p": to_f32(p64) if f32 else p64}


def _placeable(g, f32):
    """Grid points whose p is a normal number with room below it (a u = p 2^(+-k m) or p -+ 4096 ulps exists, distinct
    from p and inside (0, 1)).  Where p underflows the filter's guard u > 1e-30 sends every u to the exact pow anyway."""
    return (g["p"] >= (1e-36 if f32 else 1e-300)) & (g["p"] <= 1.0)


def margin_bands(f32, g=None):
    """Per grid point u = p 2^(s k m), s = +-1, k in MARGIN_K, m the margin formula there; 0 < u < 1."""
    g = g or grid(f32)
    ok = _placeable(g, f32)
    beta, delta, x, p = (g[k][ok] for k in ("beta", "delta", "x", "p"))
    with np.errstate(all="ignore"):
        lp = np.log2(p)
    m = margin_of(beta, lp, lp)
    out = []
    for s in (-1.0, 1.0):
        for k in MARGIN_K:
            u = p * np.exp2(s * k * m)
            keep = (u > 0) & (u < 1) & (u != p)
            out.append(_pack(f32, 2, beta[keep], delta[keep], 1.0, u[keep], k=np.full(keep.sum(), k), s=np.full(keep.sum(), s),
                             p_ref=p[keep]))
    return concat(out)


def rounding_boundary(f32, g=None):
    """Per grid point u = p moved by ULP_OFFSETS units in the last place of p (float64's, or float's in float32 mode)."""
    g = g or grid(f32)
    ok = _placeable(g, f32)
    beta, delta, p = (g[k][ok] for k in ("beta", "delta", "p"))
    out = []
    for k in ULP_OFFSETS:
        if f32:
            u = (p.astype(np.float32).view(np.int32) + np.int32(k)).view(np.float32).astype(np.float64)
        else:
            u = (p.view(np.int64) + np.int64(k)).view(np.float64)
        keep = (u > 0) & (u < 1)
        out.append(_pack(f32, 2, beta[keep], delta[keep], 1.0, u[keep], ulps=np.full(keep.sum(), k), p_ref=p[keep]))
    return concat(out)


def _around_p(f32, beta, delta, total, offsets=(-8.0, -2.0, -1.01, -0.5, 0.5, 1.01, 2.0, 8.0), extra_u=()):
    """For every (beta, delta, total): u = p 2^(j m) for the offsets j (m the margin formula) and the given extra u."""
    beta, delta, total = (a.reshape(-1) for a in np.broadcast_arrays(*(np.asarray(a, np.float64) for a in (beta, delta, total))))
    if f32:
        delta, total = to_f32(delta), to_f32(total)
    x = x_of(delta, total, f32)
    p = pow_exact_array(x, beta)
    if f32:
        p = to_f32(p)
    out = []
    with np.errstate(all="ignore"):
        lp = np.log2(p)
        m = margin_of(beta, lp, lp)
        for j in offsets:
            u = p * np.exp2(j * m)
            keep = np.isfinite(u) & (u > 0) & (u < 1)
            out.append(_pack(f32, 2, beta[keep], delta[keep], total[keep], u[keep]))
    for u in extra_u:
        out.append(_pack(f32, 2, beta, delta, total, u))
    return concat(out)


def guard_edges(f32):
    """Inputs at the filter's guards: u around 1e-30, x around 1e30, beta log2 x around 1e30, (float)u == 1,
    (float)x == 1, (float)beta == inf, beta denormal, beta < 0."""
    out = []
    f1e30 = np.float32(1e-30)
    near = [float(f1e30), float(np.nextafter(f1e30, np.float32(0))), float(np.nextafter(f1e30, np.float32(1)))]
    mids = [(near[0] + near[1]) / 2, (near[0] + near[2]) / 2]
    us = list(np.logspace(-31, -29, 81)) + near + mids + [np.nextafter(v, s) for v in mids + near for s in (0.0, 1.0)]
    us = np.array(us, np.float64)
    # (a) u across the guard: for a few x, the beta that puts p = x^-beta within a few margins of every u
    lu = np.log2(us)
    for xm1 in (2.0 ** -20, 0.5, 1.0, 999.0):
        beta0 = -lu / math.log2(float(x_of(xm1, 1.0, f32)))
        for j in (-2.0, -1.01, -0.5, -0.25, 0.25, 0.5, 1.01, 2.0):  # (never 0: u would sit on p to the last place)
            beta = beta0 * (1.0 + j * margin_of(beta0, lu, lu) / np.abs(lu))
            out.append(_pack(f32, 2, beta, xm1, 1.0, us))
    # (b) x across 1e29 ... 1e31
    g1e30 = np.float32(1e30)
    xs = list(np.logspace(29, 31, 41)) + [float(g1e30), float(np.nextafter(g1e30, np.float32(0))), float(np.nextafter(g1e30, np.float32(np.inf)))]
    xs += [np.nextafter(v, s) for v in xs[-3:] for s in (0.0, math.inf)]
    B, D = np.meshgrid(np.array([0.01, 0.1, 0.3, 1.0]), np.array(xs), indexing="ij")
    out.append(_around_p(f32, B, D, 1.0, extra_u=(2.0 ** -64, 0.5, ONE_M)))
    # (c) beta log2 x across 1e29 ... 1e31: p = 0 (also against u whose float is a denormal, or zero)
    for xm1 in (1.0, 2.0 ** -20):
        lx = math.log2(float(x_of(xm1, 1.0, f32)))
        B, U = np.meshgrid(np.logspace(29, 31, 41) / lx, np.array([1e-300, 1e-46, 1e-40, 2.0 ** -64, 1e-29, 0.5, ONE_M]), indexing="ij")
        out.append(_pack(f32, 2, B, xm1, 1.0, U))
    # (d) (float)u == 1, p close to 1 as well
    ks = np.arange(25, 54)
    B, D, U = np.meshgrid(np.array([1e-3, 1.0, 100.0, 1e4, 1e6]), 2.0 ** np.array([-52.0, -40.0, -30.0, -26.0, -23.0, -20.0]),
                          1.0 - 2.0 ** -ks.astype(np.float64), indexing="ij")
    out.append(_pack(f32, 2, B, D, 1.0, U))
    # (e) (float)x == 1 in float64 mode; in float32 mode x itself is 1 below 2^-24
    B, D = np.meshgrid(np.logspace(0, 12, 25), 2.0 ** -np.arange(25.0, 53.0), indexing="ij")
    out.append(_around_p(f32, B, D, 1.0, extra_u=(0.5, 1.0 - 2.0 ** -30, ONE_M)))
    # (f) (float)beta == inf, beta denormal, beta < 0
    B, D, U = np.meshgrid(np.array([3.5e38, 1e39, 1e100, 1e300, F64_TINY, 1e-310, -1e-3, -1.0, -100.0]),
                          np.array([2.0 ** -52, 2.0 ** -30, 2.0 ** -20, 1.0, 1e6]), np.array([2.0 ** -64, 0.5, ONE_M]), indexing="ij")
    out.append(_pack(f32, 2, B, D, 1.0, U))
    return concat(out)


def uniform01(x1, x2):
    """Rng::uniform01 (csrc/sa_sweep.h): generate_canonical<double, 53> from two 32-bit words, low word first."""
    r = (x1.astype(np.float64) + x2.astype(np.float64) * 4294967296.0) * 5.421010862427522170037e-20
    return np.where(r >= 1.0, ONE_M, r)


def kernel_draws(f32, n, seed):
    """Random cases as the kernels meet them: u from two 32-bit words, delta and total sums and differences of a few
    powers of two (costs of dims-2 networks), beta from linear_betas(0, 100, 200) and from a schedule up to 1e5."""
    from tnco_amd.synthetic import linear_betas
    rng = np.random.default_rng(seed)
    u = uniform01(rng.integers(0, 2 ** 32, n, dtype=np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint32))
    top = rng.integers(10, 60, n)
    total = 2.0 ** top + 2.0 ** rng.integers(0, 60, n) + 2.0 ** rng.integers(0, 60, n)
    d_top = top - rng.integers(0, 30, n)
    delta = 2.0 ** d_top - 2.0 ** (d_top - rng.integers(0, 12, n)) + rng.choice([-1.0, 0.0, 1.0], n) * 2.0 ** (d_top - rng.integers(0, 40, n))
    delta = np.where(rng.random(n) < 0.1, -delta, delta)
    sched = np.concatenate([linear_betas(0, 100, 200), linear_betas(0, 1e5, 1000)])
    beta = sched[rng.integers(0, sched.size, n)]
    kind = np.where(rng.random(n) < 0.05, rng.integers(0, 2, n), 2).astype(np.int32)
    return _pack(f32, kind, beta, delta, total, u)


def decide_fast(c, guard_ulps=64):
    """The reference decision of many cases: numpy's float64 pow decides where u is further than `guard_ulps` units in
    the last place from it (numpy documents its pow to a few ulps; tests/test_accept_model.py checks the guard against
    mpmath), mpmath decides every other case.  Returns (decisions, number of cases mpmath decided)."""
    f32 = c["f32"]
    assert (f32 == f32[0]).all()
    f = int(f32[0])
    x = x_of(c["delta"], c["total"], f)
    with np.errstate(all="ignore"):
        one = (c["kind"] == 0) | (c["delta"] <= 0)
        zero = ~one & ((c["kind"] == 1) | (c["total"] == 0))
        pn = np.power(x, -c["beta"])
        pr = to_f32(pn) if f else pn
        far = np.isfinite(pn) & (pn > (1e-30 if f else 1e-290)) & (np.abs(c["u"] - pr) > (2 if f else guard_ulps) * ulp_of(pr, f))
    dec = np.where(one, True, np.where(zero, c["u"] <= 0.0, c["u"] <= pr))
    slow = np.flatnonzero(~one & ~zero & ~far)
    if slow.size:
        p = pow_exact_array(x[slow], c["beta"][slow])
        dec[slow] = decide(to_f32(p) if f else p, c["u"][slow])
    return dec, slow.size
