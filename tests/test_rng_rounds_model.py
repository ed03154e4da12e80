"""The refill rounds of the sweep kernel's mt19937 producer (csrc/sa_sweep.h: Rng<>, MT_ROUND_RING, MT_ROUND_LOW), as a
model in numpy -- no GPU.  The model is Rng<> word for word (virtual positions `cons` / `prod` / `tw`, the block's inputs
read when it is requested, twist + temper when it is produced, the shadow of the words a next-generation block overwrites,
finish()) under the loop's rule: per iteration and lane group, produce what was requested, an optional draw (BEGIN's leaf),
the decision -- a group with fewer than LOW words and no block in flight opens a round for its wavefront of sixteen groups,
every group with room joins --, then up to three draws (MOVE's pick and uniform).  Every iteration of the model may hold
the draw ahead of the decision AND three behind it: the bound MT_ROUND_LOW is derived for, an upper bound of what a state of
the kernel does.  Ring size, block size, LOW, the shadow size and the prologue's blocks are read from the header.

Checked against numpy's MT19937 from every start position 0..624: the drawn stream, and state + position after finish()
at an arbitrary stop (with the host's completion of the lazy twist, tnco_hip_get_prng)."""
import re
from pathlib import Path

import numpy as np
import pytest

HDR = (Path(__file__).resolve().parent.parent / "tnco_amd" / "csrc" / "sa_sweep.h").read_text()


def _const(pattern):
    m = re.search(pattern, HDR)
    assert m, pattern
    return int(m.group(1))


RING = _const(r"constexpr int MT_ROUND_RING = (\d+);")
LOW = _const(r"constexpr int MT_ROUND_LOW = (\d+);")
MT_SHADOW = _const(r"constexpr int MT_SHADOW = (\d+);")
# words per block at four lanes per replica: SB = 4 * NL, NL = min(L, 4)
assert re.search(r"static constexpr int NL = L < 4 \? L : 4;", HDR)
SB = _const(r"static constexpr int SB = (\d+) \* NL;") * 4
FILL = _const(r"rng\.template init<ROUNDS \? (\d+) : 0>")  # blocks of the synchronous prologue
GROUPS = 16   # lane groups (replicas) per wavefront
WAVES = 40    # 640 groups: every start position 0..624, fifteen of them twice
N = 624
U32 = np.uint32


class Underflow(AssertionError):
    pass


def _temper(z):
    z = z ^ (z >> U32(11))
    z = z ^ ((z << U32(7)) & U32(0x9d2c5680))
    z = z ^ ((z << U32(15)) & U32(0xefc60000))
    return z ^ (z >> U32(18))


class Model:
    """G = WAVES * GROUPS generators side by side (rows); a wavefront = GROUPS consecutive rows."""

    def __init__(self, keys, mti, low, max_draws, ring=RING):
        G = len(mti)
        self.G, self.low, self.ringsz = G, low, ring
        self.st = keys.copy()                         # P.mt: the state words
        self.sh = np.zeros((G, MT_SHADOW), U32)       # P.mtshadow
        self.ring = np.zeros((G, ring), U32)
        mti = np.asarray(mti, np.int64)
        self.cons = np.where(mti >= N, N, mti)
        self.tw = np.full(G, N, np.int64)             # (an imported state is twisted throughout: mtw = 624)
        self.prod = self.cons & ~np.int64(SB - 1)
        self.pend = np.zeros(G, bool)
        self.ptw = np.zeros(G, bool)
        self.in_a = np.zeros((G, SB + 1), U32)        # mt[k0 .. k0 + SB] (the lanes' pa and pb)
        self.in_c = np.zeros((G, SB), U32)            # mt[k0 + 397 ..] (pc)
        self.alive = np.ones(G, bool)
        self.cons0 = self.cons.copy()
        self.out = np.zeros((G, max_draws), U32)      # the drawn stream
        self.max_ahead = 0
        self.max_shadow_idx = -1
        for _ in range(FILL):                         # init<FILL>: the synchronous prologue
            g = np.flatnonzero(self.room())
            self.request(g)
            self.produce(g)

    def gen_of_cons(self):
        return np.where(self.cons == 0, 0, (self.cons - 1) // N)

    def room(self):
        return ~self.pend & (self.prod - self.cons + SB <= self.ringsz)

    def request(self, g):
        k0 = self.prod[g] % N
        self.ptw[g] = self.prod[g] >= self.tw[g]
        ia = (k0[:, None] + np.arange(SB + 1)) % N
        ic = (k0[:, None] + 397 + np.arange(SB)) % N
        self.in_a[g] = self.st[g[:, None], ia]
        self.in_c[g] = self.st[g[:, None], ic]
        self.pend[g] = True

    def produce(self, g):
        if len(g) == 0:
            return
        a, c, tw = self.in_a[g], self.in_c[g], self.ptw[g]
        y = (a[:, :SB] & U32(0x80000000)) | (a[:, 1:] & U32(0x7fffffff))
        twisted = c ^ (y >> U32(1)) ^ np.where(y & U32(1), U32(0x9908b0df), U32(0))
        v = np.where(tw[:, None], twisted, a[:, :SB])
        slot = (self.prod[g][:, None] + np.arange(SB)) & (self.ringsz - 1)
        self.ring[g[:, None], slot] = _temper(v)
        sidx = (self.prod[g] % N)[:, None] + np.arange(SB)
        gt = g[tw]
        self.st[gt[:, None], sidx[tw]] = v[tw]
        ahead = tw & (self.prod[g] // N > self.gen_of_cons()[g])  # a block of the generation after the one consumed
        if ahead.any():
            ga = g[ahead]
            self.max_shadow_idx = max(self.max_shadow_idx, int(sidx[ahead].max()))
            assert sidx[ahead].max() < MT_SHADOW, "a next-generation block overwrites a state word beyond the shadow"
            self.sh[ga[:, None], sidx[ahead]] = a[ahead][:, :SB]
        self.tw[gt] = self.prod[gt] + SB
        self.prod[g] += SB
        self.pend[g] = False
        ahead_now = int((self.prod[g] - self.cons[g]).max())
        self.max_ahead = max(self.max_ahead, ahead_now)
        assert ahead_now <= self.ringsz, "production ran more than a ring ahead of consumption"

    def draw(self, g):
        if len(g) == 0:
            return
        if (self.cons[g] >= self.prod[g]).any():
            raise Underflow(f"a draw read a word that was not produced (LOW = {self.low})")
        self.out[g, self.cons[g] - self.cons0[g]] = self.ring[g, self.cons[g] & (self.ringsz - 1)]
        self.cons[g] += 1

    def iteration(self, begin, moves):
        """One loop iteration: `begin` (bool per group) draws ahead of the decision, `moves` (0..3 per group) behind it."""
        self.produce(np.flatnonzero(self.pend & self.alive))
        self.draw(np.flatnonzero(begin & self.alive))
        need = self.alive & ~self.pend & (self.prod - self.cons < self.low)
        rnd = np.repeat(need.reshape(-1, GROUPS).any(axis=1), GROUPS)  # the ballot: wave-uniform
        self.request(np.flatnonzero(rnd & self.alive & self.room()))
        for j in range(3):
            self.draw(np.flatnonzero((moves > j) & self.alive))

    def finish(self, g):
        """Rng::finish for the groups `g`, which leave the loop: (state words, mti) as the host exports them."""
        self.produce(g[self.pend[g]])
        self.alive[g] = False
        res = {}
        for r in g:
            gen = 0 if self.cons[r] == 0 else (self.cons[r] - 1) // N
            mti = int(self.cons[r] - N * gen)
            st = self.st[r].copy()
            if self.tw[r] > N * (gen + 1):
                nw = int(self.tw[r] - N * (gen + 1))
                assert nw <= MT_SHADOW
                st[:nw] = self.sh[r, :nw]
                mtw = N
            else:
                mtw = int(self.tw[r] - N * gen)
            if mti < N:
                _complete_twist(st, mtw)
            res[int(r)] = (st, mti)
        return res

    def streams(self):
        return [self.out[r, :k] for r, k in enumerate((self.cons - self.cons0).astype(int))]


def _complete_twist(st, mtw):
    """tnco_hip_get_prng: the host completes the lazy twist, words mtw..623 -- here in runs whose inputs are settled."""
    old = st.copy()
    mag = lambda y: (y >> U32(1)) ^ np.where(y & U32(1), U32(0x9908b0df), U32(0))  # noqa: E731
    for lo, hi in ((0, 227), (227, 454), (454, 623)):
        k = np.arange(max(lo, mtw), hi)
        if len(k):
            st[k] = st[(k + 397) % N] ^ mag((old[k] & U32(0x80000000)) | (old[k + 1] & U32(0x7fffffff)))
    if mtw <= 623:
        st[623] = st[396] ^ mag((old[623] & U32(0x80000000)) | (st[0] & U32(0x7fffffff)))


def _inputs(seed=2024):
    rng = np.random.default_rng(seed)
    G = WAVES * GROUPS
    mti = np.concatenate([np.arange(N + 1), rng.integers(0, N + 1, G - (N + 1))])
    rng.shuffle(mti)  # (neighbours in a wavefront: unrelated positions)
    keys = rng.integers(0, 1 << 32, (G, N), dtype=np.uint64).astype(U32)  # (any 624 words are a state; the top bit of
    keys[:, 0] |= U32(0x80000000)                                          #  word 0 set: never the all-zero one)
    return rng, keys, mti


_BG = np.random.MT19937(0)


def _numpy_reference(key, pos, n):
    """(the next n words, key and position behind them) of numpy's MT19937 started from (key, pos)"""
    st = _BG.state
    st["state"]["key"] = key.copy()
    st["state"]["pos"] = int(pos)
    _BG.state = st
    words = _BG.random_raw(n).astype(U32) if n else np.zeros(0, U32)
    end = _BG.state["state"]
    return words, end["key"].astype(U32), int(end["pos"])


def _run(low, iters, stop_some=True, seed=2024):
    rng, keys, mti = _inputs(seed)
    G = len(mti)
    m = Model(keys, mti, low, 4 * iters)
    stop_at = rng.integers(iters // 4, iters, G) if stop_some else np.full(G, iters)
    stop_at[rng.integers(0, G, 8)] = 0  # (some leave before their first iteration: the prologue alone)
    finished = m.finish(np.flatnonzero(stop_at == 0))
    for it in range(iters):
        begin = rng.random(G) < 0.3
        moves = rng.integers(0, 4, G)
        m.iteration(begin, moves)
        done = np.flatnonzero((stop_at == it + 1) & m.alive)
        if len(done):
            finished.update(m.finish(done))
    finished.update(m.finish(np.flatnonzero(m.alive)))
    return m, keys, mti, finished


@pytest.fixture(scope="module")
def run():
    return _run(LOW, 2000)


@pytest.fixture(scope="module")
def reference(run):
    m, keys, mti, _ = run
    return [_numpy_reference(keys[r], mti[r], int(n)) for r, n in enumerate(m.cons - m.cons0)]


def test_constants_of_the_header():
    assert SB == 16 and RING >= 2 * SB and RING <= MT_SHADOW and RING & (RING - 1) == 0
    assert LOW >= 7 and FILL * SB - (SB - 1) >= LOW  # (the loop is entered with at least LOW words: no round before a draw)


def test_no_draw_underflows_and_production_stays_inside_the_ring(run):
    """(An underflow raises in the fixture; the ring and shadow bounds are asserted at every produce.)"""
    m, _keys, mti, finished = run
    assert set(mti.tolist()) == set(range(N + 1))
    assert len(finished) == m.G
    assert SB < m.max_ahead <= RING                # rounds do run more than the default two blocks ahead
    assert 0 <= m.max_shadow_idx < MT_SHADOW       # ... and next-generation blocks were produced ahead of the wrap
    assert int((m.cons - m.cons0).max()) > 3 * N  # several generation wraps (and stops ahead of the first iteration: none)
    assert int((m.cons - m.cons0).min()) == 0


def test_stream_equals_numpys_mt19937(run, reference):
    m, _keys, mti, _ = run
    for r, got in enumerate(m.streams()):
        assert np.array_equal(got, reference[r][0]), f"group {r} (start position {mti[r]})"


def test_state_and_position_after_finish_equal_numpys(run, reference):
    m, _keys, mti, finished = run
    for r, (st, pos) in finished.items():
        _words, key, want_pos = reference[r]
        assert pos == want_pos, f"group {r}: position after {len(_words)} draws from {mti[r]}"
        assert np.array_equal(st, key), f"group {r}: state after {len(_words)} draws from {mti[r]}"


def test_a_lower_threshold_underflows():
    """The model sees an underflow: with LOW = 6 a group can draw 3 + 1 + 3 words between its last "enough" and its refill."""
    with pytest.raises(Underflow):
        _run(6, 2000, stop_some=False)
