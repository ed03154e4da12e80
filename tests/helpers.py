"""Shared test helpers: synthetic problems, oracle runs, comparisons."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from tnco_amd.synthetic import Problem, linear_betas, regular_problem, replica_seeds  # noqa: F401


def make_oracle(orc, prob: Problem, links_r, seed, **kw):
    l, r, p = links_r
    inds = prob.node_masks(l, r)
    return orc.Oracle(l, r, p, inds, n_inds=prob.n_inds, dims=prob.dims, sparse=prob.sparse_mask,
                      seed=int(seed) & 0xFFFFFFFF, **kw)


def assert_replica_equal(gpu, r, o, check_min=True):
    """Bit-exact comparison of one GPU replica with its oracle twin."""
    for which in ((False, True) if check_min else (False,)):
        gl, gr, gp, gm = gpu.tree(r, which_min=which)
        ol, orr, op, om = o.tree(which_min=which)
        assert np.array_equal(gl, ol), f"replica {r} left (min={which})"
        assert np.array_equal(gr, orr), f"replica {r} right (min={which})"
        assert np.array_equal(gp, op), f"replica {r} parent (min={which})"
        assert np.array_equal(gm, om), f"replica {r} masks (min={which})"
    cc, pc, hy = gpu.caches(r)
    occ, opc, ohy = o.caches()
    assert np.array_equal(cc.view(np.uint64), occ.view(np.uint64)), f"replica {r} ccost"
    assert np.array_equal(pc.view(np.uint64), opc.view(np.uint64)), f"replica {r} partial"
    assert np.array_equal(hy, ohy), f"replica {r} hyper"
    assert np.array_equal(gpu.prng_state(r), o.prng_state()), f"replica {r} prng"


def expected_validate(verdicts):
    """(n_bad, first_bad) as validate() reports them, from per-replica verdicts (true: not valid)."""
    bad = [r for r, v in enumerate(verdicts) if v]
    return (len(bad), bad[0] if bad else -1)


@contextlib.contextmanager
def padded_rows(core, **extra):
    """While active, tnco_hip_create gets the per-replica rows named in `extra` (links, node_masks, min_links, slices --
    the last covers min_slices too: they share a stride) as copies with that many filler elements behind every row and
    the stride to match: descriptors core.py never writes (its strides are 0 or the row length).  Leaving the block fails
    unless every named kind of row went through a create call inside it."""
    L = core._lib.load()
    real = L.tnco_hip_create
    rewritten = dict.fromkeys(extra, 0)

    def create(dref, href):
        d = dref._obj
        N, W = 2 * d.n_leaves - 1, max(1, (d.n_inds + 63) // 64)
        rows = dict(links=(3 * N, C.c_int32, "links_stride", ["links"]), node_masks=(N * W, C.c_uint64, "node_masks_stride", ["node_masks"]),
                    min_links=(3 * N, C.c_int32, "min_links_stride", ["min_links"]), slices=(W, C.c_uint64, "slices_stride", ["slices", "min_slices"]))
        keep = []
        for name, pad in extra.items():
            row, ctype, stride, fields = rows[name]
            assert getattr(d, stride) == row, f"'{name}' must come in as one contiguous row per replica"
            for f in fields:
                if getattr(d, f):
                    src = np.ctypeslib.as_array((ctype * (d.n_replicas * row)).from_address(getattr(d, f))).reshape(d.n_replicas, row)
                    wide = np.full((d.n_replicas, row + pad), 0x5A5A5A5A, src.dtype)
                    wide[:, :row] = src
                    keep.append(wide)
                    setattr(d, f, wide.ctypes.data)
                    rewritten[name] += 1
            setattr(d, stride, row + pad)
        return real(dref, href)

    L.tnco_hip_create = create
    try:
        yield
    finally:
        L.tnco_hip_create = real
    assert rewritten and all(rewritten.values()), f"rows never handed to tnco_hip_create: {rewritten}"
