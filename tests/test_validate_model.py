"""tests/validate_cases.py -- the restatement of `is_valid` the GPU validator's tests take their expected verdicts from --
held to the oracle's `is_valid()` on the state the oracle's own getters return (no GPU): valid after a run in every
configuration, "not valid" where a float32 cost has overflowed, and the same verdict as the oracle's comparison rule on
values at, inside and outside the tolerance."""
import numpy as np
import pytest

from tests import helpers as H
from tests import validate_cases as V
from tnco_amd import synthetic as syn


def _model(prob, **kw):
    return V.Model(prob.leaf_masks, prob.n_inds, dims=prob.dims, output_mask=prob.output_mask, sparse_mask=prob.sparse_mask, **kw)


def _configs():
    reg = H.regular_problem(40, graph_seed=8)
    hy = syn.random_hyper_tn(30, 50, k=3, n_output=4, seed=12)
    vec = syn.random_hyper_tn(24, 40, k=2, n_output=2, seed=5, dims_choices=(2, 3, 4, 6))
    return {
        "dims 2": (reg, {}, {}),
        "dims 3": (H.Problem(reg.ts_inds, 3, []), {}, {}),
        "per-index dims": (H.Problem(*vec), {}, {}),
        "float32": (reg, dict(cost_type="float32"), {}),
        "hyper": (H.Problem(hy[0], 2, hy[2]), {}, {}),
        "hyper, dims 3, float32": (H.Problem(hy[0], 3, hy[2]), dict(cost_type="float32"), {}),
        "finite width": (reg, {}, dict(max_width=5)),
        "finite width, float64 widths": (reg, {}, dict(max_width=6, width_type="float64")),
        "finite width, per-index dims": (H.Problem(*vec), {}, dict(max_width=9.5)),
        "finite width, per-index dims, float64 widths": (H.Problem(*vec), {}, dict(max_width=9.5, width_type="float64")),
        "finite width, hyper": (H.Problem(hy[0], 2, hy[2]), {}, dict(max_width=7)),
    }


@pytest.mark.parametrize("name", list(_configs()))
def test_restatement_agrees_with_the_oracle_after_a_run(oracle_lib, name):
    prob, ckw, fkw = _configs()[name]
    model = _model(prob, **ckw, **fkw)
    seeds = H.replica_seeds(4, S=3)
    for s in seeds:
        o = H.make_oracle(oracle_lib, prob, prob.tree(s), s, **ckw, **fkw)
        done = 0
        for sweeps in (0, 35, 40):  # (finite width: re-slices at sweeps 0, 10, ... of the run)
            o.run(oracle_lib.PROB_MH, H.linear_betas(0, 30, max(sweeps, 1))[:sweeps])
            assert o.is_valid(1e-5) == 0
            st = V.oracle_state(o)
            assert V.is_valid(model, st, 1e-5), f"{name}: seed {s} after {sweeps} more sweeps"
            # ... and bit for bit what the oracle caches, so that "valid" is no accident of the tolerance
            order = V.traverse(st["left"], st["right"])
            legs = V.derive_legs(model, st["left"], st["right"], order)
            assert np.array_equal(legs, st["legs"])
            cc, pc, _ = V.cost_cache(model, st["left"], st["right"], legs, order, st.get("slices"))
            assert np.array_equal(cc, st["ccost"])
            done += sweeps
            if done == 0:  # (the moves sum the partial costs in another order: rounded costs then differ in the last bits)
                assert np.array_equal(pc, st["partial"])
            if model.fw:
                assert np.array_equal([V.width(model, m) for m in legs], st["widths"])


def test_float32_overflow_is_not_valid_for_both(oracle_lib):
    """A float32 cost that overflows to inf during the run: log(inf) - log(inf) is NaN, not <= atol (the case
    tests/test_gpu_random.py documents).  160 tensors of dimension 4: the first tree costs 2^110, ten sweeps that accept
    every move take a partial cost beyond float32."""
    prob = H.Problem(H.regular_problem(160, graph_seed=7).ts_inds, 4, [])
    s = H.replica_seeds(10, S=160)[1]
    o = H.make_oracle(oracle_lib, prob, prob.tree(s), s, cost_type="float32")
    model = _model(prob, cost_type="float32")
    assert o.is_valid() == 0 and V.is_valid(model, V.oracle_state(o))
    o.run(oracle_lib.PROB_MH, np.zeros(10))
    st = V.oracle_state(o)
    assert np.isinf(st["partial"]).any() and np.isfinite(st["min_total_cost"])
    assert o.is_valid() != 0
    assert not V.is_valid(model, st)


def test_is_logclose_margins():
    """include/tnco/utils.hpp:78-87 at the values the GPU tests damage costs with."""
    for atol in (1e-5, 1e-2):
        for c in (1.0, 2.0 ** 40, 3.0 ** 50):
            assert V.is_logclose(c, c * np.exp(0.5 * atol), atol) and V.is_logclose(c * np.exp(-0.5 * atol), c, atol)
            assert not V.is_logclose(c, c * np.exp(2 * atol), atol) and not V.is_logclose(c * np.exp(-2 * atol), c, atol)
            for bad in (-c, 0.0, np.inf, np.nan):
                assert not V.is_logclose(c, bad, atol) and not V.is_logclose(bad, c, atol)
    assert V.is_logclose(0.0, 0.0, 1e-5) and not V.is_logclose(np.inf, np.inf, 1e-5)


def test_damaged_state_is_not_valid(oracle_lib):
    """Every class of damage the GPU tests apply, on the oracle's state: the restatement notices each."""
    prob = H.regular_problem(40, graph_seed=8)
    s = H.replica_seeds(1, S=3)[0]
    o = H.make_oracle(oracle_lib, prob, prob.tree(s), s, max_width=5)
    o.run(oracle_lib.PROB_MH, H.linear_betas(0, 30, 45))
    model = _model(prob, max_width=5)
    good = V.oracle_state(o)
    assert V.is_valid(model, good)
    n, N = model.n, model.N

    def damaged(**kw):
        st = {k: np.array(v, copy=True) for k, v in good.items()}
        for k, (i, v) in kw.items():
            if i is None:
                st[k] = v
            else:
                st[k][i] = v
        return st

    inner = n + 3
    other = n + 7 if good["parent"][inner] != n + 7 else n + 8
    leaf_other = n + 7 if good["parent"][0] != n + 7 else n + 8
    assert not V.is_valid(model, damaged(parent=(0, leaf_other)))
    assert not V.is_valid(model, damaged(parent=(inner, other)))
    assert not V.is_valid(model, damaged(parent=(N - 1, n)))
    assert not V.is_valid(model, damaged(ccost=(inner, good["ccost"][inner] * np.exp(2e-5))))
    assert V.is_valid(model, damaged(ccost=(inner, good["ccost"][inner] * np.exp(0.5e-5))))
    assert not V.is_valid(model, damaged(partial=(N - 1, -good["partial"][N - 1])))
    assert not V.is_valid(model, damaged(min_total_cost=(None, good["min_total_cost"] * np.exp(2e-5))))
    assert V.is_valid(model, damaged(min_total_cost=(None, good["min_total_cost"] * np.exp(-0.5e-5))))
    legs = good["legs"].copy()
    legs[inner, 0] ^= np.uint64(1)
    assert not V.is_valid(model, damaged(legs=(None, legs)))
    assert not V.is_valid(model, damaged(widths=(inner, good["widths"][inner] + 2e-5)))
    assert V.is_valid(model, damaged(widths=(inner, good["widths"][inner] - 0.5e-5)))
    assert not V.is_valid(model, damaged(widths=(inner, np.nan)))
    # a slice that a widest tensor needs
    wide = max(range(N), key=lambda i: V.width(model, good["legs"][i] & ~good["slices"]))
    need = good["legs"][wide] & good["slices"]
    assert V.width(model, good["legs"][wide] & ~good["slices"]) == model.max_width and need.any()  # (the seed is fixed)
    bit = V.bits(need)[0]
    sl = good["slices"].copy()
    sl[bit // 64] &= ~(np.uint64(1) << np.uint64(bit % 64))
    assert not V.is_valid(model, damaged(slices=(None, sl)))
    # exchanged children: the caches are per node, the tree is the same tree
    l, r = good["left"].copy(), good["right"].copy()
    l[inner], r[inner] = r[inner], l[inner]
    assert V.is_valid(model, damaged(left=(None, l), right=(None, r)))
