"""The cases of tests/cost_range_cases.py hold what they claim, by the oracle alone (no GPU): every pair constructs, enough
of them cross the edge of the cost type, come back and stay finite -- conditions (a) to (d) there --, the recorded counts
and is_valid() verdicts are the ones the oracle gives, no stored cost is ever NaN, the facts of the launch plan that need
no device are as each case says, and the constructor cases agree with the oracle and with totals in Python integers."""
import numpy as np
import pytest

from tests import cost_range_cases as C

CASES = C.resolved()
CTORS = C.ctor_cases()
BEST = C.best_tree_cases()


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(case):
        key = (case.net, case.dims, case.sparse)
        if key not in cache:
            cache[key] = C.problem(case)
        return cache[key]
    return get


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_meets_its_conditions(oracle_lib, problems, case):
    prob = problems(case)
    traces = [C.trace(oracle_lib, case, prob, pair) for pair in case.pairs]
    assert all(t is not None for t in traces), "(a) the oracle refuses a pair"
    cnt = C.counts(traces)
    n = len(case.pairs)
    assert 4 * cnt["crossed"] >= n, f"(b) {cnt['crossed']} of {n} pairs cross"
    assert cnt["came_back"] >= 2, "(c) the way back"
    assert cnt["finite"] >= 2, "(d) the finite side"
    assert cnt == case.counts  # (the table's counts and the positions is_valid() rejects are what the oracle gives)
    assert all(t["nonfinite"][0] is False for t in traces)  # a constructed state is finite
    # oracle/tnco_oracle.c: a stored cost is pow() of positive numbers or a product of them, a partial sum adds
    # non-negative ones, min_total_cost takes a total that compared less: none can be NaN (only the walk's local delta and
    # running total can, and they are never stored)
    assert not any(t["nan"] for t in traces)
    assert len(set(case.pairs)) == n and n <= 8


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_plan_facts(problems, case):
    prob = problems(case)
    facts = C.plan_facts(prob)
    assert case.plan and {k: facts[k] for k in case.plan} == case.plan
    if case.resident:  # what csrc/tnco_hip.hip, choose_launch asks of an LDS-resident handle that can be known here
        assert facts["cost_mode"] == 0 and case.cost_type == "float64" and not case.sparse and not case.fw
        assert facts["lanes"] == 4 and (facts["words"] <= 2 and prob.n <= 128 or int(np.log2(prob.dims)) * 64 * prob.W <= 65535)
    R = case.replicas or len(case.pairs)
    ids = C.checked_replicas(case, R, len(case.pairs))
    assert {r % len(case.pairs) for r in ids} == set(range(len(case.pairs))) and 0 in ids and R - 1 in ids and len(ids) <= 96
    if case.form == "wave":  # what the one-wavefront re-slice needs (csrc/tnco_hip.hip, fw_wave_tables)
        assert facts["cost_mode"] == 0 and case.cost_type == "float64" and not case.sparse and prob.n >= 16
    if case.fw:
        assert all(n % case.every == 0 for *_x, n in case.chunks[:-1])  # (every chunk starts with a re-slicing sweep)


def test_the_table_covers_what_it_should():
    names = {c.name for c in CASES}
    assert len(names) == len(CASES) == len(C.TABLE)
    by = {c.name: c for c in CASES}
    assert by["small63"].net[1] == 64 and by["small127"].net[1] == 84 and by["lds_k1"].net[1] == 128 and by["lds_k3"].net[1] == 512
    assert len(by["lds_k3"].pairs) <= 24 and len(by["small63"].pairs) <= 96
    assert by["cpl_spread"].replicas == 3000 and by["cpl_full_4x1"].replicas == 12300 and by["cpl_full_8x3"].replicas == 8200
    assert {by[n].form for n in ("fw_wave", "fw_rebuild")} == {"wave", "rebuild"} and by["fw_wave"].cost_range
    assert by["fw_f32"].cost_type == "float32" and by["fw_new_slices"].kw["max_number_new_slices"] == 2
    rules = {n: [c[0] for c in by[n].chunks] for n in names}
    assert rules["rule_greedy"][0] == "mh" and rules["rule_greedy"][-1] == "greedy" and rules["rule_base"][-1] == "base"
    assert any(b1 > 0 for _r, _b0, b1, _n in by["rule_mh_ramp"].chunks)


DECIDING = ["small127_greedy", "lds_k1_greedy", "lds_k3_greedy", "rule_greedy", "rule_greedy_hbm", "rule_base",
            "rule_mh_ramp", "rule_mh_ramp_f32", "rule_mh_ramp_hbm"]


@pytest.mark.parametrize("name", DECIDING)
def test_the_phases_that_look_at_delta_start_from_a_state_that_holds_an_inf(oracle_lib, problems, name):
    """Greedy, base and the ramps with beta > 0: the first such chunk starts from a boundary at which at least two pairs
    hold a non-finite cost, so the rule meets a delta of NaN or -inf there (at beta 0 every delta is accepted)."""
    case = next(c for c in CASES if c.name == name)
    first = next(k for k, (rule, _b0, b1, _n) in enumerate(case.chunks) if rule != "mh" or b1 > 0)  # boundary `first`: where it starts
    assert case.inf_at == first
    traces = [C.trace(oracle_lib, case, problems(case), pair) for pair in case.pairs]
    assert sum(t["nonfinite"][first] for t in traces) >= 2


def test_sparse_case_min_with_n_projs_brings_an_inf_back(oracle_lib, problems):
    """In the sparse case some contraction has cost(sparse legs) = inf and min(inf, n_projs) = n_projs makes its cost
    finite: recomputed here from the legs of the oracle's trees with Python integers."""
    case = next(c for c in CASES if c.name == "sparse_projs")
    prob = problems(case)
    d, sp = int(prob.dims), set(case.sparse)
    seen = 0
    for pair in case.pairs:
        o = C.make_oracle(oracle_lib, case, prob, C.start_tree(case, prob, pair[0]), pair[1])
        done = 0
        for k in range(len(case.chunks)):
            done = C.advance(o, case, k, done)
            l, r, _p, m = o.tree()
            cc = o.caches()[0]
            for x in range(prob.n, len(l)):
                legs = set(C.ct.unpack_mask(m[l[x]])) | set(C.ct.unpack_mask(m[r[x]]))
                if d ** len(legs & sp) >= 2 ** 1024 and d ** len(legs - sp) * case.kw["n_projs"] < 2 ** 1024:
                    assert cc[x] == float(d ** len(legs - sp) * case.kw["n_projs"])
                    seen += 1
    assert seen > 0


@pytest.mark.parametrize("variant", list(C.CTOR_VARIANTS))
@pytest.mark.parametrize("ctor", CTORS, ids=[c.name for c in CTORS])
def test_constructor_cases(oracle_lib, ctor, variant):
    """The oracle constructs or refuses every tree as the integer totals say; with slices drawn (finite width) the oracle
    decides, and the total of a tree it constructs is the integer total over legs | slices."""
    prob = ctor.problem()
    links = ctor.links(prob)
    kw = dict(C.CTOR_VARIANTS[variant], cost_type=ctor.cost_type)
    verdicts = []
    for r, (con, costs) in enumerate(zip(ctor.contractions, ctor.totals)):
        assert C.exact_costs(ctor.ts_inds, ctor.dims, con) == costs
        l, rr, p = links[r]
        if variant == "min_links":
            kw["min_tree"] = (l, rr, p, prob.node_masks(l, rr))
        try:
            o = oracle_lib.Oracle(l, rr, p, prob.node_masks(l, rr), n_inds=prob.n_inds, dims=prob.dims, seed=7 + r, **kw)
        except ValueError as e:
            assert "Precision is too low" in str(e)
            verdicts.append(False)
            continue
        verdicts.append(True)
        sl = C.ct.unpack_mask(o.slices()[0]) if variant.startswith("fw") else ()
        assert variant != "fw_loose" or not sl
        total = sum(C.exact_costs(ctor.ts_inds, ctor.dims, con, sl))
        assert total < 2 ** C.TOP[ctor.cost_type]
        assert o.total_cost == (float(total) if ctor.cost_type == "float64" else float(np.float32(float(total))))
    if variant != "fw_sliced":
        assert verdicts == [C.fits(t, ctor.cost_type) for t in ctor.totals]
    assert all(verdicts) == ctor.ok or variant == "fw_sliced"


def test_the_sliced_variant_draws_slices_and_they_count(oracle_lib):
    """`fw_sliced` is not vacuous: every tree the oracle constructs under it has slices, and a case that constructs without
    slices is refused with them (a sliced index is in every contraction)."""
    kw = C.CTOR_VARIANTS["fw_sliced"]
    n_sliced, turned = [], 0
    for ctor in CTORS:
        prob = ctor.problem()
        for r, (l, rr, p) in enumerate(ctor.links(prob)):
            try:
                o = oracle_lib.Oracle(l, rr, p, prob.node_masks(l, rr), n_inds=prob.n_inds, dims=prob.dims, seed=7 + r,
                                      cost_type=ctor.cost_type, **kw)
            except ValueError:
                turned += C.fits(ctor.totals[r], ctor.cost_type)
                continue
            n_sliced.append(len(C.ct.unpack_mask(o.slices()[0])))
    assert n_sliced and min(n_sliced) >= 1 and turned >= 1


@pytest.mark.parametrize("case", BEST, ids=[b.name for b in BEST])
def test_best_tree_cases(oracle_lib, case):
    """The current tree constructs on its own; with the best tree given the oracle decides as the integer total of the best
    tree (over its legs | min_slices) says, and a case that constructs has exactly that best total."""
    prob = case.problem()
    (l, r, p), (ml, mr, mp) = case.trees(prob)
    assert C.exact_costs(case.ts_inds, case.dims, case.cur) == case.cur_costs and C.fits(case.cur_costs, case.cost_type)
    assert C.exact_costs(case.ts_inds, case.dims, case.best, case.min_slices or ()) == case.best_costs
    assert C.fits(case.best_costs, case.cost_type) == case.ok
    kw = dict(case.kw, cost_type=case.cost_type)
    o = oracle_lib.Oracle(l, r, p, prob.node_masks(l, r), n_inds=prob.n_inds, dims=prob.dims, seed=3, **kw)
    assert not case.kw or not o.slices()[0].any()  # (finite width: the bound is loose, the current tree has no slices)
    kw.update(min_tree=(ml, mr, mp, prob.node_masks(ml, mr)), min_slices=case.min_slices_mask(prob))
    if not case.ok:
        with pytest.raises(ValueError, match="Precision is too low"):
            oracle_lib.Oracle(l, r, p, prob.node_masks(l, r), n_inds=prob.n_inds, dims=prob.dims, seed=3, **kw)
        return
    o = oracle_lib.Oracle(l, r, p, prob.node_masks(l, r), n_inds=prob.n_inds, dims=prob.dims, seed=3, **kw)
    to_type = float if case.cost_type == "float64" else (lambda x: float(np.float32(float(x))))
    assert o.min_total_cost == to_type(sum(case.best_costs)) and o.total_cost == to_type(sum(case.cur_costs))
