"""What `plan`, `contract` and `contract_results` (tnco_amd/contraction.py) refuse of their option keywords, without a
GPU: the exception type, the whole message and which refusal comes first, over a grid of every keyword's values.

RULES restates the module docstring as an ordered list of (when, exception, message); the first rule that holds is the
outcome, a plan when none does.  The order is that of the checks -- compute, storage, scaling, slice_batch, path_kernel,
hoist, indirect, reuse, slice_order; within a keyword its value, what it excludes, the dtype (storage and compute), the
projections -- and after them what only the network can say of a named slice order.  The list is this file's own:
nothing of it is read from the module."""
import itertools
import types

import numpy as np
import pytest

from tnco_amd import contraction as ctr

PATH = [(0, 1), (0, 1)]
TS = [("a", "b"), ("b", "c"), ("c", "a", "d")]
SHAPES = [(2, 3), (3, 2), (2, 2, 2)]
PROJS = [[0], [1]]
GRID = dict(storage=(None, "float16", "x"), scaling=(None, "tensor", "x"), slice_batch=(None, 4, 0),
            compute=(None, "bf16x3", "matrix", "x"), path_kernel=(None, 2, 0), hoist=(None, True, False),
            indirect=(None, True, False), reuse=(None, True, False), slice_order=(None, "reuse", ("a",), "x", ("b",)),
            projs=(None, PROJS), dtype=(np.float32, np.float64))
NOT = NotImplementedError
ORDER = "'slice_order' must be None, 'reuse' or every sliced index once."


def _projs(name):
    return (lambda k: k[name] is not None and k["projs"] is not None, NOT, f"projections are not supported with '{name}'.")


def _with(name, other):  # `other` is not supported in a call with `name`
    return (lambda k: k[name] is not None and k[other] is not None, NOT, f"'{other}' is not supported with '{name}'.")


def _wide(name, when):
    return (lambda k: when(k) and k["dtype"] is np.float64, TypeError,
            f"with '{name}' the compute dtype must be float32 or complex64, not float64.")


RULES = [
    (lambda k: k["compute"] not in (None, "bf16x3", "matrix"), ValueError, "'compute' must be None or 'bf16x3' or 'matrix'."),
    (lambda k: k["compute"] is not None and k["storage"] is not None, ValueError, "'compute' and 'storage' are exclusive."),
    _wide("compute", lambda k: k["compute"] == "bf16x3"),
    _projs("compute"),
    (lambda k: k["storage"] not in (None, "float16", "bfloat16"), ValueError, "'storage' must be None, 'float16' or 'bfloat16'."),
    _wide("storage", lambda k: k["storage"] is not None),
    _projs("storage"),
    (lambda k: k["scaling"] not in (None, "tensor"), ValueError, "'scaling' must be None or 'tensor'."),
    (lambda k: k["scaling"] is not None and k["storage"] is None, ValueError, "'scaling' needs 'storage'."),
    (lambda k: k["slice_batch"] not in (None, 4), ValueError, "'slice_batch' must be None or an integer from 1 to 64."),
    _projs("slice_batch"),
    (lambda k: k["path_kernel"] not in (None, 2), ValueError, "'path_kernel' must be None or an integer from 1 to 1024."),
    (lambda k: k["path_kernel"] is not None and k["slice_batch"] is not None, ValueError,
     "'path_kernel' and 'slice_batch' are exclusive."),
    _with("path_kernel", "storage"),
    _with("path_kernel", "compute"),
    _projs("path_kernel"),
    (lambda k: k["hoist"] is False, ValueError, "'hoist' must be None or True."),
    (lambda k: k["hoist"] is not None and k["path_kernel"] is not None, NOT, "'hoist' is not supported with 'path_kernel'."),
    _projs("hoist"),
    (lambda k: k["indirect"] is False, ValueError, "'indirect' must be None or True."),
    _with("indirect", "storage"),
    _with("indirect", "compute"),
    _with("indirect", "path_kernel"),
    _projs("indirect"),
    (lambda k: k["reuse"] is False, ValueError, "'reuse' must be None or True."),
    (lambda k: k["reuse"] is not None and k["hoist"] is not None, ValueError, "'reuse' includes 'hoist': give one of them."),
    _with("reuse", "slice_batch"),
    _with("reuse", "path_kernel"),
    _projs("reuse"),
    (lambda k: k["slice_order"] == "x", ValueError, ORDER),
    (lambda k: k["slice_order"] == "reuse" and k["reuse"] is not True, ValueError, "slice_order='reuse' needs reuse=True."),
    _projs("slice_order"),
]
N_OPTION_RULES = len(RULES)
RULES.append((lambda k: k["slice_order"] == ("b",), ValueError, ORDER))  # (the network's one sliced index is a)


def expected(k):
    """(index of the first rule that holds, its exception, its message), None for a plan."""
    for n, (when, exc, text) in enumerate(RULES):
        if when(k):
            return n, exc, text
    return None


def outcome(call):
    try:
        return call()
    except Exception as e:  # noqa: BLE001 (every type is compared)
        return type(e), str(e)


def combos():
    for values in itertools.product(*GRID.values()):
        yield dict(zip(GRID, values))


def split(k):
    """The keywords of a call and the dtype, which `contract` and `contract_results` take from the arrays."""
    kw = {name: v for name, v in k.items() if name != "dtype"}
    if k["projs"] is not None:
        kw["sparse_inds"] = ("d",)
    return kw, k["dtype"]


class Untouchable:
    def __getattribute__(self, name):
        raise AssertionError(f"the network was touched ({name})")


@pytest.fixture
def no_gpu(monkeypatch):
    from tnco_amd import _lib

    def refuse(*a, **kw):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "load", refuse)


def test_every_combination_is_refused_or_planned_as_the_rules_say(no_gpu):
    arrays = {dt: [np.ones(s, dt) for s in SHAPES] for dt in GRID["dtype"]}
    net = Untouchable()
    seen, plans, n = set(), 0, 0
    for k in combos():
        n += 1
        kw, dtype = split(k)
        want = expected(k)
        got = outcome(lambda: ctr.plan(PATH, TS, SHAPES, ("d",), slices=("a",), dtype=dtype, **kw))
        if want is None:
            assert isinstance(got, ctr.Plan), (k, got)
            plans += 1
            seen.add("plan")
            continue
        assert got == want[1:], (k, got, want)
        seen.add(got)
        assert outcome(lambda: ctr.contract(PATH, TS, arrays[dtype], ("d",), slices=("a",), **kw)) == want[1:], (k, want)
        if dtype is np.float32 and want[0] < N_OPTION_RULES:  # before anything of the network is looked at
            kw.pop("sparse_inds", None)
            assert outcome(lambda: ctr.contract_results(net, arrays[dtype], net, net, **kw)) == want[1:], (k, want)
    assert n == 174960 and plans == 105 and len(seen) == 33, (n, plans, len(seen))


def test_contract_results_checks_at_float32_first_and_at_the_arrays_dtype_after_the_network(no_gpu):
    """Two stages: every keyword at float32 before the network is touched, so with float64 arrays the projections
    are refused and not the dtype; compute and storage again with the arrays' dtype once the network has been looked at."""
    f64 = [np.ones(s, np.float64) for s in SHAPES]
    net = Untouchable()
    for kw in (dict(storage="float16"), dict(compute="bf16x3")):
        (name,) = kw
        with pytest.raises(NotImplementedError) as e:
            ctr.contract_results(net, f64, net, net, projs=PROJS, **kw)
        assert str(e.value) == f"projections are not supported with '{name}'."
        dense = types.SimpleNamespace(sparse_inds=())  # (all that is read of a network before the second stage)
        with pytest.raises(TypeError) as e:
            ctr.contract_results(dense, f64, dense, net, **kw)
        assert str(e.value) == f"with '{name}' the compute dtype must be float32 or complex64, not float64."
        with pytest.raises(AssertionError, match="the network was touched"):  # (the first stage passes at float32)
            ctr.contract_results(net, f64, net, net, **kw)
