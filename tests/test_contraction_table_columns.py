"""The columns of the contraction engine's flat tables have one name on each side, csrc/contract_tables.h and
tnco_amd/contraction.py, and the two sides agree: the same names, the same values.  The layout they name is the one
the comment of include/tnco_hip.h specifies (the other plan tests restate it in bare numbers).  No GPU."""
import re
from pathlib import Path

from tnco_amd import contraction as ctr

HEADER = Path(ctr.__file__).parent / "csrc" / "contract_tables.h"
PREFIXES = ("ST_", "PM_", "LS_", "RW_", "IX_")
# the names that differ between the sides: the header's -> the module's
RENAMED = {"CT_MAX_AXES": "MAX_AXES", "K_LEAF": "LEAF", "K_ARENA": "ARENA", "K_OUT": "OUT"}


def header_constants():
    """{name: value} of every `constexpr int NAME = expression;` of the header, each expression over the names before it."""
    out = {}
    for name, expr in re.findall(r"^constexpr int(?:64_t)? (\w+) = ([^;]+);", HEADER.read_text(), re.M):
        assert re.fullmatch(r"[\w\s+*()-]+", expr), expr
        out[name] = eval(expr, {"__builtins__": {}}, dict(out))  # noqa: S307 -- integers, names, + - * ( ) only
    return out


def is_shared(name):
    return name.startswith(PREFIXES) or name.endswith("_W") or name in RENAMED or name in RENAMED.values()


def test_every_name_of_the_header_has_the_value_of_the_module():
    consts = header_constants()
    assert len(consts) > 50
    for name, value in consts.items():
        assert is_shared(name) or name.startswith(("GR_", "SET_", "WK_")), name  # (device-only tables: their widths are shared)
        if is_shared(name):
            assert getattr(ctr, RENAMED.get(name, name)) == value, name


def test_every_name_of_the_module_is_in_the_header():
    consts = header_constants()
    back = {v: k for k, v in RENAMED.items()}
    mine = [n for n in vars(ctr) if is_shared(n) and isinstance(getattr(ctr, n), int)]
    assert len(mine) > 45
    for name in mine:
        assert consts.get(back.get(name, name)) == getattr(ctr, name), name


def test_the_steps_columns_are_0_to_15_and_the_perms_columns_0_to_6_and_two_blocks():
    consts = header_constants()
    st = sorted(v for n, v in consts.items() if n.startswith("ST_") and n != "ST_SIDE")
    assert st == list(range(16)) and consts["STEP_W"] == 16 and consts["ST_SIDE"] == 4
    assert [consts[f"ST_{c}"] for c in ("A_KIND", "A_REF", "A_M", "A_K", "B_KIND", "B_REF", "B_K", "B_N", "C_KIND", "C_REF",
                                        "H", "M", "N", "K", "A_SLOT", "B_SLOT")] == list(range(16))
    pm = sorted(v for n, v in consts.items() if n.startswith("PM_"))
    axes = consts["CT_MAX_AXES"]
    assert axes == 32 and pm == list(range(7)) + [8, 8 + axes]
    assert (consts["PM_DIMS"], consts["PM_STRIDES"], consts["PERM_W"]) == (8, 8 + axes, 8 + 2 * axes)
    assert (consts["LS_COUNT"], consts["LS_SLOTS"], consts["LS_STRIDES"], consts["LEAF_SL_W"]) == (0, 1, 1 + axes, 1 + 2 * axes)
    assert [consts[n] for n in ("RW_R", "RW_A_ROWS", "RW_A_MAP", "RW_B_ROWS", "RW_B_MAP", "ROW_W")] == list(range(6))
    assert [consts[n] for n in ("IX_A_H", "IX_A_M", "IX_A_K", "IX_B_H", "IX_B_K", "IX_B_N", "IND_W")] == list(range(7))
    assert (consts["K_LEAF"], consts["K_ARENA"], consts["K_OUT"]) == (0, 1, 2)
