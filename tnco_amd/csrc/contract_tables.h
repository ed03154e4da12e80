// contract_tables.h -- the one place that names the columns of the contraction engine's flat int64 tables; included by
// contract.hip inside its anonymous namespace, before the first kernel header.  The layout itself is specified by the
// comment of include/tnco_hip.h (tnco_hip_contract_desc); tnco_amd/contraction.py writes the tables under the same names
// with the same values (tests/test_contraction_table_columns.py holds the two sides together).  Plain constants: a
// subscript stays a subscript, st[ST_H].
#pragma once

constexpr int CT_MAX_AXES = 32;
// kinds of an operand or destination
constexpr int64_t K_LEAF = 0;
constexpr int64_t K_ARENA = 1;
constexpr int64_t K_OUT = 2;

// steps [n_steps][STEP_W].  An operand's four columns are kind, ref and its two strides: those of B lie ST_SIDE after
// those of A (st[ST_SIDE * side + ST_A_REF]), and its exponent slot (scaling) one after A's
constexpr int ST_A_KIND = 0;
constexpr int ST_A_REF = 1;
constexpr int ST_A_M = 2;
constexpr int ST_A_K = 3;
constexpr int ST_B_KIND = 4;
constexpr int ST_B_REF = 5;
constexpr int ST_B_K = 6;
constexpr int ST_B_N = 7;
constexpr int ST_C_KIND = 8;
constexpr int ST_C_REF = 9;
constexpr int ST_H = 10;
constexpr int ST_M = 11;
constexpr int ST_N = 12;
constexpr int ST_K = 13;
constexpr int ST_A_SLOT = 14;
constexpr int ST_B_SLOT = 15;
constexpr int STEP_W = 16;
constexpr int ST_SIDE = 4;

// perms [n_perms][PERM_W]: column 7 is 0; PM_DIMS and PM_STRIDES start blocks of CT_MAX_AXES columns
constexpr int PM_SRC_KIND = 0;
constexpr int PM_SRC_REF = 1;
constexpr int PM_DST_KIND = 2;
constexpr int PM_DST_REF = 3;
constexpr int PM_NDIM = 4;
constexpr int PM_NUMEL = 5;
constexpr int PM_GROUP = 6;
constexpr int PM_DIMS = 8;
constexpr int PM_STRIDES = 8 + CT_MAX_AXES;
constexpr int PERM_W = 8 + 2 * CT_MAX_AXES;

// leaf_sl [n_leaves][LEAF_SL_W]: the number of sliced axes, then their slice positions and their element strides
constexpr int LS_COUNT = 0;
constexpr int LS_SLOTS = 1;
constexpr int LS_STRIDES = 1 + CT_MAX_AXES;
constexpr int LEAF_SL_W = 1 + 2 * CT_MAX_AXES;

// row_steps [n_steps][ROW_W]: an operand's rows and map; those of B lie RW_SIDE after those of A
constexpr int RW_R = 0;
constexpr int RW_A_ROWS = 1;
constexpr int RW_A_MAP = 2;
constexpr int RW_B_ROWS = 3;
constexpr int RW_B_MAP = 4;
constexpr int ROW_W = 5;
constexpr int RW_SIDE = 2;

// ind_steps [n_steps][IND_W]: offsets into the pool of the tables of A by h, m, k and of B by h, k, n; -1: direct.
// Those of B lie IX_SIDE after those of A
constexpr int IX_A_H = 0;
constexpr int IX_A_M = 1;
constexpr int IX_A_K = 2;
constexpr int IX_B_H = 3;
constexpr int IX_B_K = 4;
constexpr int IX_B_N = 5;
constexpr int IND_W = 6;
constexpr int IX_SIDE = 3;

// device-only tables.  The groups section of the path kernel's table, [n_steps + 1][GR_W]: permute group g at row g + 1
constexpr int GR_FIRST = 0;
constexpr int GR_COUNT = 1;
constexpr int GR_W = 2;
// the per-leaf row of a run over leaf sets, [n_leaves][SET_W]: the leaf's pointer, the elements between two sets of it
constexpr int SET_PTR = 0;
constexpr int SET_STRIDE = 1;
constexpr int SET_W = 2;
// ... of a run over walkers, [n_leaves][WALK_W]: the pointer, the qubit whose bit picks a version (-1: none), the
// elements between the two versions
constexpr int WK_PTR = 0;
constexpr int WK_QUBIT = 1;
constexpr int WK_STRIDE = 2;
constexpr int WALK_W = 3;
