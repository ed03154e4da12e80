"""Sliced pairwise contraction of arrays along a linear path, on the GPU.

What `optimize()` returns (a linear path, and with a finite `max_width` a set of sliced indices) turned into numbers:
`contract` runs a path over numpy arrays, `contract_results` runs a result of `Optimizer.optimize` over the arrays of
the network as it was given.  Step semantics are those of the index-only `tnco_amd.app.tn.contract`: at each step the
shared indices that another tensor still holds, or that are output indices, stay as batch axes; the other shared
indices are summed; the result's axes are [kept shared][rest of the first][rest of the second].

Slicing: every assignment of values to the sliced indices runs the whole path on leaves restricted to that assignment
(the sliced axes dropped).  A sliced index that the result still holds selects a block of the output; the others are
summed over, assignment after assignment in one fixed order on the device, so a call is bit-reproducible.

The plan -- per-step layouts, which operand needs a permute, buffer liveness in one device arena -- is built here and
has no GPU dependency; `libtnco_hip.so` (csrc/contract.hip) gets it as flat int64 tables and runs the slice loop and
the step loop in one call (`tnco_hip_contract_run`).

Projections: with `sparse_inds` (output indices) and `projs`, an integer array [P, len(sparse_inds)], the result is the
dense result taken at those P assignments of the sparse indices: axes ("proj",) + the other axes, out[p] =
Z[sparse_inds = projs[p]].  A tensor that holds the subset T of the sparse indices is stored as [rows][its other
axes], a row per distinct row of projs[:, T] (numpy.unique(axis=0) order, columns in sparse_inds order): at most
min(prod dims(T), P) rows, the factor of the sparse cost model.  A step Z = X Y has T_z = T_x | T_y, and two int32 maps
give the rows of X and of Y that each row of Z restricts to; the leaves are restricted to their rows on the host.

Storage mode: with `storage="float16"` or `"bfloat16"` (float32 / complex64 arrays only) the leaves are rounded to that
type on the host, to nearest even, and every intermediate is rounded once when a step stores it; every step sums in
float32, the big steps on the matrix cores, and the output, the sum over slice assignments included, stays float32 /
complex64.  Leaves and intermediates take half the device memory.  Without `scaling` an intermediate beyond the
storage type's range becomes inf or 0, and a leaf beyond it is refused.  Projections are not supported with it.

Scaling: with `scaling="tensor"` (it needs `storage`) every stored tensor T, leaf or intermediate, has one int32
exponent e: the stored 16-bit values are round_nearest_even(x 2^-e) and the tensor means stored 2^e.  The rule, the same
on host (`scale_exponent`) and device (csrc/contract_half.h ct_scale_exponent):
    m = the largest |part| over the finite parts of the whole tensor (a complex element contributes its two parts);
    e = 0 when m == 0 or no part is finite, else e = floor(log2 m) - 14, read from the float32 bit pattern of m
    (float32 subnormals included).
The largest stored magnitude then lies in [2^14, 2^15]: finite in float16 even when it rounds up; bfloat16 uses the same
14.  x 2^-e is taken with ldexp and is exact (a part that falls below float32's normal range on the way is far below
the storage type's resolution at that scale).  Parts that are not finite do not enter m and are stored as they are; a
finite leaf is never beyond the range.  A leaf has one exponent for the whole leaf, every slice value included,
computed on the host (`scale_to_storage`).  A step whose result goes to the arena sums its stored operands in float32,
acc = sum A_stored B_stored, meaning acc 2^(e_A + e_B); with s the rule applied to the acc of the whole result it stores
round(acc 2^-s) and e_C = e_A + e_B + s.  The step for the output adds or places ldexp(acc, e_A + e_B) in float32, which
beyond float32's range is inf or 0 as float32 itself gives it; a single leaf gathered into the output is widened and
scaled the same way.  Permutes and gathers move the 16-bit values as they are.  The exponents live in a device array
(leaves first, then one slot per step) and are recomputed in every slice assignment; nothing synchronises with the host
inside a run, and the maximum is an integer max over sign-cleared bit patterns, so a call stays bit-reproducible.  Under
scaling a part smaller than 2^-28 of its tensor's largest lands in float16's subnormal range or below: that is below the
noise of the float32 sums themselves.

Slice batches: with `slice_batch=B` (1 to 64) the run takes the assignments of `slice_range` in groups of up to B
consecutive numbers, the first group starting at slice_range[0], the last one possibly partial, and every step of the
path is one launch per group instead of one per assignment: a sliced run of small steps is bound by its launches, and
this trades device memory for fewer and fuller ones.  Each member of a group works in its own copy of the arena (with
scaling: of the exponent slots and max words too), mapped to lanes, tiles and k order exactly as alone; the last step
leaves the members' blocks in a staging buffer and one more kernel per group adds or places them in the output in
assignment order.  The result is bit for bit that of `slice_batch=None`; device memory grows by B - 1 arenas and B blocks
of the output (`Plan.peak_device_bytes`).  The plan's tables do not change.  Projections are not supported with it; a
plan without steps takes the keyword and runs as without it.

Compute mode: with `compute="bf16x3"` (float32 / complex64 arrays only; exclusive with `storage`) nothing changes in
what is stored -- arrays, leaves, arena, intermediates and output stay float32 / complex64, and the plan's tables and
`peak_device_bytes` are those of `compute=None` -- but the steps of the tiled shape class (M, N >= 64 and K > 32) run on
the matrix cores: every float32 part x of an operand is split into hi = bf16(x), rounded to nearest even, and
lo = bf16(x - hi) (the subtraction is exact; lo = 0 where hi is not finite), and a product a b is summed in float32 as
a_lo b_hi + a_hi b_lo + a_hi b_hi, in that order; a_lo b_lo is dropped.  A complex product is its four real products,
each of them those three.  An element of such a step is within [2^-14 + (2 c 3 kt + 2) 2^-24] (|A| @ |B|) of the exact
one (c = 1 real, 2 complex, kt products per element).  The dot and stream classes, the gathers and the batch reduce are
the float32 kernels, so a network without a tiled-class step returns the bytes of `compute=None`.  An inf or NaN part
makes the elements it feeds non-finite and leaves the others alone.  A finite part with |x| >= 2^128 - 2^119 (about
3.396e38) has a hi that rounds to infinity and is out of range: in a leaf it is refused (ValueError), in an
intermediate the elements it feeds become non-finite.  Projections are not supported with it; `slice_batch` is, and
stays bit-equal to the unbatched run; `split_launches` of the result counts the launches of the split kernel (they
are also counted in their tiled slot of `kernel_launches`).

Matrix mode: with `compute="matrix"` (all four dtypes; exclusive with `storage`) nothing changes in what is stored
either, and the plan's tables and `peak_device_bytes` are those of `compute=None`; the steps of the tiled shape class
run on the matrix cores in the arrays' own precision (csrc/contract_matrix.h): a real product is one
v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, an fma chain of the element type with one rounding per product, and a
complex product its four real products.  Nothing is rounded or split, so an element is within (c kt + 2) u (|A| @ |B|) of
the exact one (u the unit roundoff of the type, c = 1 real, 2 complex), the bound of the plain kernels; the sums run in
another order than theirs (k in blocks of 16, within a block 0, 4, 8, 12, 1, 5, ...), so the bits differ from
`compute=None` on a tiled-class step and are equal without one.  Projections and `path_kernel` are not supported with
it; `slice_batch` and `hoist` are, bit-equal to the run without them; `matrix_launches` of the result counts the
launches of the matrix kernel (they are also counted in their tiled slot of `kernel_launches`).

Path kernel: with `path_kernel=G` (1 to 1024; exclusive with `slice_batch`; the four plain dtypes, no `storage`, `compute`
or `projs`) the run takes the assignments of `slice_range` in groups of up to G consecutive numbers, the first group
starting at slice_range[0], the last one possibly partial, and a group is two launches whatever the length of the path.
In the first, one workgroup per assignment interprets the whole path -- the gathers, the permutes and the steps, a
workgroup barrier between them -- in its own copy of the arena (csrc/contract_path.h); every step sums in the order of
the kernel the unfused run launches for its shape.  The last step leaves the members' blocks in a staging buffer and the
second launch adds or places them in the output in assignment order, from a device table of block offsets that is filled
for the whole run beforehand.  The result is bit for bit that of `path_kernel=None`.  One workgroup runs each step, so a
step may have 2^24 multiply-adds (H M N K) at most (MAX_PATH_STEP_MACS; ValueError beyond): the keyword is for width-bounded
slices, whose steps are small and whose runs are bound by their launches.  Device memory grows by G - 1 arenas, G blocks
of the output and the tables that are new on the device (`Plan.peak_device_bytes`).  The plan's tables do not change; a
plan without steps takes the keyword and runs as without it.  `path_launches` of the result counts the two kernels;
`kernel_launches`, `row_kernel_launches` and `batch_launches` are zeros on such a run.

Hoisting: with `hoist=True` (not with `path_kernel` or `projs`) what does not depend on the assignment runs once per call.
A tensor is slice-free when no leaf below it holds an index of `slices`; a step is hoisted when both its operands are
slice-free, a permute when its source is (the layout permute of a slice-free leaf, the arena-to-arena permute of a
slice-free intermediate, a permute that feeds a step which is not hoisted).  The hoisted work runs before the first
assignment of `slice_range`, in path order; everything else runs per assignment as without the keyword.  A slice-free
tensor that a step of the assignments reads is kept: its buffer is never released, and the arena is planned in two
phases on one allocator, the hoisted events first (their temporaries released, the kept buffers not), the events of an
assignment on top of what that left; `arena_elems` and `peak_device_bytes` are the peak over both.  Every step runs the
kernel it runs unhoisted on the same shapes and strides, so the result is bit for bit that of `hoist=None`, with
`storage`, `scaling`, `compute` and `slice_batch` too (a batch: the hoisted phase works in arena copy 0, every member
reads a kept tensor there).  `macs` is the sum of the hoisted steps plus assignments x the sum of the others; the launch
counts are of what ran; `hoisted` of the plan and of the result is (steps hoisted, permutes hoisted).  Without a sliced
index, or when nothing is slice-free, the plan and the run are those of `hoist=None`.

Reuse: with `reuse=True` (not with `hoist`, which it includes, nor with `slice_batch`, `path_kernel` or `projs`) a step or
permute runs only at the assignments that change a sliced index below it.  With the sliced indices s_0 .. s_{L-1} in
`Plan.slice_inds` order, place[j] the product of the dimensions after s_j and n their product, assignment a gives s_j
the value (a // place[j]) % dim(s_j).  dep(T) is the set of sliced indices (of a dimension above 1: one of dimension 1
never changes) held by a leaf below the tensor T, per(T) the smallest place in dep(T), n when dep(T) is empty: T has one
value for all a with equal a // per(T).  A step has the period of its result, min(per(A), per(B)); a permute that of its
source.  An item of period P is due at assignment a of slice_range = (lo, hi) iff a == lo or a % P == 0, so it runs
1 + (hi - 1) // P - lo // P times.  A tensor is kept when its reader has a smaller period than its writer: its buffer is
never released (`Plan.kept`, `Plan.kept_period`).  The items of one period are a phase.  The arena is planned on one
allocator with the phases in order of descending period, the events of a phase in path order, its temporaries released
and the kept buffers not; at an assignment the phases that are due run slowest first, each in path order (the rows of a
permute group that have one period are contiguous, the slowest first: one gather launch).  Roles, summed order, shape
class, result layout and kernel of every step are the plain plan's, so the result is bit for bit that of `reuse=None`
under the same `slice_order`, in the four dtypes and with `slice_range`, `storage`, `scaling`, `compute` and `indirect`
(an operand is folded iff its tables are small enough, its source is not slice-free and has the period of the step; the
permute of a slower source stays, runs at the source's period, and its copy is kept).  With scaling the exponent slot
of a kept tensor stays as written until its writer is due again.  `Plan.step_period` / `Plan.perm_period` are the
periods, `macs` is the sum over the steps of runs x H M N K, `reused` of the plan and of the result is (steps, permutes)
with a period above 1.  Without a sliced index, or when every period is 1, the plan and the run are those of
`reuse=None`.

Slice order: `slice_order=` (not with `projs`) gives the order of `Plan.slice_inds`, the slowest index first: a sequence
that names every sliced index once, or "reuse" (needs `reuse=True`).  The slice numbers of `slice_range` and the order in
which the assignments are summed follow it, so the bits may differ from `slice_order=None`, the default order (first
appearance in `ts_inds`); a call stays bit-reproducible.  "reuse" places the fastest index first: of the indices not yet
placed the one with the smallest sum of H M N K over the steps that hold it and that no faster index covers yet, of equal
ones the later in the default order; it keeps the default order unless that one has strictly fewer multiply-adds.

Operands read in place: with `indirect=True` (the four plain dtypes; not with `storage`, `compute`, `path_kernel` or
`projs`) a step operand that would be permuted into the [h][m][k] / [h][k][n] order is *folded* instead: it stays where
it lies and the step reads its element (h, m, k) at base + offH[h] + offM[m] + offK[k] through three int64 offset tables
(csrc/contract_indirect.h), the terms separable because h, m and k are disjoint groups of the source's axes.  An operand
is folded when (a) its source is not slice-free under `hoist=True` -- a permute that hoisting runs once per call stays a
permute -- and (b) its tables are no larger than the copy they replace, 8 (H + M + K) <= itemsize H M K (B: N for M).
Everything else of a step is what the plain plan decides -- the roles, the order of the summed indices (chosen as if
the operand were going to be permuted), the shape class, the layout of the result -- so every sum runs over the same k
in the same order and the result is bit for bit that of `indirect=None`, with `slices`, `slice_range`, `slice_batch` and
`hoist` too.  A folded operand keeps its kind and ref: an arena tensor stays where the step before left it and is
released after the step; a leaf, also one that is not dense after slicing, is read at the slice offset of the
assignment; its two stride columns in `steps` are 0.  `Plan.ind_steps` [n_steps][6] holds the offsets into the pool
`Plan.ind_maps` of the tables of A by h, m, k and of B by h, k, n (-1: not folded); a table's entry i is the sum of digit
x source stride over its group of axes, i linearised as the plain plan linearises the group, a leaf with the strides of
the full array.  The folded permutes are absent from `perms`, their buffers from the arena; `peak_device_bytes` adds
8 (ind_steps.size + ind_maps.size); `macs` is unchanged.  `indirect` of the plan and of the result is the number of
operands folded, `indirect_launches` of the result the launches of the three kernels in INDIRECT_KERNEL_PATHS order (they
are part of `launches` and of no slot of `kernel_launches`).  With nothing folded the plan and the run are those of
`indirect=None`.

Wide accumulation: with `accumulate="float64"` (float32 / complex64 arrays, every mode whose output is one of them:
`storage`, `scaling`, `compute` too; not with `projs`) the sum over slice assignments runs in float64.  Every assignment
computes its float32 / complex64 block of the output exactly as without the keyword -- the kernels, the shapes, the k
order; the block is the one the plain run would place with beta 0 -- into a staging block, and the blocks are added in
assignment order, each part (re, im) on its own, into a device accumulator of float64 / complex128 with one element per
output element (csrc/contract_accumulate.h): the first block that reaches an output block is placed, widened exactly,
every later one is added with one IEEE float64 addition.  After the last assignment of `slice_range` the accumulator is
rounded once, to nearest even, into the output; blocks that `slice_range` does not reach stay zero.  With b_0, b_1, ...
the blocks that hit one output block, r = float32(((float64(b_0) + float64(b_1)) + float64(b_2)) + ...).  Nothing is
atomic and the order is fixed, so a call stays bit-reproducible; r does not depend on `slice_batch`, `path_kernel`,
`hoist`, `indirect` or `reuse` under one `slice_order`; where every output block is visited once -- an unsliced call, a
sliced index that the result holds -- r is the bytes of `accumulate=None`.  The plan's tables do not change.  Device
memory grows by the accumulator, 2 itemsize out_numel, and, when neither `slice_batch` nor `path_kernel` is given, by a
staging block of itemsize block_numel (`Plan.peak_device_bytes`).  The folds are counted in `batch_launches` (unbatched:
one per assignment; with `slice_batch` one per group, as without the keyword), with `path_kernel` in `path_launches[1]`;
the one launch that rounds the accumulator is counted in `narrow_launches`; all of them are part of `launches`.  `array`
keeps the arrays' dtype.  A plan without steps places blocks and sums nothing: it takes the keyword, reserves nothing and
runs as without it.

Resident use: `contract` plans, creates a device handle, copies every leaf in, runs, copies the output back, lays it out
on the host and destroys the handle, every call.  A `Contractor` holds one plan and one handle for many runs: leaves can
be bound and stay on the device, arrays can be torch tensors on the device (any strides >= 0; the plan's dtype or one that
widens to it exactly) and the result can be written into a tensor (csrc/contract_io.h: ct_ingest_kernel copies a
tensor into the handle's leaf buffer, ct_emit_kernel the output buffer into the tensor in the result's axis order).  A
tensor's pointer is a kernel argument only -- torch's HIP runtime is not the one the library links, and memory of the one
is unknown to the other -- and the two sides are ordered by full synchronisation.  The result is that of `contract` for
the same arrays and keywords, byte for byte.

Leaf sets: `Contractor.run_many(stacks, group=, out=)` (with `path_kernel=`, a plan with steps, no `accumulate=`) runs R
leaf sets of the plan in one call: `stacks` is {leaf number: array}, each array the R versions of that leaf along one
leading axis; every other leaf is bound and shared.  A member of a launch is a pair (set i, assignment a), numbered
set-major: with slice_range = (lo, hi) and A = hi - lo, member m = i A + (a - lo); launches take `group` consecutive
members (1 to MAX_PATH_KERNEL, None: MAX_PATH_KERNEL; effective min(group, R A)), so a group may end inside a set, at its
end, or span several, and R sets are ceil(R A / group) pairs of launches (csrc/contract_sets.h: the path kernel with a
leaf's base moved on by set x stride, the stride 0 for a shared leaf; the fold kernel with set i's copy of the output).
Set i is folded in ascending assignment order with the placement and beta bits of the plan's own table, so array[i] of
the ManyResult is byte for byte `run` of leaf set i, whatever the group; blocks that slice_range does not reach are zero
in every set.  A stack lives in a device buffer of its own: a bound leaf given as a stack stays bound and untouched.
`many_bytes(R, group)` is the device memory the handle holds after such a call, term by term; what a call grew stays
until a larger call or close().

Walkers: the state of a gate-by-gate circuit sampler (tnco_amd/sampling.py) is a table of bits, R walkers x n qubits, and
it lives on the device in a `Walkers` object (csrc/contract_walk.h).  A leaf that depends on one of a walker's bits -- a
one-hot vector -- is bound once as its two versions, `Contractor.bind_versions({leaf: array of shape (2,) + leaf shape})`,
and `Contractor.run_walkers(walkers, {leaf: qubit})` is `run_many` over R sets in which walker i reads version
bits[i, qubit] of such a leaf and every other leaf where it is bound: nothing is stacked, nothing is reloaded, and the R
outputs stay on the device (`ManyResult.array` is None; `walker_outputs` copies them out, byte for byte those of
`run_many` over the explicit stacks).  Where the plan's output has 2 elements, the amplitudes of one qubit's two values,
`Contractor.choose(walkers, qubit, step)` draws the qubit's new bit for every walker: p = |a|^2 in float64, u from
Philox4x32-10 with key (seed lo, seed hi) and counter (i lo, i hi, step, 0), u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53,
bit = (u (p0 + p1) < p1); a walker whose p0 + p1 is 0 or not finite gets the bit 0 and is flagged dead.  A choice is a
function of (seed, walker, step, amplitudes): no generator state is kept.  `Walkers.permute(qubits, table)` is a classical
gate: the bits of up to 8 qubits, the first the most significant, become table[their value].
"""
from __future__ import annotations

import ctypes as C
import math
from collections import defaultdict
from dataclasses import dataclass, field, replace

import numpy as np

from .app import tn as tnmod

__all__ = ["contract", "contract_results", "plan", "Plan", "ContractionResult", "MAX_AXES", "DTYPES", "KERNEL_PATHS",
           "ROW_KERNEL_PATHS", "STORAGES", "round_to_storage", "SCALINGS", "scale_exponent", "scale_to_storage",
           "MAX_SLICE_BATCH", "COMPUTES", "split_bf16", "MAX_PATH_KERNEL", "MAX_PATH_STEP_MACS", "INDIRECT_KERNEL_PATHS",
           "ACCUMULATES", "Contractor", "merge_axes", "check_extent", "ManyResult", "Walkers", "MAX_PERMUTE_QUBITS",
           "MAX_CHOOSE_QUBITS"]

MAX_AXES = 32  # axes per tensor the kernels take (after slicing); csrc/contract.hip CT_MAX_AXES
DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2, np.dtype(np.complex128): 3}

# storage mode: leaves and intermediates in a 16-bit type, sums and the output in float32 / complex64.  The dtype code
# of include/tnco_hip.h is STORAGES[name] + (1 when complex)
STORAGES = {"float16": 4, "bfloat16": 6}
SCALINGS = ("tensor",)  # per-tensor power-of-two scaling of storage mode (module docstring)
ACCUMULATES = ("float64",)  # the sum over slice assignments in a wider type (module docstring)
SCALE_BITS = 14  # the largest stored magnitude of a scaled tensor lies in [2^14, 2^15]
# compute modes (module docstring).  "bf16x3": its code for tnco_hip_contract_set_compute; "matrix" has entry points of
# its own (tnco_hip_contract_set_matrix) and no code
COMPUTES = {"bf16x3": 1, "matrix": None}
MAX_SLICE_BATCH = 64  # slice assignments per launch at most (csrc/contract.hip MAX_SLICE_BATCH)
MAX_PATH_KERNEL = 1024  # path kernel: assignments per launch at most (csrc/contract_path.h MAX_PATH_GROUP)
# path kernel: multiply-adds (H M N K) of one step at most -- one workgroup runs it.  A guard against a step that would
# hold one compute unit of a shared card for long, not a tuned threshold (csrc/contract_path.h MAX_PATH_STEP_MACS)
MAX_PATH_STEP_MACS = 1 << 24
MAX_PERMUTE_QUBITS = 8  # qubits of one Walkers.permute at the most (csrc/contract_walk.h WALK_MAX_PERMUTE)
MAX_CHOOSE_QUBITS = 6  # qubits of one Contractor.choose_joint at the most (csrc/contract_walk.h WALK_MAX_CHOOSE)

# operand / destination kinds, table widths and columns: the layout is specified by include/tnco_hip.h
# (tnco_hip_contract_desc); the names and values are those of csrc/contract_tables.h
LEAF, ARENA, OUT = 0, 1, 2
PERM_W = 8 + 2 * MAX_AXES
STEP_W = 16
LEAF_SL_W = 1 + 2 * MAX_AXES
# steps: an operand's kind, ref and two strides, those of B ST_SIDE after those of A; the exponent slots under scaling
ST_A_KIND, ST_A_REF, ST_A_M, ST_A_K, ST_B_KIND, ST_B_REF, ST_B_K, ST_B_N = range(8)
ST_C_KIND, ST_C_REF, ST_H, ST_M, ST_N, ST_K, ST_A_SLOT, ST_B_SLOT = range(8, 16)
ST_SIDE = 4
# perms: column 7 is 0; PM_DIMS and PM_STRIDES start blocks of MAX_AXES columns
PM_SRC_KIND, PM_SRC_REF, PM_DST_KIND, PM_DST_REF, PM_NDIM, PM_NUMEL, PM_GROUP = range(7)
PM_DIMS, PM_STRIDES = 8, 8 + MAX_AXES
# leaf_sl: the number of sliced axes, then their slice positions and their element strides
LS_COUNT, LS_SLOTS, LS_STRIDES = 0, 1, 1 + MAX_AXES
# the kernel paths of csrc/contract.hip in the order tnco_hip_contract_kernel_launches counts them; a tiled name gives
# the memory order of A, then of B (mk_kn: A [m][k], B [k][n])
KERNEL_PATHS = ("gather", "tiled_km_nk", "tiled_km_kn", "tiled_mk_nk", "tiled_mk_kn", "dot", "stream")
# the row-mapped GEMM paths (steps with a row axis) in the order tnco_hip_contract_row_launches counts them
ROW_KERNEL_PATHS = ("rows_tiled", "rows_dot", "rows_stream")
# the kernels that read a folded operand in place (indirect=True) in the order tnco_hip_contract_indirect_launches counts them
INDIRECT_KERNEL_PATHS = ("ix_tiled", "ix_dot", "ix_stream")
IND_W = 6  # ind_steps: offsets into ind_maps of the tables of A by h, m, k and of B by h, k, n; -1: the operand is not folded
IX_A_H, IX_A_M, IX_A_K, IX_B_H, IX_B_K, IX_B_N = range(IND_W)
IX_SIDE = 3
ROW_W = 5  # row_steps: R, rows of A, map of A, rows of B, map of B (a map: offset into row_maps, -1 none)
RW_R, RW_A_ROWS, RW_A_MAP, RW_B_ROWS, RW_B_MAP = range(ROW_W)
RW_SIDE = 2
# words per row of the tables that exist on the device only: the permute groups of the path kernel (first row, count), the
# leaves of a run over leaf sets (pointer, set stride) and over walkers (pointer, qubit, version stride)
GR_W, SET_W, WALK_W = 2, 2, 3
PROJ = "proj"  # the first axis of a projected result
ALIGN = 64  # arena offsets in elements: 64 x (4..16 B) keeps every buffer 256-byte aligned


@dataclass(frozen=True)
class ContractionResult:
    inds: object  # tuple of the result's axes (a list of tuples when the path leaves several tensors)
    array: object  # numpy array with exactly those axes (a list of them)
    macs: int  # multiply-adds launched, all slice assignments
    n_slices: int  # slice assignments run
    peak_device_bytes: int  # device memory the plan reserved
    launches: int = 0  # kernel launches
    device_s: float = 0.0  # device time of the kernels (copies in and out excluded)
    fuse_macs: int = 0  # contract_results: multiply-adds of the fuse stage (not part of `macs`)
    kernel_launches: tuple = (0,) * len(KERNEL_PATHS)  # launches per kernel path, in KERNEL_PATHS order
    row_kernel_launches: tuple = (0, 0, 0)  # ... per row-mapped path, in ROW_KERNEL_PATHS order
    scaling: str = None  # "tensor": per-tensor scaling of storage mode
    exponents: tuple = None  # scaling: the exponents after the last slice assignment, leaves first, then one per step
    #                          (the step that writes the output: 0); None without scaling (a list of them: as `array`)
    narrow_launches: int = 0  # scaling: launches of the narrowing pass
    slice_batch: int = None  # slice assignments per launch, the effective value (`Plan.slice_batch`; of several calls
    #                          the largest, of an unsliced call 1); None: unbatched
    batch_launches: int = 0  # slice_batch: launches of the kernel that folds a group's blocks into the output;
    #                          `launches` is the four counts together
    compute: str = None  # "bf16x3": the tiled-class steps ran as three bfloat16 products on the matrix cores; "matrix":
    #                      they ran on the matrix cores in the arrays' own precision
    split_launches: int = 0  # compute: launches of the split kernel (they are part of their tiled slot of kernel_launches)
    path_kernel: int = None  # assignments per launch of the path kernel, the effective value (`Plan.path_kernel`; of several
    #                          calls the largest, of an unsliced call 1); None: the unfused run
    path_launches: tuple = (0, 0)  # path_kernel: launches of the path kernel and of the kernel that folds a group's blocks
    #                                into the output; `launches` is their sum and the other launch counts are zeros
    hoisted: tuple = None  # hoist=True: (steps, permutes) that ran once per call instead of once per assignment
    #                        (`Plan.hoisted`; of several calls the sums); None without the keyword
    reused: tuple = None  # reuse=True: (steps, permutes) that ran only at the assignments that change their slices
    #                       (`Plan.reused`; of several calls the sums); None without the keyword
    indirect: int = None  # indirect=True: step operands read in place through offset tables instead of being permuted
    #                       (`Plan.indirect`; of several calls the sum); None without the keyword
    indirect_launches: tuple = (0, 0, 0)  # indirect: launches per kernel that reads a folded operand, in
    #                                       INDIRECT_KERNEL_PATHS order; part of `launches`, of no slot of kernel_launches
    matrix_launches: int = 0  # compute="matrix": launches of the matrix kernel (they are part of their tiled slot of
    #                           kernel_launches)


@dataclass(frozen=True)
class ManyResult:
    """What `Contractor.run_many` returns: the results of R leaf sets of one plan."""
    inds: tuple  # ("set",) + Plan.inds
    array: object  # (R,) + Plan.shape: array[i] is byte for byte `run` of leaf set i; numpy array or torch tensor
    #                (run_walkers: None, the outputs stay on the device)
    sets: int  # R
    group: int  # members (set, assignment) per launch, the effective value: min(what was asked for, R x assignments)
    macs: int  # multiply-adds launched: R times a run's
    launches: int  # kernel launches
    path_launches: tuple  # launches of the path kernel over sets and of the kernel that folds a group's blocks into the
    #                       outputs: ceil(R x assignments / group) each; `launches` is their sum
    peak_device_bytes: int  # device memory the handle holds after the call (`Contractor.many_bytes`)
    device_s: float = 0.0  # device time of the kernels (copies in and out excluded)


@dataclass
class Plan:
    """Everything the device needs, as flat int64 tables (one row per leaf / permute / step)."""
    dtype: np.dtype
    inds: tuple  # the result's axes (as tnco_amd.app.tn.contract orders them)
    shape: tuple
    slice_inds: tuple  # sliced indices, the first one the most significant digit of an assignment
    slice_dims: tuple
    block_inds: tuple  # sliced indices the result holds: the output buffer is [block axes][the others]
    leaf_numel: np.ndarray
    leaf_sl: np.ndarray  # [n_leaves, LEAF_SL_W]: n, slice ids, strides of the leaf's sliced axes
    perms: np.ndarray  # [n_perms, PERM_W]: src kind, src ref, dst kind, dst ref, ndim, numel, group, 0, dims, strides
    steps: np.ndarray  # [n_steps, STEP_W]: A kind/ref/sm/sk, B kind/ref/sk/sn, C kind/ref, H, M, N, K, 0, 0
    arena_elems: int
    out_numel: int
    macs_per_slice: int
    slice_range: tuple = (0, 1)
    ops: list = field(default_factory=list)  # readable copy of the step decisions (tests, tools)
    # projections (None / empty without `projs`)
    sparse_inds: tuple = ()
    storage: str = None  # "float16" / "bfloat16": the type of leaves and arena on the device (dtype: sums, output)
    row_steps: np.ndarray = None  # [n_steps, ROW_W]
    row_maps: np.ndarray = None  # int32 pool of the maps
    leaf_rows: tuple = ()  # per leaf: None, or (axes of its sparse indices, their values [rows, len(axes)])
    out_rows: tuple = None  # (rows of the final tensor, row of it for each of the P projections)
    scaling: str = None  # "tensor": steps columns 14, 15 are the exponent slots of A and B (leaf t: t, step j: n_leaves + j)
    stage_refs: np.ndarray = None  # scaling: [n_steps] arena offset of a stored step's float32 staging buffer, -1 none
    slice_batch: int = None  # assignments per launch: min(what was asked for, assignments of slice_range); 1 without steps
    compute: str = None  # "bf16x3" / "matrix": the tiled-class steps on the matrix cores; the tables do not depend on it
    path_kernel: int = None  # assignments per launch of the path kernel: min(what was asked for, assignments of slice_range);
    #                          1 without steps
    hoisted: tuple = None  # hoist=True: (steps hoisted, permutes hoisted); None without the keyword
    step_hoist: np.ndarray = None  # hoist=True: [n_steps] 1 where the step runs once per call, before the first assignment
    perm_hoist: np.ndarray = None  # hoist=True: [n_perms] the same per row of `perms` (within a group the hoisted rows first)
    kept: tuple = ()  # hoist=True: (arena offset, elements) of every slice-free tensor that a step of the assignments reads;
    #                   reuse=True: of every tensor whose reader has a smaller period than its writer
    hoisted_macs: int = 0  # multiply-adds of the hoisted steps (they are part of macs_per_slice)
    indirect: int = None  # indirect=True: the operands folded (read in place through ind_maps); None without the keyword
    ind_steps: np.ndarray = None  # [n_steps, IND_W]; None when nothing is folded
    ind_maps: np.ndarray = None  # int64 pool of the offset tables: entry i of a table is the sum of digit x source stride
    #                              over the table's group of axes, i linearised as the plain plan linearises the group
    reused: tuple = None  # reuse=True: (steps, permutes) with a period above 1; None without the keyword
    step_period: np.ndarray = None  # reuse=True: [n_steps] the step runs at assignment a iff a is the first of slice_range
    #                                 or a % period == 0; a period is a place of a sliced index or the number of assignments
    perm_period: np.ndarray = None  # reuse=True: [n_perms] the same per row of `perms` (within a group the slowest rows first)
    kept_period: tuple = ()  # reuse=True: per entry of `kept` the period of the item that writes it
    accumulate: str = None  # "float64": the blocks of the assignments are summed in float64 / complex128 and rounded once; the
    #                         tables do not depend on it

    @property
    def n_slices(self) -> int:
        return math.prod(self.slice_dims)

    @property
    def macs(self) -> int:
        if self.step_period is not None:  # every step as often as it is due
            return sum(_runs(int(P), *self.slice_range) * _step_macs(r) for P, r in zip(self.step_period, self.steps))
        return self.hoisted_macs + (self.macs_per_slice - self.hoisted_macs) * (self.slice_range[1] - self.slice_range[0])

    @property
    def peak_device_bytes(self) -> int:
        item = self.dtype.itemsize
        held = item if self.storage is None else _storage_itemsize(self.dtype)  # of leaves and arena
        tables = 8 * (self.leaf_sl.size + self.perms.size + 2 * self.leaf_numel.size)
        maps = 0 if self.row_maps is None else 4 * self.row_maps.size + 8 * self.row_steps.size
        # scaling: an int32 exponent per leaf and step, a max word per step
        scale = 0 if self.scaling is None else 4 * (self.leaf_numel.size + 2 * len(self.steps))
        # a slice batch or a path kernel: an arena and the scale words per member, and a block of the output per member
        # as staging
        members = self.slice_batch if self.path_kernel is None else self.path_kernel
        batch, stage = 1, 0
        if members is not None and len(self.steps):
            batch = members
            stage = item * batch * self.out_numel // math.prod(self.shape[self.inds.index(x)] for x in self.block_inds)
        # a path kernel: also the tables that are new on the device: the steps, the first row and the count of every
        # permute group, the placement of every assignment
        if self.path_kernel is not None and len(self.steps):
            tables += 8 * (self.steps.size + GR_W * (len(self.steps) + 1) + self.slice_range[1] - self.slice_range[0])
        if self.ind_steps is not None:
            tables += 8 * (self.ind_steps.size + self.ind_maps.size)
        # accumulate: the wide accumulator, and unbatched a staging block of its own; a plan without steps sums nothing
        wide = 0
        if self.accumulate is not None and len(self.steps):
            block = self.out_numel // math.prod(self.shape[self.inds.index(x)] for x in self.block_inds)
            wide = 2 * item * self.out_numel + (item * block if members is None else 0)
        return held * (int(self.leaf_numel.sum()) + self.arena_elems * batch) + item * self.out_numel + tables + maps + \
            scale * batch + stage + wide


class _Arena:
    """First-fit offsets in one device buffer; a block is released after its last reader."""

    def __init__(self):
        self.free = []  # sorted (offset, size)
        self.top = self.peak = 0

    def alloc(self, n: int) -> int:
        n = max(ALIGN, -(-n // ALIGN) * ALIGN)
        for k, (off, size) in enumerate(self.free):
            if size >= n:
                self.free[k:k + 1] = [(off + n, size - n)] if size > n else []
                return off
        off, self.top = self.top, self.top + n
        self.peak = max(self.peak, self.top)
        return off

    def release(self, off: int, n: int) -> None:
        n = max(ALIGN, -(-n // ALIGN) * ALIGN)
        blocks = sorted(self.free + [(off, n)])
        merged = []
        for o, s in blocks:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + s)
            else:
                merged.append((o, s))
        if merged and merged[-1][0] + merged[-1][1] == self.top:  # the tail goes back to the top
            self.top = merged.pop()[0]
        self.free = merged


def _check_path(path, n: int) -> list:
    steps, live = [], n
    for step in path:
        try:
            a, b = (int(q) for q in step)
        except (TypeError, ValueError) as e:
            raise ValueError("'path' is not valid.") from e
        if a == b or not (0 <= a < live and 0 <= b < live):
            raise ValueError("'path' is not valid.")
        steps.append((min(a, b), max(a, b)))
        live -= 1
    return steps


def _dims_of(ts_inds, shapes) -> dict:
    if len(shapes) != len(ts_inds):
        raise ValueError("'ts_inds' is not consistent with 'arrays'.")
    dims = {}
    for xs, shape in zip(ts_inds, shapes):
        if len(shape) != len(xs) or len(set(xs)) != len(xs):
            raise ValueError("'ts_inds' is not consistent with 'arrays'.")
        for x, d in zip(xs, shape):
            if dims.setdefault(x, d) != d:
                raise ValueError("'ts_inds' is not consistent with 'arrays'.")
    return dims


def _compute_dtype(arrays) -> np.dtype:
    for a in arrays:
        if a.dtype not in DTYPES:
            raise TypeError(f"dtype {a.dtype} is not supported (float32, float64, complex64, complex128).")
    return np.result_type(*arrays) if arrays else np.dtype(np.float64)


def _storage_itemsize(dtype) -> int:
    return 4 if np.dtype(dtype).kind == "c" else 2


SLICE_ORDER_ERROR = "'slice_order' must be None, 'reuse' or every sliced index once."
_F32 = (np.dtype(np.float32), np.dtype(np.complex64))


def _is_count(most):
    return lambda v: not isinstance(v, bool) and isinstance(v, int) and 1 <= v <= most


def _is_index(v, lo, hi) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= v < hi


def _ptr(a):
    """A numpy array's memory as an argument of the library (the pointer keeps the array alive)."""
    return a.ctypes.data_as(C.c_void_p)


def _i64(v):
    """A sequence of integers as an int64 table for the library; None for an empty one."""
    return _ptr(np.array(v, np.int64)) if len(v) else None


def _is_order(v) -> bool:
    """What can be said without the network: that a sequence names every sliced index once is checked where they are known."""
    if isinstance(v, str):
        return v == "reuse"
    try:
        return len(set(v)) == len(tuple(v))
    except TypeError as e:
        raise ValueError(SLICE_ORDER_ERROR) from e


def _given(*names, text="'{0}' is not supported with '{1}'.", error=NotImplementedError):
    """Rules of the keyword `names[0]`: it is refused when one of the others is given ({0} the other, {1} the keyword)."""
    return tuple((lambda o, dtype, x=x: getattr(o, x) is not None, error, text.format(x, names[0])) for x in names[1:])


# The option keywords in the order they are checked.  Of each: the test of a value that is not None, what the value must
# be (ValueError otherwise), and the rules that follow, first match: (refused when, exception, message; {dtype}: the
# compute dtype).  The last rule of every keyword is not listed: no projections.
_RULES = {
    "compute": (lambda v: isinstance(v, str) and v in COMPUTES, "None or " + " or ".join(repr(s) for s in COMPUTES),
                _given("compute", "storage", text="'{1}' and '{0}' are exclusive.", error=ValueError) +
                ((lambda o, dtype: o.compute == "bf16x3" and dtype not in _F32, TypeError,
                  "with 'compute' the compute dtype must be float32 or complex64, not {dtype}."),)),
    "storage": (lambda v: v in STORAGES, "None, " + " or ".join(repr(s) for s in STORAGES),
                ((lambda o, dtype: dtype not in _F32, TypeError,
                  "with 'storage' the compute dtype must be float32 or complex64, not {dtype}."),)),
    "scaling": (lambda v: isinstance(v, str) and v in SCALINGS, "None or 'tensor'",
                ((lambda o, dtype: o.storage is None, ValueError, "'scaling' needs 'storage'."),)),
    "slice_batch": (_is_count(MAX_SLICE_BATCH), f"None or an integer from 1 to {MAX_SLICE_BATCH}", ()),
    "path_kernel": (_is_count(MAX_PATH_KERNEL), f"None or an integer from 1 to {MAX_PATH_KERNEL}",
                    _given("path_kernel", "slice_batch", text="'{1}' and '{0}' are exclusive.", error=ValueError) +
                    _given("path_kernel", "storage", "compute")),
    "hoist": (lambda v: v is True, "None or True", _given("hoist", "path_kernel", text="'{1}' is not supported with '{0}'.")),
    "indirect": (lambda v: v is True, "None or True", _given("indirect", "storage", "compute", "path_kernel")),
    "reuse": (lambda v: v is True, "None or True",
              _given("reuse", "hoist", text="'{1}' includes '{0}': give one of them.", error=ValueError) +
              _given("reuse", "slice_batch", "path_kernel")),
    "slice_order": (_is_order, "None, 'reuse' or every sliced index once",
                    ((lambda o, dtype: isinstance(o.slice_order, str) and o.reuse is not True, ValueError,
                      "slice_order='reuse' needs reuse=True."),)),
    "accumulate": (lambda v: isinstance(v, str) and v in ACCUMULATES, "None or 'float64'",
                   ((lambda o, dtype: dtype not in _F32, TypeError,
                     "with 'accumulate' the compute dtype must be float32 or complex64, not {dtype}."),)),
}


@dataclass(frozen=True)
class _Options:
    """The option keywords of `plan`, `contract` and `contract_results` (module docstring), as one call was given them."""
    storage: object = None
    scaling: object = None
    slice_batch: object = None
    compute: object = None
    path_kernel: object = None
    hoist: object = None
    indirect: object = None
    reuse: object = None
    slice_order: object = None
    accumulate: object = None

    def check(self, dtype, projs=None) -> None:
        """Raises what _RULES refuses of the keywords, for arrays of the compute dtype `dtype` and the projections `projs`."""
        dtype = np.dtype(dtype)
        for name, (is_valid, must_be, rules) in _RULES.items():
            if getattr(self, name) is None:
                continue
            if not is_valid(getattr(self, name)):
                raise ValueError(f"'{name}' must be {must_be}.")
            for refused, error, text in rules:
                if refused(self, dtype):
                    raise error(text.format(dtype=dtype))
            if projs is not None:
                raise NotImplementedError(f"projections are not supported with '{name}'.")

    def keywords(self, **other) -> dict:
        """The record as the keywords of a call, those of `other` in place of its own."""
        return {**vars(self), **other}


def _named_order(slice_order, slice_inds) -> tuple:
    """`slice_inds` in the order of the sequence `slice_order`, which must name each of them once."""
    order = tuple(slice_order)
    if len(order) != len(slice_inds) or set(order) != set(slice_inds):
        raise ValueError(SLICE_ORDER_ERROR)
    return order


def _step_macs(row) -> int:
    """H M N K of a row of `Plan.steps`."""
    return int(row[ST_H]) * int(row[ST_M]) * int(row[ST_N]) * int(row[ST_K])


def _runs(period: int, lo: int, hi: int) -> int:
    """The assignments a of [lo, hi) at which an item of that period is due: a == lo or a % period == 0."""
    return 1 + (hi - 1) // period - lo // period


def _reuse_macs(order, deps, each, dims, lo, hi) -> int:
    """The multiply-adds of a run under reuse=True with the sliced indices in `order`: deps[k] the sliced indices below
    step k, each[k] its H M N K."""
    place, n = {}, 1
    for x in reversed(order):
        place[x], n = n, n * dims[x]
    return sum(_runs(min((place[x] for x in d), default=n), lo, hi) * m for d, m in zip(deps, each))


def _reuse_order(default, deps, each) -> tuple:
    """slice_order="reuse": the fastest place first, each time the index with the least multiply-adds in the steps that
    hold it and that no faster index covers yet; of equal ones the later of `default`."""
    left, covered, fastest_first = list(default), set(), []
    while left:
        cost = {x: sum(m for k, (d, m) in enumerate(zip(deps, each)) if k not in covered and x in d) for x in left}
        x = min(reversed(left), key=cost.get)
        fastest_first.append(x)
        left.remove(x)
        covered |= {k for k, d in enumerate(deps) if x in d}
    return tuple(reversed(fastest_first))


def _step_deps(steps, ts_inds, sl) -> list:
    """Per step of the path: the indices of `sl` that the leaves below its result hold."""
    live = [frozenset(x for x in xs if x in sl) for xs in ts_inds]
    out = []
    for a, b in steps:
        db, da = live.pop(b), live.pop(a)
        live.append(da | db)
        out.append(da | db)
    return out


def _offset_table(group, st, dims) -> np.ndarray:
    """Entry i: the sum of digit x st[axis] over the axes of `group`, i the row-major number of the digits."""
    t = np.zeros(1, np.int64)
    for x in group:
        t = (t.reshape(-1, 1) + np.arange(dims[x], dtype=np.int64) * st[x]).reshape(-1)
    return t


def _check_path_steps(p) -> None:
    """ValueError when a step of the plan is beyond what one workgroup of the path kernel is given."""
    for k, row in enumerate(p.steps):
        H, M, N, K = (int(row[q]) for q in (ST_H, ST_M, ST_N, ST_K))
        if H * M * N * K > MAX_PATH_STEP_MACS:
            raise ValueError(f"step {k} (H M N K = {H} x {M} x {N} x {K}) has more than 2^24 multiply-adds: too large for "
                             "'path_kernel', which runs a step in one workgroup.")


def split_bf16(a):
    """(hi, lo) as the split kernel (csrc/contract_split.h) takes a float32 / complex64 array apart, both of its
    dtype and shape: per float32 part hi = bfloat16(x) to nearest even, lo = bfloat16(x - hi), and lo = 0 where hi is
    not finite."""
    a = np.asarray(a)
    x = _parts(a)
    like = np.empty(x.shape, np.float32)
    hi = _from_storage_bits(_bf16_bits(x).reshape(x.shape), "bfloat16", like)
    with np.errstate(invalid="ignore"):
        rest = np.where(np.isfinite(hi), x - hi, np.float32(0)).astype(np.float32)
    lo = _from_storage_bits(_bf16_bits(rest).reshape(x.shape), "bfloat16", like)
    if a.dtype.kind == "c":
        return tuple(q.reshape(-1).view(np.complex64).reshape(a.shape) for q in (hi, lo))
    return hi.reshape(a.shape), lo.reshape(a.shape)


def _check_split_range(a) -> None:
    """ValueError when a finite part of `a` rounds to an infinite bfloat16 (the hi of the split)."""
    x = _parts(a)
    if (np.isfinite(x) & ((_bf16_bits(x) & 0x7F80) == 0x7F80).reshape(x.shape)).any():
        raise ValueError("an array has finite values beyond the range of the bfloat16 split (|x| >= 2^128 - 2^119).")


def _bf16_bits(x) -> np.ndarray:
    """The bfloat16 nearest to each float32 of x, ties to even, as uint16; NaN stays NaN (quiet), what lies beyond the
    largest bfloat16 becomes inf."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def _storage_bits(a, storage, check=True) -> np.ndarray:
    """A float32 / complex64 array in storage layout: uint16 of the same shape (complex: one more axis of 2, re and
    im).  ValueError when a finite value is not finite in the storage type; with check=False it becomes inf, as an
    intermediate does on the device."""
    parts = _parts(a)
    if storage == "float16":
        with np.errstate(over="ignore"):
            half = parts.astype(np.float16)
        bits, finite = half.view(np.uint16), np.isfinite(half)
    else:
        bits = _bf16_bits(parts).reshape(parts.shape)
        finite = (bits & 0x7F80) != 0x7F80
    if check and (np.isfinite(parts) & ~finite).any():
        raise ValueError(f"an array has finite values beyond the range of {storage}.")
    return bits


def round_to_storage(a, storage) -> np.ndarray:
    """`a` (float32 / complex64) with every part rounded to `storage` as the engine rounds a leaf: same dtype and
    shape.  ValueError as the engine raises it."""
    a = np.asarray(a)
    _Options(storage=storage).check(a.dtype)
    return _from_storage_bits(_storage_bits(a, storage), storage, a)


def _parts(a) -> np.ndarray:
    """The float32 parts of a float32 / complex64 array (complex: one more axis of 2, re and im), contiguous."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.float32).reshape(a.shape + (2,)) if a.dtype.kind == "c" else a.astype(np.float32, copy=False)


def scale_exponent(a) -> int:
    """The exponent the scaling rule (module docstring) gives the tensor `a` (float32 / complex64), in integer
    arithmetic on the float32 bit patterns: csrc/contract_half.h ct_scale_exponent restated."""
    u = _parts(a).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)
    u = u[u < 0x7F800000]
    m = int(u.max()) if u.size else 0
    if m == 0:
        return 0
    lg = (m >> 23) - 127 if m >> 23 else (m.bit_length() - 1) - 149
    return lg - SCALE_BITS


def _scaled_bits(a, storage):
    """(_storage_bits of `a` scaled by its exponent, the exponent)."""
    e = scale_exponent(a)
    with np.errstate(under="ignore"):
        scaled = np.ldexp(_parts(a), np.int32(-e)).astype(np.float32, copy=False)
    return _storage_bits(scaled, storage, check=False), e


def scale_to_storage(a, storage):
    """(values, exponent): `a` (float32 / complex64) as the engine holds it as a leaf under scaling="tensor" -- every
    part scaled by 2^-exponent, rounded to `storage` and scaled back: same dtype and shape -- and the leaf's exponent,
    a Python int (module docstring)."""
    a = np.asarray(a)
    if storage not in STORAGES:
        raise ValueError(f"'storage' must be {' or '.join(repr(s) for s in STORAGES)}.")
    _Options(storage=storage).check(a.dtype)
    bits, e = _scaled_bits(a, storage)
    like = np.empty(bits.shape, np.float32)
    with np.errstate(over="ignore"):
        parts = np.ldexp(_from_storage_bits(bits, storage, like), np.int32(e)).astype(np.float32, copy=False)
    values = parts.reshape(-1).view(np.complex64).reshape(a.shape) if a.dtype.kind == "c" else parts.reshape(a.shape)
    return values, e


def _from_storage_bits(bits, storage, like) -> np.ndarray:
    """The values of _storage_bits, widened: the dtype and shape of `like`."""
    if storage == "float16":
        parts = bits.view(np.float16).astype(np.float32)
    else:
        parts = (bits.astype(np.uint32) << 16).view(np.float32)
    return parts.view(np.complex64).reshape(like.shape) if like.dtype.kind == "c" else parts.reshape(like.shape)


def _fits(layout, head, rest, s_order, s_first) -> bool:
    """layout == head + s_order + rest (s_first) or head + rest + s_order, `rest` in the layout's own order."""
    body = tuple(layout[len(head):])
    if tuple(layout[:len(head)]) != tuple(head):
        return False
    ns = len(s_order)
    s_part, r_part = (body[:ns], body[ns:]) if s_first else (body[len(body) - ns:], body[:len(body) - ns])
    return s_part == tuple(s_order) and set(r_part) == set(rest)


class _Live:
    """A tensor of the step loop: its axes in memory order and where it lives."""

    def __init__(self, inds, kind, ref, leaf=None):
        self.inds, self.kind, self.ref, self.leaf = tuple(inds), kind, ref, leaf


class _RowAxis:
    """The row axis of the tensors that hold the sparse indices of columns `cols` of projs: an index like any other
    to the permutes and the arena, always outermost."""

    def __init__(self, cols):
        self.cols = tuple(cols)

    def __eq__(self, other):
        return isinstance(other, _RowAxis) and other.cols == self.cols

    def __hash__(self):
        return hash(("rows", self.cols))

    def __repr__(self):
        return f"rows{self.cols}"


def _check_projs(sparse_inds, projs, dims, ts_inds, out_inds, sl):
    sparse = tuple(sparse_inds)
    held = {x for xs in ts_inds for x in xs}
    if len(set(sparse)) != len(sparse) or not set(sparse) <= held:
        raise ValueError("'sparse_inds' has indices not in 'ts_inds'.")
    if not set(sparse) <= set(out_inds):
        raise ValueError("'sparse_inds' must be output indices.")
    if set(sparse) & sl:
        raise NotImplementedError("a sliced index that is also sparse is not supported.")
    projs = np.asarray(projs)
    if projs.dtype.kind not in "iu":
        raise TypeError("'projs' must be an array of integers.")
    if projs.ndim != 2 or projs.shape[1] != len(sparse) or projs.shape[0] < 1:
        raise ValueError("'projs' must have shape [P, len(sparse_inds)], P >= 1.")
    projs = projs.astype(np.int64)
    if (projs < 0).any() or (projs >= np.array([dims[x] for x in sparse], np.int64).reshape(1, -1)).any():
        raise ValueError("'projs' has values beyond the dimensions of 'sparse_inds'.")
    return sparse, projs


def _unique_rows(table):
    """numpy.unique(axis=0) of an int64 [n, c] table, and the row of it that each of the n rows is; c == 0: one row."""
    if table.shape[1] == 0:
        return table[:1], np.zeros(len(table), np.int64)
    rows, inverse = np.unique(table, axis=0, return_inverse=True)
    return rows, inverse.reshape(-1)


def _size(xs, dims) -> int:
    return math.prod(dims[x] for x in xs)


def _dense_strides(inds, dims) -> dict:
    """index -> element stride of a dense tensor with the axes `inds`."""
    return {x: _size(inds[k + 1:], dims) for k, x in enumerate(inds)}


@dataclass(frozen=True)
class _Slices:
    """The slice set-up of a plan."""
    held: frozenset  # `slices` as given
    inds: tuple  # in order: the first one the most significant digit of an assignment
    dims: tuple
    lo: int  # the assignments of slice_range
    hi: int
    place: dict  # sliced index -> the product of the dimensions after it

    @property
    def n(self) -> int:
        return math.prod(self.dims)


def _plan_in_reuse_order(path, ts_inds, shapes, output_inds, slices, slice_range, dtype, options) -> Plan:
    """slice_order="reuse": the plan of the default order unless the greedy one has strictly fewer multiply-adds."""
    mode = dict(slices=slices, slice_range=slice_range, dtype=dtype)
    p = plan(path, ts_inds, shapes, output_inds, **mode, **options.keywords(slice_order=None))
    dims = dict(zip(p.slice_inds, p.slice_dims))
    deps = _step_deps(_check_path(path, len(p.leaf_numel)), [tuple(xs) for xs in ts_inds],
                      frozenset(x for x in slices if dims[x] > 1))
    each = [_step_macs(r) for r in p.steps]
    greedy = _reuse_order(p.slice_inds, deps, each)
    if greedy != p.slice_inds and _reuse_macs(greedy, deps, each, dims, *p.slice_range) < p.macs:
        p = plan(path, ts_inds, shapes, output_inds, **mode, **options.keywords(slice_order=greedy))
    return p


def _row_axis(xs, sparse, projs, rows_of, dims):
    """The row axis of a tensor that holds the indices xs, None when none of them is sparse; a new one enters `rows_of`
    (its table of values [rows, len(cols)]) and `dims`."""
    cols = tuple(sorted(sparse.index(x) for x in xs if x in sparse))
    if not cols:
        return None
    ax = _RowAxis(cols)
    if ax not in rows_of:
        rows_of[ax] = _unique_rows(projs[:, cols])[0]
        dims[ax] = len(rows_of[ax])
    return ax


def _project_leaves(sparse, projs, ts_inds, shapes, final, dims, rows_of):
    """The leaves and the final tensor with their sparse indices replaced by a row axis, outermost: `ts_inds` and `shapes`
    are changed in place (a leaf is restricted to its rows on the host: [rows][its other axes], sliced ones included).
    Returns (leaf_rows, the final tensor's axes)."""
    leaf_rows = []
    for t, (xs, shape) in enumerate(zip(ts_inds, shapes)):
        ax = _row_axis(xs, sparse, projs, rows_of, dims)
        if ax is None:
            leaf_rows.append(None)
            continue
        leaf_rows.append((tuple(xs.index(sparse[j]) for j in ax.cols), rows_of[ax]))
        kept = [k for k, x in enumerate(xs) if x not in sparse]
        ts_inds[t] = (ax,) + tuple(xs[k] for k in kept)
        shapes[t] = (dims[ax],) + tuple(shape[k] for k in kept)
    ax = _row_axis(final, sparse, projs, rows_of, dims)
    return tuple(leaf_rows), (() if ax is None else (ax,)) + tuple(x for x in final if x not in sparse)


def _projected_result(p, sparse, projs, leaf_rows, row_steps, row_maps, full_final, dims) -> Plan:
    """The fields of a plan with projections: the device holds the distinct rows of the final tensor; the result has one
    per projection, duplicates included."""
    p.sparse_inds, p.leaf_rows = sparse, leaf_rows
    p.row_steps = np.array(row_steps, np.int64).reshape(-1, ROW_W)
    p.row_maps = np.concatenate(row_maps + [np.zeros(0, np.int32)]).astype(np.int32)
    p.macs_per_slice = int(sum(int(w[RW_R]) * _step_macs(r) for w, r in zip(row_steps, p.steps)))
    rest = tuple(x for x in full_final if x not in sparse)
    if sparse:
        p.out_rows = (dims[p.inds[0]], _unique_rows(projs)[1])
    else:
        p.out_rows = (1, np.zeros(len(projs), np.int64))
    p.inds, p.shape = (PROJ,) + rest, (len(projs),) + tuple(dims[x] for x in rest)
    return p


def _slice_setup(sl, slice_order, slice_range, ts_inds, final, dims) -> _Slices:
    """The sliced indices in order, their dimensions and places and the range of assignments; refuses what is wrong
    with `slices`, `slice_order` and `slice_range`, and a tensor with too many axes after slicing."""
    every = list(dict.fromkeys(x for xs in ts_inds for x in xs))
    if not sl <= set(every):
        raise ValueError("'slices' has indices not in 'ts_inds'.")
    slice_inds = tuple(x for x in every if x in sl)
    if slice_order is not None:
        slice_inds = _named_order(slice_order, slice_inds)
    slice_dims = tuple(dims[x] for x in slice_inds)
    n_slices = math.prod(slice_dims)
    lo, hi = (0, n_slices) if slice_range is None else (int(slice_range[0]), int(slice_range[1]))
    if not 0 <= lo < hi <= n_slices:
        raise ValueError("'slice_range' is not valid.")
    if any(sum(x not in sl for x in xs) > MAX_AXES for xs in ts_inds + [final]):
        raise NotImplementedError(f"tensors with more than {MAX_AXES} axes (after slicing) are not supported.")
    place = {x: math.prod(slice_dims[k + 1:]) for k, x in enumerate(slice_inds)}
    return _Slices(sl, slice_inds, slice_dims, lo, hi, place)


def _period(dep, S: _Slices, hoist, reuse) -> int:
    """The period of a tensor whose leaves hold the sliced indices `dep`: it has one value for all assignments a with
    equal a // period.  reuse: the smallest place of `dep`, the number of assignments when `dep` is empty.  hoist is the
    two-level case and needs ranks only: 2 for a slice-free tensor, 1 for every other.  Without either: 1."""
    if reuse is True:
        return min((S.place[x] for x in dep), default=S.n)
    return 2 if hoist is True and bool(S.held) and not dep else 1


def _leaf_tables(ts_inds, shapes, dims, S: _Slices, hoist, reuse):
    """(leaf_numel, leaf_sl, per leaf index -> element stride of the full (unsliced) array, the leaves as the tensors
    the step loop starts from, each with its exponent slot, dep, per and free)."""
    slot = {x: k for k, x in enumerate(S.inds)}
    leaf_numel = np.array([math.prod(s) for s in shapes], np.int64)
    leaf_sl = np.zeros((len(ts_inds), LEAF_SL_W), np.int64)
    strides, live = [], []
    for t, xs in enumerate(ts_inds):
        st = _dense_strides(xs, dims)
        strides.append(st)
        cut = [x for x in xs if x in S.held]
        leaf_sl[t, LS_COUNT] = len(cut)
        leaf_sl[t, LS_SLOTS:LS_SLOTS + len(cut)] = [slot[x] for x in cut]
        leaf_sl[t, LS_STRIDES:LS_STRIDES + len(cut)] = [st[x] for x in cut]
        kept = tuple(x for x in xs if x not in S.held)
        # a leaf is read in place when its kept axes are one contiguous block (sliced axes outermost, or none)
        dense = all(st[x] == _size(kept[k + 1:], dims) for k, x in enumerate(kept))
        T = _Live(kept, LEAF if dense else None, t, t)
        T.slot = t  # (scaling: the exponent slot; a permute keeps it)
        # slice-free: no leaf below it holds a sliced index (it runs once per call; `indirect` leaves its permutes alone).
        # reuse: a sliced index of dimension 1 has one value in every assignment and counts as not held
        T.dep = frozenset(x for x in cut if dims[x] > 1) if reuse is True else frozenset(cut)
        T.per = _period(T.dep, S, hoist, reuse)
        T.free = bool(S.held) and not T.dep and (hoist is True or (reuse is True and S.n > 1))
        live.append(T)
    return leaf_numel, leaf_sl, strides, live


def _step_row_axes(A, B, projs, rows_of, dims):
    """(ra, rb, rz): the row axis of each operand and of the result of a step, each () or a 1-tuple.  Row axes stay
    outermost and out of the roles: h, m, n, k are computed over the other indices."""
    ra = tuple(x for x in A.inds[:1] if isinstance(x, _RowAxis))
    rb = tuple(x for x in B.inds[:1] if isinstance(x, _RowAxis))
    rz = (_RowAxis(sorted(set(ra[0].cols if ra else ()) | set(rb[0].cols if rb else ()))),) if ra or rb else ()
    if rz and rz[0] not in rows_of:
        rows_of[rz[0]] = _unique_rows(projs[:, rz[0].cols])[0]
        dims[rz[0]] = len(rows_of[rz[0]])
    return ra, rb, rz


def _operand_forms(A, B, head_a, head_b, xs, ys, s, dims):
    """(s_order, form_a, form_b): the order of the summed indices `s`, A's or B's, that moves the fewest elements, and
    the form in which each operand can be read as it lies -- A as head_a + xs + s_order (0) or head_a + s_order + xs (1), B
    as head_b + s_order + ys (0) or head_b + ys + s_order (1) -- None: it has to be permuted."""
    best = None
    for s_order in dict.fromkeys((tuple(q for q in A.inds if q in s), tuple(q for q in B.inds if q in s))):
        fa = [f for f in (0, 1) if A.kind is not None and _fits(A.inds, head_a, xs, s_order, f == 1)]
        fb = [f for f in (0, 1) if B.kind is not None and _fits(B.inds, head_b, ys, s_order, f == 0)]
        moved = (0 if fa else _size(A.inds, dims)) + (0 if fb else _size(B.inds, dims))
        if best is None or moved < best[0]:
            best = (moved, s_order, fa[0] if fa else None, fb[0] if fb else None)
    return best[1:]


def _row_step(ra, rb, rz, rows_of, dims, H, M, form_a, pool_len):
    """The row record of a projected step: (M of the step, its row of row_steps, the maps it adds to the pool of
    `pool_len` entries, its fields of `ops`)."""
    R = _size(rz, dims)
    if ra == rz and not rb and H == 1 and form_a == 0:
        # only the first operand has rows, stored [r][m][k]: a plain GEMM with R M rows
        return R * M, [1, 1, -1, 1, -1], [], dict(M=R * M, R=1, folded=True, a_map=None, b_map=None)
    maps = []
    for r in (ra, rb):
        if not r or r == rz:  # one row for every r / the rows of the result, in place
            maps.append(None)
            continue
        sub = rows_of[rz[0]][:, [rz[0].cols.index(c) for c in r[0].cols]]
        both, where = _unique_rows(np.concatenate([rows_of[r[0]], sub]))
        assert len(both) == len(rows_of[r[0]])  # (every row of the result restricts to a row it has)
        maps.append(where[len(both):].astype(np.int32))
    row = [0] * ROW_W
    row[RW_R], row[RW_A_ROWS], row[RW_B_ROWS] = R, _size(ra, dims), _size(rb, dims)
    for at, m in zip((RW_A_MAP, RW_B_MAP), maps):
        row[at] = -1 if m is None else pool_len
        pool_len += 0 if m is None else len(m)
    return M, row, [m for m in maps if m is not None], dict(R=R, folded=False, a_map=maps[0], b_map=maps[1])


def _replay_arena(front, events, buf_size):
    """(buffer -> arena offset, the peak).  One allocator, the phases in order of descending period (hoist: the hoisted
    phase first), the events of a phase in path order; a phase's temporaries are released, the kept buffers never.  Why
    that is sound when the phases run slowest first at every assignment at which they are due: a slower phase's
    temporaries may lie where a faster phase's kept buffers lie, because whenever the slower phase is due every faster
    one is due after it (the periods divide one another) and rewrites them.  They never lie on a slower phase's kept
    buffers, which are still allocated when the faster phase is planned."""
    arena, offset = _Arena(), {}
    for what, buf in (ev for P in sorted(set(front) | set(events), reverse=True) for ev in front[P] + events[P]):
        if what == "alloc":
            offset[buf] = arena.alloc(buf_size[buf])
        else:
            arena.release(offset[buf], buf_size[buf])
    return offset, arena.peak


def _patch_offsets(perms, rows, offset) -> None:
    """The buffer numbers of the arena refs of the permute and step rows replaced by their offsets."""
    for row in perms:
        for kind, ref in ((PM_SRC_KIND, PM_SRC_REF), (PM_DST_KIND, PM_DST_REF)):
            if row[kind] == ARENA:
                row[ref] = offset[row[ref]]
    for row in rows:
        for kind, ref in ((ST_A_KIND, ST_A_REF), (ST_B_KIND, ST_B_REF), (ST_C_KIND, ST_C_REF)):
            if row[kind] == ARENA:
                row[ref] = offset[row[ref]]


def _keyword_fields(p, o: _Options, offset, buf_size, stage, kept_bufs, kept_per, step_per, perm_per, ind_rows, ind_pool) -> None:
    """The fields of the plan that the option keywords `o` add to its tables."""
    lo, hi = p.slice_range
    if o.scaling is not None:
        p.scaling = o.scaling
        p.stage_refs = np.array([offset[b] if b >= 0 else -1 for b in stage], np.int64)
    if o.slice_batch is not None:  # (the tables are those of the unbatched plan)
        p.slice_batch = min(int(o.slice_batch), hi - lo) if len(p.steps) else 1
    if o.path_kernel is not None:  # (the tables are those of the unfused plan; projections were refused above)
        _check_path_steps(p)
        p.path_kernel = min(int(o.path_kernel), hi - lo) if len(p.steps) else 1
    p.kept = tuple((offset[b], buf_size[b]) for b in kept_bufs)  # (without hoist and reuse every period is 1: none)
    if o.hoist is not None:  # (without a hoisted step or permute the tables are those of the plan without the keyword)
        p.step_hoist, p.perm_hoist = (step_per == 2).astype(np.int64), (perm_per == 2).astype(np.int64)
        p.hoisted = (int(p.step_hoist.sum()), int(p.perm_hoist.sum()))
        p.hoisted_macs = int(sum(_step_macs(r) for r, h in zip(p.steps, p.step_hoist) if h))
    if o.reuse is not None:  # (when every period is 1 the tables are those of the plan without the keyword)
        p.step_period, p.perm_period = step_per, perm_per
        p.reused = (int((step_per > 1).sum()), int((perm_per > 1).sum()))
        p.kept_period = tuple(kept_per)
    if o.indirect is not None:  # (with nothing folded the tables are those of the plan without the keyword)
        p.indirect = sum((row[IX_A_H] >= 0) + (row[IX_B_H] >= 0) for row in ind_rows)
        if p.indirect:
            p.ind_steps = np.array(ind_rows, np.int64).reshape(-1, IND_W)
            p.ind_maps = np.concatenate(ind_pool).astype(np.int64)


def plan(path, ts_inds, shapes, output_inds=None, *, slices=(), slice_range=None, dtype=np.float64,
         sparse_inds=(), projs=None, storage=None, scaling=None, slice_batch=None, compute=None, path_kernel=None,
         hoist=None, indirect=None, reuse=None, slice_order=None, accumulate=None) -> Plan:
    """The device plan of one contraction along a path that leaves one tensor (no GPU).
    `shapes`: the leaves' shapes, in ts_inds order.  `sparse_inds`, `projs`, `storage`, `scaling`, `slice_batch`,
    `compute`, `path_kernel`, `hoist`, `indirect`, `reuse`, `slice_order`, `accumulate`: see the module docstring."""
    options = _Options(storage=storage, scaling=scaling, slice_batch=slice_batch, compute=compute, path_kernel=path_kernel,
                       hoist=hoist, indirect=indirect, reuse=reuse, slice_order=slice_order, accumulate=accumulate)
    options.check(dtype, projs)
    if isinstance(slice_order, str):
        return _plan_in_reuse_order(path, ts_inds, shapes, output_inds, slices, slice_range, dtype, options)
    ts_inds = [tuple(xs) for xs in ts_inds]
    shapes = [tuple(int(d) for d in s) for s in shapes]
    dims = _dims_of(ts_inds, shapes)
    steps = _check_path(path, len(ts_inds))
    final, out_inds = tnmod.contract(steps, ts_inds, output_inds, dims)
    if len(final) != 1:
        raise ValueError("plan() needs a path that leaves one tensor.")
    final = full_final = tuple(final[0])
    sl = frozenset(slices)
    if projs is None and tuple(sparse_inds):
        raise ValueError("'sparse_inds' need 'projs'.")
    rows_of, row_steps, row_maps = {}, [], []  # _RowAxis -> its table of values [rows, len(cols)]
    if projs is not None:
        sparse, projs = _check_projs(sparse_inds, projs, dims, ts_inds, out_inds, sl)
        leaf_rows, final = _project_leaves(sparse, projs, ts_inds, shapes, final, dims, rows_of)
    S = _slice_setup(sl, slice_order, slice_range, ts_inds, final, dims)
    leaf_numel, leaf_sl, strides, live = _leaf_tables(ts_inds, shapes, dims, S, hoist, reuse)

    # buffers are symbolic (numbers) until the event list is replayed on the arena.  One phase per period, keyed by it:
    # under `hoist` [2] the hoisted work of a call and [1] the work of an assignment, without a keyword everything in [1]
    buf_size, front, events = [], defaultdict(list), defaultdict(list)
    perms, rows, ops, stage = [], [], [], []
    perm_per, step_per, kept_bufs, kept_per = [], [], [], []
    ind_rows, ind_pool, ind_top = [], [], 0  # indirect: the rows of ind_steps, the tables of ind_maps, their length so far

    def new_buf(numel, at_start=False, h=1):
        buf_size.append(numel)
        (front if at_start else events)[h].append(("alloc", len(buf_size) - 1))
        return len(buf_size) - 1

    def permute(src, layout, group, dst_kind=ARENA):
        numel = _size(layout, dims)
        st = strides[src.leaf] if src.leaf is not None else _dense_strides(src.inds, dims)
        h = src.per if dst_kind == ARENA else 1  # (a permute has the period of its source)
        assert h == src.per or src.per == 1  # (what is copied to the output depends on every sliced index)
        perm_per.append(h)
        row = [0] * PERM_W
        row[PM_SRC_KIND], row[PM_SRC_REF] = (LEAF, src.leaf) if src.leaf is not None else (ARENA, src.ref)
        row[PM_DST_KIND], row[PM_DST_REF] = dst_kind, new_buf(numel, at_start=group < 0, h=h) if dst_kind == ARENA else 0
        row[PM_NDIM], row[PM_NUMEL], row[PM_GROUP] = len(layout), numel, group
        row[PM_DIMS:PM_DIMS + len(layout)] = [dims[x] for x in layout]
        row[PM_STRIDES:PM_STRIDES + len(layout)] = [st[x] for x in layout]
        perms.append(row)
        return row[PM_DST_REF]

    left = tnmod.get_hyper_count(ts_inds)
    keep = frozenset(out_inds) | frozenset(final)
    if not steps:  # a single leaf: copied (gathered, when sliced) into the output
        permute(live[0], tuple(x for x in final if x not in S.held), -1, OUT)
        ops.append(dict(copy=live[0].inds))
    for k, (a, b) in enumerate(steps):
        B, A = live.pop(b), live.pop(a)
        ra, rb, rz = _step_row_axes(A, B, projs, rows_of, dims)
        shared = frozenset(A.inds[len(ra):]) & frozenset(B.inds[len(rb):])
        stay = frozenset(x for x in shared if left[x] > 1) | (keep & shared)
        for x in shared:
            left[x] -= 1
        h = tuple(x for x in A.inds if x in stay)
        xs = tuple(x for x in A.inds[len(ra):] if x not in shared)
        ys = tuple(y for y in B.inds[len(rb):] if y not in shared)
        s_order, form_a, form_b = _operand_forms(A, B, ra + h, rb + h, xs, ys, shared - stay, dims)
        hst = min(A.per, B.per)  # the period of the step (hoist: 2, it is hoisted, when both operands are slice-free)
        step_per.append(hst)
        moved_from = []  # (the permutes of one step run in one launch: their sources are released after both)
        ind = [-1] * IND_W
        for side, (T, form, target) in enumerate(((A, form_a, ra + h + xs + s_order), (B, form_b, rb + h + s_order + ys))):
            # indirect: an operand that depends on the assignment is read where it lies when its three offset tables
            # are no larger than the copy they replace; roles, s_order and the result's layout stay as decided above
            groups = (h, s_order, ys) if side else (h, xs, s_order)
            if form is None and indirect is True and not T.free and T.per == hst and \
                    8 * sum(_size(g, dims) for g in groups) <= np.dtype(dtype).itemsize * _size(target, dims):
                st = strides[T.leaf] if T.leaf is not None else _dense_strides(T.inds, dims)
                for q, g in enumerate(groups):
                    ind[IX_SIDE * side + q] = ind_top
                    ind_pool.append(_offset_table(g, st, dims))
                    ind_top += len(ind_pool[-1])
                if T.leaf is not None:  # (also a leaf that is not dense after slicing: read at its slice offset)
                    T.kind, T.ref = LEAF, T.leaf
            elif form is None:
                ref = permute(T, target, -1 if T.leaf is not None else k)
                if T.kind == ARENA:
                    moved_from.append((T.ref, T.per))
                T.inds, T.kind, T.ref, T.leaf = target, ARENA, ref, None
        for q, per in moved_from:  # (a permute releases its source in its own phase)
            events[per].append(("free", q))
        form_a, form_b = form_a or 0, form_b or 0
        ind_rows.append(ind)
        H, M, N, K = _size(h, dims), _size(xs, dims), _size(ys, dims), _size(s_order, dims)
        z = rz + h + xs + ys
        assert not (hst > 1 and k == len(steps) - 1)  # (the last step is above every leaf that holds a sliced index)
        c_kind, c_ref = (OUT, 0) if k == len(steps) - 1 else (ARENA, new_buf(_size(z, dims), h=hst))
        if scaling is not None:
            # a stored result is summed into a float32 staging buffer (2 storage elements per element) and narrowed
            # from there: live beside the operands and the result for this step alone.  Allocated after everything
            # else of the step and released at once, it leaves every other offset as the plan without scaling has it.
            stage.append(new_buf(2 * _size(z, dims), h=hst) if c_kind == ARENA else -1)
            if c_kind == ARENA:
                events[hst].append(("free", stage[-1]))
        op = dict(h=h, x=xs, y=ys, s=s_order, form_a=form_a, form_b=form_b, H=H, M=M, N=N, K=K)
        if projs is not None:
            M, row, maps, fields = _row_step(ra, rb, rz, rows_of, dims, H, M, form_a, sum(len(q) for q in row_maps))
            row_steps.append(row)
            row_maps += maps
            op.update(fields)
        if indirect is not None:
            op.update(ind_a=ind[IX_A_H] >= 0, ind_b=ind[IX_B_H] >= 0)
        row = [0] * STEP_W
        row[ST_A_KIND], row[ST_A_REF], row[ST_B_KIND], row[ST_B_REF] = A.kind, A.ref, B.kind, B.ref
        row[ST_C_KIND], row[ST_C_REF] = c_kind, c_ref
        row[ST_A_M], row[ST_A_K] = (0, 0) if ind[IX_A_H] >= 0 else (K, 1) if form_a == 0 else (1, M)
        row[ST_B_K], row[ST_B_N] = (0, 0) if ind[IX_B_H] >= 0 else (N, 1) if form_b == 0 else (1, K)
        row[ST_H], row[ST_M], row[ST_N], row[ST_K] = H, M, N, K
        row[ST_A_SLOT], row[ST_B_SLOT] = (A.slot, B.slot) if scaling is not None else (0, 0)
        rows.append(row)
        ops.append(op)
        for T in (A, B):
            if T.kind == ARENA and T.per > hst:  # kept: its reader runs more often than its writer; never released
                kept_bufs.append(T.ref)
                kept_per.append(T.per)
            elif T.kind == ARENA:
                events[hst].append(("free", T.ref))
        Z = _Live(z, ARENA, c_ref)
        Z.slot, Z.dep, Z.per, Z.free = len(ts_inds) + k, A.dep | B.dep, hst, A.free and B.free
        live.append(Z)

    offset, peak = _replay_arena(front, events, buf_size)
    _patch_offsets(perms, rows, offset)
    perm_tab = np.array(perms, np.int64).reshape(-1, PERM_W)
    perm_per = np.array(perm_per, np.int64).reshape(-1)
    # slice-start gathers (group -1) first; within a group the rows of one period together, the slowest (hoisted) first
    order = np.lexsort((-perm_per, perm_tab[:, PM_GROUP]))
    p = Plan(dtype=np.dtype(dtype), inds=final, shape=tuple(dims[x] for x in final), slice_inds=S.inds,
             slice_dims=S.dims, block_inds=tuple(x for x in S.inds if x in final), leaf_numel=leaf_numel,
             leaf_sl=leaf_sl, perms=perm_tab[order], steps=np.array(rows, np.int64).reshape(-1, STEP_W), arena_elems=peak,
             out_numel=_size(final, dims), macs_per_slice=int(sum(_step_macs(r) for r in rows)), slice_range=(S.lo, S.hi),
             ops=ops, storage=storage, compute=compute, accumulate=accumulate)
    _keyword_fields(p, options, offset, buf_size, stage, kept_bufs, kept_per, np.array(step_per, np.int64).reshape(-1),
                    perm_per[order], ind_rows, ind_pool)
    if projs is None:
        return p
    return _projected_result(p, sparse, projs, leaf_rows, row_steps, row_maps, full_final, dims)


def check_memory(p: Plan, free_bytes: int) -> None:
    """RuntimeError when the plan's device memory exceeds what the device has free."""
    if p.peak_device_bytes > free_bytes:
        raise RuntimeError(f"the contraction needs {p.peak_device_bytes} bytes of device memory, "
                           f"{free_bytes} are free.")


def _split(path, n: int) -> list:
    """The tensors a linear path leaves, each as (its leaves in order, the steps that build it as a path over
    those leaves alone)."""
    ids = list(range(n))
    members = {t: (t,) for t in range(n)}
    made = {}  # new id -> (id of the first operand, id of the second)
    for a, b in path:
        ib, ia = ids.pop(b), ids.pop(a)
        new = n + len(made)
        made[new] = (ia, ib)
        members[new] = tuple(sorted(members[ia] + members[ib]))
        ids.append(new)
    out = []
    for root in ids:
        leaves = members[root]
        order = list(leaves)
        steps = []
        for new in sorted(q for q in made if set(members[q]) <= set(leaves)):
            ia, ib = made[new]
            pa, pb = order.index(ia), order.index(ib)
            steps.append((pa, pb))
            for q in sorted((pa, pb), reverse=True):
                del order[q]
            order.append(new)
        out.append((leaves, steps))
    return out


def _sub_output(ts_inds, leaves, output) -> frozenset:
    """Output indices of the sub-network of `leaves`: the network's own, plus what tensors outside it hold."""
    inside = {x for t in leaves for x in ts_inds[t]}
    outside = {x for t in range(len(ts_inds)) if t not in set(leaves) for x in ts_inds[t]}
    return frozenset(output) & inside | (inside & outside)


def contract(path, ts_inds, arrays, output_inds=None, *, slices=(), slice_range=None, device=None,
             sparse_inds=(), projs=None, storage=None, scaling=None, slice_batch=None, compute=None, path_kernel=None,
             hoist=None, indirect=None, reuse=None, slice_order=None, accumulate=None, _intermediates=()) -> ContractionResult:
    """Contract `arrays` (numpy, in ts_inds order) along the linear `path` on the GPU; see the module docstring.
    A path that leaves several tensors gives lists in `inds` / `array` (the sliced and the projected form need one
    tensor).  `_intermediates` (contract_results): positions of arrays that are results of earlier storage-mode calls,
    not leaves of the user: a value of theirs beyond the storage range becomes inf instead of being refused (with
    `scaling` they are scaled as leaves and nothing finite is beyond the range)."""
    loose = frozenset(_intermediates)
    ts_inds = [tuple(xs) for xs in ts_inds]
    arrays = [np.asarray(a) for a in arrays]
    dims = _dims_of(ts_inds, [a.shape for a in arrays])
    dtype = _compute_dtype(arrays)
    options = _Options(storage=storage, scaling=scaling, slice_batch=slice_batch, compute=compute, path_kernel=path_kernel,
                       hoist=hoist, indirect=indirect, reuse=reuse, slice_order=slice_order, accumulate=accumulate)
    options.check(dtype, projs)
    steps = _check_path(path, len(ts_inds))
    final, out = tnmod.contract(steps, ts_inds, output_inds, dims)
    if len(final) == 1:
        p = plan(steps, ts_inds, [a.shape for a in arrays], out, slices=slices, slice_range=slice_range, dtype=dtype,
                 sparse_inds=sparse_inds, projs=projs, **options.keywords())
        return _run(p, arrays, device, loose)
    if slices:
        raise NotImplementedError("slices need a path that leaves one tensor.")
    if projs is not None or tuple(sparse_inds):
        raise NotImplementedError("projections need a path that leaves one tensor.")
    parts = []
    if slice_order is not None and not isinstance(slice_order, str):
        _named_order(slice_order, ())
    # every part is unsliced: one assignment, nothing to hoist, nothing folded, every item runs once
    unsliced = dict(slice_batch=None if slice_batch is None else 1, path_kernel=None if path_kernel is None else 1,
                    hoisted=None if hoist is None else (0, 0), indirect=None if indirect is None else 0,
                    reused=None if reuse is None else (0, 0))
    for leaves, sub in _split(steps, len(ts_inds)):
        if not sub:  # a tensor the path does not touch: as the single-leaf plan gives it, rounded to storage
            a, e = arrays[leaves[0]].astype(dtype, copy=True), None
            if scaling is not None:
                a, e = scale_to_storage(a, storage)
            elif storage is not None:
                a = _from_storage_bits(_storage_bits(a, storage, leaves[0] not in loose), storage, a)
            elif compute == "bf16x3" and leaves[0] not in loose:
                _check_split_range(a)
            parts.append(ContractionResult(ts_inds[leaves[0]], a, 0, 1, 0, scaling=scaling, compute=compute,
                                           exponents=None if e is None else (e,), **unsliced))
            continue
        parts.append(contract(sub, [ts_inds[t] for t in leaves], [arrays[t].astype(dtype, copy=False) for t in leaves],
                              _sub_output(ts_inds, leaves, out), device=device, **options.keywords(slice_order=None),
                              _intermediates=[k for k, t in enumerate(leaves) if t in loose]))
    assert [tuple(r.inds) for r in parts] == [tuple(f) for f in final]
    return _sum_results(parts, inds=[r.inds for r in parts], array=[r.array for r in parts], n_slices=1,
                        exponents=None if scaling is None else [r.exponents for r in parts])


def _sum_results(parts, **given) -> ContractionResult:
    """The results of several calls as one.  `given`: inds, array, n_slices, exponents and fuse_macs, which are the
    caller's to say.  Of the others the counters are sums and `peak_device_bytes` the largest; `slice_batch` and
    `path_kernel` are the largest, `hoisted`, `reused` and `indirect` the sums, over the parts that have one, None when
    none has; `scaling` and `compute` are what the parts have in common."""
    def add(name):  # None is no part of a sum; tuples are added element by element
        values = [v for v in (getattr(r, name) for r in parts) if v is not None]
        if not values:
            return None
        return tuple(sum(c) for c in zip(*values)) if isinstance(values[0], tuple) else sum(values)

    def common(name):
        (value,) = {getattr(r, name) for r in parts}
        return value

    sums = ("macs", "launches", "device_s", "kernel_launches", "row_kernel_launches", "narrow_launches", "batch_launches",
            "split_launches", "path_launches", "hoisted", "reused", "indirect", "indirect_launches", "matrix_launches")
    return ContractionResult(peak_device_bytes=max(r.peak_device_bytes for r in parts),
                             slice_batch=max((r.slice_batch for r in parts if r.slice_batch is not None), default=None),
                             path_kernel=max((r.path_kernel for r in parts if r.path_kernel is not None), default=None),
                             scaling=common("scaling"), compute=common("compute"), **{name: add(name) for name in sums},
                             **given)


def _host_leaf(p: Plan, t: int, a, loose: bool = False):
    """(leaf t as the handle takes it from host memory, its exponent under scaling, else None): contiguous in the plan's
    dtype; with scaling scaled and rounded to storage; with storage rounded, a value beyond its range refused (not of a
    `loose` leaf); with compute="bf16x3" checked against the range of the split; with projections restricted to its rows."""
    a, e = np.ascontiguousarray(a, dtype=p.dtype), None
    if p.scaling is not None:  # one exponent per leaf; nothing finite is beyond the range
        a, e = _scaled_bits(a, p.storage)
    elif p.storage is not None:
        a = _storage_bits(a, p.storage, not loose)
    elif p.compute == "bf16x3" and not loose:
        _check_split_range(a)
    if p.leaf_rows and p.leaf_rows[t] is not None:  # [rows][the other axes]: the leaf at the distinct projections of its sparse indices
        axes, values = p.leaf_rows[t]
        a = np.ascontiguousarray(np.moveaxis(a, axes, range(len(axes)))[tuple(values.T)])
    return a, e


def _run(p: Plan, arrays, device, loose=frozenset()) -> ContractionResult:
    from . import _lib, parallel
    # (before the device is touched: a leaf beyond the range of the storage type or of the split is refused)
    leaves, leaf_exps = zip(*(_host_leaf(p, t, a, t in loose) for t, a in enumerate(arrays))) if arrays else ((), ())
    leaf_exps = np.array(leaf_exps, np.int32) if p.scaling is not None else None
    L = _lib.load()
    device = parallel.local_device() if device is None else int(device)
    h = _create(L, p, device)
    return _run_handle(L, h, p, list(leaves), leaf_exps)


def _create(L, p: Plan, device: int):
    """A new handle of the plan on that device."""
    from . import _lib
    d, keep = _describe(p, device)
    h = C.c_void_p()
    _lib.check(L.tnco_hip_contract_create(C.byref(d), C.byref(h)))
    del keep  # (the tables are copied by create)
    return h


def _describe(p: Plan, device: int):
    """(the tnco_hip_contract_desc of the plan, the arrays its pointers refer to: to be kept until create returns)."""
    from . import _lib
    keep = dict(leaf_numel=np.ascontiguousarray(p.leaf_numel), leaf_sl=np.ascontiguousarray(p.leaf_sl),
                perms=np.ascontiguousarray(p.perms), steps=np.ascontiguousarray(p.steps),
                slice_dims=np.array(p.slice_dims, np.int64).reshape(-1),
                block=np.array([p.slice_inds.index(x) for x in p.block_inds], np.int64).reshape(-1))
    d = _lib.ContractDesc()
    code = DTYPES[p.dtype] if p.storage is None else STORAGES[p.storage] + (p.dtype.kind == "c")
    d.dtype, d.device, d.max_axes = code, device, MAX_AXES
    d.n_leaves, d.leaf_numel, d.leaf_sl = len(p.leaf_numel), _ptr(keep["leaf_numel"]), _ptr(keep["leaf_sl"])
    d.n_perms, d.perms = len(p.perms), _ptr(keep["perms"])
    d.n_steps, d.steps = len(p.steps), _ptr(keep["steps"])
    d.arena_elems, d.out_numel = p.arena_elems, p.out_numel
    d.n_slice_dims, d.slice_dims = len(p.slice_dims), _ptr(keep["slice_dims"])
    d.n_block, d.block_slices = len(p.block_inds), _ptr(keep["block"])
    d.slice_start, d.slice_stop = p.slice_range
    if p.row_steps is not None:
        keep.update(row_steps=np.ascontiguousarray(p.row_steps), row_maps=np.ascontiguousarray(p.row_maps))
        d.row_steps, d.n_row_maps, d.row_maps = _ptr(keep["row_steps"]), p.row_maps.size, _ptr(keep["row_maps"])
    if p.scaling is not None:
        keep.update(stage_refs=np.ascontiguousarray(p.stage_refs, np.int64))
        d.scaling, d.stage_refs = 1, _ptr(keep["stage_refs"])
    return d, keep


def _run_handle(L, h, p: Plan, leaves, leaf_exps) -> ContractionResult:
    from . import _lib
    try:
        _set_modes(L, h, p)
        if p.scaling is not None:
            _lib.check(L.tnco_hip_contract_set_exponents(h, _ptr(leaf_exps)))
        staging = np.empty(p.out_numel, p.dtype)
        ptrs = (C.c_void_p * max(1, len(leaves)))(*[a.ctypes.data for a in leaves])
        _lib.check(L.tnco_hip_contract_run(h, ptrs, _ptr(staging)))
        fields = _read_counters(L, h, p)
    finally:
        L.tnco_hip_contract_destroy(h)
    return ContractionResult(p.inds, _host_layout(p, staging), **fields)


def _set_modes(L, h, p: Plan) -> None:
    """The set calls of the plan's keywords on a new handle (the leaves' exponents of scaling apart: they belong to the arrays)."""
    from . import _lib
    i64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64)  # noqa: E731 -- (an array: passed below)
    matrix, split = p.compute == "matrix", p.compute not in (None, "matrix")
    # (is it on, entry point, arguments), in an order the library takes.  Nothing hoisted, every period 1 or nothing
    # folded: the run of the plan without the keyword
    setters = (
        (matrix, L.tnco_hip_contract_set_matrix, (1,)),
        (split, L.tnco_hip_contract_set_compute, (COMPUTES.get(p.compute),)),
        (p.slice_batch is not None, L.tnco_hip_contract_set_slice_batch, (p.slice_batch,)),
        (p.path_kernel is not None, L.tnco_hip_contract_set_path_kernel, (p.path_kernel,)),
        (p.hoisted is not None and any(p.hoisted), L.tnco_hip_contract_set_hoist, (i64(p.step_hoist), i64(p.perm_hoist))),
        (p.reused is not None and any(p.reused), L.tnco_hip_contract_set_reuse, (i64(p.step_period), i64(p.perm_period))),
        (p.indirect, L.tnco_hip_contract_set_indirect, (i64(p.ind_steps), np.size(p.ind_maps), i64(p.ind_maps))),
        (p.accumulate is not None, L.tnco_hip_contract_set_accumulate, (1,)))
    for on, entry, args in setters:
        if on:
            _lib.check(entry(h, *(_ptr(a) if isinstance(a, np.ndarray) else a for a in args)))


def _read_counters(L, h, p: Plan) -> dict:
    """The fields of a ContractionResult that the handle knows after a run: every one but `inds` and `array`."""
    from . import _lib
    matrix, split = p.compute == "matrix", p.compute not in (None, "matrix")
    wide = p.accumulate is not None
    # (is it on, entry point, length, field of the result)
    counters = (
        (True, L.tnco_hip_contract_kernel_launches, len(KERNEL_PATHS), "kernel_launches"),
        (True, L.tnco_hip_contract_row_launches, len(ROW_KERNEL_PATHS), "row_kernel_launches"),
        (p.scaling is not None or wide, L.tnco_hip_contract_narrow_launches, 1, "narrow_launches"),
        (p.slice_batch is not None or wide, L.tnco_hip_contract_batch_launches, 1, "batch_launches"),
        (matrix, L.tnco_hip_contract_matrix_launches, 1, "matrix_launches"),
        (split, L.tnco_hip_contract_split_launches, 1, "split_launches"),
        (p.path_kernel is not None, L.tnco_hip_contract_path_launches, 2, "path_launches"),
        (p.indirect, L.tnco_hip_contract_indirect_launches, len(INDIRECT_KERNEL_PATHS), "indirect_launches"))
    exponents, counted = None, {}
    stats = np.zeros(4, np.int64)
    _lib.check(L.tnco_hip_contract_stats(h, _ptr(stats)))
    if p.scaling is not None:
        slots = np.zeros(len(p.leaf_numel) + len(p.steps), np.int32)
        _lib.check(L.tnco_hip_contract_exponents(h, _ptr(slots)))
        exponents = tuple(int(v) for v in slots)
    for on, entry, length, name in counters:
        if on:
            counts = np.zeros(length, np.int64)
            _lib.check(entry(h, _ptr(counts)))
            counted[name] = int(counts[0]) if length == 1 else tuple(int(v) for v in counts)
    return dict(macs=int(stats[0]), n_slices=p.slice_range[1] - p.slice_range[0], peak_device_bytes=int(stats[2]),
                launches=int(stats[1]), device_s=float(stats[3]) * 1e-9, scaling=p.scaling, exponents=exponents,
                slice_batch=p.slice_batch, compute=p.compute, path_kernel=p.path_kernel, hoisted=p.hoisted,
                reused=p.reused, indirect=p.indirect, **counted)


def _held_axes(p: Plan) -> tuple:
    """The axes of one output buffer of a plan without projections, [block axes][the others], by name."""
    return p.block_inds + tuple(x for x in p.inds if x not in set(p.slice_inds))


def _result_view(p: Plan, staging, sets=None) -> np.ndarray:
    """`staging`, one output buffer ([block axes][the others]) or `sets` of them back to back, in the result's own axis
    order, the set axis first: a view."""
    held, lead = _held_axes(p), () if sets is None else (sets,)
    array = staging.reshape(lead + tuple(p.shape[p.inds.index(x)] for x in held))
    return array.transpose(list(range(len(lead))) + [len(lead) + held.index(x) for x in p.inds])


def _result_axes(p: Plan, sets=None) -> tuple:
    """(dims, strides): where the elements of the output buffers, in the order `_result_view` reads them, lie in a
    C-contiguous result of shape (sets,) + p.shape."""
    lead = () if sets is None else (sets,)
    at = [p.inds.index(x) for x in _held_axes(p)]
    steps = _c_strides(lead + tuple(p.shape))
    return merge_axes(list(lead) + [p.shape[q] for q in at], list(steps[:len(lead)]) + [steps[len(lead) + q] for q in at])


def _host_layout(p: Plan, staging) -> np.ndarray:
    """The output buffer, [block axes][the others] (with projections: [block axes][rows of the final tensor][the
    others]), in the result's own axis order; the distinct rows expanded to the P projections with one take."""
    if p.out_rows is None:
        return _result_view(p, staging).copy(order="C")  # (0-d stays 0-d)
    n_rows, row_of_proj = p.out_rows
    named = p.inds[1:]  # (position 0 is the projection axis)
    rest = tuple(x for x in named if x not in set(p.slice_inds))
    held = p.block_inds + (None,) + rest
    array = staging.reshape(tuple(n_rows if x is None else p.shape[1 + named.index(x)] for x in held))
    array = array.transpose([held.index(None)] + [held.index(x) for x in named])
    return array.take(row_of_proj, axis=0)


def contract_results(tn0, arrays, tn, result, *, device=None, projs=None, sparse_inds=None,
                     storage=None, scaling=None, slice_batch=None, compute=None, path_kernel=None,
                     hoist=None, indirect=None, reuse=None, slice_order=None, accumulate=None) -> ContractionResult:
    """Run a result of `Optimizer.optimize` over the arrays of the network as given.

    tn0: the network before pre-fusing (`load_tn(obj, fuse=None)`); arrays: in tn0.tensors order, or {name: array}
    by the tensors' `name` tag; tn, result: what `optimize` returned.  The fuse stage (tn.tags['fuse_path']) runs
    unsliced, its multiply-adds go to `fuse_macs`; then `result.path` with `result.slices`, every connected component
    of a finite-width result sliced by its own set (`disconnected_slices`).

    A network with sparse indices needs `projs`, [P, number of sparse indices]: the result is then taken at those
    assignments of the sparse indices (axes ("proj",) + the others).  The columns are the sparse indices in
    `sorted(tn.sparse_inds, key=str)` order, or in the order of `sparse_inds` when that is given.

    storage: "float16" / "bfloat16" runs `result.path` in storage mode (module docstring); the fuse stage, unsliced and
    small, stays in the arrays' own precision.  scaling: "tensor" adds per-tensor scaling to it; the results of the fuse
    stage, and the components' results that enter a later call, are then scaled as leaves (`exponents`: those of the
    last call made).  slice_batch: that many slice assignments per launch in every sliced call (module docstring);
    `batch_launches` is the sum over the calls, `slice_batch` of the result the largest effective value of a component.
    compute: "bf16x3" / "matrix" runs the tiled-class steps of `result.path` on the matrix cores (module docstring); the
    fuse stage stays on the plain kernels; `split_launches` / `matrix_launches` is the sum over the calls.
    path_kernel: that many slice assignments per launch of the path kernel in every call over `result.path` (module
    docstring); the fuse stage stays as it is;
    `path_launches` is the sum over the calls, `path_kernel` of the result the largest effective value of a component.
    hoist: True runs the slice-independent steps and permutes of every call over `result.path` once per call (module
    docstring); the fuse stage, unsliced, stays as it is; `hoisted` is the sum over the calls.
    indirect: True reads the step operands of every call over `result.path` that would be permuted per assignment in
    place (module docstring); the fuse stage stays as it is; `indirect` and `indirect_launches` are sums over the calls.
    reuse: True runs every step and permute of every call over `result.path` only at the assignments that change the slices
    below it (module docstring); the fuse stage, unsliced, stays as it is; `reused` is the sum over the calls.
    slice_order: the order of the sliced indices, slowest first (module docstring): "reuse" for every sliced call, or a
    sequence that names every index of `result.slices` once (of several components: each takes its own, in that order).
    accumulate: "float64" sums the slice assignments of every call over `result.path` in float64 (module docstring); the
    fuse stage, unsliced, runs without it; `batch_launches`, `path_launches` and `narrow_launches` count its launches."""
    options = _Options(storage=storage, scaling=scaling, slice_batch=slice_batch, compute=compute, path_kernel=path_kernel,
                       hoist=hoist, indirect=indirect, reuse=reuse, slice_order=slice_order, accumulate=accumulate)
    options.check(np.float32, projs)  # (before the network is looked at; the arrays' dtype: below)
    if (tn0.sparse_inds or tn.sparse_inds) and projs is None:
        raise NotImplementedError("sparse indices (n_projs) have an array meaning only at given projections: "
                                  "pass projs=, an integer array [P, number of sparse indices].")
    if projs is not None:
        if sparse_inds is None:
            sparse_inds = sorted(tn.sparse_inds, key=str)
        if set(sparse_inds) != set(tn.sparse_inds) or set(tn0.sparse_inds) != set(tn.sparse_inds):
            raise ValueError("'sparse_inds' are not the sparse indices of the network.")
        if tn.tags.get("fuse_path") or len([q for q in getattr(result, "disconnected_paths", ()) if q]) > 1:
            raise NotImplementedError("projections need one connected network that was not pre-fused.")
    elif sparse_inds is not None:
        raise ValueError("'sparse_inds' need 'projs'.")
    if isinstance(arrays, dict):
        try:
            arrays = [arrays[t.tags["name"]] for t in tn0.tensors]
        except KeyError as e:
            raise ValueError("'ts_inds' is not consistent with 'arrays'.") from e
    arrays = [np.asarray(a) for a in arrays]
    options.check(_compute_dtype(arrays))  # (what compute and storage say of the dtype; the rest passed above)
    fuse_macs = 0
    if tn.tags.get("fuse_path"):
        fused = contract(tn.tags["fuse_path"], tn0.ts_inds, arrays, tn0.output_inds, device=device)
        inds, arrays = (fused.inds, fused.array) if isinstance(fused.array, list) else ([fused.inds], [fused.array])
        fuse_macs = fused.macs
        if [tuple(x) for x in inds] != [tuple(x) for x in tn.ts_inds]:
            raise ValueError("the fuse path does not reproduce the network that was optimized.")
    elif [tuple(x) for x in tn0.ts_inds] != [tuple(x) for x in tn.ts_inds]:
        raise ValueError("the network that was optimized is not the one given.")
    comp_paths = [list(q) for q in getattr(result, "disconnected_paths", ()) if q]
    if len(comp_paths) <= 1:  # one component to contract: the path with its slices, in one call
        r = contract(result.path, tn.ts_inds, arrays, tn.output_inds, slices=getattr(result, "slices", ()),
                     device=device, sparse_inds=sparse_inds or (), projs=projs, **options.keywords())
        return replace(r, fuse_macs=fuse_macs)
    # several: each component with its own slices, then the remaining steps of the merged path over their results
    ts, n = [tuple(x) for x in tn.ts_inds], len(tn.ts_inds)
    done, results = set(), []
    named = slice_order is not None and not isinstance(slice_order, str)
    if named:  # every index of every component's set, once
        _named_order(slice_order, tuple(dict.fromkeys(x for cut in result.disconnected_slices for x in cut)))
    n_comp_steps = 0
    for q, cut in zip(result.disconnected_paths, result.disconnected_slices):
        if not q:
            continue
        n_comp_steps += len(q)
        (leaves, sub), = [(lv, s) for lv, s in _split(_check_path(q, n), n) if s]
        r = contract(sub, [ts[t] for t in leaves], [arrays[t] for t in leaves], _sub_output(ts, leaves, tn.output_inds),
                     slices=cut, device=device,
                     **options.keywords(slice_order=[x for x in slice_order if x in set(cut)] if named else slice_order))
        done |= set(leaves)
        results.append(r)
    state_inds = [ts[t] for t in range(n) if t not in done] + [tuple(r.inds) for r in results]
    state_arrays = [arrays[t] for t in range(n) if t not in done] + [r.array for r in results]
    expect = tnmod.contract(_check_path(result.path[:n_comp_steps], n), ts, tn.output_inds)[0]
    if [tuple(x) for x in expect] != state_inds:
        raise ValueError("'path' is not valid.")
    tail = result.path[n_comp_steps:]
    calls = list(results)
    if tail:  # (unsliced: it adds no slice assignments; its slice_batch and path_kernel are 1)
        r = contract(tail, state_inds, state_arrays, frozenset(tn.output_inds) & {x for xs in state_inds for x in xs},
                     device=device, **options.keywords(slice_order=None),
                     _intermediates=range(len(state_arrays) - len(results), len(state_arrays)))
        calls.append(r)
        inds, array = r.inds, r.array
    else:
        inds, array = (state_inds[0], state_arrays[0]) if len(state_inds) == 1 else (state_inds, state_arrays)
    return _sum_results(calls, inds=inds, array=array, n_slices=sum(r.n_slices for r in results),
                        exponents=calls[-1].exponents, fuse_macs=fuse_macs)


def merge_axes(shape, strides) -> tuple:
    """(dims, strides) of the same elements in the same order with as few axes as it takes: axes of dimension 1 dropped,
    neighbours merged where the outer stride is the inner stride times the inner dimension (so two expanded neighbours,
    both of stride 0, merge too).  Strides in elements.  A 0-d or one-element array gives ((), ()).  ValueError for a
    negative stride, NotImplementedError when more than MAX_AXES axes are left."""
    dims, steps = [], []
    for d, s in zip(shape, strides):
        d, s = int(d), int(s)
        if d == 1:
            continue
        if s < 0:
            raise ValueError("a tensor with a negative stride is not supported.")
        if dims and steps[-1] == s * d:
            dims[-1], steps[-1] = dims[-1] * d, s
        else:
            dims.append(d)
            steps.append(s)
    if len(dims) > MAX_AXES:
        raise NotImplementedError(f"a tensor with more than {MAX_AXES} axes that do not merge is not supported.")
    return tuple(dims), tuple(steps)


def check_extent(offset: int, dims, strides, storage_elems: int) -> None:
    """ValueError unless every element that `dims` and `strides` (>= 0, in elements) reach from `offset` lies inside a
    storage of `storage_elems` elements."""
    last = int(offset) + sum((int(d) - 1) * int(s) for d, s in zip(dims, strides))
    if offset < 0 or last >= storage_elems:
        raise ValueError(f"a tensor reaches element {last} of a storage of {storage_elems} elements.")


def _c_strides(shape) -> tuple:
    out, n = [], 1
    for d in reversed(shape):
        out.append(n)
        n *= int(d)
    return tuple(reversed(out))


def _is_tensor(a) -> bool:
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(a, torch.Tensor)


def _torch_dtypes() -> dict:
    import torch
    return {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64),
            torch.complex64: np.dtype(np.complex64), torch.complex128: np.dtype(np.complex128)}


def _check_plain(a, what: str) -> None:
    """ValueError unless the numbers of the tensor `a` are those its memory holds, at shape, strides and storage offset:
    that is all a kernel is told of it.  A lazily conjugated or negated tensor (`t.conj()`, torch's conjugate and negative
    bits) shares memory and strides with the tensor it came from, and a layout that is not strided has no strides."""
    import torch
    if a.layout != torch.strided:
        raise ValueError(f"{what} has the layout {a.layout}: only strided tensors are supported.")
    if a.is_conj():
        raise ValueError(f"{what} is lazily conjugated (is_conj()): pass tensor.resolve_conj().")
    if a.is_neg():
        raise ValueError(f"{what} is lazily negated (is_neg()): pass tensor.resolve_neg().")


# the exact widenings of csrc/contract_io.h besides the identity: source -> what it may become
_WIDENS = {np.dtype(np.float32): (np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)),
           np.dtype(np.float64): (np.dtype(np.complex128),), np.dtype(np.complex64): (np.dtype(np.complex128),),
           np.dtype(np.complex128): ()}
_SPLIT_LIMIT = float(np.array(0x7F7F8000, np.uint32).view(np.float32))  # 2^128 - 2^119: its bfloat16 is infinite


class Contractor:
    """One planned contraction that is run many times: the plan is made once, the device handle lives until close(), leaves
    may stay on the device between runs (`bind`), and arrays may be numpy arrays or torch tensors on `device`.

        with Contractor(path, ts_inds, shapes, output_inds, dtype=np.complex64, slices=cut, path_kernel=64) as c:
            c.bind({0: a0, 3: t3})        # loaded now; they stay
            r = c.run({1: a1, 2: a2})     # the other leaves, for this run
            r = c.run(out=t)              # every leaf bound or given before: into the caller's tensor

    The constructor takes what `plan` takes (`shapes`, not arrays) and refuses what it refuses; `plan` is that Plan.  It does
    not touch the device: the handle is created at the first `bind` or `run`.  `run` returns the ContractionResult that
    `contract` returns for the same path, arrays and keywords, `array` byte for byte (`device_s` is measured per run).
    A numpy array must cast safely to the plan's dtype; a torch tensor must be on `device`, of any strides >= 0, of the
    plan's dtype or one that widens to it exactly (float32 -> float64, complex64, complex128; float64, complex64 ->
    complex128).  The arrays of one run are all numpy or all torch (bound leaves may be of either kind); `array` of the result
    is of the kind of `out` when
    that is given, else of the call's arrays, numpy without any.  `out`: C-contiguous, of the result's shape and dtype.
    Torch operands and a torch `out` are not supported with `storage`, `scaling` or `projs`, which prepare leaves and
    result on the host; numpy arrays are.  A torch tensor's memory is read and written by kernels only, after
    torch.cuda.synchronize(device); what a tensor's strides reach is checked against its storage before its pointer is used,
    and a tensor that is lazily conjugated or negated (`t.conj()`) or not strided is refused (ValueError: pass
    `t.resolve_conj()`), since the kernels see its memory, not those bits."""

    def __init__(self, path, ts_inds, shapes, output_inds=None, *, dtype=np.float64, slices=(), slice_range=None, device=None,
                 sparse_inds=(), projs=None, storage=None, scaling=None, slice_batch=None, compute=None, path_kernel=None,
                 hoist=None, indirect=None, reuse=None, slice_order=None, accumulate=None):
        from . import parallel
        shapes = [tuple(int(d) for d in s) for s in shapes]
        self.plan = plan(path, ts_inds, shapes, output_inds, slices=slices, slice_range=slice_range, dtype=dtype,
                         sparse_inds=sparse_inds, projs=projs, storage=storage, scaling=scaling, slice_batch=slice_batch,
                         compute=compute, path_kernel=path_kernel, hoist=hoist, indirect=indirect, reuse=reuse,
                         slice_order=slice_order, accumulate=accumulate)
        self.device = parallel.local_device() if device is None else int(device)
        self._shapes = shapes
        self._host_only = next((name for name, v in (("storage", storage), ("scaling", scaling), ("projs", projs))
                                if v is not None), None)
        self._lib, self._h, self._closed = None, None, False
        self._bound = set()
        self._exps = np.zeros(len(shapes), np.int32)  # scaling: the exponents of the leaves the handle holds
        # run_many: what its calls made the handle reserve (sets per stacked leaf, members, outputs), the leaves last stacked
        self._many = dict(stacks={}, members=0, out=0, last=(), walked=False)
        self._versions = set()  # bind_versions: the leaves whose two versions the handle holds
        self._walked = None  # run_walkers: the Walkers of the handle's last run, if that was one

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def close(self) -> None:
        """Destroys the handle; the object refuses every use afterwards.  Closing twice is fine."""
        if self._h is not None:
            self._lib.tnco_hip_contract_destroy(self._h)
        self._h, self._closed = None, True

    @property
    def io_launches(self) -> tuple:
        """(launches of the ingest kernel, of the emit kernel) since the handle was created."""
        self._check_open()
        if self._h is None:
            return (0, 0)
        from . import _lib
        counts = np.zeros(2, np.int64)
        _lib.check(self._lib.tnco_hip_contract_io_launches(self._h, _ptr(counts)))
        return (int(counts[0]), int(counts[1]))

    def bind(self, leaves) -> None:
        """Loads the leaves {leaf number: array} now; they stay until bound again or until close()."""
        self._check_open()
        given, _ = self._check_arrays(leaves, one_kind=False)
        # numpy arrays and tensors may come together here; every check of both kinds before anything is loaded
        kinds = [(kind, self._prepare({t: a for t, a in given.items() if _is_tensor(a) == kind}, kind)) for kind in (False, True)]
        for kind, ready in kinds:
            self._bound -= set(ready)  # (a leaf is bound once it is loaded, not while a failed load may have left it half written)
            self._load(ready, kind)
            self._bound |= set(ready)

    def run(self, arrays=None, *, out=None) -> ContractionResult:
        """Runs the plan over the bound leaves and `arrays`: a sequence with every leaf, or {leaf number: array} with the
        leaves that are not bound.  The given leaves are for this run: the next run needs them again.  A bound leaf may be
        given too: the run takes the given one, and the leaf is bound no longer."""
        from . import _lib
        self._check_open()
        p = self.plan
        given, torch_in = self._check_arrays({} if arrays is None else arrays)
        self._walked = None
        torch_out = _is_tensor(out)
        if torch_out and self._host_only:
            raise NotImplementedError(f"a torch tensor as 'out' is not supported with '{self._host_only}'.")
        ready = self._prepare(given, torch_in)
        if out is not None:
            self._check_out(out, torch_out)
        missing = [t for t in range(len(self._shapes)) if t not in self._bound and t not in ready]
        if missing:
            raise ValueError(f"leaf {missing[0]} is neither bound nor given.")
        to_device = torch_out or (out is None and torch_in)
        L, h = self._handle()
        # before anything is loaded: a bound leaf that a run is given another array for is no longer the one the handle
        # holds, also when the run fails half way
        self._bound -= set(ready)
        if not torch_in and not to_device and len(ready) == len(self._shapes):  # as contract(): one call, one wait
            self._note_exponents(ready)
            staging = np.empty(p.out_numel, p.dtype)
            ptrs = (C.c_void_p * max(1, len(ready)))(*[ready[t][0].ctypes.data for t in range(len(ready))])
            _lib.check(L.tnco_hip_contract_run(h, ptrs, _ptr(staging)))
        else:
            self._load(ready, torch_in)
            if to_device:
                import torch
                if out is None:
                    kind = next(k for k, v in _torch_dtypes().items() if v == p.dtype)
                    out = torch.empty(p.shape, dtype=kind, device=f"cuda:{self.device}")
                dims, strides = _result_axes(p)
                torch.cuda.synchronize(self.device)
                _lib.check(L.tnco_hip_contract_run_loaded(h, C.c_void_p(out.data_ptr()), 1, len(dims), _i64(dims), _i64(strides)))
            else:
                staging = np.empty(p.out_numel, p.dtype)
                _lib.check(L.tnco_hip_contract_run_loaded(h, _ptr(staging), 0, 0, None, None))
        fields = _read_counters(L, h, p)
        if to_device:
            return ContractionResult(p.inds, out, **fields)
        array = _host_layout(p, staging)
        if out is not None:
            np.copyto(out, array)
            array = out
        return ContractionResult(p.inds, array, **fields)

    def run_many(self, stacks, *, group=None, out=None) -> ManyResult:
        """Runs the plan over R leaf sets in one call: `stacks` is {leaf number: array}, each array the R versions of that
        leaf along one leading axis, (R,) + the leaf's shape; every other leaf must be bound and is shared by the sets.
        `array[i]` of the result is byte for byte `run({t: stacks[t][i]}).array` (module docstring, Leaf sets).  The
        arrays follow the rules of `run`; a set axis of stride 0 gives R equal sets.  A bound leaf may be given as a stack:
        the call reads the stack, and the leaf stays bound and as it was.  `group`: members (set, assignment) per launch,
        None or 1 to MAX_PATH_KERNEL (None: MAX_PATH_KERNEL); `out`: C-contiguous, of shape (R,) + plan.shape and of the
        plan's dtype.  It needs `path_kernel=` and a plan with steps, and is not supported with `accumulate=`."""
        from . import _lib
        self._check_open()
        p = self.plan
        group = self._check_many(group)
        if not isinstance(stacks, dict) or not stacks:
            raise ValueError("'stacks' must be a dict {leaf number: array} with at least one leaf.")
        given, torch_in = self._check_arrays(stacks)
        self._walked = None
        sets, ready = self._prepare_stacks(given, torch_in)
        missing = [t for t in range(len(self._shapes)) if t not in self._bound and t not in ready]
        if missing:
            raise ValueError(f"leaf {missing[0]} is neither bound nor given.")
        torch_out = _is_tensor(out)
        if out is not None:
            self._check_out(out, torch_out, (sets,) + tuple(p.shape))
        to_device = torch_out or (out is None and torch_in)
        L, h = self._handle()
        if torch_in or to_device:
            import torch
            torch.cuda.synchronize(self.device)
        for t, (a, code, dims, strides) in ready.items():
            where = 1 if torch_in else 0
            src = C.c_void_p(a.data_ptr()) if torch_in else _ptr(a)
            _lib.check(L.tnco_hip_contract_load_leaf_sets(h, t, sets, src, where, code, len(dims), _i64(dims), _i64(strides)))
        if to_device:
            if out is None:
                kind = next(k for k, v in _torch_dtypes().items() if v == p.dtype)
                out = torch.empty((sets,) + tuple(p.shape), dtype=kind, device=f"cuda:{self.device}")
            dims, strides = _result_axes(p, sets)
            _lib.check(L.tnco_hip_contract_run_sets(h, sets, group, C.c_void_p(out.data_ptr()), 1, len(dims), _i64(dims), _i64(strides)))
            array = out
        else:
            staging = np.empty((sets, p.out_numel), p.dtype)
            _lib.check(L.tnco_hip_contract_run_sets(h, sets, group, _ptr(staging), 0, 0, None, None))
            array = _result_view(p, staging, sets).copy(order="C")
            if out is not None:
                np.copyto(out, array)
                array = out
        self._grow(sets, group, ready)
        return self._many_result(sets, group, array)

    def bind_versions(self, versions) -> None:
        """Loads the two versions of the leaves {leaf number: array of shape (2,) + the leaf's shape} now; they stay until
        bound again or until close(), apart from what `bind` holds of the leaf.  `run_walkers` reads version b of such a
        leaf for a walker whose bit of the leaf's qubit is b.  Arrays as `bind` takes them, numpy or torch.  It needs
        `path_kernel=` and a plan with steps, and is not supported with `accumulate=`."""
        from . import _lib
        self._check_open()
        self._check_many(None, "bind_versions")
        if not isinstance(versions, dict) or not versions:
            raise ValueError("'versions' must be a dict {leaf number: array} with at least one leaf.")
        given, _ = self._check_arrays(versions, one_kind=False)
        for t in sorted(given):
            shape = tuple(given[t].shape) if _is_tensor(given[t]) else np.shape(given[t])
            if shape != (2,) + self._shapes[t]:
                raise ValueError(f"the versions of leaf {t} have the shape {shape}, not (2,) + the leaf's {self._shapes[t]}.")
        kinds = [(kind, self._prepare_stacks({t: a for t, a in given.items() if _is_tensor(a) == kind}, kind)[1])
                 for kind in (False, True)]
        for kind, ready in kinds:
            if not ready:
                continue
            L, h = self._handle()
            if kind:
                import torch
                torch.cuda.synchronize(self.device)
            for t, (a, code, dims, strides) in ready.items():
                self._versions.discard(t)
                src = C.c_void_p(a.data_ptr()) if kind else _ptr(a)
                _lib.check(L.tnco_hip_contract_load_leaf_versions(h, t, 2, src, int(kind), code, len(dims), _i64(dims), _i64(strides)))
                self._versions.add(t)

    def _check_walk(self, walkers) -> None:
        """What run_walkers and choose refuse of `walkers`."""
        if not isinstance(walkers, Walkers):
            raise TypeError(f"'walkers' must be a Walkers object, not {type(walkers).__name__}.")
        walkers._check_open()
        if walkers.device != self.device:
            raise ValueError(f"the walkers are on device {walkers.device}, the Contractor on device {self.device}.")

    def run_walkers(self, walkers, leaf_qubit, *, group=None) -> ManyResult:
        """`run_many` over the walkers of `walkers` as sets: `leaf_qubit` is {leaf number: qubit}; walker i reads such a
        leaf at version walkers.bits[i, qubit] of the two that `bind_versions` loaded, and every other leaf where it is
        bound.  The outputs stay on the device for `choose` (or `walker_outputs`): `array` of the result is None.  With an
        empty `leaf_qubit` no output depends on the walker: one set is run for all of them (`sets` of the result is 1).
        `group` as in `run_many`.  Refuses what `run_many` refuses of the Contractor."""
        from . import _lib
        self._check_open()
        n = len(self._shapes)
        group = self._check_many(group, "run_walkers")
        self._check_walk(walkers)
        if not isinstance(leaf_qubit, dict):
            raise ValueError("'leaf_qubit' must be a dict {leaf number: qubit}.")
        table = np.full(max(n, 1), -1, np.int64)
        for t, q in leaf_qubit.items():
            if not _is_index(t, 0, n):
                raise ValueError(f"{t!r} is not a leaf of the plan (0 to {n - 1}).")
            if not _is_index(q, 0, walkers.n_qubits):
                raise ValueError(f"{q!r} is not a qubit of the walkers (0 to {walkers.n_qubits - 1}).")
            if int(t) not in self._versions:
                raise ValueError(f"leaf {int(t)} has no versions: call bind_versions first.")
            table[int(t)] = int(q)
        missing = [t for t in range(n) if table[t] < 0 and t not in self._bound]
        if missing:
            raise ValueError(f"leaf {missing[0]} is neither bound nor indexed by a qubit.")
        L, h = self._handle()
        self._walked = None
        _lib.check(L.tnco_hip_contract_run_walkers(h, walkers._handle(), _ptr(table), group))
        self._walked = walkers
        sets = walkers.n_walkers if leaf_qubit else 1  # (no leaf indexed: one output serves every walker, one set is run)
        self._grow(sets, group)
        self._many["walked"], self._walked_sets = True, sets
        return self._many_result(sets, group, None)

    def walker_outputs(self, walkers) -> np.ndarray:
        """The outputs that the last `run_walkers` over `walkers` left on the device, as `run_many` lays its array out:
        (walkers,) + plan.shape.  A copy to the host: for tests and for callers that do not `choose` on the device."""
        from . import _lib
        self._check_open()
        self._check_walk(walkers)
        if self._walked is not walkers:
            raise ValueError("the last run of the Contractor was not a 'run_walkers' over these walkers.")
        p, sets = self.plan, self._walked_sets
        L, h = self._handle()
        staging = np.empty((sets, p.out_numel), p.dtype)
        _lib.check(L.tnco_hip_contract_walkers_output(h, walkers._handle(), _ptr(staging)))
        array = _result_view(p, staging, sets)
        return np.broadcast_to(array, (walkers.n_walkers,) + array.shape[1:]).copy(order="C")

    def choose(self, walkers, qubit, step) -> None:
        """Draws the new bit of `qubit` for every walker from the two amplitudes that the last `run_walkers` over
        `walkers` left (module docstring, Walkers): the plan's output must hold exactly 2 elements.  `step` (0 to
        2^32 - 1) numbers the draw: with the walkers' seed and the walker's number it fixes the uniform."""
        from . import _lib
        self._check_open()
        self._check_many(None, "choose")
        self._check_walk(walkers)
        if self.plan.out_numel != 2:
            raise ValueError(f"the output of the plan holds {self.plan.out_numel} elements, not the 2 amplitudes of a choice.")
        if not _is_index(qubit, 0, walkers.n_qubits):
            raise ValueError(f"{qubit!r} is not a qubit of the walkers (0 to {walkers.n_qubits - 1}).")
        if not _is_index(step, 0, 2 ** 32):
            raise ValueError("'step' must be an integer from 0 to 2^32 - 1.")
        if self._walked is not walkers:
            raise ValueError("the last run of the Contractor was not a 'run_walkers' over these walkers.")
        L, h = self._handle()
        _lib.check(L.tnco_hip_walkers_choose(walkers._handle(), h, int(qubit), int(step)))

    def choose_joint(self, walkers, qubits, step, inds=None) -> None:
        """Draws the new bits of the 1 to 6 distinct `qubits` jointly for every walker, from the 2^k amplitudes that the
        last `run_walkers` over `walkers` left (csrc/contract_walk.h, ct_walk_choose_joint_kernel).  `inds` is the open
        index of each qubit, in the qubits' order (None: `plan.inds` in order); it names every index of the plan's
        output once, and each has dimension 2.  Outcome v, the first qubit its most significant bit, has the amplitude
        out[inds = the bits of v]: the strides come from the layout of the output on the device, so a draw does not
        depend on the path.  With p_v = |a_v|^2 and tail(v) = p_v + ... + p_{N-1} summed from the top in float64, the
        outcome is the largest v >= 1 with u tail(0) < tail(v), or 0; u is `choose`'s, one draw per call.  A walker
        whose tail(0) is 0 or not finite gets 0 in all k bits and its dead flag.  At k = 1 the bytes are `choose`'s."""
        from . import _lib
        self._check_open()
        self._check_many(None, "choose_joint")
        self._check_walk(walkers)
        p = self.plan
        qubits = tuple(qubits)
        if not 1 <= len(qubits) <= MAX_CHOOSE_QUBITS:
            raise ValueError(f"'qubits' must name 1 to {MAX_CHOOSE_QUBITS} qubits.")
        for q in qubits:
            if not _is_index(q, 0, walkers.n_qubits):
                raise ValueError(f"{q!r} is not a qubit of the walkers (0 to {walkers.n_qubits - 1}).")
        if len(set(qubits)) != len(qubits):
            raise ValueError("'qubits' names a qubit twice.")
        if p.block_inds:  # (projections, the other output that is not one block, are refused with path_kernel)
            raise NotImplementedError("'choose_joint' needs an output whose axes are all held at once: this plan's is a block "
                                      "that a sliced index selects.")
        if any(d != 2 for d in p.shape):
            raise ValueError(f"every axis of the output must have dimension 2, not {tuple(p.shape)}.")
        if p.out_numel != 1 << len(qubits):
            raise ValueError(f"the output of the plan holds {p.out_numel} elements, not the {1 << len(qubits)} amplitudes of a "
                             f"choice of {len(qubits)} qubits.")
        inds = tuple(p.inds) if inds is None else tuple(inds)
        if len(inds) != len(p.inds) or set(inds) != set(p.inds):
            raise ValueError(f"'inds' must name every index of the output {tuple(p.inds)} once, one per qubit.")
        if not _is_index(step, 0, 2 ** 32):
            raise ValueError("'step' must be an integer from 0 to 2^32 - 1.")
        if self._walked is not walkers:
            raise ValueError("the last run of the Contractor was not a 'run_walkers' over these walkers.")
        held = _held_axes(p)  # the device layout, every dimension 2: the last axis has stride 1
        strides = np.array([1 << (len(held) - 1 - held.index(x)) for x in inds], np.int64)
        qs = np.array(qubits, np.int64)
        L, h = self._handle()
        _lib.check(L.tnco_hip_walkers_choose_joint(walkers._handle(), h, len(qubits), _ptr(qs), _ptr(strides), int(step)))

    def many_bytes(self, n_sets, group=None, leaves=None) -> int:
        """The device bytes the handle holds after `run_many` of `n_sets` sets with that `group` and stacks of the leaves
        `leaves` (None: those of the last `run_many`, none before the first), `peak_device_bytes` of its result: what the
        handle holds without the call; a stack of n_sets versions per stacked leaf; the arenas and staging blocks that
        min(group, n_sets x assignments) members need beyond `Plan.path_kernel`; n_sets outputs; a pointer and a stride
        per leaf.  What an earlier call grew stays until close(): each term is the largest so far.  The walkers' terms
        are part of it: two versions per leaf of `bind_versions`, and three words per leaf once `run_walkers` has run."""
        self._check_open()
        p = self.plan
        group = self._check_many(group)
        if not _is_index(n_sets, 1, math.inf):
            raise ValueError("'n_sets' must be a positive integer.")
        n = len(self._shapes)
        leaves = self._many["last"] if leaves is None else tuple(leaves)
        for t in leaves:
            if not _is_index(t, 0, n):
                raise ValueError(f"{t!r} is not a leaf of the plan (0 to {n - 1}).")
        item, A = p.dtype.itemsize, p.slice_range[1] - p.slice_range[0]
        block = p.out_numel // math.prod(p.shape[p.inds.index(x)] for x in p.block_inds)
        # what the handle of this plan holds (csrc/contract.hip: create and tnco_hip_contract_set_path_kernel): the leaves,
        # each padded to 64 elements, path_kernel arenas and staging blocks, the output, the tables and a pointer per leaf
        held = item * sum(-(-int(v) // ALIGN) * ALIGN for v in p.leaf_numel) + item * max(p.arena_elems, 1) + item * p.out_numel
        held += 8 * (p.perms.size + p.leaf_sl.size + 2 * len(p.slice_dims)) + 8 * max(n, 1)
        held += item * ((p.path_kernel - 1) * p.arena_elems + p.path_kernel * block) + 8 * (p.steps.size + GR_W * (len(p.steps) + 1) + A)
        caps = self._many
        stacked = dict(caps["stacks"])
        for t in leaves:
            stacked[int(t)] = max(stacked.get(int(t), 0), int(n_sets))
        stacks = item * sum(r * int(p.leaf_numel[t]) for t, r in stacked.items())
        members = max(caps["members"], min(group, int(n_sets) * A))
        grown = item * max(members - p.path_kernel, 0) * (p.arena_elems + block)
        outputs = item * max(caps["out"], int(n_sets)) * p.out_numel
        # (walkers: two versions per leaf of bind_versions; three words per leaf once run_walkers has run)
        walked = item * 2 * sum(int(p.leaf_numel[t]) for t in self._versions) + (8 * WALK_W * n if caps["walked"] else 0)
        return held + stacks + grown + outputs + 8 * SET_W * n + walked

    # -- the checks; none of them touches the device through this library

    def _check_many(self, group, name="run_many") -> int:
        """What run_many (or its kin `name`) refuses of the Contractor and of `group`; the group as a number."""
        p = self.plan
        if p.path_kernel is None:
            raise NotImplementedError(f"'{name}' needs a Contractor with 'path_kernel'.")
        if p.accumulate is not None:
            raise NotImplementedError(f"'accumulate' is not supported with '{name}'.")
        if not len(p.steps):
            raise NotImplementedError(f"'{name}' needs a plan with steps.")
        if group is None:
            return MAX_PATH_KERNEL
        if not _is_index(group, 1, MAX_PATH_KERNEL + 1):
            raise ValueError(f"'group' must be None or an integer from 1 to {MAX_PATH_KERNEL}.")
        return int(group)

    def _prepare_stacks(self, given, torch_in):
        """(R, {leaf number: (array or tensor, dtype code, dims, strides)} in leaf order): what load_leaf_sets takes."""
        p, sets = self.plan, None
        for t in sorted(given):
            a = given[t] if torch_in else np.asarray(given[t])
            given[t] = a
            if len(a.shape) < 1:
                raise ValueError(f"the stack of leaf {t} has no set axis.")
            if tuple(a.shape[1:]) != self._shapes[t]:
                raise ValueError(f"the stack of leaf {t} has the shape {tuple(a.shape[1:])} after its set axis, not the leaf's "
                                 f"{self._shapes[t]}.")
            if a.shape[0] < 1:
                raise ValueError(f"the stack of leaf {t} holds no set.")
            sets = int(a.shape[0]) if sets is None else sets
            if a.shape[0] != sets:
                raise ValueError(f"the stack of leaf {t} holds {a.shape[0]} sets, the first stack {sets}.")
        ready = {}
        for t in sorted(given):
            a = given[t]
            if not torch_in:
                if not np.can_cast(a.dtype, p.dtype, "safe"):
                    raise TypeError(f"an array of dtype {a.dtype} does not cast safely to {p.dtype}.")
                a = np.ascontiguousarray(a, dtype=p.dtype)
                ready[t] = (a, DTYPES[p.dtype], (a.size,), ())
                continue
            src = _torch_dtypes().get(a.dtype)
            if src is None or not (src == p.dtype or p.dtype in _WIDENS[src]):
                raise TypeError(f"a tensor of dtype {a.dtype} does not widen exactly to {p.dtype}.")
            _check_plain(a, "a tensor")
            if a.device.type != "cuda" or a.device.index != self.device:
                raise ValueError(f"a tensor is on {a.device}, not on cuda:{self.device}.")
            dims, strides = merge_axes(a.shape, a.stride())
            check_extent(a.storage_offset(), dims, strides, a.untyped_storage().nbytes() // a.element_size())
            if not dims:  # (one element in all: an axis for the library to count)
                dims, strides = (1,), (1,)
            ready[t] = (a, DTYPES[src], dims, strides)
        return sets, ready

    def _grow(self, sets, group, ready=None) -> None:
        """Notes what a run_many (`ready`: its stacks) or a run_walkers (None: the leaves last stacked stay those of the
        last run_many) made the handle reserve (many_bytes)."""
        caps, p = self._many, self.plan
        caps["members"] = max(caps["members"], min(group, sets * (p.slice_range[1] - p.slice_range[0])))
        caps["out"] = max(caps["out"], sets)
        if ready is not None:
            for t in ready:
                caps["stacks"][t] = max(caps["stacks"].get(t, 0), sets)
            caps["last"] = tuple(ready)

    def _many_result(self, sets, group, array) -> ManyResult:
        """The ManyResult of the run over `sets` sets that the handle has just made."""
        from . import _lib
        p, (L, h) = self.plan, self._handle()
        stats, counts = np.zeros(4, np.int64), np.zeros(2, np.int64)
        _lib.check(L.tnco_hip_contract_stats(h, _ptr(stats)))
        _lib.check(L.tnco_hip_contract_sets_launches(h, _ptr(counts)))
        members = sets * (p.slice_range[1] - p.slice_range[0])
        return ManyResult(("set",) + tuple(p.inds), array, sets, min(group, members), int(stats[0]), int(stats[1]),
                          (int(counts[0]), int(counts[1])), int(stats[2]), float(stats[3]) * 1e-9)

    def _check_open(self) -> None:
        if self._closed:
            raise ValueError("the Contractor is closed.")

    def _check_arrays(self, arrays, one_kind=True):
        """({leaf number: array}, whether they are torch tensors); one_kind: they must be all numpy or all torch."""
        n = len(self._shapes)
        if isinstance(arrays, dict):
            given = dict(arrays)
            for t in given:
                if not _is_index(t, 0, n):
                    raise ValueError(f"{t!r} is not a leaf of the plan (0 to {n - 1}).")
            given = {int(t): a for t, a in given.items()}
        else:
            given = dict(enumerate(arrays))
            if len(given) != n:
                raise ValueError("'ts_inds' is not consistent with 'arrays'.")
        kinds = {_is_tensor(a) for a in given.values()}
        if len(kinds) > 1 and one_kind:
            raise TypeError("the arrays of one run must be all numpy arrays or all torch tensors.")
        torch_in = True in kinds
        if torch_in and self._host_only:
            raise NotImplementedError(f"torch tensors are not supported with '{self._host_only}'.")
        return given, torch_in

    def _prepare(self, given, torch_in) -> dict:
        """{leaf number: what _load takes}, in leaf order: a numpy leaf as (array as the handle takes it, exponent), a
        tensor as (tensor, dtype code, dims, strides)."""
        p, ready = self.plan, {}
        for t in sorted(given):
            a = given[t]
            if not torch_in:
                a = np.asarray(a)
                if tuple(a.shape) != self._shapes[t]:
                    raise ValueError("'ts_inds' is not consistent with 'arrays'.")
                if not np.can_cast(a.dtype, p.dtype, "safe"):
                    raise TypeError(f"an array of dtype {a.dtype} does not cast safely to {p.dtype}.")
                ready[t] = _host_leaf(p, t, a)
                continue
            if tuple(a.shape) != self._shapes[t]:
                raise ValueError("'ts_inds' is not consistent with 'arrays'.")
            src = _torch_dtypes().get(a.dtype)
            if src is None or not (src == p.dtype or p.dtype in _WIDENS[src]):
                raise TypeError(f"a tensor of dtype {a.dtype} does not widen exactly to {p.dtype}.")
            _check_plain(a, "a tensor")
            if a.device.type != "cuda" or a.device.index != self.device:
                raise ValueError(f"a tensor is on {a.device}, not on cuda:{self.device}.")
            dims, strides = merge_axes(a.shape, a.stride())
            check_extent(a.storage_offset(), dims, strides, a.untyped_storage().nbytes() // a.element_size())
            ready[t] = (a, DTYPES[src], dims, strides)
        if torch_in and p.compute == "bf16x3":
            import torch
            for a, *_ in ready.values():
                x = (torch.view_as_real(a) if a.is_complex() else a).abs()
                if bool((torch.isfinite(x) & (x >= _SPLIT_LIMIT)).any()):
                    raise ValueError("an array has finite values beyond the range of the bfloat16 split (|x| >= 2^128 - 2^119).")
        return ready

    def _check_out(self, out, torch_out, shape=None) -> None:
        p = self.plan
        shape = tuple(p.shape) if shape is None else shape
        if torch_out:
            if _torch_dtypes().get(out.dtype) != p.dtype:
                raise TypeError(f"'out' must be of dtype {p.dtype}, not {out.dtype}.")
            _check_plain(out, "'out'")
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError(f"'out' is on {out.device}, not on cuda:{self.device}.")
            if tuple(out.shape) != shape or not out.is_contiguous():
                raise ValueError(f"'out' must be C-contiguous and of shape {shape}.")
            check_extent(out.storage_offset(), out.shape, _c_strides(out.shape), out.untyped_storage().nbytes() // out.element_size())
            return
        if not isinstance(out, np.ndarray):
            raise TypeError("'out' must be a numpy array or a torch tensor.")
        if out.dtype != p.dtype:
            raise TypeError(f"'out' must be of dtype {p.dtype}, not {out.dtype}.")
        if tuple(out.shape) != shape or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"'out' must be C-contiguous and of shape {shape}.")

    # -- the device

    def _handle(self):
        if self._h is None:
            from . import _lib
            L = _lib.load()
            h = _create(L, self.plan, self.device)
            try:
                _set_modes(L, h, self.plan)
            except Exception:
                L.tnco_hip_contract_destroy(h)
                raise
            self._lib, self._h = L, h
        return self._lib, self._h

    def _note_exponents(self, ready) -> None:
        from . import _lib
        if self.plan.scaling is None:
            return
        for t, (_a, e) in ready.items():
            self._exps[t] = e
        _lib.check(self._lib.tnco_hip_contract_set_exponents(self._h, _ptr(self._exps)))

    def _load(self, ready, torch_in) -> None:
        from . import _lib
        if not ready:
            return
        L, h = self._handle()
        p = self.plan
        if not torch_in:
            code = DTYPES[p.dtype] if p.storage is None else STORAGES[p.storage] + (p.dtype.kind == "c")
            self._note_exponents(ready)
            for t, (a, _e) in ready.items():
                _lib.check(L.tnco_hip_contract_load_leaf(h, t, _ptr(a), 0, code, 1, _i64([p.leaf_numel[t]]), None))
            return
        import torch
        torch.cuda.synchronize(self.device)
        for t, (a, code, dims, strides) in ready.items():
            _lib.check(L.tnco_hip_contract_load_leaf(h, t, C.c_void_p(a.data_ptr()), 1, code, len(dims), _i64(dims), _i64(strides)))


class Walkers:
    """The walkers of a circuit sampler on the device (module docstring, Walkers): `bits`, n_walkers x n_qubits and all 0
    at first, a `dead` flag per walker, and the seed of the draws of `Contractor.choose`.

        with Walkers(4096, n_qubits, seed=7) as w:
            w.permute((0, 1), (0, 1, 3, 2))       # a CNOT of qubit 0 on qubit 1
            c.run_walkers(w, {5: 0, 6: 2}); c.choose(w, 1, step=0)
            w.bits, w.dead                         # numpy: uint8 [n_walkers, n_qubits], bool [n_walkers]

    The constructor does not touch the device: the object there is created at the first use."""

    def __init__(self, n_walkers, n_qubits, seed=0, device=None):
        from . import parallel
        if not _is_index(n_walkers, 1, 1 << 62):
            raise ValueError("'n_walkers' must be a positive integer.")
        if not _is_index(n_qubits, 1, 1 << 62):
            raise ValueError("'n_qubits' must be a positive integer.")
        if int(n_walkers) * int(n_qubits) > 1 << 40:
            raise ValueError("'n_walkers' x 'n_qubits' must be 2^40 at the most.")
        if not _is_index(seed, 0, 1 << 64):
            raise ValueError("'seed' must be an integer from 0 to 2^64 - 1.")
        self.n_walkers, self.n_qubits, self.seed = int(n_walkers), int(n_qubits), int(seed)
        self.device = parallel.local_device() if device is None else int(device)
        self._lib, self._w, self._closed = None, None, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def close(self) -> None:
        """Destroys the object on the device; every use afterwards is refused.  Closing twice is fine."""
        if self._w is not None:
            self._lib.tnco_hip_walkers_destroy(self._w)
        self._w, self._closed = None, True

    def _check_open(self) -> None:
        if self._closed:
            raise ValueError("the Walkers are closed.")

    def _handle(self):
        from . import _lib
        self._check_open()
        if self._w is None:
            L, w = _lib.load(), C.c_void_p()
            _lib.check(L.tnco_hip_walkers_create(self.device, self.n_walkers, self.n_qubits, self.seed, C.byref(w)))
            self._lib, self._w = L, w
        return self._w

    def _read(self):
        from . import _lib
        w = self._handle()
        bits, dead = np.empty((self.n_qubits, self.n_walkers), np.uint8), np.empty(self.n_walkers, np.uint8)
        _lib.check(self._lib.tnco_hip_walkers_read(w, _ptr(bits), _ptr(dead)))
        return np.ascontiguousarray(bits.T), dead.astype(bool)

    @property
    def bits(self) -> np.ndarray:
        """uint8 [n_walkers, n_qubits], a copy."""
        return self._read()[0]

    @property
    def dead(self) -> np.ndarray:
        """bool [n_walkers]: the walkers that a `choose` found without a finite, positive probability."""
        return self._read()[1]

    def write(self, bits) -> None:
        """Sets the table from an integer array [n_walkers, n_qubits] of zeros and ones; the dead flags stay."""
        from . import _lib
        self._check_open()
        bits = np.asarray(bits)
        if bits.shape != (self.n_walkers, self.n_qubits) or bits.dtype.kind not in "biu":
            raise ValueError(f"'bits' must be an integer array of shape {(self.n_walkers, self.n_qubits)}.")
        if bits.size and not ((bits == 0) | (bits == 1)).all():
            raise ValueError("'bits' must hold zeros and ones only.")
        table = np.ascontiguousarray(bits.T, dtype=np.uint8)
        w = self._handle()
        _lib.check(self._lib.tnco_hip_walkers_write(w, _ptr(table)))

    def reset(self) -> None:
        """Every bit and every dead flag 0."""
        from . import _lib
        w = self._handle()
        _lib.check(self._lib.tnco_hip_walkers_reset(w))

    def permute(self, qubits, table) -> None:
        """A classical gate on every walker: with v the number that its bits of `qubits` spell, the first qubit the most
        significant, those bits become table[v]; `table` is a permutation of 0 .. 2^k - 1, k = len(qubits) <= 8."""
        from . import _lib
        self._check_open()
        qubits, table = tuple(qubits), tuple(table)
        if not 1 <= len(qubits) <= MAX_PERMUTE_QUBITS:
            raise ValueError(f"'qubits' must name 1 to {MAX_PERMUTE_QUBITS} qubits.")
        for q in qubits:
            if not _is_index(q, 0, self.n_qubits):
                raise ValueError(f"{q!r} is not a qubit of the walkers (0 to {self.n_qubits - 1}).")
        if len(set(qubits)) != len(qubits):
            raise ValueError("'qubits' names a qubit twice.")
        n = 1 << len(qubits)
        if len(table) != n or any(not _is_index(v, 0, n) for v in table) or len(set(table)) != n:
            raise ValueError(f"'table' must be a permutation of 0 to {n - 1}.")
        qs, tb = np.array(qubits, np.int64), np.array(table, np.uint8)
        w = self._handle()
        _lib.check(self._lib.tnco_hip_walkers_permute(w, len(qubits), _ptr(qs), _ptr(tb)))
