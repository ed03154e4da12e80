// contract_path.h -- a whole slice assignment in one kernel (tnco_hip_contract_set_path_kernel); included by contract.hip
// inside its anonymous namespace, after ct_slice_offset, ct_zero / ct_mac / ct_add and contract_tables.h.
// The sliced runs are bound by launches: a width-bounded assignment is a few hundred small gathers and steps.  Here one
// workgroup interprets the whole path for one assignment, so a group of up to MAX_PATH_GROUP assignments is one launch,
// and a second launch folds the group's blocks into the output:
//   ct_path_kernel         block b = assignment first + b, in its own copy of the arena: permute group -1, then for each
//                          step its permute group and the step, a workgroup barrier between consecutive operations; the
//                          last step leaves the member's block, unrounded and with beta 0, in stage[b];
//   ct_path_reduce_kernel  stage [n][block] -> the output, one lane per element, the members in assignment order, block
//                          offsets and beta bits from a device table filled before the first launch.
// The four plain dtypes only.  Every sum keeps the order of the kernel launch_gemm would have chosen for the step, so a
// run is bit for bit that of the unfused loop (see ct_path_step).  The tables are read through uniform addresses only,
// and every loop bound and branch around a barrier is a table value: all lanes of a block pass the same barriers.
// What a member does is written once, here (ct_path_member, over ct_path_permutes, ct_path_leaf and ct_path_step), for
// the three kinds of member (PathMember): an assignment of the plan (ct_path_kernel), a pair (leaf set, assignment)
// (ct_sets_path_kernel, contract_sets.h) and a pair (walker, assignment) (ct_walk_path_kernel, contract_walk.h).  The
// kinds differ in where a leaf is read (ct_path_leaf), and the kernels in how a block finds its member.
#pragma once

constexpr int MAX_PATH_GROUP = 1024;  // assignments per launch at most (tnco_amd/contraction.py MAX_PATH_KERNEL)
// One workgroup runs each step: a step beyond this many multiply-adds (H M N K) would hold one compute unit of a shared
// card for long, so a plan that has one is refused.  A guard, not a tuned threshold.  It also bounds every operand, every
// result and every permuted intermediate of a step by 2^24 elements: the element arithmetic below is 32-bit.
constexpr int64_t MAX_PATH_STEP_MACS = (int64_t)1 << 24;
constexpr int PATH_LANES = 1024;  // lanes of a block: four 256-lane quarters, each ct_dot_body's block for one output

struct PathArgs {
  const int64_t* perms;        // [n_perms][PERM_W], sorted by group
  const int64_t* leaf_sl;      // [n_leaves][LEAF_SL_W]
  const int64_t* slice_place;  // place value of every slice position
  const int64_t* slice_dims;
  const int64_t* steps;        // [n_steps][STEP_W]
  const int64_t* groups;       // [n_steps + 1][GR_W]: first row and number of rows of permute group g at g + 1
  const void* const* leaves;
  void* arena;                 // a copy of arena_elems elements per member
  void* stage;                 // [members][block_numel]
  int64_t arena_elems, block_numel;
  int64_t sid0;                // the assignment of block 0
  int n_steps;
};

// The kinds of member, and where a member's leaves come from beyond the plan's tables: nothing for MEMBER_PLAN.
enum PathMember { MEMBER_PLAN, MEMBER_SETS, MEMBER_WALK };
struct LeafFrom {
  const int64_t* table = nullptr;   // MEMBER_SETS: [n_leaves][SET_W]; MEMBER_WALK: [n_leaves][WALK_W]
  int64_t set = 0;                  // MEMBER_SETS: the member's set; MEMBER_WALK: the number of walkers
  const uint8_t* column = nullptr;  // MEMBER_WALK: the walker's column of the table of bits
};

// Leaf t as assignment sid reads it: at the slice offset of the assignment.  MEMBER_SETS: the leaf comes from the table,
// [n_leaves][SET_W]: its pointer and the elements between two sets of it (0 or the leaf's elements), and the base moves on by
// set times that, a 64-bit product; pointer and stride lie side by side, one read, and it is asked for before the slice
// offset is worked out, as a MEMBER_PLAN asks for its pointer (every block of a launch reads the same entry at about the
// same time: read after the offset loop, its latency lay open once per leaf and cost the kernel a quarter of its time).
// MEMBER_WALK: the table is [n_leaves][WALK_W], the leaf's pointer, the qubit whose bit picks one of its two versions
// (-1: none) and the elements between them; column[qubit * number of walkers] is the member's bit, a uniform address,
// asked for right after the entry and before the offset too.  MEMBER_PLAN: nothing is added and nothing more is read.
template <class T, PathMember MODE>
__device__ inline const T* ct_path_leaf(const PathArgs& p, int64_t t, int64_t sid, const LeafFrom& from) {
  if constexpr (MODE == MEMBER_SETS) {
    // (asked for before the offset is worked out)
    const int64_t base = from.table[SET_W * t + SET_PTR], step = from.table[SET_W * t + SET_STRIDE];
    return (const T*)base + (ct_slice_offset(p.leaf_sl + t * LEAF_SL_W, p.slice_place, p.slice_dims, sid) + from.set * step);
  } else if constexpr (MODE == MEMBER_WALK) {
    const int64_t base = from.table[WALK_W * t + WK_PTR], qubit = from.table[WALK_W * t + WK_QUBIT], step = from.table[WALK_W * t + WK_STRIDE];
    const int64_t version = qubit < 0 ? 0 : from.column[qubit * from.set] & 1;  // (both before the offset is worked out)
    return (const T*)base + (ct_slice_offset(p.leaf_sl + t * LEAF_SL_W, p.slice_place, p.slice_dims, sid) + version * step);
  } else {
    return (const T*)p.leaves[t] + ct_slice_offset(p.leaf_sl + t * LEAF_SL_W, p.slice_place, p.slice_dims, sid);
  }
}

// the rows of one permute group, one after the other (they are independent of each other: one launch in the unfused
// loop): ct_gather_body's element loop, strided over the block.  A permute feeds a step, so numel < 2^24.
template <class T, PathMember MODE>
__device__ inline void ct_path_permutes(const PathArgs& p, int64_t group, T* arena, int64_t sid, const LeafFrom& from) {
  const int64_t first = p.groups[GR_W * (group + 1) + GR_FIRST], count = p.groups[GR_W * (group + 1) + GR_COUNT];
  for (int64_t r = first; r < first + count; ++r) {
    const int64_t* row = p.perms + r * PERM_W;
    const uint32_t numel = (uint32_t)row[PM_NUMEL];
    const int nd = (int)row[PM_NDIM];
    const T* src;
    if (row[PM_SRC_KIND] == K_LEAF)
      src = ct_path_leaf<T, MODE>(p, row[PM_SRC_REF], sid, from);
    else
      src = arena + row[PM_SRC_REF];
    T* dst = arena + row[PM_DST_REF];
    for (uint32_t e = threadIdx.x; e < numel; e += PATH_LANES) {
      uint32_t rem = e;
      int64_t off = 0;  // (a stride of a leaf's axis may be beyond 32 bits: the sliced axes lie between the kept ones)
      for (int k = nd - 1; k >= 0; --k) {
        const uint32_t d = (uint32_t)row[PM_DIMS + k], q = rem / d;
        off += (int64_t)(rem - q * d) * row[PM_STRIDES + k];
        rem = q;
      }
      dst[e] = src[off];
    }
  }
}

// One step, C = A B with beta 0, in the summation order of the kernel launch_gemm picks for its shape:
//   tiled and stream class: one lane per output element, k ascending from ct_zero with ct_mac -- ct_stream_body's order,
//     and ct_gemm_tiled_kernel's too (its zero fill at a k tail adds fma(0, 0, acc) = acc);
//   dot class (K >= 512, at most 8192 outputs, not tiled): an output per 256-lane quarter of the block, lane t of the
//     quarter k = t, t + 256, ..., then ct_dot_body's tree over the quarter's 256 partials; four outputs per trip.
// The trip count of the dot loop is the same for every lane: a quarter without an output (1 or 5 outputs) sums nothing,
// stores nothing and passes the barriers.  H M N K <= 2^24: every offset inside an operand fits 32 bits.
template <class T>
__device__ inline void ct_path_step(const int64_t* st, const T* A, const T* B, T* C, T* part) {
  const uint32_t a_m = (uint32_t)st[ST_A_M], a_k = (uint32_t)st[ST_A_K], b_k = (uint32_t)st[ST_B_K], b_n = (uint32_t)st[ST_B_N];
  const uint32_t H = (uint32_t)st[ST_H], M = (uint32_t)st[ST_M], N = (uint32_t)st[ST_N], K = (uint32_t)st[ST_K];
  const uint32_t total = H * M * N;
  const bool tiled = M >= 64 && N >= 64 && K > 32;
  if (!tiled && K >= 512 && total <= 8192) {
    const uint32_t quarter = threadIdx.x / 256, t = threadIdx.x % 256;
    T* mine = part + 256 * quarter;
    const uint32_t trips = (total + 3) / 4;
    for (uint32_t trip = 0; trip < trips; ++trip) {
      const uint32_t e = 4 * trip + quarter;
      const bool active = e < total;
      T acc = ct_zero<T>();
      if (active) {
        const uint32_t n = e % N, r = e / N, m = r % M, h = r / M;
        const T* a = A + (h * M * K + m * a_m);
        const T* b = B + (h * K * N + n * b_n);
        for (uint32_t k = t; k < K; k += 256) acc = ct_mac(acc, a[k * a_k], b[k * b_k]);
      }
      mine[t] = acc;
      __syncthreads();
      for (uint32_t w = 128; w > 0; w >>= 1) {
        if (t < w) mine[t] = ct_add(mine[t], mine[t + w]);
        __syncthreads();
      }
      if (active && t == 0) C[e] = mine[0];
      __syncthreads();
    }
    return;
  }
  for (uint32_t e = threadIdx.x; e < total; e += PATH_LANES) {
    const uint32_t n = e % N, r = e / N, m = r % M, h = r / M;
    const T* a = A + (h * M * K + m * a_m);
    const T* b = B + (h * K * N + n * b_n);
    T acc = ct_zero<T>();
    for (uint32_t k = 0; k < K; ++k) acc = ct_mac(acc, a[k * a_k], b[k * b_k]);
    C[e] = acc;
  }
}

// What the block of a member does: block b of the launch runs assignment sid in arena copy b and leaves the member's
// block in stage[b]; `part`: the block's PATH_LANES partials of the dot class.  b, sid and `from` are uniform over the
// block.  __syncthreads() orders the block's global writes for the block, and an arena copy and a block of the staging
// belong to one block only.
template <class T, PathMember MODE>
__device__ inline void ct_path_member(const PathArgs& p, int64_t b, int64_t sid, const LeafFrom& from, T* part) {
  T* arena = (T*)p.arena + b * p.arena_elems;
  ct_path_permutes<T, MODE>(p, -1, arena, sid, from);
  __syncthreads();
  for (int k = 0; k < p.n_steps; ++k) {
    ct_path_permutes<T, MODE>(p, k, arena, sid, from);
    __syncthreads();
    const int64_t* st = p.steps + (int64_t)k * STEP_W;
    const T* opnd[2];
    for (int side = 0; side < 2; ++side) {
      const int64_t kind = st[ST_SIDE * side + ST_A_KIND], ref = st[ST_SIDE * side + ST_A_REF];
      // (a leaf read in place: at the slice offset of this member's assignment, as ct_member has it)
      opnd[side] = kind == K_LEAF ? ct_path_leaf<T, MODE>(p, ref, sid, from) : arena + ref;
    }
    T* C = st[ST_C_KIND] == K_OUT ? (T*)p.stage + b * p.block_numel : arena + st[ST_C_REF];
    ct_path_step<T>(st, opnd[0], opnd[1], C, part);
    __syncthreads();
  }
}

// One block per member of the group, PATH_LANES lanes (the four quarters of the dot class; 16 wavefronts leave a lane
// 128 registers).  Registers (gfx950, ROCm 7.0 hipcc): 34 VGPRs for float, 38 for double, 38 for cplx<float>, 44 for
// cplx<double>; no scratch; LDS: the 1024 partials of the dot class, 4 to 16 KiB.
template <class T>
__global__ __launch_bounds__(PATH_LANES) void ct_path_kernel(PathArgs p) {
  __shared__ T part[PATH_LANES];
  const int64_t b = blockIdx.x;
  ct_path_member<T, MEMBER_PLAN>(p, b, p.sid0 + b, LeafFrom{}, part);
}

// What ct_batch_reduce_kernel does, for up to MAX_PATH_GROUP members: place[b] = (element offset of member b's block of
// the output) * 2 + beta, beta 1 when an earlier assignment of the run wrote that block (the host's `visited`
// bookkeeping, which does not depend on the data: the table of the whole run is on the device before the first launch).
// One lane per element of a block, the members one after the other in assignment order, each exactly the store of an
// unfused last step (ct_store).  No atomics.
template <class T>
__global__ __launch_bounds__(256) void ct_path_reduce_kernel(T* out, const T* stage, int64_t numel, int n, const int64_t* place) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    for (int b = 0; b < n; ++b) {
      const int64_t pl = place[b];
      T* o = out + (pl >> 1) + e;
      const T v = stage[b * numel + e];
      *o = pl & 1 ? ct_add(*o, v) : v;
    }
}
