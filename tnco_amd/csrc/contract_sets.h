// contract_sets.h -- many leaf sets of one plan per launch of the path kernel (tnco_hip_contract_load_leaf_sets,
// tnco_hip_contract_run_sets); included by contract.hip inside its anonymous namespace, after contract_path.h.
// A caller that runs one plan thousands of times changes a few small leaves between runs.  Here a member of a launch is
// a pair (leaf set i, slice assignment a), numbered set-major: with A = stop - start assignments per set, member
// m = i A + (a - start).  R sets are ceil(R A / group) pairs of launches:
//   ct_sets_path_kernel    block b = member m0 + b, in arena copy b: ct_path_member (contract_path.h) for assignment a as a
//                          MEMBER_SETS, every leaf read at its pointer + i times its set stride (+ the slice offset of a);
//                          the stride is the leaf's elements for a leaf that has a stack [n_sets][leaf_numel], 0 for a
//                          leaf that every set shares, and the pointer is the stack's or the single buffer's;
//   ct_sets_reduce_kernel  stage [n][block] -> out [n_sets][out_numel], one lane per element of a block, the members in
//                          order, member m to set i's copy of the output at the block offset and with the beta bit of
//                          entry a - start of the plan's placement table (ct_path_reduce_kernel's, A entries: nothing here
//                          is proportional to R A).
// Set i is folded in ascending assignment order with the plan's own placement and beta bits, and a member's block does not
// depend on its neighbours: out[i] is bit for bit the output of a run of the plan over leaf set i, however the groups cut
// the sets.  (i, a) come from blockIdx and kernel arguments: every table address and every branch around a barrier stays
// uniform over the block, as in ct_path_kernel.  No atomics.
#pragma once

struct SetsArgs {
  PathArgs p;                 // leaves and sid0 are not read
  const int64_t* set_leaves;  // [n_leaves][SET_W]: the leaf's pointer (its stack, or its single buffer) and the elements between
                              // two sets of it (leaf_numel[t], or 0), side by side: one read per leaf
  int64_t m0;                 // the member of block 0
  int64_t n_assign, start;    // A and the first assignment of the plan's slice range
};

// One block per member, PATH_LANES lanes.  Registers (gfx950, ROCm 7.0 hipcc): 34 VGPRs for float, 38 for double, 38 for
// cplx<float>, 44 for cplx<double>, those of ct_path_kernel (the set lives in scalar registers: 80 SGPRs against 78); no
// scratch, no spill; LDS: the 1024 partials of the dot class, 4 to 16 KiB, as ct_path_kernel.
template <class T>
__global__ __launch_bounds__(PATH_LANES) void ct_sets_path_kernel(SetsArgs s) {
  __shared__ T part[PATH_LANES];
  const int64_t b = blockIdx.x, m = s.m0 + b;
  const int64_t set = m / s.n_assign, sid = s.start + m % s.n_assign;
  ct_path_member<T, MEMBER_SETS>(s.p, b, sid, LeafFrom{s.set_leaves, set, nullptr}, part);
}

// ct_path_reduce_kernel with the set axis: lane e of a block's elements takes the n members one after the other, so the
// members of one set meet their output block in assignment order and two sets never share an element.  Registers: 18
// VGPRs for float, 20 for double and cplx<float>, 24 for cplx<double>; no scratch, no spill, no LDS.
// The members of one set are walked with the sum in a register while they stay on one block of the output: the value
// is written when the block changes and read again when a later member adds to it, so every element sees the places and
// additions of ct_path_reduce_kernel in the same order -- the same bits -- without a store and a load of the output between
// two members (measured on an amplitude, one block per set, 1024 members: 0.15 ms against ct_path_reduce_kernel's 0.22 ms).
template <class T>
__global__ __launch_bounds__(256) void ct_sets_reduce_kernel(T* __restrict__ out, const T* __restrict__ stage, int64_t numel,
                                                             int n, int64_t m0, int64_t n_assign, int64_t out_numel,
                                                             const int64_t* __restrict__ place) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t set = m0 / n_assign, a = m0 % n_assign;
    for (int b = 0; b < n; a = 0, ++set) {
      const int stop = (int)(n - b < n_assign - a ? n : b + (n_assign - a));  // the members of this set end here
      const int64_t* pl_of = place + (a - b);                                 // member b's entry is pl_of[b]
      T* o = out + set * out_numel + e;
      int64_t at = pl_of[b] >> 1;
      T acc = pl_of[b] & 1 ? ct_add(o[at], stage[b * numel + e]) : stage[b * numel + e];
      for (++b; b < stop; ++b) {
        const int64_t pl = pl_of[b];
        const T v = stage[b * numel + e];
        if ((pl >> 1) != at) {
          o[at] = acc;
          at = pl >> 1;
          acc = pl & 1 ? ct_add(o[at], v) : v;
        } else {
          acc = pl & 1 ? ct_add(acc, v) : v;
        }
      }
      o[at] = acc;
    }
  }
}
