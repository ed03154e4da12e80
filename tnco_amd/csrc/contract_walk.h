// contract_walk.h -- walkers of a gate-by-gate circuit sampler on the device (tnco_hip_walkers_*,
// tnco_hip_contract_load_leaf_versions, tnco_hip_contract_run_walkers); included by contract.hip inside its anonymous
// namespace, after contract_sets.h.
// A sampler's state is a table of bits, bits[qubit][walker], and the leaves that differ between its walkers are one-hot
// vectors: two constant versions and a bit that says which.  So the table stays on the device, a leaf's two versions lie
// in a buffer [2][leaf_numel] of the handle's that is loaded once, and a member (walker i, assignment a) of a launch
// reads an indexed leaf at versions + bits[qubit of the leaf][i] leaf_numel:
//   ct_walk_path_kernel    ct_path_member (contract_path.h) for a MEMBER_WALK, numbered as ct_sets_path_kernel numbers its
//                          members; the blocks are folded by ct_sets_reduce_kernel as they are there: out[i] is bit for
//                          bit the output of a run over the leaves that walker i's bits select;
//   ct_walk_choose_kernel  one lane per walker: the two amplitudes of the walker's output, a Philox4x32-10 draw and the
//                          new bit of one qubit;
//   ct_walk_permute_kernel one lane per walker: k <= 8 of its bits through a table of 2^k entries (a classical gate).
// No atomics, no state between draws: a choice is a function of (seed, walker, step, amplitudes).
#pragma once

struct WalkArgs {
  PathArgs p;                  // leaves and sid0 are not read
  const int64_t* walk_leaves;  // [n_leaves][WALK_W]: the leaf's pointer (its versions, or its single buffer), the qubit whose
                               // bit picks the version (-1: none), the elements between two versions
  const uint8_t* bits;         // [n_qubits][n_walkers]
  int64_t n_walkers;
  int64_t m0;                  // the member of block 0
  int64_t n_assign, start;     // A and the first assignment of the plan's slice range
};

// One block per member, PATH_LANES lanes, the set being the walker.  bits + walker is the walker's column of the table;
// the bit of qubit q lies q n_walkers bytes further, an address that is uniform over the block, as every table address
// is.  (Reading the bits of the first 64 qubits once per block instead, lane by lane and through a ballot, took the same
// 39 ms on the timing leg: not kept.)  Registers as ct_sets_path_kernel's (82 SGPRs); no scratch, no spill; LDS: the
// 1024 partials of the dot class.
template <class T>
__global__ __launch_bounds__(PATH_LANES) void ct_walk_path_kernel(WalkArgs s) {
  __shared__ T part[PATH_LANES];
  const int64_t b = blockIdx.x, m = s.m0 + b;
  const int64_t walker = m / s.n_assign, sid = s.start + m % s.n_assign;
  ct_path_member<T, MEMBER_WALK>(s.p, b, sid, LeafFrom{s.walk_leaves, s.n_walkers, s.bits + walker}, part);
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
// the key raised by (W0, W1) between two rounds.
__host__ __device__ inline void ct_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// |a|^2 in float64, the parts widened exactly, every operation rounded on its own
__device__ inline double ct_walk_prob(float a) { return __dmul_rn((double)a, (double)a); }
__device__ inline double ct_walk_prob(double a) { return __dmul_rn(a, a); }
template <class R>
__device__ inline double ct_walk_prob(cplx<R> a) {
  return __dadd_rn(__dmul_rn((double)a.re, (double)a.re), __dmul_rn((double)a.im, (double)a.im));
}

// One lane per walker i: (a0, a1) = out[each i], out[each i + 1] (each: 2, or 0 where one output serves every walker),
// p = |a|^2, s = p0 + p1; u in [0, 1) from the Philox block of key (seed lo, seed hi) and counter (i lo, i hi, step, 0),
// 53 bits of its first two words; bits[qubit][i] = u s < p1.  A walker whose s is 0 or not finite has nothing to choose
// from: its bit becomes 0 and dead[i] is set.  Registers (gfx950, ROCm 7.0 hipcc): 14 VGPRs for float, 16 for double and
// cplx<float>, 20 for cplx<double>; no scratch, no spill, no LDS.
template <class T>
__global__ __launch_bounds__(256) void ct_walk_choose_kernel(uint8_t* __restrict__ bit_row, uint8_t* __restrict__ dead,
                                                             const T* __restrict__ out, int64_t each, int64_t n_walkers,
                                                             uint64_t seed, uint32_t step) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_walkers; i += (int64_t)gridDim.x * blockDim.x) {
    const double p0 = ct_walk_prob(out[each * i]), p1 = ct_walk_prob(out[each * i + 1]);
    const double s = __dadd_rn(p0, p1);
    uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), step, 0u};
    ct_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = __dmul_rn(__dadd_rn(__dmul_rn((double)(c[0] >> 5), 67108864.0), (double)(c[1] >> 6)), 0x1p-53);
    const bool alive = s > 0.0 && s < __builtin_inf();  // (false for a NaN too)
    bit_row[i] = alive && __dmul_rn(u, s) < p1 ? 1 : 0;
    if (!alive) dead[i] = 1;
  }
}

constexpr int WALK_MAX_PERMUTE = 8;  // qubits of a classical gate at the most

// One lane per walker: value = the bits of the k qubits, the first the most significant; table[value] goes back the same
// way.  perm: [WALK_MAX_PERMUTE] qubits as int64, then the 2^k bytes of the table.  9 VGPRs; no scratch, no spill, no LDS.
__global__ __launch_bounds__(256) void ct_walk_permute_kernel(uint8_t* __restrict__ bits, int64_t n_walkers, int k,
                                                              const int64_t* __restrict__ perm) {
  const uint8_t* table = (const uint8_t*)(perm + WALK_MAX_PERMUTE);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_walkers; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t value = 0;
    for (int j = 0; j < k; ++j) value = 2 * value + (bits[perm[j] * n_walkers + i] & 1);
    const uint32_t next = table[value];
    for (int j = 0; j < k; ++j) bits[perm[j] * n_walkers + i] = (uint8_t)((next >> (k - 1 - j)) & 1);
  }
}
