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
//   ct_walk_choose_joint_kernel  one lane per walker: the 2^k amplitudes of the walker's output, the same draw and the
//                          new bits of k <= 6 qubits, drawn jointly;
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

constexpr int WALK_MAX_CHOOSE = 6;  // qubits of a joint choice at the most: 64 amplitudes per walker

struct WalkChoose {
  int64_t qubit[WALK_MAX_CHOOSE];   // the k qubits, the first the most significant bit of an outcome
  int64_t stride[WALK_MAX_CHOOSE];  // elements between the amplitudes with qubit j's open index 0 and 1
};

// tail(0) of a walker's N = 2^k amplitudes, tail(v) = p_v + ... + p_{N-1} summed from the top, one rounding per addition
// (0 + p_{N-1} is exact), and in `outcome` the largest v >= 1 with t < tail(v), 0 if there is none: the tails do not fall
// as v falls, so the first hit of the descending pass is kept, by a select.  NATURAL: the strides are 2^(k-1-j), amplitude
// v lies at block[v], and a lane reads its block in chunks of C elements (C sizeof(T) <= 16 bytes, to which the block is
// aligned); else amplitude v lies at the sum of the strides of v's set bits, an offset that is uniform over the lanes.
template <class T, int C, bool NATURAL>
__device__ inline double ct_walk_tails(const T* __restrict__ block, int k, const WalkChoose& a, double t, int& outcome) {
  struct alignas(sizeof(T) * C) Chunk {
    T e[C];
  };
  const int N = 1 << k;
  double tail = 0.0;
  outcome = 0;
  for (int v0 = N - C; v0 >= 0; v0 -= C) {
    Chunk c;
    if constexpr (NATURAL) {
      c = *(const Chunk*)(block + v0);
    } else {
      int64_t off = 0;
      for (int j = 0; j < k; ++j) off += ((v0 >> (k - 1 - j)) & 1) * a.stride[j];
      c.e[0] = block[off];
    }
#pragma unroll
    for (int e = C - 1; e >= 0; --e) {
      tail = __dadd_rn(tail, ct_walk_prob(c.e[e]));
      if (outcome == 0 && v0 + e >= 1 && t < tail) outcome = v0 + e;
    }
  }
  return tail;
}

template <class T>
__device__ inline double ct_walk_tails(const T* __restrict__ block, int k, bool natural, const WalkChoose& a, double t, int& outcome) {
  constexpr int C = 16 / (int)sizeof(T);  // elements of a 16-byte load: 4 floats, 2 doubles or cplx<float>, 1 cplx<double>
  if (!natural) return ct_walk_tails<T, 1, false>(block, k, a, t, outcome);
  if constexpr (C > 2)
    if (k == 1) return ct_walk_tails<T, 2, true>(block, k, a, t, outcome);  // (two floats: one 8-byte load)
  return ct_walk_tails<T, C, true>(block, k, a, t, outcome);
}

// One lane per walker i: the k <= 6 qubits a.qubit[0 .. k) are drawn jointly from the N = 2^k amplitudes of the walker's
// output block out + each i (each: N, or 0 where one output serves every walker).  Outcome v has the first qubit as its
// most significant bit; p_v = |a_v|^2 and the tails as ct_walk_tails has them, s = tail(0); u is ct_walk_choose_kernel's
// u, one draw whatever k is; t = u s; the outcome is the largest v >= 1 with t < tail(v), or 0.  Two descending passes
// over the block, the first for s, the second for the outcome (its reads hit the cache): no tail is held between them.  A
// walker whose s is 0 or not finite gets outcome 0 and dead[i].  At k = 1 these are ct_walk_choose_kernel's bytes: s =
// p1 + p0, bit = (u s < p1).  An outcome v >= 1 with p_v = 0 is never drawn (tail(v) = tail(v + 1)); outcome 0 with p_0 =
// 0 only where u s rounds up to s.  natural: the strides are 2^(k-1-j), the layout of a plan whose held axes are the
// qubits in order.  The qubits and strides are kernel arguments, read through scalar loads.  Registers (gfx950, ROCm 7.0
// hipcc), VGPRs / SGPRs: 24 / 54 for float, 22 / 52 for double, 26 / 52 for cplx<float>, 24 / 49 for cplx<double>; no
// scratch, no spill, no LDS, no atomics.
template <class T>
__global__ __launch_bounds__(256) void ct_walk_choose_joint_kernel(uint8_t* __restrict__ bits, uint8_t* __restrict__ dead,
                                                                   const T* __restrict__ out, int64_t each, int64_t n_walkers,
                                                                   uint64_t seed, uint32_t step, int k, int natural, WalkChoose a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_walkers; i += (int64_t)gridDim.x * blockDim.x) {
    const T* block = out + each * i;
    int outcome;
    const double s = ct_walk_tails(block, k, natural != 0, a, 0.0, outcome);
    uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), step, 0u};
    ct_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = __dmul_rn(__dadd_rn(__dmul_rn((double)(c[0] >> 5), 67108864.0), (double)(c[1] >> 6)), 0x1p-53);
    const bool alive = s > 0.0 && s < __builtin_inf();  // (false for a NaN too)
    ct_walk_tails(block, k, natural != 0, a, __dmul_rn(u, s), outcome);
    if (!alive) outcome = 0;
    for (int j = 0; j < k; ++j) bits[a.qubit[j] * n_walkers + i] = (uint8_t)((outcome >> (k - 1 - j)) & 1);
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
