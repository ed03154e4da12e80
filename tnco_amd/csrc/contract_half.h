// contract_half.h -- the half-precision storage mode of the contraction engine (tnco_hip.h, dtype codes 4..7); included
// by contract.hip inside its anonymous namespace, after cplx / ct_zero / ct_mac / ct_add / ct_acc / MemberArgs.
// Leaves and intermediates are float16 or bfloat16 (a complex element an interleaved (re, im) pair), every sum is
// float32, a value is rounded once, to nearest even, when it is stored to the arena; the output stays float32.
//   ct_mfma_tiled_kernel   the tiled shape class on the matrix cores (v_mfma_f32_16x16x32_{f16,bf16});
//   the dot and stream classes and the gathers are the bodies of contract.hip, instantiated with a widening load and a
//   store chosen by the destination.
// Per-tensor scaling (tnco_hip_contract_desc.scaling): every stored tensor has one int32 exponent e in a device array,
// stored = round(x 2^-e), e = floor(log2 m) - 14 with m the largest finite |part| of the tensor (ct_scale_exponent).  The
// SC instantiations of the three GEMM kernels write an arena-destined result unrounded to a float32 staging buffer and
// keep the largest sign-cleared bit pattern of its finite parts (one atomicMax per wavefront into the step's max word);
//   ct_scale_narrow_kernel derives the exponent from that word, rounds the staged values to storage and records it.
// A result for the output is scaled back with ldexpf by the operands' exponents.
#pragma once

struct st_f16 {
  uint16_t v;
};
struct st_bf16 {
  uint16_t v;
};

// the 16-bit storage types are summed in float32 (ct_acc: contract.hip)
template <>
struct ct_acc<st_f16> {
  using type = float;
};
template <>
struct ct_acc<st_bf16> {
  using type = float;
};
template <>
struct ct_acc<cplx<st_f16>> {
  using type = cplx<float>;
};
template <>
struct ct_acc<cplx<st_bf16>> {
  using type = cplx<float>;
};
template <class E>
struct ct_storage_of {
  using type = E;
};
template <class S>
struct ct_storage_of<cplx<S>> {
  using type = S;
};

__device__ inline float ct_widen(st_f16 s) { return (float)__builtin_bit_cast(_Float16, s.v); }
__device__ inline float ct_widen(st_bf16 s) { return __uint_as_float((uint32_t)s.v << 16); }
template <class S>
__device__ inline cplx<float> ct_widen(cplx<S> s) {
  return cplx<float>{ct_widen(s.re), ct_widen(s.im)};
}
// to nearest, ties to even; beyond the range: inf, as the conversion instruction gives it
__device__ inline void ct_narrow(float x, st_f16* d) { d->v = __builtin_bit_cast(uint16_t, (_Float16)x); }
__device__ inline void ct_narrow(float x, st_bf16* d) {  // (the integer form of contraction.py _bf16_bits)
  const uint32_t u = __float_as_uint(x);
  d->v = (u & 0x7fffffffu) > 0x7f800000u ? (uint16_t)((u >> 16) | 0x40u) : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
template <class S>
__device__ inline void ct_narrow(cplx<float> x, cplx<S>* d) {
  ct_narrow(x.re, &d->re);
  ct_narrow(x.im, &d->im);
}

// the exponent of a tensor whose largest finite |part| has the float32 bit pattern m (sign cleared, m < 0x7f800000):
// floor(log2 m) - 14, float32 subnormals included; 0 for m == 0 (a zero tensor, or none of its parts finite).  The one
// statement of the rule on the device; contraction.py scale_exponent is the same integer arithmetic on the host.
__host__ __device__ inline int32_t ct_scale_exponent(uint32_t m) {
  if (m == 0) return 0;
  const int32_t lg = (m >> 23) ? (int32_t)(m >> 23) - 127 : (31 - __builtin_clz(m)) - 149;
  return lg - 14;
}
__device__ inline float ct_ldexp(float x, int e) { return ldexpf(x, e); }
__device__ inline cplx<float> ct_ldexp(cplx<float> x, int e) { return cplx<float>{ldexpf(x.re, e), ldexpf(x.im, e)}; }
// the sign-cleared pattern of a finite part, 0 for inf and NaN; of a pair: the larger
__device__ inline uint32_t ct_finite_bits(float x) {
  const uint32_t u = __float_as_uint(x) & 0x7fffffffu;
  return u < 0x7f800000u ? u : 0u;
}
__device__ inline uint32_t ct_finite_bits(cplx<float> x) { return max(ct_finite_bits(x.re), ct_finite_bits(x.im)); }

// GemmArgs of a storage-mode step: operands in storage, the result to the arena in storage (Cs) or to the output in
// float32 (C, with beta); exactly one of the two is set.  Scaling (the SC instantiations; the others read none of it):
// exps, the exponent slots of the handle, sa and sb the operands' slots; a result for the output is C with exps set, a
// result for the arena is C = the float32 staging buffer with beta 0 and amax = the step's max word
template <class E>
struct HalfGemmArgs {
  const E* A;
  const E* B;
  E* Cs;
  ct_acc_t<E>* C;
  int64_t a_m, a_k, b_k, b_n;
  int64_t H, M, N, K;
  int beta;
  int a_vec, b_vec;  // the operand's runs of 8 elements along its contiguous axis are 16-byte aligned
  const int32_t* exps;
  int sa, sb;
  uint32_t* amax;
  MemberArgs mb;
};

// the operands, the result, the exponent slots and the max word of this block's member (contract.hip, MemberArgs).
// a_vec / b_vec are checked again at the member's own base: a precaution only, since with the row stride a multiple of 8
// elements every slice offset is one too, and the arenas are a multiple of 64 elements apart, so a member's alignment
// is that of the base the host looked at (no test reaches a member where they differ)
template <class E>
__device__ inline void ct_member(HalfGemmArgs<E>& p) {
  const MemberArgs& mb = p.mb;
  const int64_t b = blockIdx.z;
  p.A = ct_shift(p.A, b * mb.a_step) + (mb.a_ls ? ct_slice_offset(mb.a_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.B = ct_shift(p.B, b * mb.b_step) + (mb.b_ls ? ct_slice_offset(mb.b_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.a_vec = p.a_vec && (uintptr_t)p.A % 16 == 0;
  p.b_vec = p.b_vec && (uintptr_t)p.B % 16 == 0;
  if (p.Cs) p.Cs = ct_shift(p.Cs, b * mb.c_step);
  if (p.C) p.C = ct_shift(p.C, b * mb.c_step);
  if (p.exps) p.exps += b * mb.exp_step;
  if (p.amax) p.amax += b * mb.amax_step;
}

template <class E>
__device__ inline void ct_store(const HalfGemmArgs<E>& p, int64_t e, ct_acc_t<E> acc) {
  if (p.Cs) ct_narrow(acc, p.Cs + e);
  else p.C[e] = p.beta ? ct_add(p.C[e], acc) : acc;
}

// ... of an SC instantiation.  sh: exps[sa] + exps[sb], read once per lane (ct_scale_shift); mx: the lane's running max
template <class E>
__device__ inline int ct_scale_shift(const HalfGemmArgs<E>& p) {
  return p.amax ? 0 : p.exps[p.sa] + p.exps[p.sb];
}
template <class E>
__device__ inline void ct_store_scaled(const HalfGemmArgs<E>& p, int64_t e, ct_acc_t<E> acc, int sh, uint32_t& mx) {
  if (p.amax) {
    p.C[e] = acc;
    mx = max(mx, ct_finite_bits(acc));
  } else {
    acc = ct_ldexp(acc, sh);
    p.C[e] = p.beta ? ct_add(p.C[e], acc) : acc;
  }
}
// the lane maxima of a wavefront reduced across its lanes, one atomicMax per wavefront (an integer max: the word does
// not depend on the order the wavefronts arrive in).  Every lane of the wavefront comes here.
__device__ inline void ct_amax_finish(uint32_t* amax, uint32_t mx) {
  if (!amax) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(amax, mx);
}

typedef float ct_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ct_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ct_u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 ct_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ct_bf16x8 __attribute__((ext_vector_type(8)));

// D = A B + C of one 16 x 16 x 32 tile: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15]
// in element j of its fragments, and D[row 4 (l >> 4) + r][col l & 15] in register r
__device__ inline ct_f32x4 ct_mfma(st_f16*, ct_u32x4 a, ct_u32x4 b, ct_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ct_f16x8, a), __builtin_bit_cast(ct_f16x8, b), c, 0, 0, 0);
}
__device__ inline ct_f32x4 ct_mfma(st_bf16*, ct_u32x4 a, ct_u32x4 b, ct_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ct_bf16x8, a), __builtin_bit_cast(ct_bf16x8, b), c, 0, 0, 0);
}

constexpr int HB = 128;  // block tile in m and in n
constexpr int HK = 32;   // k block: one MFMA deep
constexpr int HLD = 20;  // 32-bit words between two rows of an LDS image: 16 of data (32 k) + 4, see the kernel comment

// One operand tile, HB rows (m of A, n of B) x HK k, global -> registers: element (r, k) is G[r sr + k sk].  KC: the
// operand is contiguous along k (sk == 1), else along its rows (sr == 1).  A lane takes two runs of 8 elements along
// the contiguous axis: KC: rows tid / 4 and tid / 4 + 64, k 8 (tid % 4) ...; else: k 2 (tid % 16) and + 1, rows
// 8 (tid / 16) ....  w: the runs as they lie in memory (real: 2 x 4 words, complex: 2 x 8), zeros beyond R and K.
template <class E, bool KC>
__device__ inline void ct_half_fetch(uint32_t (&w)[4 * sizeof(E)], const E* G, int64_t sr, int64_t sk, int64_t r0, int64_t R,
                                     int64_t k0, int64_t K, int vec, int tid) {
  constexpr int NW = 2 * sizeof(E);  // words of a run
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int64_t r = KC ? r0 + tid / 4 + 64 * g : r0 + 8 * (tid / 16);
    const int64_t k = KC ? k0 + 8 * (tid % 4) : k0 + 2 * (tid % 16) + g;
    const int64_t left = KC ? (r < R ? K - k : 0) : (k < K ? R - r : 0);  // elements of the run inside the operand
    const E* src = G + r * sr + k * sk;
    if (vec && left >= 8) {
#pragma unroll
      for (int q = 0; q < NW / 4; ++q) {
        const ct_u32x4 v = ((const ct_u32x4*)src)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[g * NW + 4 * q + j] = v[j];
      }
    } else {
      const uint16_t* s16 = (const uint16_t*)src;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const bool in = j * 4 < left * (int64_t)sizeof(E);  // word j holds elements 2 j, 2 j + 1 (real) or element j
        const bool in_hi = sizeof(E) == 4 ? in : 2 * j + 1 < left;
        const uint32_t lo = in ? s16[2 * j] : 0u, hi = in_hi ? s16[2 * j + 1] : 0u;
        w[g * NW + j] = lo | (hi << 16);
      }
    }
  }
}

// ... registers -> the LDS image(s) [row][k], k contiguous: one plane, or the planes of the real and of the imaginary
// parts.  The runs along rows are transposed here: a word takes the same row at k and k + 1 from the lane's two runs.
template <class E, bool KC>
__device__ inline void ct_half_stash(uint32_t (*img)[HB][HLD], const uint32_t (&w)[4 * sizeof(E)], int tid) {
  constexpr bool CPLX = sizeof(E) == 4;
  if constexpr (KC) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      ct_u32x4 re, im;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (CPLX) {
          const uint32_t e0 = w[8 * g + 2 * j], e1 = w[8 * g + 2 * j + 1];
          re[j] = (e0 & 0xffffu) | (e1 << 16);
          im[j] = (e0 >> 16) | (e1 & 0xffff0000u);
        } else {
          re[j] = w[4 * g + j];
        }
      }
      *(ct_u32x4*)&img[0][tid / 4 + 64 * g][4 * (tid % 4)] = re;
      if constexpr (CPLX) *(ct_u32x4*)&img[1][tid / 4 + 64 * g][4 * (tid % 4)] = im;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (CPLX) {
        const uint32_t e0 = w[j], e1 = w[8 + j];
        img[0][8 * (tid / 16) + j][tid % 16] = (e0 & 0xffffu) | (e1 << 16);
        img[1][8 * (tid / 16) + j][tid % 16] = (e0 >> 16) | (e1 & 0xffff0000u);
      } else {
        const uint32_t e0 = (w[j / 2] >> (16 * (j & 1))) & 0xffffu, e1 = (w[4 + j / 2] >> (16 * (j & 1))) & 0xffffu;
        img[0][8 * (tid / 16) + j][tid % 16] = e0 | (e1 << 16);
      }
    }
  }
}

// C[h] = beta C[h] + A[h] B[h] on the matrix cores: the shape class of ct_gemm_tiled_kernel (M, N >= 64, K > 32).
// S: st_f16 / st_bf16; CPLX: elements are (re, im) pairs; AK, BN: the operand layouts as in ct_gemm_tiled_kernel.
// A block of 4 wavefronts takes a 128 x 128 tile, a wavefront 64 x 64 of it as 4 x 4 MFMA tiles of 16 x 16, k in blocks
// of 32 (one v_mfma_f32_16x16x32 per tile and block).  Both operands are staged as [row][k] images with k contiguous,
// whatever their layout in memory (ct_half_stash transposes the other one), so every fragment is one 16-byte LDS read;
// K tails and edge rows are zeros in LDS.  The next k block's global loads are issued before the MFMAs of this one.
// Complex: real and imaginary planes, four real products per k block in the fixed order re += Ar Br, re += (-Ai) Bi,
// im += Ar Bi, im += Ai Br; -Ai is Ai with the sign bits flipped (exact).  Accumulators are float32; the epilogue rounds
// once to storage for an arena destination, or writes / adds float32 to the output.  No atomics.
// LDS: rows of 80 bytes (64 of data): the 16 rows a 16-byte read takes per quarter wavefront start 20 banks apart, which
// covers the 64 banks once.  The writes of the stage are not free of conflicts: the 16-byte writes of an operand that is
// contiguous along k are 2-way (4 rows x 4 chunks per quarter wavefront; row 3 wraps onto the banks of row 0), and so are
// the 32-bit writes of the transposing stage (a wavefront writes 4 rows 8 apart, 160 words: two pairs of rows share banks).
// One LDS buffer, two barriers per k block; what that costs against the plain tiled kernel is measured, not estimated
// (profiles/contract_timing.txt, the storage leg).  Real: 2 x 128 x 80 B = 20 KiB a block; complex: 40 KiB.  Registers: 64 accumulators real,
// 128 complex, 32 / 80 of fragments, 16 / 32 of staging; the compiler gives about 180 real (two blocks a CU) and about
// 300 complex (one block a CU: a wavefront per SIMD, which 64 MFMAs per k block keep busy), no scratch.
// SC: per-tensor scaling (ct_store_scaled, and the reduction of the lane maxima after the last tile).
template <class S, bool CPLX, bool AK, bool BN, bool SC>
__global__ __launch_bounds__(256) void ct_mfma_tiled_kernel(HalfGemmArgs<typename std::conditional<CPLX, cplx<S>, S>::type> p) {
  using E = typename std::conditional<CPLX, cplx<S>, S>::type;
  constexpr int NP = CPLX ? 2 : 1;
  ct_member(p);
  __shared__ __attribute__((aligned(16))) uint32_t As[NP][HB][HLD];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[NP][HB][HLD];
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int lr = lane & 15, lq = lane >> 4, wm = 64 * (wave / 2), wn = 64 * (wave % 2);
  const int64_t tm = (p.M + HB - 1) / HB, tn = (p.N + HB - 1) / HB;
  [[maybe_unused]] uint32_t mx = 0;
  [[maybe_unused]] int sh = 0;
  if constexpr (SC) sh = ct_scale_shift(p);
  for (int64_t t = blockIdx.x; t < p.H * tm * tn; t += gridDim.x) {
    const int64_t h = t / (tm * tn), m0 = (t / tn % tm) * HB, n0 = t % tn * HB;
    const E* A = p.A + h * p.M * p.K;
    const E* B = p.B + h * p.K * p.N;
    ct_f32x4 acc[NP][4][4];
#pragma unroll
    for (int c = 0; c < NP; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[c][i][j] = ct_f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t wa[4 * sizeof(E)], wb[4 * sizeof(E)];
    ct_half_fetch<E, AK>(wa, A, p.a_m, p.a_k, m0, p.M, 0, p.K, p.a_vec, tid);
    ct_half_fetch<E, !BN>(wb, B, p.b_n, p.b_k, n0, p.N, 0, p.K, p.b_vec, tid);
    for (int64_t k0 = 0; k0 < p.K; k0 += HK) {
      ct_half_stash<E, AK>(As, wa, tid);
      ct_half_stash<E, !BN>(Bs, wb, tid);
      __syncthreads();
      if (k0 + HK < p.K) {
        ct_half_fetch<E, AK>(wa, A, p.a_m, p.a_k, m0, p.M, k0 + HK, p.K, p.a_vec, tid);
        ct_half_fetch<E, !BN>(wb, B, p.b_n, p.b_k, n0, p.N, k0 + HK, p.K, p.b_vec, tid);
      }
      ct_u32x4 a[NP][4], b[NP][4];
#pragma unroll
      for (int c = 0; c < NP; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[c][i] = *(const ct_u32x4*)&As[c][wm + 16 * i + lr][4 * lq];
          b[c][i] = *(const ct_u32x4*)&Bs[c][wn + 16 * i + lr][4 * lq];
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ct_u32x4 a_neg;
        if constexpr (CPLX) a_neg = a[NP - 1][i] ^ 0x80008000u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[0][i][j] = ct_mfma((S*)nullptr, a[0][i], b[0][j], acc[0][i][j]);
          if constexpr (CPLX) {
            acc[0][i][j] = ct_mfma((S*)nullptr, a_neg, b[NP - 1][j], acc[0][i][j]);
            acc[NP - 1][i][j] = ct_mfma((S*)nullptr, a[0][i], b[NP - 1][j], acc[NP - 1][i][j]);
            acc[NP - 1][i][j] = ct_mfma((S*)nullptr, a[NP - 1][i], b[0][j], acc[NP - 1][i][j]);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = m0 + wm + 16 * i + 4 * lq + r, n = n0 + wn + 16 * j + lr;
          if (m < p.M && n < p.N) {
            ct_acc_t<E> v;
            if constexpr (CPLX) v = cplx<float>{acc[0][i][j][r], acc[NP - 1][i][j][r]};
            else v = acc[0][i][j][r];
            if constexpr (SC) ct_store_scaled(p, (h * p.M + m) * p.N + n, v, sh, mx);
            else ct_store(p, (h * p.M + m) * p.N + n, v);
          }
        }
  }
  if constexpr (SC) ct_amax_finish(p.amax, mx);
}

// The narrowing pass of a scaled step whose result goes to the arena: n float32 parts of the staging buffer (a complex
// element is two of them, interleaved there as in storage) -> 16-bit parts at dst, each round(ldexpf(x, -s)) with s the
// rule applied to the step's max word; inf and NaN pass as they are.  Four parts per lane and trip: one 16-byte load,
// one 8-byte store (both buffers start at multiples of 64 elements of the arena); the last n % 4 parts one lane each.
// Thread 0 of block 0 records the result's exponent exps[sc] = exps[sa] + exps[sb] + s; the operands' slots were
// written by earlier kernels of the stream or by the host, nobody else writes sc during this kernel.
// Member b = blockIdx.z of a batched launch (contract.hip, MemberArgs) has stage and dst arena_step bytes, its slots
// exp_step and its max word amax_step entries further on; all three 0 when unbatched.
template <class S, bool CPLX>
__global__ __launch_bounds__(256) void ct_scale_narrow_kernel(const float* stage, S* dst, int64_t numel, const uint32_t* amax,
                                                              int32_t* exps, int sa, int sb, int sc, int64_t arena_step,
                                                              int exp_step, int amax_step) {
  stage = ct_shift(stage, blockIdx.z * arena_step), dst = ct_shift(dst, blockIdx.z * arena_step);
  exps += blockIdx.z * exp_step, amax += blockIdx.z * amax_step;
  const int64_t n = numel * (CPLX ? 2 : 1);
  const int s = ct_scale_exponent(*amax);
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if (first == 0) exps[sc] = exps[sa] + exps[sb] + s;
  for (int64_t q = first; q < n / 4; q += stride) {
    const ct_f32x4 v = ((const ct_f32x4*)stage)[q];
    S r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ct_narrow(ldexpf(v[j], -s), &r[j]);
    ct_u32x2 w;
    w[0] = (uint32_t)r[0].v | ((uint32_t)r[1].v << 16);
    w[1] = (uint32_t)r[2].v | ((uint32_t)r[3].v << 16);
    ((ct_u32x2*)dst)[q] = w;
  }
  for (int64_t e = n / 4 * 4 + first; e < n; e += stride) ct_narrow(ldexpf(stage[e], -s), dst + e);
}
