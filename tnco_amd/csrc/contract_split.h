// contract_split.h -- the split-bfloat16 compute mode of the contraction engine (tnco_hip_contract_set_compute, mode 1);
// included by contract.hip inside its anonymous namespace, after GemmArgs / ct_member / ct_store and contract_half.h
// (st_bf16, ct_narrow, ct_widen, the fragment types, HB / HK / HLD).
// Leaves, arena and output stay float32 / complex64; only the tiled shape class (M, N >= 64, K > 32) comes here.  Every
// float32 part x of an operand is split as it is staged into LDS:
//   hi = bf16(x), to nearest even;  lo = bf16(x - hi), the subtraction exact in float32;  lo = 0 where hi is not finite,
// and a product a b is summed as a_lo b_hi + a_hi b_lo + a_hi b_hi, in that order (the small terms first), each one
// v_mfma_f32_16x16x32_bf16 into the float32 accumulators; a_lo b_lo is dropped (at most 2^-16 |a| |b|).
//   ct_split_tiled_kernel  the geometry of ct_mfma_tiled_kernel with hi and lo planes per operand.
#pragma once

typedef float ct_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ct_bf16x2 __attribute__((ext_vector_type(2)));

// two float32 -> two bfloat16 in one word (x0 in the low half), to nearest even: the packed convert of gfx950 where
// the compiler has it.  ct_narrow(float, st_bf16*) is the specification: the same value for every input that is not
// NaN, and a NaN stays a NaN
__device__ inline uint32_t ct_bf16_pair(float x0, float x1) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(ct_f32x2{x0, x1}, ct_bf16x2));
}

// (hi, lo) of two parts, packed as ct_bf16_pair packs them
__device__ inline void ct_split_pair(float x0, float x1, uint32_t& hi, uint32_t& lo) {
  hi = ct_bf16_pair(x0, x1);
  const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
  const float r0 = (hi & 0x7f80u) != 0x7f80u ? x0 - h0 : 0.f;
  const float r1 = (hi & 0x7f800000u) != 0x7f800000u ? x1 - h1 : 0.f;
  lo = ct_bf16_pair(r0, r1);
}

// One operand tile, HB rows (m of A, n of B) x HK k, global -> registers: element (r, k) is G[r sr + k sk].  A lane takes
// four groups of 4 elements along the contiguous axis.  KC (contiguous along k, sk == 1): group g is row tid / 8 + 32 g,
// k 4 (tid % 8) ... + 3; else (sr == 1): group g is k 4 (tid % 8) + g, rows 4 (tid / 8) ... + 3.  w[g][j]: element j of
// group g, zeros beyond R and K.  vec: every group that lies inside the operand is read with 16-byte loads (one per
// group real, two complex); else element by element.
template <class T, bool KC>
__device__ inline void ct_split_fetch(T (&w)[4][4], const T* G, int64_t sr, int64_t sk, int64_t r0, int64_t R, int64_t k0,
                                      int64_t K, bool vec, int tid) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t r = KC ? r0 + tid / 8 + 32 * g : r0 + 4 * (tid / 8);
    const int64_t k = KC ? k0 + 4 * (tid % 8) : k0 + 4 * (tid % 8) + g;
    const int64_t left = KC ? (r < R ? K - k : 0) : (k < K ? R - r : 0);  // elements of the group inside the operand
    const T* src = G + r * sr + k * sk;
    if (vec && left >= 4) {
      ct_f32x4 v[sizeof(T) / 4];
#pragma unroll
      for (int q = 0; q < (int)(sizeof(T) / 4); ++q) v[q] = ((const ct_f32x4*)src)[q];
      __builtin_memcpy(&w[g][0], v, sizeof(v));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[g][j] = j < left ? src[j] : ct_zero<T>();
    }
  }
}

__device__ inline float ct_part(float x, int) { return x; }
__device__ inline float ct_part(cplx<float> x, int c) { return c ? x.im : x.re; }

// ... registers -> the LDS images [row][k], k contiguous: plane 2 c + s holds part c (0 re, 1 im) and s = 0 hi, 1 lo.
// A lane writes 4 consecutive k of a row, 8 bytes, per plane: KC: of its four rows; else: of its rows 4 (tid / 8) + j,
// the k taken across its four groups (the transpose).  A quarter wavefront writes two rows (rows 4 apart when
// transposing: 80 words, 16 banks on) x 8 chunks of 2 words: the 32 banks once when transposing, two chunks of the second
// row on the banks of the first otherwise.
template <class T, bool KC>
__device__ inline void ct_split_stash(uint32_t (*img)[HB][HLD], const T (&w)[4][4], int tid) {
  constexpr int NP = sizeof(T) / 4;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      ct_u32x2 hi, lo;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float x0 = KC ? ct_part(w[q][2 * e], c) : ct_part(w[2 * e][q], c);
        const float x1 = KC ? ct_part(w[q][2 * e + 1], c) : ct_part(w[2 * e + 1][q], c);
        uint32_t h, l;
        ct_split_pair(x0, x1, h, l);
        hi[e] = h, lo[e] = l;
      }
      const int row = KC ? tid / 8 + 32 * q : 4 * (tid / 8) + q;
      *(ct_u32x2*)&img[2 * c][row][2 * (tid % 8)] = hi;
      *(ct_u32x2*)&img[2 * c + 1][row][2 * (tid % 8)] = lo;
    }
}

__device__ inline ct_f32x4 ct_mfma_bf16(ct_u32x4 a, ct_u32x4 b, ct_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ct_bf16x8, a), __builtin_bit_cast(ct_bf16x8, b), c, 0, 0, 0);
}

// acc[i] += a[i] b for the four row tiles of a column, as lo hi, hi lo, hi hi: a, b index 0 hi, 1 lo
__device__ inline void ct_split_mac(ct_f32x4 (&acc)[4], const ct_u32x4 (&a_hi)[4], const ct_u32x4 (&a_lo)[4], ct_u32x4 b_hi,
                                    ct_u32x4 b_lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = ct_mfma_bf16(a_lo[i], b_hi, acc[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = ct_mfma_bf16(a_hi[i], b_lo, acc[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = ct_mfma_bf16(a_hi[i], b_hi, acc[i]);
}

// C[h] = beta C[h] + A[h] B[h] in float32 / complex64 on the matrix cores, every product as three bfloat16 products (the
// head of this file).  CPLX: elements are (re, im) pairs; AK, BN: the operand layouts as in ct_gemm_tiled_kernel.
// Geometry of ct_mfma_tiled_kernel (contract_half.h): a block of 4 wavefronts takes a 128 x 128 tile, a wavefront 64 x 64
// of it as 4 x 4 MFMA tiles, k in blocks of 32; [row][k] LDS images with the 80-byte row pitch, so every fragment is one
// 16-byte LDS read; K tails and edge rows are zeros in LDS; the next k block's global loads are issued before the MFMAs
// of this one; one LDS buffer, two barriers per k block; blockIdx.z is the member of a slice batch (ct_member).
// LDS: a hi and a lo plane per operand and part: 4 x 128 x 80 B = 40 KiB a block real, 80 KiB complex.
// Per k block a wavefront keeps the A fragments of its four row tiles (hi and lo of every part) and reads the B
// fragments of one column of tiles at a time.  Order of the sums into an accumulator, per k block: real: a_lo b_hi,
// a_hi b_lo, a_hi b_hi; complex: re += Ar Br (those three), re += (-Ai) Bi (those three), im += Ar Bi, im += Ai Br; -Ai is
// hi and lo of Ai with the sign bits flipped (exact: rounding to nearest even is symmetric).  3 MFMAs per tile and k
// block real, 12 complex.  The result is stored unrounded (ct_store: beta in float32).  No atomics.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ROCm 7.0, gfx950), the four layouts alike:
//   real:    125 to 154 VGPRs + 64 AGPRs (the accumulators), no scratch, 2 wavefronts a SIMD (two blocks a CU);
//   complex: 230 to 254 VGPRs + 128 AGPRs, no scratch, 1 wavefront a SIMD (one block a CU, which 192 MFMAs per k
//            block and wavefront keep busy).
// The conversions compile to v_cvt_pk_bf16_f32.
template <bool CPLX, bool AK, bool BN>
__global__ __launch_bounds__(256) void ct_split_tiled_kernel(GemmArgs<typename std::conditional<CPLX, cplx<float>, float>::type> p) {
  using T = typename std::conditional<CPLX, cplx<float>, float>::type;
  constexpr int NP = CPLX ? 2 : 1;
  ct_member(p);
  __shared__ __attribute__((aligned(16))) uint32_t As[2 * NP][HB][HLD];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[2 * NP][HB][HLD];
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int lr = lane & 15, lq = lane >> 4, wm = 64 * (wave / 2), wn = 64 * (wave % 2);
  const int64_t tm = (p.M + HB - 1) / HB, tn = (p.N + HB - 1) / HB;
  // 16-byte loads: the member's base and the operand's leading stride (which divides the batch stride) aligned
  const bool a_vec = (uintptr_t)p.A % 16 == 0 && (AK ? p.a_m : p.a_k) * sizeof(T) % 16 == 0;
  const bool b_vec = (uintptr_t)p.B % 16 == 0 && (BN ? p.b_k : p.b_n) * sizeof(T) % 16 == 0;
  for (int64_t t = blockIdx.x; t < p.H * tm * tn; t += gridDim.x) {
    const int64_t h = t / (tm * tn), m0 = (t / tn % tm) * HB, n0 = t % tn * HB;
    const T* A = p.A + h * p.M * p.K;
    const T* B = p.B + h * p.K * p.N;
    ct_f32x4 acc[NP][4][4];  // [part][column tile j][row tile i]
#pragma unroll
    for (int c = 0; c < NP; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[c][j][i] = ct_f32x4{0.f, 0.f, 0.f, 0.f};
    T wa[4][4], wb[4][4];
    ct_split_fetch<T, AK>(wa, A, p.a_m, p.a_k, m0, p.M, 0, p.K, a_vec, tid);
    ct_split_fetch<T, !BN>(wb, B, p.b_n, p.b_k, n0, p.N, 0, p.K, b_vec, tid);
    for (int64_t k0 = 0; k0 < p.K; k0 += HK) {
      ct_split_stash<T, AK>(As, wa, tid);
      ct_split_stash<T, !BN>(Bs, wb, tid);
      __syncthreads();
      if (k0 + HK < p.K) {
        ct_split_fetch<T, AK>(wa, A, p.a_m, p.a_k, m0, p.M, k0 + HK, p.K, a_vec, tid);
        ct_split_fetch<T, !BN>(wb, B, p.b_n, p.b_k, n0, p.N, k0 + HK, p.K, b_vec, tid);
      }
      ct_u32x4 a[2 * NP][4];
#pragma unroll
      for (int s = 0; s < 2 * NP; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[s][i] = *(const ct_u32x4*)&As[s][wm + 16 * i + lr][4 * lq];
      [[maybe_unused]] ct_u32x4 a_neg[2][4];
      if constexpr (CPLX) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int i = 0; i < 4; ++i) a_neg[s][i] = a[2 + s][i] ^ 0x80008000u;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ct_u32x4 b[2 * NP];
#pragma unroll
        for (int s = 0; s < 2 * NP; ++s) b[s] = *(const ct_u32x4*)&Bs[s][wn + 16 * j + lr][4 * lq];
        ct_split_mac(acc[0][j], a[0], a[1], b[0], b[1]);
        if constexpr (CPLX) {
          ct_split_mac(acc[0][j], a_neg[0], a_neg[1], b[2], b[3]);
          ct_split_mac(acc[NP - 1][j], a[0], a[1], b[2], b[3]);
          ct_split_mac(acc[NP - 1][j], a[2], a[3], b[0], b[1]);
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
            T v;
            if constexpr (CPLX) v = cplx<float>{acc[0][j][i][r], acc[NP - 1][j][i][r]};
            else v = acc[0][j][i][r];
            ct_store(p, (h * p.M + m) * p.N + n, v);
          }
        }
  }
}
