// contract_matrix.h -- the matrix compute mode of the contraction engine (tnco_hip_contract_set_matrix); included by
// contract.hip inside its anonymous namespace, after GemmArgs / ct_member / ct_store and contract_split.h (ct_f32x4).
// Leaves, arena and output keep their dtype, any of the four; only the tiled shape class (M, N >= 64, K > 32) comes here.
// Nothing is rounded on the way: a real product is one v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, which sums the
// four products of its k depth into the accumulator as an fma chain of the element type, one rounding per product.
//   ct_matrix_tiled_kernel  the geometry of ct_split_tiled_kernel on the operands as they are.
#pragma once

typedef double ct_f64x2 __attribute__((ext_vector_type(2)));
typedef double ct_f64x4 __attribute__((ext_vector_type(4)));

constexpr int MK = 16;  // k block: four MFMAs of depth 4 per tile

// R: the real type of T; NP: parts per element; TI x TJ: the 16 x 16 MFMA tiles of a wavefront (rows x columns); a block
// is 2 x 2 wavefronts; BLOCKS: blocks a compute unit must hold at once (the register budget: 256 a lane with two).
// complex128: a 16 x 16 tile is 16 registers a lane (re and im), so a wavefront takes 2 x 2 of them.  Measured on the
// 4096^3 step: that tile with two blocks a compute unit 55.8 TFLOP/s, 2 x 4 tiles with one block 49.2; complex64 with
// 4 x 2 tiles and two blocks 113.1, no better than the 4 x 4 with one block it has.
template <class T>
struct ct_mx;
template <>
struct ct_mx<float> {
  using R = float;
  using acc_t = ct_f32x4;
  using vec_t = ct_f32x4;  // 16 bytes of R
  static constexpr int NP = 1, TI = 4, TJ = 4, BLOCKS = 2;
};
template <>
struct ct_mx<double> {
  using R = double;
  using acc_t = ct_f64x4;
  using vec_t = ct_f64x2;
  static constexpr int NP = 1, TI = 4, TJ = 4, BLOCKS = 2;
};
template <>
struct ct_mx<cplx<float>> {
  using R = float;
  using acc_t = ct_f32x4;
  using vec_t = ct_f32x4;  // 16 bytes of R
  static constexpr int NP = 2, TI = 4, TJ = 4, BLOCKS = 1;
};
template <>
struct ct_mx<cplx<double>> {
  using R = double;
  using acc_t = ct_f64x4;
  using vec_t = ct_f64x2;
  static constexpr int NP = 2, TI = 2, TJ = 2, BLOCKS = 2;
};

// R elements between two rows of an LDS image: MK of data + 16 bytes (80-byte rows float, 144-byte rows double), so the
// 16 rows a fragment read touches start 20 / 36 words apart and every read of 16 bytes is aligned
template <class R>
constexpr int ct_mx_ld() { return MK + 16 / (int)sizeof(R); }

__device__ inline float ct_mx_part(float x, int) { return x; }
__device__ inline double ct_mx_part(double x, int) { return x; }
template <class R>
__device__ inline R ct_mx_part(cplx<R> x, int c) { return c ? x.im : x.re; }

__device__ inline ct_f32x4 ct_mx_mfma(float a, float b, ct_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ inline ct_f64x4 ct_mx_mfma(double a, double b, ct_f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the row of a 16 x 16 result tile that register r of a lane with quarter q = lane >> 4 holds (the column is lane & 15):
// the float64 instruction interleaves the quarters, the float32 one gives each four consecutive rows
__device__ inline int ct_mx_row(float, int q, int r) { return 4 * q + r; }
__device__ inline int ct_mx_row(double, int q, int r) { return q + 4 * r; }

// four consecutive k of a row, registers -> LDS, in writes of 16 bytes
__device__ inline void ct_mx_put4(float* d, const float (&x)[4]) { *(ct_f32x4*)d = ct_f32x4{x[0], x[1], x[2], x[3]}; }
__device__ inline void ct_mx_put4(double* d, const double (&x)[4]) {
  *(ct_f64x2*)d = ct_f64x2{x[0], x[1]};
  *(ct_f64x2*)(d + 2) = ct_f64x2{x[2], x[3]};
}

// One operand tile, ROWS rows (m of A, n of B) x MK k, global -> registers: element (r, k) is G[r sr + k sk].  A lane
// takes ROWS / 64 groups of 4 elements along the contiguous axis; group g of lane tid is number n = tid + 256 g.
// KC (contiguous along k, sk == 1): row n / 4, k 4 (n % 4) ... + 3; else (sr == 1): rows 4 (n % 8 + 8 (n / 128)) ... + 3,
// k n / 8 % 16 (a wavefront: 8 k x 32 consecutive rows).
template <bool KC>
__device__ inline void ct_mx_group(int n, int& row, int& k) {
  row = KC ? n / 4 : 4 * (n % 8 + 8 * (n / 128));
  k = KC ? 4 * (n % 4) : n / 8 % 16;
}

// w[g][NP j + c]: part c of element j of group g, zeros beyond R and K.  vec: every group that lies inside the operand is
// read with 16-byte loads; else element by element.
template <class T, bool KC, int ROWS>
__device__ inline void ct_mx_fetch(typename ct_mx<T>::R (&w)[ROWS / 64][4 * ct_mx<T>::NP], const T* G, int64_t sr, int64_t sk,
                                   int64_t r0, int64_t R, int64_t k0, int64_t K, bool vec, int tid) {
  using V = typename ct_mx<T>::vec_t;
  constexpr int NP = ct_mx<T>::NP, VN = 16 / (int)sizeof(typename ct_mx<T>::R);
#pragma unroll
  for (int g = 0; g < ROWS / 64; ++g) {
    int row, kk;
    ct_mx_group<KC>(tid + 256 * g, row, kk);
    const int64_t r = r0 + row, k = k0 + kk;
    const int64_t left = KC ? (r < R ? K - k : 0) : (k < K ? R - r : 0);  // elements of the group inside the operand
    const T* src = G + r * sr + k * sk;
    if (vec && left >= 4) {
#pragma unroll
      for (int q = 0; q < 4 * NP / VN; ++q) {
        const V v = ((const V*)src)[q];
#pragma unroll
        for (int e = 0; e < VN; ++e) w[g][VN * q + e] = v[e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T x = j < left ? src[j] : ct_zero<T>();
#pragma unroll
        for (int c = 0; c < NP; ++c) w[g][NP * j + c] = ct_mx_part(x, c);
      }
    }
  }
}

// ... registers -> the LDS images [part][row][k], k contiguous.  KC: a lane writes the 4 consecutive k of its row, 16
// bytes at a time; else: one k of each of its 4 rows, element by element (a wavefront: 8 k of 32 rows).
template <class T, bool KC, int ROWS>
__device__ inline void ct_mx_stash(typename ct_mx<T>::R (*img)[ROWS][ct_mx_ld<typename ct_mx<T>::R>()],
                                   const typename ct_mx<T>::R (&w)[ROWS / 64][4 * ct_mx<T>::NP], int tid) {
  using R = typename ct_mx<T>::R;
  constexpr int NP = ct_mx<T>::NP;
#pragma unroll
  for (int g = 0; g < ROWS / 64; ++g) {
    int row, kk;
    ct_mx_group<KC>(tid + 256 * g, row, kk);
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      if constexpr (KC) {
        const R x[4] = {w[g][c], w[g][NP + c], w[g][2 * NP + c], w[g][3 * NP + c]};
        ct_mx_put4(&img[c][row][kk], x);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) img[c][row + j][kk] = w[g][NP * j + c];
      }
    }
  }
}

// C[h] = beta C[h] + A[h] B[h] on the matrix cores in the precision of T (float, double, cplx<float>, cplx<double>).
// AK, BN: the operand layouts as in ct_gemm_tiled_kernel.
// Geometry: a block of 4 wavefronts (2 x 2) takes a tile of 32 TI x 32 TJ (128 x 128; complex128 64 x 64), a wavefront
// TI x TJ MFMA tiles of 16 x 16; k in blocks of MK = 16; [part][row][k] LDS images, k contiguous, with the padded pitch of
// ct_mx_ld; K tails and edge rows are zeros in LDS; the next k block's global loads are issued before the MFMAs of this
// one; one LDS buffer, two barriers per k block; blockIdx.z is the member of a slice batch (ct_member).
// Fragments: the instruction wants one scalar per lane, A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15].  The sum
// over k does not care which k a lane holds as long as A and B agree: a lane with quarter q = l >> 4 reads k 4 q ...
// 4 q + 3 of its row of a k block, 16 bytes at a time (all four float, two and then the other two double), and feeds
// element j to MFMA j of the k block, A and B alike.  MFMA j therefore sums k = j, 4 + j, 8 + j, 12 + j.
// Order of the sums into one accumulator: k blocks ascending; in a k block of 16 the offsets
//   0, 4, 8, 12,  1, 5, 9, 13,  2, 6, 10, 14,  3, 7, 11, 15
// (MFMA 0 ... 3, each an fma chain over its four k in ascending order); complex, at every MFMA j: the real part takes
// Ar Br and then (-Ai) Bi, the imaginary part Ar Bi and then Ai Br (four real MFMAs; -Ai is Ai with the sign bit
// flipped, exact).  The result is stored unrounded (ct_store).  No atomics: a call is bit-reproducible.
// The float64 result tile has its own lane-to-row map (ct_mx_row).
// Registers and LDS (hipcc -Rpass-analysis=kernel-resource-usage, ROCm 7.0, gfx950), over the four layouts of a type; no
// scratch and no spill in any of the 16:
//   float:      150 to 164 VGPRs, no AGPRs, 3 wavefronts a SIMD, LDS 20 KiB a block;
//   double:     242 to 248 VGPRs, no AGPRs, 2 wavefronts a SIMD, LDS 36 KiB;
//   complex64:  170 to 180 VGPRs + 128 AGPRs (the accumulators), 1 wavefront a SIMD, LDS 40 KiB;
//   complex128: 196 to 204 VGPRs, no AGPRs, 2 wavefronts a SIMD, LDS 36 KiB.
// Measured on an MI355X, the 4096^3 step (profiles/contract_timing.txt): 87.6, 56.0, 113.6 and 55.8 TFLOP/s.
template <class T, bool AK, bool BN>
__global__ __launch_bounds__(256, ct_mx<T>::BLOCKS) void ct_matrix_tiled_kernel(GemmArgs<T> p) {
  using X = ct_mx<T>;
  using R = typename X::R;
  using V = typename X::vec_t;
  using acc_t = typename X::acc_t;
  constexpr int NP = X::NP, TI = X::TI, TJ = X::TJ, BM = 32 * TI, BNN = 32 * TJ, LD = ct_mx_ld<R>();
  constexpr int VN = 16 / (int)sizeof(R);
  ct_member(p);
  __shared__ __attribute__((aligned(16))) R As[NP][BM][LD];
  __shared__ __attribute__((aligned(16))) R Bs[NP][BNN][LD];
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int lr = lane & 15, lq = lane >> 4, wm = 16 * TI * (wave / 2), wn = 16 * TJ * (wave % 2);
  const int64_t tm = (p.M + BM - 1) / BM, tn = (p.N + BNN - 1) / BNN;
  // 16-byte loads: the member's base and the operand's leading stride (which divides the batch stride) aligned
  const bool a_vec = (uintptr_t)p.A % 16 == 0 && (AK ? p.a_m : p.a_k) * sizeof(T) % 16 == 0;
  const bool b_vec = (uintptr_t)p.B % 16 == 0 && (BN ? p.b_k : p.b_n) * sizeof(T) % 16 == 0;
  for (int64_t t = blockIdx.x; t < p.H * tm * tn; t += gridDim.x) {
    const int64_t h = t / (tm * tn), m0 = (t / tn % tm) * BM, n0 = t % tn * BNN;
    const T* A = p.A + h * p.M * p.K;
    const T* B = p.B + h * p.K * p.N;
    acc_t acc[NP][TJ][TI];  // [part][column tile j][row tile i]
#pragma unroll
    for (int c = 0; c < NP; ++c)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int i = 0; i < TI; ++i) acc[c][j][i] = acc_t{R(0), R(0), R(0), R(0)};
    R wa[BM / 64][4 * NP], wb[BNN / 64][4 * NP];
    ct_mx_fetch<T, AK, BM>(wa, A, p.a_m, p.a_k, m0, p.M, 0, p.K, a_vec, tid);
    ct_mx_fetch<T, !BN, BNN>(wb, B, p.b_n, p.b_k, n0, p.N, 0, p.K, b_vec, tid);
    for (int64_t k0 = 0; k0 < p.K; k0 += MK) {
      ct_mx_stash<T, AK, BM>(As, wa, tid);
      ct_mx_stash<T, !BN, BNN>(Bs, wb, tid);
      __syncthreads();
      if (k0 + MK < p.K) {
        ct_mx_fetch<T, AK, BM>(wa, A, p.a_m, p.a_k, m0, p.M, k0 + MK, p.K, a_vec, tid);
        ct_mx_fetch<T, !BN, BNN>(wb, B, p.b_n, p.b_k, n0, p.N, k0 + MK, p.K, b_vec, tid);
      }
      // one read of 16 bytes per fragment at a time: all four k of a lane (float), or two and then the other two (double)
#pragma unroll
      for (int rd = 0; rd < 4 / VN; ++rd) {
        V a[NP][TI];
#pragma unroll
        for (int c = 0; c < NP; ++c)
#pragma unroll
          for (int i = 0; i < TI; ++i) a[c][i] = *(const V*)&As[c][wm + 16 * i + lr][4 * lq + VN * rd];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          V b[NP];
#pragma unroll
          for (int c = 0; c < NP; ++c) b[c] = *(const V*)&Bs[c][wn + 16 * j + lr][4 * lq + VN * rd];
#pragma unroll
          for (int e = 0; e < VN; ++e) {
#pragma unroll
            for (int i = 0; i < TI; ++i) acc[0][j][i] = ct_mx_mfma(a[0][i][e], b[0][e], acc[0][j][i]);
            if constexpr (NP == 2) {
#pragma unroll
              for (int i = 0; i < TI; ++i) acc[NP - 1][j][i] = ct_mx_mfma(a[0][i][e], b[NP - 1][e], acc[NP - 1][j][i]);
#pragma unroll
              for (int i = 0; i < TI; ++i) acc[0][j][i] = ct_mx_mfma(-a[NP - 1][i][e], b[NP - 1][e], acc[0][j][i]);
#pragma unroll
              for (int i = 0; i < TI; ++i) acc[NP - 1][j][i] = ct_mx_mfma(a[NP - 1][i][e], b[0][e], acc[NP - 1][j][i]);
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = m0 + wm + 16 * i + ct_mx_row(R(0), lq, r), n = n0 + wn + 16 * j + lr;
          if (m < p.M && n < p.N) {
            T v;
            if constexpr (NP == 2) v = T{acc[0][j][i][r], acc[NP - 1][j][i][r]};
            else v = acc[0][j][i][r];
            ct_store(p, (h * p.M + m) * p.N + n, v);
          }
        }
  }
}
