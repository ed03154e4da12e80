// contract_indirect.h -- step operands read in place through offset tables (tnco_hip_contract_set_indirect); included by
// contract.hip inside its anonymous namespace, after GemmArgs / ct_member / ct_store and the plain GEMM kernels (TB, TK).
// An operand that the plain plan would permute into [h][m][k] / [h][k][n] stays where it lies: its element (h, m, k) is
// at base + offH[h] + offM[m] + offK[k], the three terms separable because h, m and k are disjoint groups of the source's
// axes.  The tables are int64 element offsets in one device pool, validated on the host against the operand's extent
// before any launch.  An operand without tables (null pointers) is direct and is read through its strides as in the
// plain kernels.  Three kernels, each the twin of a plain one, each output element the same products in the same order:
//   ct_ix_tiled_kernel   ct_gemm_tiled_kernel: 64 x 64 x 16 tiles, zeros beyond M, N and K in LDS, kk ascending;
//   ct_ix_dot_kernel     ct_gemm_dot_kernel: 256 partials at stride 256, then the same tree;
//   ct_ix_stream_kernel  ct_gemm_stream_kernel: one lane per output element, k ascending.
// Only the address computation differs, so a run is bit for bit that of the permuted plan.
#pragma once

template <class T>
struct IxGemmArgs {
  const T* A;
  const T* B;
  T* C;
  int64_t a_m, a_k, b_k, b_n;  // strides of a direct operand inside a batch, as in GemmArgs; 0, 0 of a folded one
  int64_t H, M, N, K;
  int beta;  // 1: C += A B, 0: C = A B
  MemberArgs mb;
  const int64_t* a_h;  // folded A: offsets by h, by m and by k; all null: A is direct
  const int64_t* a_mo;
  const int64_t* a_ko;
  const int64_t* b_h;  // folded B: offsets by h, by k and by n; all null: B is direct
  const int64_t* b_ko;
  const int64_t* b_no;
  int a_kfast, b_nfast;  // tiled: consecutive lanes stage consecutive k of A / consecutive n of B (else m / k)
};

// the operands and the result of this block's member (ct_member of GemmArgs)
template <class T>
__device__ inline void ct_ix_member(IxGemmArgs<T>& p) {
  const MemberArgs& mb = p.mb;
  const int64_t b = blockIdx.z;
  p.A = ct_shift(p.A, b * mb.a_step) + (mb.a_ls ? ct_slice_offset(mb.a_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.B = ct_shift(p.B, b * mb.b_step) + (mb.b_ls ? ct_slice_offset(mb.b_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.C = ct_shift(p.C, b * mb.c_step);
}

// where row m of batch h of A starts, and column n of batch h of B; k is added per product (ct_ix_ak, ct_ix_bk)
template <class T>
__device__ inline const T* ct_ix_a(const IxGemmArgs<T>& p, int64_t h, int64_t m) {
  return p.a_h ? p.A + p.a_h[h] + p.a_mo[m] : p.A + h * p.M * p.K + m * p.a_m;
}
template <class T>
__device__ inline const T* ct_ix_b(const IxGemmArgs<T>& p, int64_t h, int64_t n) {
  return p.b_h ? p.B + p.b_h[h] + p.b_no[n] : p.B + h * p.K * p.N + n * p.b_n;
}
template <class T>
__device__ inline int64_t ct_ix_ak(const IxGemmArgs<T>& p, int64_t k) {
  return p.a_ko ? p.a_ko[k] : k * p.a_k;
}
template <class T>
__device__ inline int64_t ct_ix_bk(const IxGemmArgs<T>& p, int64_t k) {
  return p.b_ko ? p.b_ko[k] : k * p.b_k;
}

template <class T>
__device__ inline void ct_ix_store(const IxGemmArgs<T>& p, int64_t e, T acc) {
  p.C[e] = p.beta ? ct_add(p.C[e], acc) : acc;
}

// The tile loop of ct_gemm_tiled_kernel.  How lanes map to the staged elements does not enter the sums; it is chosen per
// operand on the host (a_kfast, b_nfast), uniform over the launch: a folded operand whose source's innermost axis lies in
// its k table (the k table's second entry is the smaller step) is staged with consecutive lanes along k, 16 of them a
// row, otherwise along m (n of B), 64 a row, so that a wavefront reads the longest runs of consecutive addresses the
// source has; a direct operand as the plain kernel stages it (its contiguous axis).  The h offset is uniform per tile and
// read once; the m / n and k offsets are read per staged element, inside the bounds of M, N and K only.
// Registers and LDS (the code objects' metadata, ROCm 7.0, gfx950); no AGPRs, no scratch and no spill in any:
//   float:      116 VGPRs, 4 wavefronts a SIMD, LDS 8320 B a block;
//   double:     139 VGPRs, 3 wavefronts a SIMD, LDS 16640 B;
//   complex64:  146 VGPRs, 3 wavefronts a SIMD, LDS 16640 B;
//   complex128: 238 VGPRs, 2 wavefronts a SIMD, LDS 33280 B.
// The dot twin: 29 VGPRs (complex128: 38), LDS 256 elements; the stream twin: 22 VGPRs (complex128: 28), no LDS; 8
// wavefronts a SIMD and no scratch in all eight.
template <class T>
__global__ __launch_bounds__(256) void ct_ix_tiled_kernel(IxGemmArgs<T> p) {
  ct_ix_member(p);
  __shared__ T As[TK][TB + 1];
  __shared__ T Bs[TK][TB + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int64_t tm = (p.M + TB - 1) / TB, tn = (p.N + TB - 1) / TB;
  for (int64_t t = blockIdx.x; t < p.H * tm * tn; t += gridDim.x) {
    const int64_t h = t / (tm * tn), m0 = (t / tn % tm) * TB, n0 = t % tn * TB;
    const T* A = p.a_h ? p.A + p.a_h[h] : p.A + h * p.M * p.K;
    const T* B = p.b_h ? p.B + p.b_h[h] : p.B + h * p.K * p.N;
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = ct_zero<T>();
    for (int64_t k0 = 0; k0 < p.K; k0 += TK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int ak = p.a_kfast ? e % TK : e / TB, am = p.a_kfast ? e / TK : e % TB;
        const int64_t m = m0 + am, k = k0 + ak;
        T a = ct_zero<T>();
        if (m < p.M && k < p.K) a = p.a_h ? A[p.a_mo[m] + p.a_ko[k]] : A[m * p.a_m + k * p.a_k];
        As[ak][am] = a;
        const int bk = p.b_nfast ? e / TB : e % TK, bn = p.b_nfast ? e % TB : e / TK;
        const int64_t n = n0 + bn, k2 = k0 + bk;
        T b = ct_zero<T>();
        if (n < p.N && k2 < p.K) b = p.b_h ? B[p.b_ko[k2] + p.b_no[n]] : B[k2 * p.b_k + n * p.b_n];
        Bs[bk][bn] = b;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < TK; ++kk) {
        T a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx + 16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = ct_mac(acc[i][j], a[i], b[j]);
      }
      __syncthreads();
    }
    T* Cb = p.C + h * p.M * p.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
        if (m < p.M && n < p.N) {
          T* c = Cb + m * p.N + n;
          *c = p.beta ? ct_add(*c, acc[i][j]) : acc[i][j];
        }
      }
  }
}

// ct_dot_body: one block per output element, 256 partials at stride 256 over k, then the tree
template <class T>
__global__ __launch_bounds__(256) void ct_ix_dot_kernel(IxGemmArgs<T> p) {
  ct_ix_member(p);
  __shared__ T part[256];
  const int tid = threadIdx.x;
  const int64_t total = p.H * p.M * p.N;
  for (int64_t e = blockIdx.x; e < total; e += gridDim.x) {
    const int64_t n = e % p.N, r = e / p.N, m = r % p.M, h = r / p.M;
    const T* a = ct_ix_a(p, h, m);
    const T* b = ct_ix_b(p, h, n);
    T acc = ct_zero<T>();
    for (int64_t k = tid; k < p.K; k += 256) acc = ct_mac(acc, a[ct_ix_ak(p, k)], b[ct_ix_bk(p, k)]);
    part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) part[tid] = ct_add(part[tid], part[tid + w]);
      __syncthreads();
    }
    if (tid == 0) ct_ix_store(p, e, part[0]);
    __syncthreads();
  }
}

// ct_stream_body: one lane per output element (h, m, n), n fastest, k ascending.  I: the integer type of the element
// arithmetic (uint32_t while the result has fewer than 2^31 elements, as ct_rows_stream_kernel splits it)
template <class T, class I>
__device__ inline void ct_ix_stream_body(const IxGemmArgs<T>& p) {
  const I N = (I)p.N, M = (I)p.M, total = (I)(p.H * p.M * p.N);
  const I stride = (I)gridDim.x * (I)blockDim.x;
  const I first = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x;
  const I trips = first < total ? (total - first + stride - 1) / stride : 0;  // (no wrap of e + stride)
  I e = first;
  for (I t = 0; t < trips; ++t, e += stride) {
    const I n = e % N, q = e / N, m = q % M, h = q / M;
    const T* a = ct_ix_a(p, (int64_t)h, (int64_t)m);
    const T* b = ct_ix_b(p, (int64_t)h, (int64_t)n);
    T acc = ct_zero<T>();
    for (int64_t k = 0; k < p.K; ++k) acc = ct_mac(acc, a[ct_ix_ak(p, k)], b[ct_ix_bk(p, k)]);
    ct_ix_store(p, (int64_t)e, acc);
  }
}

template <class T>
__global__ __launch_bounds__(256) void ct_ix_stream_kernel(IxGemmArgs<T> p) {
  ct_ix_member(p);
  if (p.H * p.M * p.N < (int64_t)1 << 31) ct_ix_stream_body<T, uint32_t>(p);
  else ct_ix_stream_body<T, uint64_t>(p);
}
