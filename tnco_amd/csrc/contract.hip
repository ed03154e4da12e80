// contract.hip -- sliced pairwise contraction of arrays (include/tnco_hip.h, tnco_hip_contract_*).
// The plan comes from tnco_amd/contraction.py as flat tables; here: its validation, device memory, and the slice loop
// x step loop on one stream.  Kernels, each templated over float / double / complex<float> / complex<double>:
//   ct_gather_kernel       strided gather with a per-assignment base offset: slicing + permuting of every leaf of an
//                          assignment in one launch (one row of the table per grid row), permutes of intermediates;
//   ct_gemm_tiled_kernel   C[h] = beta C[h] + A[h] B[h] through LDS, 64 x 64 tiles, 4 x 4 per lane: M, N, K large;
//   ct_gemm_stream_kernel  one lane per output element: skinny steps (K or N small, outer products), memory-bound;
//   ct_gemm_dot_kernel     one block per output element, K split over the block: few outputs, long K;
//   ct_rows_tiled_kernel, ct_rows_stream_kernel, ct_rows_dot_kernel
//                          the same three with a row axis outermost (the distinct projections of the sparse indices a
//                          tensor holds): Z[r][h] = X[a_map[r]][h] Y[b_map[r]][h], the operand rows taken through int32
//                          maps (tnco_hip.h, row_steps).  Steps without a row axis do not come here.
// Storage mode (dtype codes 4..7, contract_half.h): leaves and intermediates in float16 / bfloat16, sums in float32; its
// tiled class runs on the matrix cores (ct_mfma_tiled_kernel), dot, stream and gather are the bodies below with a
// widening load.  Steps with a row axis do not come there.  With per-tensor scaling (contract_half.h) a stored result
// passes through a float32 staging buffer of the arena and ct_scale_narrow_kernel.
// Compute mode bf16x3 (tnco_hip_contract_set_compute, contract_split.h): float32 / complex64 plans keep their storage and
// run the tiled class on the matrix cores, every product as three bfloat16 products (ct_split_tiled_kernel); every other
// kernel is the one of the plain mode.
// Matrix mode (tnco_hip_contract_set_matrix, contract_matrix.h): plans of the four plain dtypes keep their storage and run
// the tiled class on the matrix cores in the element type's own precision (ct_matrix_tiled_kernel: v_mfma_f32_16x16x4_f32
// / v_mfma_f64_16x16x4_f64, nothing rounded on the way, the sums in another order than ct_gemm_tiled_kernel); every other
// kernel is the one of the plain mode.
// Slice batches (tnco_hip_contract_set_slice_batch): B consecutive assignments per launch.  Every kernel of the slice
// loop has a member axis, blockIdx.z = b for assignment sid0 + b (MemberArgs): member b works in its own copy of the arena
// (and of the exponent slots and max words), reads a leaf in place at the slice offset of its own assignment, computed on
// the device from the tables, and is mapped to lanes, tiles and k order as an unbatched launch is.  The last step writes
// the members' blocks to a staging buffer [B][block] and
//   ct_batch_reduce_kernel folds them into the output, one lane per element, the members in assignment order,
// so the sum over assignments keeps its order and a batched run is bit-equal to the unbatched one.  An unbatched launch
// is the same kernel with one member and every member stride 0.
// Path kernel (tnco_hip_contract_set_path_kernel, contract_path.h): a group of up to 1024 assignments per launch, one
// workgroup per assignment interpreting the whole path in its own copy of the arena (ct_path_kernel), and
//   ct_path_reduce_kernel  folds the group's blocks into the output as ct_batch_reduce_kernel does;
// two launches per group, the sums in the order of the unfused kernels: bit-equal to the loop above.
// The schedule (Schedule, make_schedule): every step and permute has a period and is due at assignment a iff a is the first
// of the run or a % period == 0; the slice loop runs the phases (the items of one period) that are due, the slowest first.
// Every period 1: the plain loop.  Reuse periods (tnco_hip_contract_set_reuse): the plan's.  Hoisting
// (tnco_hip_contract_set_hoist): the steps and permutes the plan flags -- their operands hold no sliced axis anywhere
// below them -- have the period that is due once per run, as one-member launches of the same kernels; a step of period 1
// reads what they left (a kept tensor) in arena copy 0.  No kernel knows of it.
// Indirect operands (tnco_hip_contract_set_indirect, contract_indirect.h): a step operand that the plan folded is read
// where it lies, element (h, m, k) at base + offH[h] + offM[m] + offK[k] through three int64 tables, by
//   ct_ix_tiled_kernel, ct_ix_dot_kernel, ct_ix_stream_kernel
//                          the twins of the three plain GEMM kernels, the same sums in the same order; its permute, the
//                          launch and the arena buffer of the copy are not in the plan.  Plain dtypes only.
// Wide accumulation (tnco_hip_contract_set_accumulate, contract_accumulate.h; float32 / complex64 outputs): the step that
// writes the output always writes with beta 0 to a staging block (unbatched: one of its own) and the fold goes into a
// float64 / complex128 accumulator, placed or added in assignment order by
//   ct_acc_reduce_kernel, ct_acc_path_reduce_kernel  the twins of the two reduce kernels, and
//   ct_acc_narrow_kernel   rounds the accumulator into the output once, after the last assignment.
// Every other kernel, shape, k order and block is that of the run without the call.
// Resident use (tnco_hip_contract_load_leaf, tnco_hip_contract_run_loaded; contract_io.h): a run is "load every leaf, then
// run what is loaded", and the halves are entry points of their own; a leaf or the result may lie in a caller's device
// memory, which only
//   ct_ingest_kernel, ct_emit_kernel  ever touch (a caller's pointer may belong to another HIP runtime in the process).
// Leaf sets (tnco_hip_contract_load_leaf_sets, tnco_hip_contract_run_sets; contract_sets.h): on a handle with a path
// kernel a member of a launch is a pair (leaf set, assignment); a leaf that differs between the sets lies in a stack
// [n_sets][leaf_numel] of the handle's own, and
//   ct_sets_path_kernel, ct_sets_reduce_kernel  the twins of the two path kernels
// leave the output of every set in [n_sets][out_numel], each bit-equal to a run of that set alone.
// Walkers (tnco_hip_walkers_*, tnco_hip_contract_load_leaf_versions, tnco_hip_contract_run_walkers; contract_walk.h): the
// sets are the walkers of a circuit sampler, whose bits lie in a table on the device; a leaf with two versions is read
// at the version the walker's bit of one qubit picks, and the versions stay loaded from run to run:
//   ct_walk_path_kernel    ct_sets_path_kernel with the indexed leaves; ct_sets_reduce_kernel folds its blocks;
//   ct_walk_choose_kernel, ct_walk_permute_kernel  the new bit of a qubit from the two amplitudes and a Philox draw; a
//                          classical gate on up to 8 qubits;
//   ct_walk_choose_joint_kernel  the new bits of up to 6 qubits, drawn jointly from the 2^k amplitudes.
// No atomics in any sum: every sum runs in one fixed order, so a run is bit-reproducible (the one atomic, the integer max
// behind a scaled tensor's exponent, does not depend on order).
#include "../../include/tnco_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <functional>
#include <iterator>
#include <string>
#include <type_traits>
#include <vector>

namespace tnco {
int set_error(int code, const std::string& msg);
}

namespace {

#include "contract_tables.h"

int fail(int code, const std::string& msg) { return tnco::set_error(code, msg); }

#define CT_TRY(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(TNCO_HIP_ERUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class R>
struct cplx {
  R re, im;
};

// multiply-add and zero of each element type (a complex MAC: 4 real FMAs)
__device__ inline float ct_zero(float*) { return 0.f; }
__device__ inline double ct_zero(double*) { return 0.0; }
template <class R>
__device__ inline cplx<R> ct_zero(cplx<R>*) { return cplx<R>{R(0), R(0)}; }
__device__ inline float ct_mac(float c, float a, float b) { return fmaf(a, b, c); }
__device__ inline double ct_mac(double c, double a, double b) { return fma(a, b, c); }
template <class R>
__device__ inline cplx<R> ct_mac(cplx<R> c, cplx<R> a, cplx<R> b) {
  c.re = fma(a.re, b.re, c.re);
  c.re = fma(-a.im, b.im, c.re);
  c.im = fma(a.re, b.im, c.im);
  c.im = fma(a.im, b.re, c.im);
  return c;
}
__device__ inline float ct_add(float a, float b) { return a + b; }
__device__ inline double ct_add(double a, double b) { return a + b; }
template <class R>
__device__ inline cplx<R> ct_add(cplx<R> a, cplx<R> b) { return cplx<R>{a.re + b.re, a.im + b.im}; }
template <class T>
__device__ inline T ct_zero() { return ct_zero((T*)nullptr); }

// the type an element is summed in: itself; contract_half.h adds the 16-bit storage types, summed in float32, and their
// ct_widen
template <class E>
struct ct_acc {
  using type = E;
};
template <class E>
using ct_acc_t = typename ct_acc<E>::type;

// the offset that assignment sid gives a leaf through its sliced axes (ls: the leaf's row of leaf_sl)
__host__ __device__ inline int64_t ct_slice_offset(const int64_t* ls, const int64_t* place, const int64_t* dims, int64_t sid) {
  int64_t off = 0;
  for (int j = 0; j < (int)ls[LS_COUNT]; ++j) {
    const int64_t s = ls[LS_SLOTS + j];
    off += ((sid / place[s]) % dims[s]) * ls[LS_STRIDES + j];
  }
  return off;
}

// The member axis of a GEMM launch: block z is member b = blockIdx.z, assignment sid0 + b.  Steps are in bytes between
// two members' A, B, C (a copy of the arena, a block of the batch staging, 0 for a leaf); a leaf read in place comes
// without a slice offset and with its row of leaf_sl, and the member adds the offset of its assignment.  All zero: an
// unbatched launch, the operands as the host resolved them.
struct MemberArgs {
  const int64_t* a_ls;
  const int64_t* b_ls;
  const int64_t* slice_place;
  const int64_t* slice_dims;
  int64_t sid0;
  int64_t a_step, b_step, c_step;
  int exp_step, amax_step;  // exponent slots / max words between two members (scaling)
};

template <class X>
__device__ inline X* ct_shift(X* p, int64_t bytes) {
  return (X*)((const char*)p + bytes);
}

#include "contract_half.h"

template <class E>
__device__ inline ct_acc_t<E> ct_load(const E* p) {
  if constexpr (std::is_same<ct_acc_t<E>, E>::value) return *p;
  else return ct_widen(*p);
}

struct GatherArgs {
  const int64_t* rows;         // the rows of this launch
  const int64_t* leaf_sl;      // [n_leaves][LEAF_SL_W]
  const int64_t* slice_place;  // place value of every slice position
  const int64_t* slice_dims;
  const void* const* leaves;
  void* arena;
  void* out;
  int64_t sid;      // the assignment (of member 0)
  int64_t out_off;  // its block of the output
  int64_t arena_step;  // elements between two members' arenas (member b = blockIdx.z: assignment sid + b), 0 unbatched
};

// D: the element as it is written, SI: as it is read (another type only where storage is widened into the output)
// SC: the source is widened and scaled by its exponent, exps[leaf] (a scaled plan without steps: its single leaf)
template <class D, class SI, bool SC = false>
__device__ inline void ct_gather_body(const GatherArgs& g, const int32_t* exps = nullptr) {
  const int64_t* row = g.rows + (int64_t)blockIdx.y * PERM_W;
  const int64_t numel = row[PM_NUMEL];
  const int nd = (int)row[PM_NDIM];
  const SI* src;
  int64_t base = 0;
  const int64_t member = (int64_t)blockIdx.z * g.arena_step;
  if (row[PM_SRC_KIND] == K_LEAF) {
    base = ct_slice_offset(g.leaf_sl + row[PM_SRC_REF] * LEAF_SL_W, g.slice_place, g.slice_dims, g.sid + blockIdx.z);
    src = (const SI*)g.leaves[row[PM_SRC_REF]];
  } else {
    src = (const SI*)g.arena + member + row[PM_SRC_REF];
  }
  D* dst = row[PM_DST_KIND] == K_ARENA ? (D*)g.arena + member + row[PM_DST_REF] : (D*)g.out + g.out_off;
  [[maybe_unused]] int sh = 0;
  if constexpr (SC) sh = row[PM_SRC_KIND] == K_LEAF ? exps[row[PM_SRC_REF]] : 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t rem = e, off = base;
    for (int k = nd - 1; k >= 0; --k) {
      const int64_t d = row[PM_DIMS + k], q = rem / d;
      off += (rem - q * d) * row[PM_STRIDES + k];
      rem = q;
    }
    if constexpr (SC) dst[e] = ct_ldexp(ct_load(src + off), sh);
    else dst[e] = ct_load(src + off);
  }
}

template <class T>
__global__ __launch_bounds__(256) void ct_gather_kernel(GatherArgs g) {
  ct_gather_body<T, T>(g);
}

// the gathers of storage mode: D = SI = uint16_t / uint32_t moves real elements / (re, im) pairs as they are; the single
// leaf of a plan without steps is widened into the float32 output (SI the storage element, D float / cplx<float>)
template <class D, class SI>
__global__ __launch_bounds__(256) void ct_half_gather_kernel(GatherArgs g) {
  ct_gather_body<D, SI>(g);
}
template <class D, class SI>
__global__ __launch_bounds__(256) void ct_half_gather_scaled_kernel(GatherArgs g, const int32_t* exps) {
  ct_gather_body<D, SI, true>(g, exps);
}

template <class T>
struct GemmArgs {
  const T* A;
  const T* B;
  T* C;
  int64_t a_m, a_k, b_k, b_n;  // strides inside a batch; batches are dense: M K, K N, M N
  int64_t H, M, N, K;
  int beta;  // 1: C += A B, 0: C = A B
  MemberArgs mb;
};

// the operands and the result of this block's member
template <class T>
__device__ inline void ct_member(GemmArgs<T>& p) {
  const MemberArgs& mb = p.mb;
  const int64_t b = blockIdx.z;
  p.A = ct_shift(p.A, b * mb.a_step) + (mb.a_ls ? ct_slice_offset(mb.a_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.B = ct_shift(p.B, b * mb.b_step) + (mb.b_ls ? ct_slice_offset(mb.b_ls, mb.slice_place, mb.slice_dims, mb.sid0 + b) : 0);
  p.C = ct_shift(p.C, b * mb.c_step);
}

template <class T>
__device__ inline void ct_store(const GemmArgs<T>& p, int64_t e, T acc) {
  p.C[e] = p.beta ? ct_add(p.C[e], acc) : acc;
}

#include "contract_split.h"
#include "contract_matrix.h"

constexpr int TB = 64, TK = 16;

// AK: A contiguous along k (A[h][m][k]), else along m; BN: B contiguous along n (B[h][k][n]), else along k
template <class T, bool AK, bool BN>
__global__ __launch_bounds__(256) void ct_gemm_tiled_kernel(GemmArgs<T> p) {
  ct_member(p);
  __shared__ T As[TK][TB + 1];
  __shared__ T Bs[TK][TB + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int64_t tm = (p.M + TB - 1) / TB, tn = (p.N + TB - 1) / TB;
  for (int64_t t = blockIdx.x; t < p.H * tm * tn; t += gridDim.x) {
    const int64_t h = t / (tm * tn), m0 = (t / tn % tm) * TB, n0 = t % tn * TB;
    const T* A = p.A + h * p.M * p.K;
    const T* B = p.B + h * p.K * p.N;
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = ct_zero<T>();
    for (int64_t k0 = 0; k0 < p.K; k0 += TK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int ak = AK ? e % TK : e / TB, am = AK ? e / TK : e % TB;
        const int64_t m = m0 + am, k = k0 + ak;
        As[ak][am] = (m < p.M && k < p.K) ? A[m * p.a_m + k * p.a_k] : ct_zero<T>();
        const int bk = BN ? e / TB : e % TK, bn = BN ? e % TB : e / TK;
        const int64_t n = n0 + bn, k2 = k0 + bk;
        Bs[bk][bn] = (n < p.N && k2 < p.K) ? B[k2 * p.b_k + n * p.b_n] : ct_zero<T>();
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

// E: the element as the operands hold it, P: GemmArgs<E>, or HalfGemmArgs<E> (sums in float32, contract_half.h)
// SC: per-tensor scaling of a storage-mode step (contract_half.h: ct_store_scaled, ct_amax_finish)
template <class E, class P, bool SC = false>
__device__ inline void ct_stream_body(const P& p) {
  using T = ct_acc_t<E>;
  const int64_t total = p.H * p.M * p.N;
  [[maybe_unused]] uint32_t mx = 0;
  [[maybe_unused]] int sh = 0;
  if constexpr (SC) sh = ct_scale_shift(p);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = e % p.N, r = e / p.N, m = r % p.M, h = r / p.M;
    const E* a = p.A + h * p.M * p.K + m * p.a_m;
    const E* b = p.B + h * p.K * p.N + n * p.b_n;
    T acc = ct_zero<T>();
    for (int64_t k = 0; k < p.K; ++k) acc = ct_mac(acc, ct_load(a + k * p.a_k), ct_load(b + k * p.b_k));
    if constexpr (SC) ct_store_scaled(p, e, acc, sh, mx);
    else ct_store(p, e, acc);
  }
  if constexpr (SC) ct_amax_finish(p.amax, mx);
}

template <class T>
__global__ __launch_bounds__(256) void ct_gemm_stream_kernel(GemmArgs<T> p) {
  ct_member(p);
  ct_stream_body<T>(p);
}

template <class E, bool SC>
__global__ __launch_bounds__(256) void ct_half_stream_kernel(HalfGemmArgs<E> p) {
  ct_member(p);
  ct_stream_body<E, HalfGemmArgs<E>, SC>(p);
}

template <class E, class P, bool SC = false>
__device__ inline void ct_dot_body(const P& p) {
  using T = ct_acc_t<E>;
  __shared__ T part[256];
  const int tid = threadIdx.x;
  const int64_t total = p.H * p.M * p.N;
  [[maybe_unused]] uint32_t mx = 0;  // (of thread 0, which stores)
  [[maybe_unused]] int sh = 0;
  if constexpr (SC) sh = ct_scale_shift(p);
  for (int64_t e = blockIdx.x; e < total; e += gridDim.x) {
    const int64_t n = e % p.N, r = e / p.N, m = r % p.M, h = r / p.M;
    const E* a = p.A + h * p.M * p.K + m * p.a_m;
    const E* b = p.B + h * p.K * p.N + n * p.b_n;
    T acc = ct_zero<T>();
    for (int64_t k = tid; k < p.K; k += 256) acc = ct_mac(acc, ct_load(a + k * p.a_k), ct_load(b + k * p.b_k));
    part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) part[tid] = ct_add(part[tid], part[tid + w]);
      __syncthreads();
    }
    if constexpr (SC) {
      if (tid == 0) ct_store_scaled(p, e, part[0], sh, mx);
    } else {
      if (tid == 0) ct_store(p, e, part[0]);
    }
    __syncthreads();
  }
  if constexpr (SC) ct_amax_finish(p.amax, mx);
}

template <class T>
__global__ __launch_bounds__(256) void ct_gemm_dot_kernel(GemmArgs<T> p) {
  ct_member(p);
  ct_dot_body<T>(p);
}

template <class E, bool SC>
__global__ __launch_bounds__(256) void ct_half_dot_kernel(HalfGemmArgs<E> p) {
  ct_member(p);
  ct_dot_body<E, HalfGemmArgs<E>, SC>(p);
}

// Where the members of a batch go in the output: member b adds its block of the staging buffer to the output at element
// off[b] when bit b of beta is set, and places it there otherwise (the host's `visited` bookkeeping, by value).
constexpr int MAX_SLICE_BATCH = 64;
struct BatchPlace {
  int64_t off[MAX_SLICE_BATCH];
  uint64_t beta;
};

// stage [n][numel], as the last step of every member left it (unrounded, beta 0) -> out: one lane per element of a
// block, the members one after the other in assignment order, each exactly the store of an unbatched last step
// (ct_store).  Members of one batch may share a block: the lane then adds to what it wrote itself.  No atomics.
template <class T>
__global__ __launch_bounds__(256) void ct_batch_reduce_kernel(T* out, const T* stage, int64_t numel, int n, BatchPlace pl) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    for (int b = 0; b < n; ++b) {
      T* o = out + pl.off[b] + e;
      const T v = stage[b * numel + e];
      *o = (pl.beta >> b) & 1 ? ct_add(*o, v) : v;
    }
}

#include "contract_path.h"
#include "contract_sets.h"
#include "contract_walk.h"
#include "contract_accumulate.h"

// A step with a row axis: row r of the result reads row a_map[r] of A and row b_map[r] of B.  A null map with a row
// stride: row r itself; a row stride of 0: the operand has one row, read for every r.
template <class T>
struct RowGemmArgs {
  const T* A;
  const T* B;
  T* C;
  const int32_t* a_map;
  const int32_t* b_map;
  int64_t a_row, b_row;        // elements between two rows of A / of B (H M K, H K N, or 0)
  int64_t a_m, a_k, b_k, b_n;  // strides inside a batch, as in GemmArgs
  int64_t R, H, M, N, K;
  int beta;
};

template <class T>
__device__ inline const T* ct_row_of(const T* base, const int32_t* map, int64_t stride, int64_t r) {
  return base + (map ? (int64_t)map[r] : r) * stride;
}

// the tile loop of ct_gemm_tiled_kernel, batches (r, h): the operand bases go through the maps
template <class T, bool AK, bool BN>
__global__ __launch_bounds__(256) void ct_rows_tiled_kernel(RowGemmArgs<T> p) {
  __shared__ T As[TK][TB + 1];
  __shared__ T Bs[TK][TB + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int64_t tm = (p.M + TB - 1) / TB, tn = (p.N + TB - 1) / TB;
  for (int64_t t = blockIdx.x; t < p.R * p.H * tm * tn; t += gridDim.x) {
    const int64_t rh = t / (tm * tn), r = rh / p.H, h = rh % p.H, m0 = (t / tn % tm) * TB, n0 = t % tn * TB;
    const T* A = ct_row_of(p.A, p.a_map, p.a_row, r) + h * p.M * p.K;
    const T* B = ct_row_of(p.B, p.b_map, p.b_row, r) + h * p.K * p.N;
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = ct_zero<T>();
    for (int64_t k0 = 0; k0 < p.K; k0 += TK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int ak = AK ? e % TK : e / TB, am = AK ? e / TK : e % TB;
        const int64_t m = m0 + am, k = k0 + ak;
        As[ak][am] = (m < p.M && k < p.K) ? A[m * p.a_m + k * p.a_k] : ct_zero<T>();
        const int bk = BN ? e / TB : e % TK, bn = BN ? e % TB : e / TK;
        const int64_t n = n0 + bn, k2 = k0 + bk;
        Bs[bk][bn] = (n < p.N && k2 < p.K) ? B[k2 * p.b_k + n * p.b_n] : ct_zero<T>();
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
    T* Cb = p.C + rh * p.M * p.N;
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

// One lane per output element (r, h, m, n), n fastest: a wavefront covers consecutive n, then m, of one row, or of
// adjacent rows when H M N < 64, so the lanes of a row read its two map entries from one address, once, before the k
// loop, and the result is written in full lines.  I: the integer type of the element arithmetic (uint32_t while the
// result has fewer than 2^31 elements: three 32-bit divisions per element instead of 64-bit ones).
template <class T, class I>
__device__ inline void ct_rows_stream_body(const RowGemmArgs<T>& p) {
  const I N = (I)p.N, M = (I)p.M, H = (I)p.H, total = (I)(p.R * p.H * p.M * p.N);
  const I stride = (I)gridDim.x * (I)blockDim.x;
  const I first = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x;
  const I trips = first < total ? (total - first + stride - 1) / stride : 0;  // (no wrap of e + stride)
  I e = first;
  for (I t = 0; t < trips; ++t, e += stride) {
    const I n = e % N, q = e / N, m = q % M, rh = q / M, h = rh % H, r = rh / H;
    const T* a = ct_row_of(p.A, p.a_map, p.a_row, (int64_t)r) + (int64_t)h * p.M * p.K + (int64_t)m * p.a_m;
    const T* b = ct_row_of(p.B, p.b_map, p.b_row, (int64_t)r) + (int64_t)h * p.K * p.N + (int64_t)n * p.b_n;
    T acc = ct_zero<T>();
    for (int64_t k = 0; k < p.K; ++k) acc = ct_mac(acc, a[k * p.a_k], b[k * p.b_k]);
    p.C[e] = p.beta ? ct_add(p.C[e], acc) : acc;
  }
}

template <class T>
__global__ __launch_bounds__(256) void ct_rows_stream_kernel(RowGemmArgs<T> p) {
  if (p.R * p.H * p.M * p.N < (int64_t)1 << 31) ct_rows_stream_body<T, uint32_t>(p);
  else ct_rows_stream_body<T, uint64_t>(p);
}

template <class T>
__global__ __launch_bounds__(256) void ct_rows_dot_kernel(RowGemmArgs<T> p) {
  __shared__ T part[256];
  const int tid = threadIdx.x;
  const int64_t total = p.R * p.H * p.M * p.N;
  for (int64_t e = blockIdx.x; e < total; e += gridDim.x) {
    const int64_t n = e % p.N, q = e / p.N, m = q % p.M, rh = q / p.M, h = rh % p.H, r = rh / p.H;
    const T* a = ct_row_of(p.A, p.a_map, p.a_row, r) + h * p.M * p.K + m * p.a_m;
    const T* b = ct_row_of(p.B, p.b_map, p.b_row, r) + h * p.K * p.N + n * p.b_n;
    T acc = ct_zero<T>();
    for (int64_t k = tid; k < p.K; k += 256) acc = ct_mac(acc, a[k * p.a_k], b[k * p.b_k]);
    part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) part[tid] = ct_add(part[tid], part[tid + w]);
      __syncthreads();
    }
    if (tid == 0) p.C[e] = p.beta ? ct_add(p.C[e], part[0]) : part[0];
    __syncthreads();
  }
}

#include "contract_indirect.h"
#include "contract_io.h"

}  // namespace

// The schedule of the slice loop.  Every step and permute has a period: it is due at assignment a of [lo, hi) iff a == lo
// or a % period == 0.  Every period 1: the plain loop; hoist flags: the number of assignments for a flagged item, 1 for
// the others; reuse periods: as given.
struct Schedule {
  enum Set { NEVER, HOIST, REUSE } set = NEVER;  // the setter the periods came from; NEVER: none, or one that left every period 1
  std::vector<int64_t> step_period;  // [n_steps]
  std::vector<int64_t> phase;        // the distinct periods, the largest first: the phases of an assignment in running order
  std::vector<int64_t> first, count, largest;  // per phase q and permute group g, at q (n_steps + 1) + g + 1: the first row of
                                     // that period, how many there are (they are contiguous), their largest numel
  std::vector<char> kept_opnd;       // [n_steps][2]: the operand is a kept tensor, read in arena copy 0 by every member
};

struct tnco_hip_contract_s {
  int device = 0, dtype = 0;
  size_t elem = 4, out_elem = 4;  // bytes of an element of the leaves and the arena / of the output (storage mode: not the same)
  std::vector<int64_t> leaf_numel, leaf_off, leaf_sl, perms, steps, slice_dims, place, block;
  std::vector<int64_t> group_first, group_count;  // perm rows of group g at index g + 1
  std::vector<int64_t> row_steps;  // [n_steps][ROW_W], empty: no step has a row axis
  std::vector<int32_t> row_maps;
  int scaling = 0;                 // per-tensor scaling of a storage dtype (tnco_hip.h)
  std::vector<int64_t> stage_refs;  // [n_steps]: arena offset of a stored step's float32 staging buffer, -1: none
  std::vector<int32_t> leaf_exps;  // the leaves' exponents (tnco_hip_contract_set_exponents)
  int32_t* d_exps = nullptr;       // [n_leaves + n_steps] exponent slots
  uint32_t* d_amax = nullptr;      // [n_steps] max words
  int64_t narrow_launches = 0;     // launches of ct_scale_narrow_kernel in the last run
  int64_t batch = 0;               // tnco_hip_contract_set_slice_batch: assignments per launch, 0: never set
  void* d_batch_out = nullptr;     // [batch][block_numel] of the output's type: the members' last steps
  int64_t batch_launches = 0;      // launches of ct_batch_reduce_kernel in the last run
  int compute = 0;                 // tnco_hip_contract_set_compute: 0 plain, 1 bf16x3
  int64_t split_launches = 0;      // launches of ct_split_tiled_kernel in the last run
  int matrix = 0;                  // tnco_hip_contract_set_matrix: 1: the tiled class runs ct_matrix_tiled_kernel
  int64_t matrix_launches = 0;     // launches of ct_matrix_tiled_kernel in the last run
  int64_t path_group = 0;          // tnco_hip_contract_set_path_kernel: assignments per launch of ct_path_kernel, 0: never set
  void* d_path_stage = nullptr;    // [path_group][block_numel] of the output's type: the members' last steps
  int64_t* d_path_tables = nullptr;  // steps | first row and count of every permute group | placement of every assignment
  std::vector<int64_t> path_image;   // the host copy of d_path_tables
  int64_t path_launches[2] = {0, 0};  // launches of ct_path_kernel and of ct_path_reduce_kernel in the last run
  Schedule sched;                  // which items an assignment runs (make_schedule); create: every item at every one
  bool folded = false;             // a step has an operand with both stride columns 0: it runs with indirect tables only
  std::vector<int64_t> ind_steps;  // tnco_hip_contract_set_indirect: [n_steps][IND_W]; empty: never set, or nothing folded
  std::vector<char> ind_fast;      // [n_steps][2]: lanes of the tiled kernel stage A along k / B along n
  int64_t* d_ind = nullptr;        // ind_steps | the pool of the offset tables
  int64_t ind_bytes = 0;           // what the tables add to `bytes`
  int64_t by_ix[TNCO_HIP_CONTRACT_N_IX_KERNELS] = {};  // launches of the last run per indirect kernel (tnco_hip.h)
  int accumulate = 0;              // tnco_hip_contract_set_accumulate: 1: the sum over assignments in float64
  void* d_acc = nullptr;           // [out_numel] of the wide type: the accumulator
  void* d_acc_stage = nullptr;     // [block_numel] of the output's type: the block of an unbatched assignment
  int64_t acc_launches[2] = {0, 0};  // fold launches and narrowing launches of the last run
  int64_t last_member = 0;         // the member that ran the last assignment of the last run (its exponent slots)
  int64_t base_bytes = 0;          // `bytes` as create reserved them
  std::vector<int32_t> exps_image;  // the leaves' exponents, once per member
  int64_t arena_elems = 0, out_numel = 0, block_numel = 1, n_blocks = 1, start = 0, stop = 1;
  char* d_leaves = nullptr;  // every leaf, back to back
  void* d_arena = nullptr;
  void* d_out = nullptr;
  int64_t* d_tables = nullptr;  // perms | leaf_sl | place | slice_dims
  void** d_leaf_ptrs = nullptr;
  int32_t* d_row_maps = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the kernels of a run
  int64_t macs = 0, launches = 0, bytes = 0, device_ns = 0;
  int64_t by_kernel[TNCO_HIP_CONTRACT_N_KERNELS] = {};  // launches of the last run per kernel path (tnco_hip.h)
  int64_t by_row_kernel[TNCO_HIP_CONTRACT_N_ROW_KERNELS] = {};  // the same of the row-mapped paths
  std::vector<char> loaded;        // [n_leaves]: the leaf buffer holds a leaf (tnco_hip_contract_load_leaf, tnco_hip_contract_run)
  int64_t io_launches[2] = {0, 0};  // launches of ct_ingest_kernel and of ct_emit_kernel since create
  // leaf sets (tnco_hip_contract_load_leaf_sets, tnco_hip_contract_run_sets); every buffer grows and never shrinks
  std::vector<void*> d_stack;      // [n_leaves]: the leaf's stack [sets][leaf_numel], apart from its single buffer
  std::vector<int64_t> stack_cap;  // [n_leaves]: sets the stack has room for
  std::vector<int64_t> stack_sets;  // [n_leaves]: sets the stack holds for the next tnco_hip_contract_run_sets, 0: none
  int64_t path_cap = 0;            // members d_arena and d_path_stage have room for (tnco_hip_contract_set_path_kernel: path_group)
  void* d_sets_out = nullptr;      // [sets_out_cap][out_numel]
  int64_t sets_out_cap = 0;
  char* d_sets_tables = nullptr;   // [n_leaves][SET_W]: a leaf's pointer and its set stride
  std::vector<int64_t> sets_image;  // the host copy of d_sets_tables of the last run
  int64_t sets_launches[2] = {0, 0};  // launches of ct_sets_path_kernel and of ct_sets_reduce_kernel in the last run
  // walkers (tnco_hip_contract_load_leaf_versions, tnco_hip_contract_run_walkers)
  std::vector<void*> d_versions;   // [n_leaves]: the leaf's two versions [2][leaf_numel], nullptr: never loaded
  std::vector<int64_t> versions_cap, versions;  // [n_leaves]: versions d_versions[t] has room for / holds (0 or 2)
  char* d_walk_tables = nullptr;   // [n_leaves][WALK_W]: a leaf's pointer, its qubit and its version stride
  std::vector<int64_t> walk_image;  // the host copy of d_walk_tables of the last run
  uint64_t last_walk = 0;          // the id of the walkers of the last run if that was a tnco_hip_contract_run_walkers, else 0
  int64_t walk_sets = 0;           // the outputs that run left: one per walker, or 1 for all of them (no leaf was indexed)
};

// The state of a sampler's walkers: a table of bits and a dead flag per walker, on one device, and the seed of the draws.
struct tnco_hip_walkers_s {
  int device = 0;
  int64_t n_walkers = 0, n_qubits = 0;
  uint64_t seed = 0, id = 0;       // id: unique in the process, never 0
  uint8_t* d_bits = nullptr;       // [n_qubits][n_walkers]
  uint8_t* d_dead = nullptr;       // [n_walkers]
  int64_t* d_perm = nullptr;       // ct_walk_permute_kernel's qubits and table
  hipStream_t stream = nullptr;
};

namespace {

int64_t leaf_slice_offset(const tnco_hip_contract_s* c, int64_t leaf, int64_t sid) {
  return ct_slice_offset(&c->leaf_sl[leaf * LEAF_SL_W], c->place.data(), c->slice_dims.data(), sid);
}

// H, M, N, K of a row of `steps`
struct StepShape {
  int64_t H, M, N, K;
};
StepShape step_shape(const int64_t* st) { return StepShape{st[ST_H], st[ST_M], st[ST_N], st[ST_K]}; }

int64_t leaf_slice_reach(const tnco_hip_contract_s* c, int64_t leaf) {  // the largest offset an assignment gives
  const int64_t* ls = &c->leaf_sl[leaf * LEAF_SL_W];
  int64_t off = 0;
  for (int j = 0; j < (int)ls[LS_COUNT]; ++j) off += (c->slice_dims[ls[LS_SLOTS + j]] - 1) * ls[LS_STRIDES + j];
  return off;
}

const char* validate(tnco_hip_contract_s* c, const tnco_hip_contract_desc* d) {
  const int64_t L = d->n_leaves, P = d->n_perms, S = d->n_steps;
  if (d->dtype < 0 || d->dtype > 7) return "'dtype' is not valid.";
  if (d->dtype > 3 && (d->row_steps || d->n_row_maps)) return "row axes are not supported with a storage dtype.";
  if (d->scaling != 0 && d->scaling != 1) return "'scaling' is not valid.";
  if (d->scaling && d->dtype < 4) return "scaling needs a storage dtype.";
  if (d->scaling && S > 0 && !d->stage_refs) return "null table.";
  if (d->max_axes != CT_MAX_AXES) return "'max_axes' must be 32.";
  if (L < 0 || P < 0 || S < 0 || d->n_slice_dims < 0 || d->n_block < 0 || d->arena_elems < 0 || d->out_numel < 1)
    return "negative sizes.";
  if ((L && (!d->leaf_numel || !d->leaf_sl)) || (P && !d->perms) || (S && !d->steps) ||
      (d->n_slice_dims && !d->slice_dims) || (d->n_block && !d->block_slices))
    return "null table.";
  if (d->n_row_maps < 0 || (d->n_row_maps && (!d->row_maps || !d->row_steps))) return "row-map tables are not valid.";
  if (d->row_steps) c->row_steps.assign(d->row_steps, d->row_steps + S * ROW_W);
  if (d->n_row_maps) c->row_maps.assign(d->row_maps, d->row_maps + d->n_row_maps);
  c->leaf_numel.assign(d->leaf_numel, d->leaf_numel + L);
  c->leaf_sl.assign(d->leaf_sl, d->leaf_sl + L * LEAF_SL_W);
  c->perms.assign(d->perms, d->perms + P * PERM_W);
  c->steps.assign(d->steps, d->steps + S * STEP_W);
  c->scaling = d->scaling;
  if (d->scaling) c->stage_refs.assign(d->stage_refs, d->stage_refs + S);
  c->slice_dims.assign(d->slice_dims, d->slice_dims + d->n_slice_dims);
  c->block.assign(d->block_slices, d->block_slices + d->n_block);
  const int64_t NS = d->n_slice_dims;
  c->place.assign(NS, 1);
  int64_t n_slices = 1;
  for (int64_t s = NS - 1; s >= 0; --s) {
    if (c->slice_dims[s] < 1) return "slice dimensions must be positive.";
    c->place[s] = n_slices;
    if (n_slices > (INT64_MAX >> 2) / c->slice_dims[s]) return "too many slice assignments.";
    n_slices *= c->slice_dims[s];
  }
  if (!(0 <= d->slice_start && d->slice_start < d->slice_stop && d->slice_stop <= n_slices)) return "'slice_range' is not valid.";
  c->start = d->slice_start, c->stop = d->slice_stop;
  std::vector<char> seen(NS, 0);
  for (int64_t b : c->block) {
    if (b < 0 || b >= NS || seen[b]) return "'block_slices' is not valid.";
    seen[b] = 1;
    c->n_blocks *= c->slice_dims[b];
  }
  if (d->out_numel % c->n_blocks) return "'out_numel' is not a whole number of blocks.";
  c->out_numel = d->out_numel, c->block_numel = d->out_numel / c->n_blocks, c->arena_elems = d->arena_elems;
  c->leaf_off.assign(L + 1, 0);
  for (int64_t t = 0; t < L; ++t) {
    const int64_t* ls = &c->leaf_sl[t * LEAF_SL_W];
    if (c->leaf_numel[t] < 1 || ls[LS_COUNT] < 0 || ls[LS_COUNT] > CT_MAX_AXES) return "leaf table is not valid.";
    for (int j = 0; j < (int)ls[LS_COUNT]; ++j)
      if (ls[LS_SLOTS + j] < 0 || ls[LS_SLOTS + j] >= NS || ls[LS_STRIDES + j] < 0) return "leaf table is not valid.";
    if (leaf_slice_reach(c, t) >= c->leaf_numel[t]) return "leaf slices reach beyond the leaf.";
    c->leaf_off[t + 1] = c->leaf_off[t] + ((c->leaf_numel[t] + 63) / 64) * 64;
  }
  // permutes: sizes, reach of the source, room at the destination; rows sorted by group
  c->group_first.assign(S + 1, 0), c->group_count.assign(S + 1, 0);
  int64_t prev_group = -1;
  for (int64_t r = 0; r < P; ++r) {
    const int64_t* row = &c->perms[r * PERM_W];
    const int64_t nd = row[PM_NDIM], numel = row[PM_NUMEL], g = row[PM_GROUP];
    if (nd < 0 || nd > CT_MAX_AXES || g < -1 || g >= S || g < prev_group) return "permute table is not valid.";
    if (g != prev_group || r == 0) c->group_first[g + 1] = r;
    prev_group = g;
    c->group_count[g + 1] += 1;
    int64_t prod = 1, reach = 0;
    for (int k = 0; k < nd; ++k) {
      if (row[PM_DIMS + k] < 1 || row[PM_STRIDES + k] < 0) return "permute table is not valid.";
      prod *= row[PM_DIMS + k];
      reach += (row[PM_DIMS + k] - 1) * row[PM_STRIDES + k];
    }
    if (prod != numel) return "permute table is not valid.";
    const int64_t src = row[PM_SRC_REF], dst = row[PM_DST_REF];
    if (row[PM_SRC_KIND] == K_LEAF) {
      if (src < 0 || src >= L || reach + leaf_slice_reach(c, src) >= c->leaf_numel[src]) return "permute source out of range.";
    } else if (row[PM_SRC_KIND] == K_ARENA) {
      if (src < 0 || src + reach >= c->arena_elems) return "permute source out of range.";
    } else {
      return "permute table is not valid.";
    }
    if (row[PM_DST_KIND] == K_ARENA) {
      if (dst < 0 || dst + numel > c->arena_elems) return "permute destination out of range.";
      if (row[PM_SRC_KIND] == K_ARENA && src < dst + numel && dst < src + reach + 1) return "permute in place.";
    } else if (row[PM_DST_KIND] != K_OUT || numel != c->block_numel || S != 0) {
      return "permute table is not valid.";
    }
  }
  if (S == 0 && !(P == 1 && c->perms[PM_DST_KIND] == K_OUT)) return "a path without steps needs one copy to the output.";
  for (int64_t k = 0; k < S; ++k) {
    const int64_t* st = &c->steps[k * STEP_W];
    const auto [H, M, N, K] = step_shape(st);
    if (H < 1 || M < 1 || N < 1 || K < 1) return "step sizes must be positive.";
    // the row axis: an operand has one row, or the result's rows (no map), or rows of its own reached through a map
    static const int64_t no_rows[ROW_W] = {1, 1, -1, 1, -1};
    const int64_t* rw = c->row_steps.empty() ? no_rows : &c->row_steps[k * ROW_W];
    const int64_t R = rw[RW_R];
    if (R < 1) return "step row counts must be positive.";
    for (int side = 0; side < 2; ++side) {
      const int64_t rows = rw[RW_SIDE * side + RW_A_ROWS], map = rw[RW_SIDE * side + RW_A_MAP];
      if (rows < 1) return "step row counts must be positive.";
      if (map == -1) {
        if (rows != 1 && rows != R) return "an operand without a row map has one row or the result's rows.";
        continue;
      }
      if (map < 0 || map > (int64_t)c->row_maps.size() || R > (int64_t)c->row_maps.size() - map) return "row map out of range.";
      for (int64_t r = 0; r < R; ++r)
        if (c->row_maps[map + r] < 0 || c->row_maps[map + r] >= rows) return "row map entry beyond the operand's rows.";
    }
    // (0, 0): a folded operand, read through the tables of tnco_hip_contract_set_indirect, which a run then needs
    const bool ind_a = st[ST_A_M] == 0 && st[ST_A_K] == 0, ind_b = st[ST_B_K] == 0 && st[ST_B_N] == 0;
    if (!ind_a && !((st[ST_A_M] == K && st[ST_A_K] == 1) || (st[ST_A_M] == 1 && st[ST_A_K] == M))) return "A strides are not valid.";
    if (!ind_b && !((st[ST_B_K] == N && st[ST_B_N] == 1) || (st[ST_B_K] == 1 && st[ST_B_N] == K))) return "B strides are not valid.";
    if ((ind_a || ind_b) && (d->dtype > 3 || d->row_steps)) return "folded operands need a plain dtype and no row axes.";
    c->folded |= ind_a || ind_b;
    int64_t lo[2], hi[2];
    for (int side = 0; side < 2; ++side) {
      const int64_t kind = st[ST_SIDE * side + ST_A_KIND], ref = st[ST_SIDE * side + ST_A_REF];
      const int64_t n = rw[RW_SIDE * side + RW_A_ROWS] * H * K * (side ? N : M);
      if (kind == K_LEAF) {
        if (ref < 0 || ref >= L || n + leaf_slice_reach(c, ref) > c->leaf_numel[ref]) return "step operand out of range.";
        lo[side] = hi[side] = -1;
      } else if (kind == K_ARENA) {
        if (ref < 0 || ref + n > c->arena_elems) return "step operand out of range.";
        lo[side] = ref, hi[side] = ref + n;
      } else {
        return "step operand kind is not valid.";
      }
    }
    if (c->scaling) {  // the operands' exponent slots: a leaf's own, or that of an earlier step's result
      for (int side = 0; side < 2; ++side) {
        const int64_t slot = st[ST_A_SLOT + side];
        // (an operand in the arena: an earlier step's result, or a leaf that a gather moved there)
        const int64_t kind = st[ST_SIDE * side + ST_A_KIND], ref = st[ST_SIDE * side + ST_A_REF];
        if (kind == K_LEAF ? slot != ref : (slot < 0 || slot >= L + k)) return "step exponent slot is not valid.";
      }
    }
    const int64_t nc = R * H * M * N;
    if (st[ST_C_KIND] == K_OUT) {
      if (k != S - 1 || nc != c->block_numel) return "only the last step writes the output, one block.";
    } else if (st[ST_C_KIND] == K_ARENA && k != S - 1) {
      if (st[ST_C_REF] < 0 || st[ST_C_REF] + nc > c->arena_elems) return "step result out of range.";
      for (int side = 0; side < 2; ++side)
        if (lo[side] >= 0 && st[ST_C_REF] < hi[side] && lo[side] < st[ST_C_REF] + nc) return "step result overlaps an operand.";
      if (c->scaling) {  // the float32 staging buffer: 2 nc storage elements, apart from the operands and the result
        const int64_t sg = c->stage_refs[k];
        if (sg < 0 || sg % 8 || st[ST_C_REF] % 8 || sg + 2 * nc > c->arena_elems) return "step staging out of range.";
        if (sg < st[ST_C_REF] + nc && st[ST_C_REF] < sg + 2 * nc) return "step staging overlaps the result.";
        for (int side = 0; side < 2; ++side)
          if (lo[side] >= 0 && sg < hi[side] && lo[side] < sg + 2 * nc) return "step staging overlaps an operand.";
      }
    } else {
      return "the last step must write the output.";
    }
  }
  return nullptr;
}

// the rows of permute group `group` that have the period of phase `phase`, in one launch
template <class D, class SI = D, bool half = false, bool scaled = false>
int launch_gathers(tnco_hip_contract_s* c, int64_t group, int64_t phase, int64_t sid, int64_t out_off, int64_t members = 0) {
  const int64_t at = phase * (int64_t)c->group_first.size() + group + 1;
  const int64_t n = c->sched.count[at], largest = c->sched.largest[at], first = c->sched.first[at];
  if (!n) return TNCO_HIP_OK;
  const int64_t P = (int64_t)c->perms.size() / PERM_W;
  GatherArgs g;
  g.rows = c->d_tables + first * PERM_W;
  g.leaf_sl = c->d_tables + P * PERM_W;
  g.slice_place = g.leaf_sl + c->leaf_sl.size();
  g.slice_dims = g.slice_place + c->place.size();
  g.leaves = (const void* const*)c->d_leaf_ptrs;
  g.arena = c->d_arena, g.out = c->d_out, g.sid = sid, g.out_off = out_off;
  g.arena_step = members ? c->arena_elems : 0;  // (members: of a batch, 0: an unbatched launch)
  const int64_t blocks = std::min<int64_t>((largest + 255) / 256, 2048);
  const dim3 grid((unsigned)blocks, (unsigned)n, (unsigned)std::max<int64_t>(members, 1));
  if constexpr (!half)
    hipLaunchKernelGGL(ct_gather_kernel<D>, grid, dim3(256), 0, c->stream, g);
  else if constexpr (scaled)
    hipLaunchKernelGGL((ct_half_gather_scaled_kernel<D, SI>), grid, dim3(256), 0, c->stream, g, (const int32_t*)c->d_exps);
  else
    hipLaunchKernelGGL((ct_half_gather_kernel<D, SI>), grid, dim3(256), 0, c->stream, g);
  CT_TRY(hipGetLastError());
  c->launches += 1;
  c->by_kernel[0] += 1;
  return TNCO_HIP_OK;
}

// The shape class of a step: every launcher picks the kernel of its family by it.  outs: the outputs as the launcher
// counts them, H M N (with rows: R H M N); the members of a batch (grid z) do not enter the choice.  (The path kernel
// restates the rule on the device: contract_path.h ct_path_step.)
enum ShapeClass { TILED, DOT, STREAM };
ShapeClass shape_class(int64_t M, int64_t N, int64_t K, int64_t outs) {
  if (M >= 64 && N >= 64 && K > 32) return TILED;  // every operand element reused 64 times from LDS
  return K >= 512 && outs <= 8192 ? DOT : STREAM;  // few outputs, long sums: K split over a block
}

// the slot of tnco_hip_contract_kernel_launches of a plain or storage-mode step: the tiled class by the order of A and B
int kernel_slot(ShapeClass cls, bool ak, bool bn) { return cls == TILED ? 1 + 2 * (ak ? 1 : 0) + (bn ? 1 : 0) : cls == DOT ? 5 : 6; }

// the grid of a tiled kernel: a block per bm x bn tile of each of the `batches` products, the members of a batch along z
dim3 tiled_grid(int64_t batches, int64_t M, int64_t N, int bm, int bn, unsigned members) {
  return dim3((unsigned)std::min<int64_t>(batches * ((M + bm - 1) / bm) * ((N + bn - 1) / bn), 1 << 20), 1, members);
}
dim3 stream_grid(int64_t outs, unsigned members) { return dim3((unsigned)std::min<int64_t>((outs + 255) / 256, 1 << 16), 1, members); }

// launch(AK, BN) with the memory order of the operands of a tiled kernel, a_k == 1 and b_n == 1, as two
// std::integral_constant<bool, ...>: the kernel takes them as template arguments
template <class Launch>
void with_orders(bool ak, bool bn, Launch launch) {
  if (ak && bn) launch(std::true_type{}, std::true_type{});
  else if (ak) launch(std::true_type{}, std::false_type{});
  else if (bn) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
}

// after the launch of a step: its error, then the counts; slot: the launch's entry of its family's table
int count_step(tnco_hip_contract_s* c, int64_t* slot, int64_t macs) {
  CT_TRY(hipGetLastError());
  c->launches += 1;
  *slot += 1;
  c->macs += macs;
  return TNCO_HIP_OK;
}

template <class T>
int launch_gemm(tnco_hip_contract_s* c, const GemmArgs<T>& p, unsigned members = 1) {
  const bool ak = p.a_k == 1, bn = p.b_n == 1;
  const int64_t outs = p.H * p.M * p.N;
  const ShapeClass cls = shape_class(p.M, p.N, p.K, outs);
  constexpr bool single = std::is_same<T, float>::value || std::is_same<T, cplx<float>>::value;
  if (cls == TILED && c->matrix) {  // on the matrix cores in T's precision (contract_matrix.h)
    const dim3 grid = tiled_grid(p.H, p.M, p.N, 32 * ct_mx<T>::TI, 32 * ct_mx<T>::TJ, members);
    with_orders(ak, bn, [&](auto AK, auto BN) {
      hipLaunchKernelGGL((ct_matrix_tiled_kernel<T, decltype(AK)::value, decltype(BN)::value>), grid, dim3(256), 0, c->stream, p);
    });
    c->matrix_launches += 1;
  } else if (cls == TILED && single && c->compute == 1) {  // on the matrix cores, split (contract_split.h)
    if constexpr (single) {
      constexpr bool CP = std::is_same<T, cplx<float>>::value;
      const dim3 grid = tiled_grid(p.H, p.M, p.N, HB, HB, members);
      with_orders(ak, bn, [&](auto AK, auto BN) {
        hipLaunchKernelGGL((ct_split_tiled_kernel<CP, decltype(AK)::value, decltype(BN)::value>), grid, dim3(256), 0, c->stream, p);
      });
    }
    c->split_launches += 1;
  } else if (cls == TILED) {
    const dim3 grid = tiled_grid(p.H, p.M, p.N, TB, TB, members);
    with_orders(ak, bn, [&](auto AK, auto BN) {
      hipLaunchKernelGGL((ct_gemm_tiled_kernel<T, decltype(AK)::value, decltype(BN)::value>), grid, dim3(256), 0, c->stream, p);
    });
  } else if (cls == DOT) {
    hipLaunchKernelGGL(ct_gemm_dot_kernel<T>, dim3((unsigned)outs, 1, members), dim3(256), 0, c->stream, p);
  } else {
    hipLaunchKernelGGL(ct_gemm_stream_kernel<T>, stream_grid(outs, members), dim3(256), 0, c->stream, p);
  }
  return count_step(c, &c->by_kernel[kernel_slot(cls, ak, bn)], outs * p.K * members);
}

// launch_gemm in storage mode: the same shape classes and slots, the tiled class on the matrix cores
template <class S, bool CPLX, bool SC>
int launch_half_gemm(tnco_hip_contract_s* c, HalfGemmArgs<typename std::conditional<CPLX, cplx<S>, S>::type> p, unsigned members = 1) {
  using E = typename std::conditional<CPLX, cplx<S>, S>::type;
  const bool ak = p.a_k == 1, bn = p.b_n == 1;
  const int64_t outs = p.H * p.M * p.N;
  const ShapeClass cls = shape_class(p.M, p.N, p.K, outs);
  // 16-byte loads of 8 elements along the contiguous axis: the base and every row (column) of it aligned (the base of a
  // member of a batch: ct_member)
  p.a_vec = (uintptr_t)p.A % 16 == 0 && (ak ? p.a_m : p.a_k) % 8 == 0;
  p.b_vec = (uintptr_t)p.B % 16 == 0 && (bn ? p.b_k : p.b_n) % 8 == 0;
  if (cls == TILED) {
    const dim3 grid = tiled_grid(p.H, p.M, p.N, HB, HB, members);
    with_orders(ak, bn, [&](auto AK, auto BN) {
      hipLaunchKernelGGL((ct_mfma_tiled_kernel<S, CPLX, decltype(AK)::value, decltype(BN)::value, SC>), grid, dim3(256), 0, c->stream, p);
    });
  } else if (cls == DOT) {
    hipLaunchKernelGGL((ct_half_dot_kernel<E, SC>), dim3((unsigned)outs, 1, members), dim3(256), 0, c->stream, p);
  } else {
    hipLaunchKernelGGL((ct_half_stream_kernel<E, SC>), stream_grid(outs, members), dim3(256), 0, c->stream, p);
  }
  return count_step(c, &c->by_kernel[kernel_slot(cls, ak, bn)], outs * p.K * members);
}

// launch_gemm for a step with a row axis: the same shape classes, outputs counted with the rows
template <class T>
int launch_rows_gemm(tnco_hip_contract_s* c, const RowGemmArgs<T>& p) {
  const int64_t outs = p.R * p.H * p.M * p.N;
  const ShapeClass cls = shape_class(p.M, p.N, p.K, outs);
  if (cls == TILED) {
    const dim3 grid = tiled_grid(p.R * p.H, p.M, p.N, TB, TB, 1);
    with_orders(p.a_k == 1, p.b_n == 1, [&](auto AK, auto BN) {
      hipLaunchKernelGGL((ct_rows_tiled_kernel<T, decltype(AK)::value, decltype(BN)::value>), grid, dim3(256), 0, c->stream, p);
    });
  } else if (cls == DOT) {
    hipLaunchKernelGGL(ct_rows_dot_kernel<T>, dim3((unsigned)outs), dim3(256), 0, c->stream, p);
  } else {
    hipLaunchKernelGGL(ct_rows_stream_kernel<T>, stream_grid(outs, 1), dim3(256), 0, c->stream, p);
  }
  return count_step(c, &c->by_row_kernel[cls], outs * p.K);  // (slot of tnco_hip_contract_row_launches: the class)
}

// launch_gemm for a step with a folded operand: the same shape classes, the kernels of contract_indirect.h
template <class T>
int launch_ix_gemm(tnco_hip_contract_s* c, const IxGemmArgs<T>& p, unsigned members = 1) {
  const int64_t outs = p.H * p.M * p.N;
  const ShapeClass cls = shape_class(p.M, p.N, p.K, outs);
  if (cls == TILED)
    hipLaunchKernelGGL(ct_ix_tiled_kernel<T>, tiled_grid(p.H, p.M, p.N, TB, TB, members), dim3(256), 0, c->stream, p);
  else if (cls == DOT)
    hipLaunchKernelGGL(ct_ix_dot_kernel<T>, dim3((unsigned)outs, 1, members), dim3(256), 0, c->stream, p);
  else
    hipLaunchKernelGGL(ct_ix_stream_kernel<T>, stream_grid(outs, members), dim3(256), 0, c->stream, p);
  return count_step(c, &c->by_ix[cls], outs * p.K * members);  // (slot of tnco_hip_contract_indirect_launches: the class)
}

// What the argument structs of the four families have in common, from a row of `steps`: the operands, the strides and
// sizes, beta and, where the family's launches have members, the member record
template <class Args, class = void>
struct has_members : std::false_type {};
template <class Args>
struct has_members<Args, std::void_t<decltype(Args::mb)>> : std::true_type {};
template <class Args, class E>
void fill_step(Args& p, const int64_t* st, const E* const* opnd, int beta, const MemberArgs& mb) {
  p.A = opnd[0], p.B = opnd[1];
  p.a_m = st[ST_A_M], p.a_k = st[ST_A_K], p.b_k = st[ST_B_K], p.b_n = st[ST_B_N];
  p.H = st[ST_H], p.M = st[ST_M], p.N = st[ST_N], p.K = st[ST_K];
  p.beta = beta;
  if constexpr (has_members<Args>::value) p.mb = mb;
}

// wide accumulation, after the last assignment of a run: the accumulator rounded once into the output
template <class T>
int narrow_accumulator(tnco_hip_contract_s* c) {
  const dim3 grid((unsigned)std::min<int64_t>((c->out_numel + 255) / 256, 2048));
  hipLaunchKernelGGL(ct_acc_narrow_kernel<T>, grid, dim3(256), 0, c->stream, (T*)c->d_out, (const ct_wide_t<T>*)c->d_acc,
                     c->out_numel);
  CT_TRY(hipGetLastError());
  c->launches += 1;
  c->narrow_launches += 1;
  c->acc_launches[1] += 1;
  return TNCO_HIP_OK;
}

// T: the type of the sums and of the output; E: of the leaves and the arena (storage mode: st_f16 / st_bf16 or a pair)
template <class T, class E = T>
int run_impl(tnco_hip_contract_s* c) {
  constexpr bool half = !std::is_same<T, E>::value;
  // gathers move elements as they are, by width; only a single leaf gathered into the output is widened
  using W = typename std::conditional<!half, T, typename std::conditional<sizeof(E) == 2, uint16_t, uint32_t>::type>::type;
  std::vector<char> visited(c->n_blocks, 0);
  const int64_t S = (int64_t)c->steps.size() / STEP_W, L = (int64_t)c->leaf_numel.size();
  // a batch: up to c->batch assignments per launch, each in its own arena; a plan without steps runs as it does unbatched
  const bool batched = c->batch > 0 && S > 0;
  const int64_t per = batched ? c->batch : 1;
  // wide accumulation: the folds go into the accumulator; a plan without steps places blocks only and runs as it is
  constexpr bool single = std::is_same<T, float>::value || std::is_same<T, cplx<float>>::value;
  const bool wide = single && c->accumulate && S > 0;
  E* arena = (E*)c->d_arena;
  T* out = (T*)c->d_out;
  const int64_t* d_leaf_sl = c->d_tables + c->perms.size();
  MemberArgs mb0{};
  if (batched) {
    mb0.slice_place = d_leaf_sl + c->leaf_sl.size(), mb0.slice_dims = mb0.slice_place + c->place.size();
    mb0.exp_step = (int)(L + S), mb0.amax_step = (int)S;
  }
  const int64_t arena_bytes = batched ? c->arena_elems * (int64_t)sizeof(E) : 0;
  const Schedule& sc = c->sched;
  // Step k of the path.  bat: as members launches of a batch starting at assignment sid (the last step to the batch
  // staging buffer), else one unbatched launch: an assignment's, or a step's of a period above 1 (which works in arena
  // copy 0)
  auto run_step = [&](int64_t k, int64_t sid, bool bat, unsigned members, int beta, int64_t out_off) -> int {
    int rc;
    const int64_t* st = &c->steps[k * STEP_W];
    const int64_t member_bytes = bat ? arena_bytes : 0;
    const E* opnd[2];
    MemberArgs mb = bat ? mb0 : MemberArgs{};
    mb.sid0 = sid;
    for (int side = 0; side < 2; ++side) {
      const int64_t kind = st[ST_SIDE * side + ST_A_KIND], ref = st[ST_SIDE * side + ST_A_REF];
      if (kind != K_LEAF) {  // (of a batch: each member's own arena; a kept tensor: copy 0 for every member)
        opnd[side] = arena + ref;
        (side ? mb.b_step : mb.a_step) = sc.kept_opnd[2 * k + side] ? 0 : member_bytes;
        continue;
      }
      // a leaf read in place: at the slice offset of the assignment, which a member of a batch adds for its own
      opnd[side] = (const E*)(c->d_leaves + c->leaf_off[ref] * c->elem) + (bat ? 0 : leaf_slice_offset(c, ref, sid));
      if (bat) (side ? mb.b_ls : mb.a_ls) = d_leaf_sl + ref * LEAF_SL_W;
    }
    // batched: the last step writes every member's block, with beta 0, to the batch staging buffer
    const bool last = st[ST_C_KIND] == K_OUT;
    // (wide accumulation, unbatched: the same, one block, to the staging block of the accumulator)
    T* out_dest = bat ? (T*)c->d_batch_out : wide ? (T*)c->d_acc_stage : out + out_off;
    const int out_beta = bat || wide ? 0 : beta;
    if (bat) mb.c_step = last ? c->block_numel * (int64_t)sizeof(T) : arena_bytes;
    if constexpr (half) {
      HalfGemmArgs<E> p;
      fill_step(p, st, opnd, last ? out_beta : 0, mb);
      p.Cs = last ? nullptr : arena + st[ST_C_REF];
      p.C = last ? out_dest : nullptr;
      p.a_vec = p.b_vec = 0;
      p.exps = nullptr, p.sa = p.sb = 0, p.amax = nullptr;
      using St = typename ct_storage_of<E>::type;
      if (!c->scaling) return launch_half_gemm<St, sizeof(E) == 4, false>(c, p, members);
      p.exps = c->d_exps, p.sa = (int)st[ST_A_SLOT], p.sb = (int)st[ST_B_SLOT];
      if (!last) {  // unrounded to the staging buffer, then narrowed at the exponent of the whole result
        p.Cs = nullptr, p.C = (T*)(arena + c->stage_refs[k]), p.amax = c->d_amax + k;
      }
      if ((rc = launch_half_gemm<St, sizeof(E) == 4, true>(c, p, members))) return rc;
      if (!last) {
        const int64_t nc = p.H * p.M * p.N, quads = nc * (sizeof(E) == 4 ? 2 : 1) / 4;
        const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>((quads + 255) / 256, 1), 2048), 1, members);
        hipLaunchKernelGGL((ct_scale_narrow_kernel<St, sizeof(E) == 4>), grid, dim3(256), 0, c->stream, (const float*)p.C,
                           (St*)(arena + st[ST_C_REF]), nc, (const uint32_t*)p.amax, c->d_exps, p.sa, p.sb, (int)(L + k),
                           member_bytes, mb.exp_step, mb.amax_step);
        CT_TRY(hipGetLastError());
        c->launches += 1;
        c->narrow_launches += 1;
      }
      return TNCO_HIP_OK;
    } else {
      T* dest = last ? out_dest : arena + st[ST_C_REF];
      const int64_t* rw = c->row_steps.empty() ? nullptr : &c->row_steps[k * ROW_W];
      if (rw && (rw[RW_R] > 1 || rw[RW_A_MAP] >= 0 || rw[RW_B_MAP] >= 0)) {
        RowGemmArgs<T> p;
        fill_step(p, st, opnd, last ? beta : 0, mb);
        p.C = dest;
        p.a_map = rw[RW_A_MAP] >= 0 ? c->d_row_maps + rw[RW_A_MAP] : nullptr;
        p.b_map = rw[RW_B_MAP] >= 0 ? c->d_row_maps + rw[RW_B_MAP] : nullptr;
        p.R = rw[RW_R];
        p.a_row = rw[RW_A_MAP] < 0 && rw[RW_A_ROWS] == 1 ? 0 : p.H * p.M * p.K;
        p.b_row = rw[RW_B_MAP] < 0 && rw[RW_B_ROWS] == 1 ? 0 : p.H * p.K * p.N;
        return launch_rows_gemm<T>(c, p);
      }
      const int64_t* ix = c->ind_steps.empty() ? nullptr : &c->ind_steps[k * IND_W];
      if (ix && (ix[IX_A_H] >= 0 || ix[IX_B_H] >= 0)) {  // a folded operand: read in place through its tables
        const int64_t* pool = c->d_ind + c->ind_steps.size();
        IxGemmArgs<T> p;
        fill_step(p, st, opnd, last ? out_beta : 0, mb);
        p.C = dest;
        const bool fa = ix[IX_A_H] >= 0, fb = ix[IX_B_H] >= 0;
        p.a_h = fa ? pool + ix[IX_A_H] : nullptr, p.a_mo = fa ? pool + ix[IX_A_M] : nullptr, p.a_ko = fa ? pool + ix[IX_A_K] : nullptr;
        p.b_h = fb ? pool + ix[IX_B_H] : nullptr, p.b_ko = fb ? pool + ix[IX_B_K] : nullptr, p.b_no = fb ? pool + ix[IX_B_N] : nullptr;
        p.a_kfast = c->ind_fast[2 * k], p.b_nfast = c->ind_fast[2 * k + 1];
        return launch_ix_gemm<T>(c, p, members);
      }
      GemmArgs<T> p;
      fill_step(p, st, opnd, last ? out_beta : 0, mb);
      p.C = dest;
      return launch_gemm<T>(c, p, members);
    }
  };
  for (int64_t sid = c->start; sid < c->stop; sid += per) {
    const int64_t n = std::min(per, c->stop - sid);  // members of this launch
    const unsigned members = (unsigned)n;
    BatchPlace pl{};
    for (int64_t m = 0; m < n; ++m) {
      int64_t blk = 0;
      for (int64_t b : c->block) blk = blk * c->slice_dims[b] + ((sid + m) / c->place[b]) % c->slice_dims[b];
      pl.off[m] = blk * c->block_numel;
      pl.beta |= (uint64_t)visited[blk] << m;  // (visited by an earlier batch, or by an earlier member of this one)
      visited[blk] = 1;
    }
    const int beta = (int)(pl.beta & 1);
    const int64_t out_off = pl.off[0];
    c->last_member = n - 1;
    // scaling: the max words of every step are cleared at the start of an assignment (of a batch: of all its members),
    // in stream order after the narrowing passes of the one before
    if (half && c->scaling && S) CT_TRY(hipMemsetAsync(c->d_amax, 0, (size_t)(S * per) * sizeof(uint32_t), c->stream));
    // Every phase that is due at this assignment, the slowest first, each in path order.  (Not path order across the
    // phases: a slower phase's temporaries may lie where a faster phase keeps a tensor, which that phase, due whenever
    // the slower one is, then writes again.)  A phase of a period above 1 is one unbatched launch per item in arena copy
    // 0; the phase of period 1, which holds the step that writes the output, is the batch when the handle has one
    for (int64_t q = 0; q < (int64_t)sc.phase.size(); ++q) {
      const int64_t period = sc.phase[q];
      if (sid != c->start && sid % period) continue;
      const bool bat = batched && period == 1;
      // scaling in a batch: every member reads the exponents of the kept tensors in its own copy of the slots (the
      // assignments clear the max words only, d_amax, never a slot)
      if (half && c->scaling && bat && q && sid == c->start)
        for (int64_t b = 1; b < c->batch; ++b)
          CT_TRY(hipMemcpyAsync(c->d_exps + b * (L + S), c->d_exps, (size_t)(L + S) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
      int rc = half && S == 0 ? (c->scaling ? launch_gathers<T, E, half, half>(c, -1, q, sid, out_off) : launch_gathers<T, E, half>(c, -1, q, sid, out_off))
                              : launch_gathers<W, W, half>(c, -1, q, sid, out_off, bat ? n : 0);
      if (rc) return rc;
      for (int64_t k = 0; k < S; ++k) {
        if ((rc = launch_gathers<W, W, half>(c, k, q, sid, out_off, bat ? n : 0))) return rc;
        if (sc.step_period[k] == period && (rc = run_step(k, sid, bat, bat ? members : 1, beta, out_off))) return rc;
      }
    }
    if (batched || wide) {  // the members' blocks into the output (the accumulator), in assignment order
      const dim3 grid((unsigned)std::min<int64_t>((c->block_numel + 255) / 256, 2048));
      if constexpr (single) {
        if (wide)
          hipLaunchKernelGGL(ct_acc_reduce_kernel<T>, grid, dim3(256), 0, c->stream, (ct_wide_t<T>*)c->d_acc,
                             (const T*)(batched ? c->d_batch_out : c->d_acc_stage), c->block_numel, (int)n, pl);
      }
      if (!wide)
        hipLaunchKernelGGL(ct_batch_reduce_kernel<T>, grid, dim3(256), 0, c->stream, out, (const T*)c->d_batch_out, c->block_numel,
                           (int)n, pl);
      CT_TRY(hipGetLastError());
      c->launches += 1;
      c->batch_launches += 1;
      c->acc_launches[0] += wide;
    }
  }
  if constexpr (single) {
    if (wide) return narrow_accumulator<T>(c);
  }
  return TNCO_HIP_OK;
}

// the arguments of the path kernel but the first assignment; *d_place: the placement table of the run's assignments
PathArgs path_args(const tnco_hip_contract_s* c, const int64_t** d_place) {
  const int64_t S = (int64_t)c->steps.size() / STEP_W, P = (int64_t)c->perms.size() / PERM_W;
  PathArgs a;
  a.perms = c->d_tables;
  a.leaf_sl = c->d_tables + P * PERM_W;
  a.slice_place = a.leaf_sl + c->leaf_sl.size();
  a.slice_dims = a.slice_place + c->place.size();
  a.steps = c->d_path_tables;
  a.groups = a.steps + S * STEP_W;
  a.leaves = (const void* const*)c->d_leaf_ptrs;
  a.arena = c->d_arena, a.stage = c->d_path_stage;
  a.arena_elems = c->arena_elems, a.block_numel = c->block_numel;
  a.sid0 = 0;
  a.n_steps = (int)S;
  *d_place = a.groups + GR_W * (S + 1);
  return a;
}

int64_t macs_per_assignment(const tnco_hip_contract_s* c) {
  int64_t per_slice = 0;
  for (size_t k = 0; k < c->steps.size() / STEP_W; ++k) {
    const auto [H, M, N, K] = step_shape(&c->steps[k * STEP_W]);
    per_slice += H * M * N * K;
  }
  return per_slice;
}

// The fused loop of every kind of member (contract_path.h): `members` members in groups of `group` consecutive ones, per
// group member(m0, n), the launch of the path kernel of the kind over the members [m0, m0 + n), and fold(m0, n), the
// launch of the kernel that folds their blocks; counters: the two launch counts of the kind.
template <class Member, class Fold>
int run_groups(tnco_hip_contract_s* c, int64_t members, int64_t group, int64_t* counters, Member member, Fold fold) {
  const int64_t per_slice = macs_per_assignment(c);
  for (int64_t m0 = 0; m0 < members; m0 += group) {
    const int64_t n = std::min(group, members - m0);
    member(m0, n);
    CT_TRY(hipGetLastError());
    fold(m0, n);
    CT_TRY(hipGetLastError());
    c->launches += 2;
    counters[0] += 1, counters[1] += 1;
    c->macs += per_slice * n;
  }
  return TNCO_HIP_OK;
}

dim3 fold_grid(const tnco_hip_contract_s* c) { return dim3((unsigned)std::min<int64_t>((c->block_numel + 255) / 256, 2048)); }

// A handle with a path kernel: the members are the assignments of the plan's range, c->path_group per ct_path_kernel, and
// ct_path_reduce_kernel folds them.
template <class T>
int run_path(tnco_hip_contract_s* c) {
  constexpr bool single = std::is_same<T, float>::value || std::is_same<T, cplx<float>>::value;
  const bool wide = single && c->accumulate;  // the folds go into the accumulator (run_path: a plan with steps)
  const int64_t* d_place = nullptr;
  PathArgs a = path_args(c, &d_place);
  const dim3 grid = fold_grid(c);
  const int rc = run_groups(
      c, c->stop - c->start, c->path_group, c->path_launches,
      [&](int64_t m0, int64_t n) {
        a.sid0 = c->start + m0;
        hipLaunchKernelGGL(ct_path_kernel<T>, dim3((unsigned)n), dim3(PATH_LANES), 0, c->stream, a);
      },
      [&](int64_t m0, int64_t n) {
        if constexpr (single) {
          if (wide)
            hipLaunchKernelGGL(ct_acc_path_reduce_kernel<T>, grid, dim3(256), 0, c->stream, (ct_wide_t<T>*)c->d_acc,
                               (const T*)c->d_path_stage, c->block_numel, (int)n, d_place + m0);
        }
        if (!wide)
          hipLaunchKernelGGL(ct_path_reduce_kernel<T>, grid, dim3(256), 0, c->stream, (T*)c->d_out, (const T*)c->d_path_stage,
                             c->block_numel, (int)n, d_place + m0);
        c->acc_launches[0] += wide;
      });
  if (rc) return rc;
  if constexpr (single) {
    if (wide) return narrow_accumulator<T>(c);
  }
  return TNCO_HIP_OK;
}

// Leaf sets and walkers: the members (set, assignment) of n_sets sets, set-major, `group` per launch of `kernel`
// (ct_sets_path_kernel over SetsArgs, ct_walk_path_kernel over WalkArgs: contract_sets.h, contract_walk.h; the caller
// has filled in what says where the leaves are), and ct_sets_reduce_kernel folds them.  The caller has made room for
// `group` members and n_sets outputs and has uploaded the table of the leaves.
template <class T, class Args>
int run_set_members(tnco_hip_contract_s* c, int64_t n_sets, int64_t group, Args s, void (*kernel)(Args)) {
  const int64_t A = c->stop - c->start;
  const int64_t* d_place = nullptr;
  s.p = path_args(c, &d_place);
  s.n_assign = A, s.start = c->start;
  const dim3 grid = fold_grid(c);
  return run_groups(
      c, n_sets * A, group, c->sets_launches,
      [&](int64_t m0, int64_t n) {
        s.m0 = m0;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(PATH_LANES), 0, c->stream, s);
      },
      [&](int64_t m0, int64_t n) {
        hipLaunchKernelGGL(ct_sets_reduce_kernel<T>, grid, dim3(256), 0, c->stream, (T*)c->d_sets_out, (const T*)c->d_path_stage,
                           c->block_numel, (int)n, m0, A, c->out_numel, d_place);
      });
}

// what the leaf-set entry points refuse of a handle, or nullptr
const char* sets_refusal(const tnco_hip_contract_s* c) {
  if (!c->row_steps.empty() || !c->row_maps.empty()) return "leaf sets are not supported with row axes.";
  if (!c->path_group) return "leaf sets need a path kernel: call tnco_hip_contract_set_path_kernel first.";
  if (c->accumulate) return "leaf sets are not supported with wide accumulation.";
  if (c->steps.empty()) return "leaf sets need a plan with steps.";
  return nullptr;
}

// f(ct_type<T>()) for the element type T of a handle of a plain dtype (codes 0 to 3)
template <class T>
struct ct_type {
  using type = T;
};
template <class F>
int with_plain_type(const tnco_hip_contract_s* c, F f) {
  switch (c->dtype) {
    case 0: return f(ct_type<float>());
    case 1: return f(ct_type<double>());
    case 2: return f(ct_type<cplx<float>>());
    default: return f(ct_type<cplx<double>>());
  }
}

// every counter of a run, and whose walkers it ran over, before the run starts
void zero_run_counters(tnco_hip_contract_s* c) {
  c->macs = c->launches = c->narrow_launches = c->batch_launches = c->split_launches = c->matrix_launches = c->last_member = 0;
  c->path_launches[0] = c->path_launches[1] = c->acc_launches[0] = c->acc_launches[1] = 0;
  c->sets_launches[0] = c->sets_launches[1] = 0;
  c->last_walk = 0;
  std::fill(std::begin(c->by_kernel), std::end(c->by_kernel), 0);
  std::fill(std::begin(c->by_row_kernel), std::end(c->by_row_kernel), 0);
  std::fill(std::begin(c->by_ix), std::end(c->by_ix), 0);
}

// Room for G members and n_sets outputs, and for the `tables` bytes of *d_tables once.  The new buffers first: a handle
// that this fails on stays as it was.  (The arenas and the staging hold nothing between runs.)  `what` needs the bytes.
int sets_room(tnco_hip_contract_s* c, int64_t n_sets, int64_t G, char** d_tables, size_t tables, const char* what) {
  const size_t arena = (size_t)c->arena_elems * c->elem, block = (size_t)c->block_numel * c->out_elem;
  const size_t outb = (size_t)c->out_numel * c->out_elem;
  const bool more_members = G > c->path_cap, more_out = n_sets > c->sets_out_cap, new_tables = !*d_tables;
  const size_t need = (more_members ? (size_t)G * (arena + block) : 0) + (more_out ? (size_t)n_sets * outb : 0) + (new_tables ? tables : 0);
  if (!need) return TNCO_HIP_OK;
  CT_TRY(hipStreamSynchronize(c->stream));
  size_t free_b = 0, total_b = 0;
  CT_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return fail(TNCO_HIP_ERUNTIME, std::string(what) + " need " + std::to_string(need) + " bytes of device memory, " +
                                       std::to_string(free_b) + " are free.");
  void *d_arena = nullptr, *d_stage = nullptr, *d_out = nullptr, *d_tab = nullptr;
  if ((more_members && (hipMalloc(&d_arena, std::max<size_t>((size_t)G * arena, c->elem)) != hipSuccess ||
                        hipMalloc(&d_stage, (size_t)G * block) != hipSuccess)) ||
      (more_out && hipMalloc(&d_out, (size_t)n_sets * outb) != hipSuccess) ||
      (new_tables && hipMalloc(&d_tab, tables) != hipSuccess)) {
    for (void* p : {d_arena, d_stage, d_out, d_tab})
      if (p) (void)hipFree(p);
    return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  if (more_members) {
    (void)hipFree(c->d_arena), (void)hipFree(c->d_path_stage);
    c->bytes += (G - c->path_cap) * (int64_t)(arena + block);
    c->d_arena = d_arena, c->d_path_stage = d_stage, c->path_cap = G;
  }
  if (more_out) {
    if (c->d_sets_out) (void)hipFree(c->d_sets_out);
    c->bytes += (n_sets - c->sets_out_cap) * (int64_t)outb;
    c->d_sets_out = d_out, c->sets_out_cap = n_sets;
  }
  if (new_tables) *d_tables = (char*)d_tab, c->bytes += (int64_t)tables;
  return TNCO_HIP_OK;
}

// What a run over leaf sets or walkers does before its first launch: room for G members and n_sets outputs (sets_room);
// the table of the leaves, `width` words per leaf that row(t, words) fills in, built in *image and uploaded to
// *d_tables; the outputs and the counters zeroed; the first event.
template <class Row>
int begin_sets_run(tnco_hip_contract_s* c, int64_t n_sets, int64_t G, char** d_tables, std::vector<int64_t>* image, int width,
                   const char* what, Row row) {
  const int64_t L = (int64_t)c->leaf_numel.size();
  static_assert(sizeof(void*) == sizeof(int64_t), "the pointers and the other words share one table");
  if (int rc = sets_room(c, n_sets, G, d_tables, (size_t)L * width * sizeof(int64_t), what)) return rc;
  image->assign(width * L, 0);
  for (int64_t t = 0; t < L; ++t) row(t, image->data() + width * t);
  CT_TRY(hipMemcpyAsync(*d_tables, image->data(), width * L * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  CT_TRY(hipMemsetAsync(c->d_sets_out, 0, (size_t)n_sets * c->out_numel * c->out_elem, c->stream));
  zero_run_counters(c);
  CT_TRY(hipEventRecord(c->ev[0], c->stream));
  return TNCO_HIP_OK;
}

int64_t n_assignments(const tnco_hip_contract_s* c) {
  int64_t n = 1;
  for (int64_t d : c->slice_dims) n *= d;
  return n;
}

// What tnco_hip_contract_set_hoist refuses beyond tnco_hip_contract_set_reuse (hoist), and the wording of each setter for
// the checks they share.
struct ScheduleRules {
  bool hoist;
  const char *out_step, *out_perm, *order, *leaf_perm, *leaf_step, *perm_source, *step_source;
};
const ScheduleRules HOIST_RULES = {true,
                                   "a hoisted step must write the arena.",
                                   "a hoisted permute must write the arena.",
                                   "the hoisted rows of a permute group must come first.",
                                   "a hoisted permute reads a leaf with a sliced axis.",
                                   "a hoisted step reads a leaf with a sliced axis.",
                                   "a permute and the item that writes its source must both be hoisted or both not.",
                                   "a hoisted step reads an arena tensor that no hoisted item wrote."};
const ScheduleRules REUSE_RULES = {false,
                                   "the step that writes the output must have period 1.",
                                   "the permute that writes the output must have period 1.",
                                   "the rows of a permute group must be ordered by period, the largest first.",
                                   "a permute is slower than a sliced leaf it reads allows.",
                                   "a step is slower than a sliced leaf it reads allows.",
                                   "a permute is slower than the item that wrote its source.",
                                   "a step is slower than the item that wrote its operand."};

// The schedule of the periods given (each one valid: a place, the number of assignments, or what set_hoist makes of a
// flag) into *s, or the text of what is wrong with them: nothing may be due less often than what it reads changes, and
// what a slower item left for a faster one must still be there when that one runs.
const char* make_schedule(const tnco_hip_contract_s* c, const int64_t* step_period, const int64_t* perm_period, const ScheduleRules& t,
                          Schedule* s) {
  const int64_t S = (int64_t)c->steps.size() / STEP_W, P = (int64_t)c->perms.size() / PERM_W, G = S + 1;
  for (int64_t k = 0; k < S; ++k)
    if (c->steps[k * STEP_W + ST_C_KIND] == K_OUT && step_period[k] != 1) return t.out_step;
  for (int64_t r = 0; r < P; ++r) {
    const int64_t* row = &c->perms[r * PERM_W];
    if (row[PM_DST_KIND] == K_OUT && perm_period[r] != 1) return t.out_perm;
    if (r && row[PM_GROUP] == row[PM_GROUP - PERM_W] && perm_period[r] > perm_period[r - 1]) return t.order;
  }
  // what a leaf allows an item that reads it: the smallest place of its sliced axes, everything without one (an axis of
  // dimension 1 has one value in every assignment and allows everything; not so for hoist flags, which take a leaf with
  // any sliced axis to change with the assignment)
  auto leaf_period = [&](int64_t leaf) {
    const int64_t* ls = &c->leaf_sl[leaf * LEAF_SL_W];
    int64_t per = t.hoist && ls[LS_COUNT] ? 1 : INT64_MAX;
    for (int j = 0; j < (int)ls[LS_COUNT]; ++j)
      if (c->slice_dims[ls[LS_SLOTS + j]] > 1) per = std::min(per, c->place[ls[LS_SLOTS + j]]);
    return per;
  };
  for (int64_t r = 0; r < P; ++r) {
    const int64_t* row = &c->perms[r * PERM_W];
    if (row[PM_SRC_KIND] == K_LEAF && perm_period[r] > leaf_period(row[PM_SRC_REF])) return t.leaf_perm;
  }
  for (int64_t k = 0; k < S; ++k)
    for (int side = 0; side < 2; ++side) {
      const int64_t* st = &c->steps[k * STEP_W];
      if (st[ST_SIDE * side + ST_A_KIND] == K_LEAF && step_period[k] > leaf_period(st[ST_SIDE * side + ST_A_REF])) return t.leaf_step;
    }
  // Replay the path: who wrote what an item reads.  A write: [lo, hi) of the arena and the period of its item, in path
  // order; read: an item has consumed it (every tensor has one reader) or nothing reads it (a staging buffer)
  struct Write {
    int64_t lo, hi, period;
    char read;
  };
  struct Kept {
    int64_t lo, hi;
    size_t writer;
  };
  std::vector<Write> writes;
  std::vector<Kept> kept;
  // The write an item of that period reads at ref, -1: none, and marks it read.  The phases run one after the other, so
  // an item sees the latest write of its own phase there, or else what the nearest slower phase kept; a write of a faster
  // phase is returned last, for the caller to refuse.  This rests on one property of a sound arena, which the check of
  // the kept tensors below enforces for what matters: when an item reads at ref, at most one unread write of its own
  // phase starts there (a buffer is written, read, and only then given to the next tensor of the phase), and a kept
  // tensor shares its start with no write of its own or a faster phase
  auto writer_of = [&](int64_t ref, int64_t period) -> int64_t {
    int64_t best = -1;
    for (int64_t w = (int64_t)writes.size() - 1; w >= 0; --w) {
      if (writes[w].lo != ref || writes[w].read) continue;
      if (writes[w].period == period) {
        best = w;
        break;
      }
      const bool slower = writes[w].period > period;
      if (best < 0 || (slower && (writes[best].period < period || writes[w].period < writes[best].period))) best = w;
    }
    if (best >= 0) writes[best].read = 1;
    return best;
  };
  const char* e = nullptr;
  // An item of that period reads [ref, ref + numel) of the arena: refused when a faster item wrote it; kept, and true, when
  // a slower one did.  Hoist flags refuse more: a flagged item that reads what no item wrote, and a permute of a kept
  // tensor (kept_opnd covers step operands only: in a slice batch such a permute would read the arena copy of its member)
  auto source = [&](int64_t ref, int64_t period, int64_t numel, bool perm) {
    const int64_t w = writer_of(ref, period);
    const bool slower = w >= 0 && writes[w].period > period;
    if (w < 0 ? t.hoist && period > 1 : writes[w].period < period || (slower && t.hoist && perm)) e = perm ? t.perm_source : t.step_source;
    else if (slower) kept.push_back(Kept{ref, ref + numel, (size_t)w});
    return slower && !e;
  };
  s->step_period.assign(step_period, step_period + S);
  s->kept_opnd.assign(2 * S, 0);
  std::vector<int64_t>& phase = s->phase;
  phase.assign(step_period, step_period + S);
  phase.insert(phase.end(), perm_period, perm_period + P);
  std::sort(phase.begin(), phase.end(), std::greater<int64_t>());
  phase.erase(std::unique(phase.begin(), phase.end()), phase.end());
  s->first.assign(phase.size() * G, 0), s->count.assign(phase.size() * G, 0), s->largest.assign(phase.size() * G, 0);
  auto perm_rows = [&](int64_t g) {  // the rows of permute group g
    for (int64_t r = c->group_first[g + 1], n = 0; n < c->group_count[g + 1] && !e; ++r, ++n) {
      const int64_t* row = &c->perms[r * PERM_W];
      const int64_t per = perm_period[r];
      if (row[PM_SRC_KIND] == K_ARENA) source(row[PM_SRC_REF], per, row[PM_NUMEL], true);
      if (row[PM_DST_KIND] == K_ARENA) writes.push_back(Write{row[PM_DST_REF], row[PM_DST_REF] + row[PM_NUMEL], per, 0});
      const int64_t at = (std::find(phase.begin(), phase.end(), per) - phase.begin()) * G + g + 1;
      if (!s->count[at]++) s->first[at] = r;
      s->largest[at] = std::max(s->largest[at], row[PM_NUMEL]);
    }
  };
  perm_rows(-1);
  for (int64_t k = 0; k < S && !e; ++k) {
    perm_rows(k);
    const int64_t* st = &c->steps[k * STEP_W];
    const auto [H, M, N, K] = step_shape(st);
    const int64_t nc = H * M * N;
    for (int side = 0; side < 2 && !e; ++side)
      if (st[ST_SIDE * side + ST_A_KIND] == K_ARENA)
        s->kept_opnd[2 * k + side] = source(st[ST_SIDE * side + ST_A_REF], step_period[k], H * K * (side ? N : M), false);
    if (st[ST_C_KIND] == K_ARENA) {
      writes.push_back(Write{st[ST_C_REF], st[ST_C_REF] + nc, step_period[k], 0});
      if (c->scaling) writes.push_back(Write{c->stage_refs[k], c->stage_refs[k] + 2 * nc, step_period[k], 1});
    }
  }
  if (e) return e;
  // a kept tensor stays until its writer is due again: no item of its writer's phase writes into it after the writer, and
  // no item of a faster phase at all (a slower phase may: whenever it is due, the writer is due after it)
  for (size_t q = 0; q < kept.size(); ++q) {
    const Write& own = writes[kept[q].writer];
    for (size_t w = 0; w < writes.size(); ++w)
      if (w != kept[q].writer && (writes[w].period < own.period || (writes[w].period == own.period && w > kept[q].writer)) &&
          writes[w].lo < kept[q].hi && kept[q].lo < writes[w].hi)
        return "a kept tensor is written over.";
  }
  return nullptr;
}

// What wide accumulation adds to stats[2] in mode `mode`: the accumulator, and the staging block of an unbatched run (a
// batch and the path kernel stage in their own buffers).  A plan without steps sums nothing and reserves nothing.
int64_t accumulate_bytes(const tnco_hip_contract_s* c, int mode) {
  if (!mode || c->steps.empty()) return 0;
  const bool own_stage = !c->batch && !c->path_group;
  return (int64_t)c->out_elem * (2 * c->out_numel + (own_stage ? c->block_numel : 0));
}

// a slice batch or a path kernel set after tnco_hip_contract_set_accumulate: the members' staging buffer takes its place
void drop_accumulate_stage(tnco_hip_contract_s* c) {
  if (c->d_acc_stage) (void)hipFree(c->d_acc_stage);
  c->d_acc_stage = nullptr;
}

// a host leaf (C-contiguous, in the handle's element type) into its leaf buffer, on the handle's stream; the caller
// synchronises
int load_host_leaf(tnco_hip_contract_s* c, int64_t t, const void* src) {
  CT_TRY(hipMemcpyAsync(c->d_leaves + c->leaf_off[t] * c->elem, src, (size_t)c->leaf_numel[t] * c->elem, hipMemcpyHostToDevice,
                        c->stream));
  c->loaded[t] = 1;
  return TNCO_HIP_OK;
}

// dtype code `from` is `to`, or one of the five exact widenings of contract_io.h
bool io_widens(int from, int to) {
  return from == to || (from == 0 && to >= 1) || (from == 1 && to == 3) || (from == 2 && to == 3);
}

template <class D, class S>
void launch_ingest_as(tnco_hip_contract_s* c, void* dst, const void* src, int64_t numel, const IoAxes& ax) {
  hipLaunchKernelGGL((ct_ingest_kernel<D, S>), dim3(io_blocks(numel, sizeof(D), ax.nd < 0)), dim3(256), 0, c->stream, (D*)dst,
                     (const S*)src, numel, ax);
}

// `src`, a caller's device memory of dtype code `from`, into `dst` of the handle's dtype (io_widens holds)
int launch_ingest(tnco_hip_contract_s* c, void* dst, const void* src, int from, int64_t numel, const IoAxes& ax) {
  using F = float;
  using Dd = double;
  using CF = cplx<float>;
  using CD = cplx<double>;
  switch (c->dtype * 4 + from) {
    case 0: launch_ingest_as<F, F>(c, dst, src, numel, ax); break;
    case 4: launch_ingest_as<Dd, F>(c, dst, src, numel, ax); break;
    case 5: launch_ingest_as<Dd, Dd>(c, dst, src, numel, ax); break;
    case 8: launch_ingest_as<CF, F>(c, dst, src, numel, ax); break;
    case 10: launch_ingest_as<CF, CF>(c, dst, src, numel, ax); break;
    case 12: launch_ingest_as<CD, F>(c, dst, src, numel, ax); break;
    case 13: launch_ingest_as<CD, Dd>(c, dst, src, numel, ax); break;
    case 14: launch_ingest_as<CD, CF>(c, dst, src, numel, ax); break;
    case 15: launch_ingest_as<CD, CD>(c, dst, src, numel, ax); break;
    default: return fail(TNCO_HIP_EINVAL, "'src_dtype' does not widen to the plan's dtype.");
  }
  CT_TRY(hipGetLastError());
  c->io_launches[0] += 1;
  return TNCO_HIP_OK;
}

// launch_ingest of a source whose axes io_axes gave as `ax` and `contiguous`: a contiguous one is one axis, and of the
// plan's dtype it takes the vector path
int ingest_source(tnco_hip_contract_s* c, void* dst, const void* src, int from, int64_t numel, IoAxes ax, bool contiguous) {
  if (contiguous) {
    ax.nd = from == c->dtype ? -1 : 1;
    ax.dim[0] = numel, ax.stride[0] = 1;
  }
  return launch_ingest(c, dst, src, from, numel, ax);
}

template <class T>
void launch_emit_as(tnco_hip_contract_s* c, void* dst, const IoAxes& ax, const void* src, int64_t numel) {
  hipLaunchKernelGGL(ct_emit_kernel<T>, dim3(io_blocks(numel, sizeof(T), ax.nd < 0)), dim3(256), 0, c->stream, (T*)dst,
                     (const T*)src, numel, ax);
}

// the output buffer (leaf sets: `sets` of them, back to back) into `dst`, a caller's device memory of the output's type
// (a storage dtype: float32 / complex64)
int launch_emit(tnco_hip_contract_s* c, void* dst, const IoAxes& ax, int64_t sets = 0) {
  const void* src = sets ? c->d_sets_out : c->d_out;
  const int64_t numel = c->out_numel * std::max<int64_t>(sets, 1);
  switch (c->dtype) {
    case 1: launch_emit_as<double>(c, dst, ax, src, numel); break;
    case 3: launch_emit_as<cplx<double>>(c, dst, ax, src, numel); break;
    case 2: case 5: case 7: launch_emit_as<cplx<float>>(c, dst, ax, src, numel); break;
    default: launch_emit_as<float>(c, dst, ax, src, numel);
  }
  CT_TRY(hipGetLastError());
  c->io_launches[1] += 1;
  return TNCO_HIP_OK;
}

// A stack [n][leaf_numel] of leaf `leaf` from `src` into *buf, which has room for *cap of them and grows to n (the new
// buffer first, so that a failure leaves the old one); *held: how many the buffer holds, 0 while it holds none whole.
int load_stack(tnco_hip_contract_s* c, int64_t leaf, int64_t n, const void* src, int32_t where, int32_t src_dtype, int64_t ndim,
               const int64_t* dims, const int64_t* strides, void** buf, int64_t* cap, int64_t* held, const char* dims_text) {
  const int64_t leaf_numel = c->leaf_numel[leaf];
  const int64_t numel = n * leaf_numel;
  IoAxes ax;
  bool contiguous = false;
  if (const char* e = io_axes(ndim, dims, strides, numel, dims_text, &ax, &contiguous)) return fail(TNCO_HIP_EINVAL, e);
  if (where == 0) {
    if (src_dtype != c->dtype) return fail(TNCO_HIP_EINVAL, "a host stack must have the plan's dtype.");
    if (strides) return fail(TNCO_HIP_EINVAL, "a host stack must be C-contiguous: 'strides' must be NULL.");
  } else if (src_dtype < 0 || src_dtype > 3 || !io_widens(src_dtype, c->dtype)) {
    return fail(TNCO_HIP_EINVAL, "'src_dtype' does not widen to the plan's dtype.");
  }
  CT_TRY(hipSetDevice(c->device));
  if (n > *cap) {
    const size_t bytes = (size_t)numel * c->elem;
    size_t free_b = 0, total_b = 0;
    CT_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b)
      return fail(TNCO_HIP_ERUNTIME, "the stack needs " + std::to_string(bytes) + " bytes of device memory, " +
                                         std::to_string(free_b) + " are free.");
    void* d_new = nullptr;
    if (hipMalloc(&d_new, bytes) != hipSuccess) return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
    if (*buf) (void)hipFree(*buf);
    c->bytes += (n - *cap) * leaf_numel * (int64_t)c->elem;
    *buf = d_new, *cap = n, *held = 0;
  }
  if (where == 0) {
    CT_TRY(hipMemcpyAsync(*buf, src, (size_t)numel * c->elem, hipMemcpyHostToDevice, c->stream));
  } else if (int rc = ingest_source(c, *buf, src, src_dtype, numel, ax, contiguous)) {
    return rc;
  }
  CT_TRY(hipStreamSynchronize(c->stream));
  *held = n;
  return TNCO_HIP_OK;
}

// The axes of a result of `numel` elements in a caller's device memory: no stride 0, and a contiguous one takes the
// vector path.  dims_text: what is said of dims that do not multiply to numel.
int dest_axes(int64_t ndim, const int64_t* dims, const int64_t* dst_strides, int64_t numel, const char* dims_text, IoAxes* ax) {
  if (ndim && !dst_strides) return fail(TNCO_HIP_EINVAL, "null argument.");
  bool contiguous = false;
  if (const char* e = io_axes(ndim, dims, dst_strides, numel, dims_text, ax, &contiguous)) return fail(TNCO_HIP_EINVAL, e);
  for (int k = 0; k < ax->nd; ++k)
    if (ax->dim[k] > 1 && ax->stride[k] == 0) return fail(TNCO_HIP_EINVAL, "a destination stride is 0.");
  if (contiguous) ax->nd = -1;
  return TNCO_HIP_OK;
}

// What a run does after its last kernel: the second event; the result (sets == 0: the output buffer, else `sets` outputs
// of d_sets_out) to `out` -- through ct_emit_kernel into a caller's device memory with the axes *emit, as it lies into
// host memory when emit == nullptr, nowhere when out == nullptr --; the wait; the time between the events.
int finish_run(tnco_hip_contract_s* c, void* out, const IoAxes* emit, int64_t sets = 0) {
  CT_TRY(hipEventRecord(c->ev[1], c->stream));
  if (emit) {
    if (int rc = launch_emit(c, out, *emit, sets)) return rc;
  } else if (out) {
    CT_TRY(hipMemcpyAsync(out, sets ? c->d_sets_out : c->d_out, (size_t)std::max<int64_t>(sets, 1) * c->out_numel * c->out_elem,
                          hipMemcpyDeviceToHost, c->stream));
  }
  CT_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  CT_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  c->device_ns = (int64_t)((double)ms * 1e6);
  return TNCO_HIP_OK;
}

// The run over the leaves that the leaf buffers hold, from the zeroing of the output on.  emit == nullptr: `out` is host
// memory and gets the raw output buffer; otherwise `out` is a caller's device memory and ct_emit_kernel writes it
int run_loaded(tnco_hip_contract_s* c, void* out, const IoAxes* emit) {
  CT_TRY(hipMemsetAsync(c->d_out, 0, (size_t)c->out_numel * c->out_elem, c->stream));
  const size_t n_steps = c->steps.size() / STEP_W;
  if (c->d_acc) CT_TRY(hipMemsetAsync(c->d_acc, 0, (size_t)c->out_numel * 2 * c->out_elem, c->stream));
  if (c->scaling && !c->leaf_exps.empty()) {
    if (c->batch && n_steps) {  // every member's copy of the slots starts with the same leaf exponents
      const size_t n_slots = c->leaf_exps.size() + n_steps;
      c->exps_image.assign((size_t)c->batch * n_slots, 0);
      for (int64_t b = 0; b < c->batch; ++b) std::copy(c->leaf_exps.begin(), c->leaf_exps.end(), c->exps_image.begin() + b * n_slots);
      CT_TRY(hipMemcpyAsync(c->d_exps, c->exps_image.data(), c->exps_image.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    } else {
      CT_TRY(hipMemcpyAsync(c->d_exps, c->leaf_exps.data(), c->leaf_exps.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
  }
  zero_run_counters(c);
  CT_TRY(hipEventRecord(c->ev[0], c->stream));
  const bool fused = c->path_group > 0 && n_steps > 0;  // (a plan without steps runs as it does without the call)
  auto plain = [&](auto t) {  // (a path kernel is set on a plain dtype only)
    using T = typename decltype(t)::type;
    return fused ? run_path<T>(c) : run_impl<T>(c);
  };
  int rc = c->dtype < 4    ? with_plain_type(c, plain)
           : c->dtype == 4 ? run_impl<float, st_f16>(c)
           : c->dtype == 5 ? run_impl<cplx<float>, cplx<st_f16>>(c)
           : c->dtype == 6 ? run_impl<float, st_bf16>(c)
                           : run_impl<cplx<float>, cplx<st_bf16>>(c);
  if (rc) return rc;
  return finish_run(c, out, emit);
}

}  // namespace

extern "C" {

int tnco_hip_contract_create(const tnco_hip_contract_desc* d, tnco_hip_contract* out) {
  if (!d || !out) return fail(TNCO_HIP_EINVAL, "null argument.");
  *out = nullptr;
  auto* c = new tnco_hip_contract_s();
  if (const char* e = validate(c, d)) {
    delete c;
    return fail(TNCO_HIP_EINVAL, e);
  }
  const std::vector<int64_t> ones(std::max(c->steps.size() / STEP_W, c->perms.size() / PERM_W), 1);
  (void)make_schedule(c, ones.data(), ones.data(), REUSE_RULES, &c->sched);  // every period 1: nothing there to refuse
  static const size_t elem[8] = {4, 8, 8, 16, 2, 4, 2, 4}, out_elem[8] = {4, 8, 8, 16, 4, 8, 4, 8};
  c->dtype = d->dtype, c->elem = elem[d->dtype], c->out_elem = out_elem[d->dtype], c->device = d->device;
  c->loaded.assign(c->leaf_numel.size(), 0);
  c->d_stack.assign(c->leaf_numel.size(), nullptr);
  c->stack_cap.assign(c->leaf_numel.size(), 0), c->stack_sets.assign(c->leaf_numel.size(), 0);
  c->d_versions.assign(c->leaf_numel.size(), nullptr);
  c->versions_cap.assign(c->leaf_numel.size(), 0), c->versions.assign(c->leaf_numel.size(), 0);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || d->device < 0 || d->device >= ndev) {
    delete c;
    return fail(TNCO_HIP_EINVAL, "'device' is not valid.");
  }
  const size_t n_tab = c->perms.size() + c->leaf_sl.size() + c->place.size() + c->slice_dims.size();
  const size_t leaves = (size_t)c->leaf_off.back() * c->elem;
  const size_t arena = (size_t)std::max<int64_t>(c->arena_elems, 1) * c->elem, outb = (size_t)c->out_numel * c->out_elem;
  const size_t ptrs = std::max<size_t>(c->leaf_numel.size(), 1) * sizeof(void*);
  const size_t maps = c->row_maps.size() * sizeof(int32_t);
  const size_t n_slots = c->leaf_numel.size() + c->steps.size() / STEP_W, n_words = c->steps.size() / STEP_W;
  const size_t scale_b = c->scaling ? 4 * (n_slots + n_words) : 0;  // exponent slots, then the steps' max words
  c->bytes = c->base_bytes = (int64_t)(leaves + arena + outb + n_tab * 8 + ptrs + maps + scale_b);
  auto bail = [&](int code, const std::string& msg) {
    tnco_hip_contract_destroy(c);
    return fail(code, msg);
  };
  if (hipSetDevice(d->device) != hipSuccess) return bail(TNCO_HIP_ERUNTIME, "hipSetDevice failed.");
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return bail(TNCO_HIP_ERUNTIME, "hipMemGetInfo failed.");
  if ((size_t)c->bytes > free_b)
    return bail(TNCO_HIP_ERUNTIME, "the contraction needs " + std::to_string(c->bytes) + " bytes of device memory, " +
                                       std::to_string(free_b) + " are free.");
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev[0]) != hipSuccess || hipEventCreate(&c->ev[1]) != hipSuccess ||
      hipMalloc((void**)&c->d_leaves, std::max<size_t>(leaves, 64)) != hipSuccess ||
      hipMalloc(&c->d_arena, arena) != hipSuccess || hipMalloc(&c->d_out, outb) != hipSuccess ||
      hipMalloc((void**)&c->d_tables, std::max<size_t>(n_tab, 1) * 8) != hipSuccess ||
      hipMalloc((void**)&c->d_leaf_ptrs, ptrs) != hipSuccess ||
      (maps && hipMalloc((void**)&c->d_row_maps, maps) != hipSuccess) ||
      (c->scaling && hipMalloc((void**)&c->d_exps, std::max<size_t>(scale_b, 4)) != hipSuccess))
    return bail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  if (c->scaling) {
    c->d_amax = (uint32_t*)(c->d_exps + n_slots);
    c->leaf_exps.assign(c->leaf_numel.size(), 0);
    if (hipMemsetAsync(c->d_exps, 0, std::max<size_t>(scale_b, 4), c->stream) != hipSuccess)
      return bail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  std::vector<int64_t> tab;
  tab.reserve(n_tab);
  for (auto* v : {&c->perms, &c->leaf_sl, &c->place, &c->slice_dims}) tab.insert(tab.end(), v->begin(), v->end());
  std::vector<void*> lp(c->leaf_numel.size());
  for (size_t t = 0; t < lp.size(); ++t) lp[t] = c->d_leaves + c->leaf_off[t] * c->elem;
  // on the handle's own stream: a plain hipMemcpy from pageable memory may return before its DMA lands, and the
  // non-blocking stream of the kernels would not wait for it
  if ((n_tab && hipMemcpyAsync(c->d_tables, tab.data(), n_tab * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
      (!lp.empty() && hipMemcpyAsync(c->d_leaf_ptrs, lp.data(), lp.size() * sizeof(void*), hipMemcpyHostToDevice,
                                     c->stream) != hipSuccess) ||
      (maps && hipMemcpyAsync(c->d_row_maps, c->row_maps.data(), maps, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return bail(TNCO_HIP_ERUNTIME, "copy of the plan failed.");
  *out = c;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_run(tnco_hip_contract c, const void* const* leaves, void* out) {
  if (!c || !out || (!leaves && !c->leaf_numel.empty())) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (c->folded && c->ind_steps.empty())
    return fail(TNCO_HIP_EINVAL, "the plan has folded operands: call tnco_hip_contract_set_indirect before the run.");
  CT_TRY(hipSetDevice(c->device));
  for (size_t t = 0; t < c->leaf_numel.size(); ++t) {
    if (!leaves[t]) return fail(TNCO_HIP_EINVAL, "null leaf.");
    if (int rc = load_host_leaf(c, (int64_t)t, leaves[t])) return rc;
  }
  return run_loaded(c, out, nullptr);
}

int tnco_hip_contract_load_leaf(tnco_hip_contract c, int64_t leaf, const void* src, int32_t where, int32_t src_dtype,
                                int64_t ndim, const int64_t* dims, const int64_t* strides) {
  if (!c || !src) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (leaf < 0 || leaf >= (int64_t)c->leaf_numel.size()) return fail(TNCO_HIP_EINVAL, "'leaf' is not a leaf of the plan.");
  if (where != 0 && where != 1) return fail(TNCO_HIP_EINVAL, "'where' must be 0 (host) or 1 (device).");
  IoAxes ax;
  bool contiguous = false;
  if (const char* e = io_axes(ndim, dims, strides, c->leaf_numel[leaf], "dims do not multiply to the leaf's elements.", &ax, &contiguous))
    return fail(TNCO_HIP_EINVAL, e);
  if (where == 0) {
    if (src_dtype != c->dtype) return fail(TNCO_HIP_EINVAL, "a host leaf must have the plan's dtype.");
    if (strides) return fail(TNCO_HIP_EINVAL, "a host leaf must be C-contiguous: 'strides' must be NULL.");
    CT_TRY(hipSetDevice(c->device));
    if (int rc = load_host_leaf(c, leaf, src)) return rc;
    CT_TRY(hipStreamSynchronize(c->stream));
    return TNCO_HIP_OK;
  }
  if (c->dtype > 3 || c->scaling)
    return fail(TNCO_HIP_EINVAL, "a device leaf is not supported with a storage dtype or scaling.");
  if (src_dtype < 0 || src_dtype > 3 || !io_widens(src_dtype, c->dtype))
    return fail(TNCO_HIP_EINVAL, "'src_dtype' does not widen to the plan's dtype.");
  CT_TRY(hipSetDevice(c->device));
  if (int rc = ingest_source(c, c->d_leaves + c->leaf_off[leaf] * c->elem, src, src_dtype, c->leaf_numel[leaf], ax, contiguous))
    return rc;
  CT_TRY(hipStreamSynchronize(c->stream));
  c->loaded[leaf] = 1;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_run_loaded(tnco_hip_contract c, void* out, int32_t where, int64_t ndim, const int64_t* dims,
                                 const int64_t* dst_strides) {
  if (!c || !out) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (where != 0 && where != 1) return fail(TNCO_HIP_EINVAL, "'where' must be 0 (host) or 1 (device).");
  if (c->folded && c->ind_steps.empty())
    return fail(TNCO_HIP_EINVAL, "the plan has folded operands: call tnco_hip_contract_set_indirect before the run.");
  IoAxes ax;
  if (where == 1) {
    if (!c->row_steps.empty() || !c->row_maps.empty())
      return fail(TNCO_HIP_EINVAL, "a device result is not supported with row axes.");
    if (int rc = dest_axes(ndim, dims, dst_strides, c->out_numel, "dims do not multiply to the output's elements.", &ax)) return rc;
  }
  for (size_t t = 0; t < c->loaded.size(); ++t)
    if (!c->loaded[t]) return fail(TNCO_HIP_EINVAL, "leaf " + std::to_string(t) + " was never loaded.");
  CT_TRY(hipSetDevice(c->device));
  return run_loaded(c, out, where == 1 ? &ax : nullptr);
}

int tnco_hip_contract_io_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  counts[0] = c->io_launches[0], counts[1] = c->io_launches[1];
  return TNCO_HIP_OK;
}

int tnco_hip_contract_load_leaf_sets(tnco_hip_contract c, int64_t leaf, int64_t n_sets, const void* src, int32_t where,
                                     int32_t src_dtype, int64_t ndim, const int64_t* dims, const int64_t* strides) {
  if (!c || !src) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (leaf < 0 || leaf >= (int64_t)c->leaf_numel.size()) return fail(TNCO_HIP_EINVAL, "'leaf' is not a leaf of the plan.");
  if (n_sets < 1) return fail(TNCO_HIP_EINVAL, "'n_sets' must be at least 1.");
  if (const char* e = sets_refusal(c)) return fail(TNCO_HIP_EINVAL, e);
  if (where != 0 && where != 1) return fail(TNCO_HIP_EINVAL, "'where' must be 0 (host) or 1 (device).");
  if (n_sets > (INT64_MAX >> 8) / c->leaf_numel[leaf]) return fail(TNCO_HIP_EINVAL, "'n_sets' is too large.");
  return load_stack(c, leaf, n_sets, src, where, src_dtype, ndim, dims, strides, &c->d_stack[leaf], &c->stack_cap[leaf],
                    &c->stack_sets[leaf], "dims do not multiply to the sets' elements.");
}

int tnco_hip_contract_run_sets(tnco_hip_contract c, int64_t n_sets, int64_t group, void* out, int32_t where, int64_t ndim,
                               const int64_t* dims, const int64_t* dst_strides) {
  if (!c || !out) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (n_sets < 1) return fail(TNCO_HIP_EINVAL, "'n_sets' must be at least 1.");
  if (group < 1 || group > MAX_PATH_GROUP) return fail(TNCO_HIP_EINVAL, "'group' must be from 1 to 1024.");
  if (const char* e = sets_refusal(c)) return fail(TNCO_HIP_EINVAL, e);
  if (where != 0 && where != 1) return fail(TNCO_HIP_EINVAL, "'where' must be 0 (host) or 1 (device).");
  const int64_t A = c->stop - c->start, L = (int64_t)c->leaf_numel.size();
  if (n_sets > (INT64_MAX >> 8) / std::max(c->out_numel, A)) return fail(TNCO_HIP_EINVAL, "'n_sets' is too large.");
  IoAxes ax;
  if (where == 1)
    if (int rc = dest_axes(ndim, dims, dst_strides, n_sets * c->out_numel, "dims do not multiply to the sets' outputs.", &ax)) return rc;
  for (int64_t t = 0; t < L; ++t) {
    if (c->stack_sets[t] && c->stack_sets[t] != n_sets)
      return fail(TNCO_HIP_EINVAL, "leaf " + std::to_string(t) + " has a stack of " + std::to_string(c->stack_sets[t]) +
                                       " sets loaded, not of " + std::to_string(n_sets) + ".");
    if (!c->stack_sets[t] && !c->loaded[t]) return fail(TNCO_HIP_EINVAL, "leaf " + std::to_string(t) + " was never loaded.");
  }
  CT_TRY(hipSetDevice(c->device));
  // room for min(group, members) members and n_sets outputs; the tables once
  const int64_t G = std::min(group, n_sets * A);
  auto row = [&](int64_t t, int64_t* words) {  // the leaf's pointer (its stack, or its single buffer), its set stride
    words[SET_PTR] = (int64_t)(uintptr_t)(c->stack_sets[t] ? c->d_stack[t] : (void*)(c->d_leaves + c->leaf_off[t] * c->elem));
    words[SET_STRIDE] = c->stack_sets[t] ? c->leaf_numel[t] : 0;
  };
  if (int rc = begin_sets_run(c, n_sets, G, &c->d_sets_tables, &c->sets_image, SET_W, "the leaf sets", row)) return rc;
  SetsArgs s{};
  s.set_leaves = (const int64_t*)c->d_sets_tables;
  if (int rc = with_plain_type(c, [&](auto t) {
        using T = typename decltype(t)::type;
        return run_set_members<T>(c, n_sets, G, s, ct_sets_path_kernel<T>);
      }))
    return rc;
  if (int rc = finish_run(c, out, where == 1 ? &ax : nullptr, n_sets)) return rc;
  std::fill(c->stack_sets.begin(), c->stack_sets.end(), 0);  // the stacks were for this run
  return TNCO_HIP_OK;
}

int tnco_hip_contract_sets_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  counts[0] = c->sets_launches[0], counts[1] = c->sets_launches[1];
  return TNCO_HIP_OK;
}

int tnco_hip_contract_load_leaf_versions(tnco_hip_contract c, int64_t leaf, int64_t n_versions, const void* src, int32_t where,
                                         int32_t src_dtype, int64_t ndim, const int64_t* dims, const int64_t* strides) {
  if (!c || !src) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (leaf < 0 || leaf >= (int64_t)c->leaf_numel.size()) return fail(TNCO_HIP_EINVAL, "'leaf' is not a leaf of the plan.");
  if (n_versions != 2) return fail(TNCO_HIP_EINVAL, "'n_versions' must be 2.");
  if (const char* e = sets_refusal(c)) return fail(TNCO_HIP_EINVAL, e);
  if (where != 0 && where != 1) return fail(TNCO_HIP_EINVAL, "'where' must be 0 (host) or 1 (device).");
  return load_stack(c, leaf, n_versions, src, where, src_dtype, ndim, dims, strides, &c->d_versions[leaf], &c->versions_cap[leaf],
                    &c->versions[leaf], "dims do not multiply to the versions' elements.");
}

int tnco_hip_contract_run_walkers(tnco_hip_contract c, tnco_hip_walkers w, const int64_t* leaf_qubit, int64_t group) {
  if (!c || !w || (!leaf_qubit && !c->leaf_numel.empty())) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (group < 1 || group > MAX_PATH_GROUP) return fail(TNCO_HIP_EINVAL, "'group' must be from 1 to 1024.");
  if (const char* e = sets_refusal(c)) return fail(TNCO_HIP_EINVAL, e);
  if (w->device != c->device)
    return fail(TNCO_HIP_EINVAL, "the walkers are on device " + std::to_string(w->device) + ", the handle on device " +
                                     std::to_string(c->device) + ".");
  const int64_t A = c->stop - c->start, L = (int64_t)c->leaf_numel.size();
  if (w->n_walkers > (INT64_MAX >> 8) / std::max(c->out_numel, A)) return fail(TNCO_HIP_EINVAL, "there are too many walkers.");
  bool any_indexed = false;
  for (int64_t t = 0; t < L; ++t) {
    any_indexed |= leaf_qubit[t] >= 0;
    if (leaf_qubit[t] < -1 || leaf_qubit[t] >= w->n_qubits)
      return fail(TNCO_HIP_EINVAL, "the qubit " + std::to_string(leaf_qubit[t]) + " of leaf " + std::to_string(t) +
                                       " is not -1 or a qubit of the walkers (0 to " + std::to_string(w->n_qubits - 1) + ").");
    if (leaf_qubit[t] >= 0 && !c->versions[t]) return fail(TNCO_HIP_EINVAL, "leaf " + std::to_string(t) + " has no versions loaded.");
    if (leaf_qubit[t] < 0 && !c->loaded[t]) return fail(TNCO_HIP_EINVAL, "leaf " + std::to_string(t) + " was never loaded.");
  }
  CT_TRY(hipSetDevice(c->device));
  // without an indexed leaf no output depends on the walker: one set is run, and every walker reads its output
  const int64_t R = any_indexed ? w->n_walkers : 1;
  const int64_t G = std::min(group, R * A);
  auto row = [&](int64_t t, int64_t* words) {  // the leaf's pointer (its versions, or its single buffer), qubit, version stride
    const bool indexed = leaf_qubit[t] >= 0;
    words[WK_PTR] = (int64_t)(uintptr_t)(indexed ? c->d_versions[t] : (void*)(c->d_leaves + c->leaf_off[t] * c->elem));
    words[WK_QUBIT] = leaf_qubit[t];
    words[WK_STRIDE] = indexed ? c->leaf_numel[t] : 0;
  };
  if (int rc = begin_sets_run(c, R, G, &c->d_walk_tables, &c->walk_image, WALK_W, "the walkers", row)) return rc;
  WalkArgs s{};
  s.walk_leaves = (const int64_t*)c->d_walk_tables;
  s.bits = w->d_bits, s.n_walkers = w->n_walkers;
  if (int rc = with_plain_type(c, [&](auto t) {
        using T = typename decltype(t)::type;
        return run_set_members<T>(c, R, G, s, ct_walk_path_kernel<T>);
      }))
    return rc;
  if (int rc = finish_run(c, nullptr, nullptr)) return rc;
  c->last_walk = w->id, c->walk_sets = R;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_walkers_output(tnco_hip_contract c, tnco_hip_walkers w, void* out) {
  if (!c || !w || !out) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (c->last_walk != w->id)
    return fail(TNCO_HIP_EINVAL, "the handle's last run was not a tnco_hip_contract_run_walkers over these walkers.");
  CT_TRY(hipSetDevice(c->device));
  CT_TRY(hipMemcpyAsync(out, c->d_sets_out, (size_t)c->walk_sets * c->out_numel * c->out_elem, hipMemcpyDeviceToHost, c->stream));
  CT_TRY(hipStreamSynchronize(c->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_create(int32_t device, int64_t n_walkers, int64_t n_qubits, uint64_t seed, tnco_hip_walkers* out) {
  if (!out) return fail(TNCO_HIP_EINVAL, "null argument.");
  *out = nullptr;
  if (n_walkers < 1) return fail(TNCO_HIP_EINVAL, "'n_walkers' must be at least 1.");
  if (n_qubits < 1) return fail(TNCO_HIP_EINVAL, "'n_qubits' must be at least 1.");
  if (n_walkers > ((int64_t)1 << 40) / n_qubits) return fail(TNCO_HIP_EINVAL, "the table of bits is too large (2^40 at the most).");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(TNCO_HIP_EINVAL, "'device' is not valid.");
  CT_TRY(hipSetDevice(device));
  const size_t table = (size_t)n_walkers * n_qubits, perm = WALK_MAX_PERMUTE * sizeof(int64_t) + ((size_t)1 << WALK_MAX_PERMUTE);
  size_t free_b = 0, total_b = 0;
  CT_TRY(hipMemGetInfo(&free_b, &total_b));
  if (table + (size_t)n_walkers + perm > free_b)
    return fail(TNCO_HIP_ERUNTIME, "the walkers need " + std::to_string(table + (size_t)n_walkers + perm) +
                                       " bytes of device memory, " + std::to_string(free_b) + " are free.");
  static std::atomic<uint64_t> next_id{0};  // (walkers may be created from several threads at once)
  auto* w = new tnco_hip_walkers_s();
  w->device = device, w->n_walkers = n_walkers, w->n_qubits = n_qubits, w->seed = seed, w->id = ++next_id;
  if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void**)&w->d_bits, table) != hipSuccess || hipMalloc((void**)&w->d_dead, (size_t)n_walkers) != hipSuccess ||
      hipMalloc((void**)&w->d_perm, perm) != hipSuccess || hipMemsetAsync(w->d_bits, 0, table, w->stream) != hipSuccess ||
      hipMemsetAsync(w->d_dead, 0, (size_t)n_walkers, w->stream) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) {
    tnco_hip_walkers_destroy(w);
    return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  *out = w;
  return TNCO_HIP_OK;
}

void tnco_hip_walkers_destroy(tnco_hip_walkers w) {
  if (!w) return;
  if (w->stream) (void)hipStreamSynchronize(w->stream);
  for (void* p : {(void*)w->d_bits, (void*)w->d_dead, (void*)w->d_perm})
    if (p) (void)hipFree(p);
  if (w->stream) (void)hipStreamDestroy(w->stream);
  delete w;
}

int tnco_hip_walkers_read(tnco_hip_walkers w, uint8_t* bits_out, uint8_t* dead_out) {
  if (!w || (!bits_out && !dead_out)) return fail(TNCO_HIP_EINVAL, "null argument.");
  CT_TRY(hipSetDevice(w->device));
  if (bits_out) CT_TRY(hipMemcpyAsync(bits_out, w->d_bits, (size_t)w->n_walkers * w->n_qubits, hipMemcpyDeviceToHost, w->stream));
  if (dead_out) CT_TRY(hipMemcpyAsync(dead_out, w->d_dead, (size_t)w->n_walkers, hipMemcpyDeviceToHost, w->stream));
  CT_TRY(hipStreamSynchronize(w->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_write(tnco_hip_walkers w, const uint8_t* bits_in) {
  if (!w || !bits_in) return fail(TNCO_HIP_EINVAL, "null argument.");
  const size_t table = (size_t)w->n_walkers * w->n_qubits;
  for (size_t e = 0; e < table; ++e)
    if (bits_in[e] > 1) return fail(TNCO_HIP_EINVAL, "a bit is neither 0 nor 1.");
  CT_TRY(hipSetDevice(w->device));
  CT_TRY(hipMemcpyAsync(w->d_bits, bits_in, table, hipMemcpyHostToDevice, w->stream));
  CT_TRY(hipStreamSynchronize(w->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_reset(tnco_hip_walkers w) {
  if (!w) return fail(TNCO_HIP_EINVAL, "null argument.");
  CT_TRY(hipSetDevice(w->device));
  CT_TRY(hipMemsetAsync(w->d_bits, 0, (size_t)w->n_walkers * w->n_qubits, w->stream));
  CT_TRY(hipMemsetAsync(w->d_dead, 0, (size_t)w->n_walkers, w->stream));
  CT_TRY(hipStreamSynchronize(w->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_choose(tnco_hip_walkers w, tnco_hip_contract c, int64_t qubit, int64_t step) {
  if (!w || !c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (c->last_walk != w->id)
    return fail(TNCO_HIP_EINVAL, "the handle's last run was not a tnco_hip_contract_run_walkers over these walkers.");
  if (c->out_numel != 2)
    return fail(TNCO_HIP_EINVAL, "the output of the handle holds " + std::to_string(c->out_numel) + " elements, not the 2 amplitudes of a choice.");
  if (qubit < 0 || qubit >= w->n_qubits)
    return fail(TNCO_HIP_EINVAL, "'qubit' is not a qubit of the walkers (0 to " + std::to_string(w->n_qubits - 1) + ").");
  if (step < 0 || step > (int64_t)UINT32_MAX) return fail(TNCO_HIP_EINVAL, "'step' must be from 0 to 2^32 - 1.");
  CT_TRY(hipSetDevice(w->device));
  // (the run has synchronised the handle's stream: its outputs are there)
  const dim3 grid((unsigned)std::min<int64_t>((w->n_walkers + 255) / 256, 65536));
  uint8_t* row = w->d_bits + qubit * w->n_walkers;
  const int64_t each = c->walk_sets == 1 ? 0 : 2;  // elements between two walkers' amplitudes (one output for all: 0)
  switch (c->dtype) {
    case 0: hipLaunchKernelGGL(ct_walk_choose_kernel<float>, grid, dim3(256), 0, w->stream, row, w->d_dead, (const float*)c->d_sets_out, each, w->n_walkers, w->seed, (uint32_t)step); break;
    case 1: hipLaunchKernelGGL(ct_walk_choose_kernel<double>, grid, dim3(256), 0, w->stream, row, w->d_dead, (const double*)c->d_sets_out, each, w->n_walkers, w->seed, (uint32_t)step); break;
    case 2: hipLaunchKernelGGL(ct_walk_choose_kernel<cplx<float>>, grid, dim3(256), 0, w->stream, row, w->d_dead, (const cplx<float>*)c->d_sets_out, each, w->n_walkers, w->seed, (uint32_t)step); break;
    default: hipLaunchKernelGGL(ct_walk_choose_kernel<cplx<double>>, grid, dim3(256), 0, w->stream, row, w->d_dead, (const cplx<double>*)c->d_sets_out, each, w->n_walkers, w->seed, (uint32_t)step);
  }
  CT_TRY(hipGetLastError());
  CT_TRY(hipStreamSynchronize(w->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_choose_joint(tnco_hip_walkers w, tnco_hip_contract c, int64_t k, const int64_t* qubits, const int64_t* strides,
                                  int64_t step) {
  if (!w || !c || !qubits || !strides) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (c->last_walk != w->id)
    return fail(TNCO_HIP_EINVAL, "the handle's last run was not a tnco_hip_contract_run_walkers over these walkers.");
  if (k < 1 || k > WALK_MAX_CHOOSE) return fail(TNCO_HIP_EINVAL, "'k' must be from 1 to 6.");
  const int64_t n = (int64_t)1 << k;
  if (c->out_numel != n)
    return fail(TNCO_HIP_EINVAL, "the output of the handle holds " + std::to_string(c->out_numel) + " elements, not the " +
                                     std::to_string(n) + " amplitudes of a joint choice of " + std::to_string(k) + " qubits.");
  for (int64_t j = 0; j < k; ++j) {
    if (qubits[j] < 0 || qubits[j] >= w->n_qubits)
      return fail(TNCO_HIP_EINVAL, "a qubit is not a qubit of the walkers (0 to " + std::to_string(w->n_qubits - 1) + ").");
    if (std::count(qubits, qubits + j, qubits[j])) return fail(TNCO_HIP_EINVAL, "a qubit is named twice.");
  }
  WalkChoose a{};
  bool natural = true;
  int64_t seen = 0;  // the strides met, a bit each
  for (int64_t j = 0; j < k; ++j) {
    const int64_t s = strides[j];
    if (s < 1 || s >= n || (s & (s - 1)) || (seen & s)) return fail(TNCO_HIP_EINVAL, "'strides' is not a permutation of 1, 2, ..., 2^(k - 1).");
    seen |= s;
    natural &= s == (int64_t)1 << (k - 1 - j);
    a.qubit[j] = qubits[j], a.stride[j] = s;
  }
  if (step < 0 || step > (int64_t)UINT32_MAX) return fail(TNCO_HIP_EINVAL, "'step' must be from 0 to 2^32 - 1.");
  CT_TRY(hipSetDevice(w->device));
  // (the run has synchronised the handle's stream: its outputs are there)
  const dim3 grid((unsigned)std::min<int64_t>((w->n_walkers + 255) / 256, 65536));
  const int64_t each = c->walk_sets == 1 ? 0 : n;  // elements between two walkers' amplitudes (one output for all: 0)
  if (int rc = with_plain_type(c, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(ct_walk_choose_joint_kernel<T>, grid, dim3(256), 0, w->stream, w->d_bits, w->d_dead, (const T*)c->d_sets_out,
                           each, w->n_walkers, w->seed, (uint32_t)step, (int)k, (int)natural, a);
        return (int)TNCO_HIP_OK;
      }))
    return rc;
  CT_TRY(hipGetLastError());
  CT_TRY(hipStreamSynchronize(w->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_walkers_permute(tnco_hip_walkers w, int64_t k, const int64_t* qubits, const uint8_t* table) {
  if (!w || !qubits || !table) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (k < 1 || k > WALK_MAX_PERMUTE) return fail(TNCO_HIP_EINVAL, "'k' must be from 1 to 8.");
  for (int64_t j = 0; j < k; ++j) {
    if (qubits[j] < 0 || qubits[j] >= w->n_qubits)
      return fail(TNCO_HIP_EINVAL, "a qubit is not a qubit of the walkers (0 to " + std::to_string(w->n_qubits - 1) + ").");
    if (std::count(qubits, qubits + j, qubits[j])) return fail(TNCO_HIP_EINVAL, "a qubit is named twice.");
  }
  const int64_t n = (int64_t)1 << k;
  std::vector<char> seen(n, 0);
  for (int64_t v = 0; v < n; ++v) {
    if (table[v] >= n || seen[table[v]]) return fail(TNCO_HIP_EINVAL, "'table' is not a permutation of 0 to 2^k - 1.");
    seen[table[v]] = 1;
  }
  int64_t image[WALK_MAX_PERMUTE + (1 << WALK_MAX_PERMUTE) / sizeof(int64_t)] = {};
  std::copy(qubits, qubits + k, image);
  std::memcpy(image + WALK_MAX_PERMUTE, table, (size_t)n);
  CT_TRY(hipSetDevice(w->device));
  CT_TRY(hipMemcpyAsync(w->d_perm, image, sizeof(image), hipMemcpyHostToDevice, w->stream));
  const dim3 grid((unsigned)std::min<int64_t>((w->n_walkers + 255) / 256, 65536));
  hipLaunchKernelGGL(ct_walk_permute_kernel, grid, dim3(256), 0, w->stream, w->d_bits, w->n_walkers, (int)k, (const int64_t*)w->d_perm);
  CT_TRY(hipGetLastError());
  CT_TRY(hipStreamSynchronize(w->stream));  // (the image lies on this call's stack)
  return TNCO_HIP_OK;
}

int tnco_hip_contract_stats(tnco_hip_contract c, int64_t* stats) {
  if (!c || !stats) return fail(TNCO_HIP_EINVAL, "null argument.");
  stats[0] = c->macs, stats[1] = c->launches, stats[2] = c->bytes + accumulate_bytes(c, c->accumulate), stats[3] = c->device_ns;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_kernel_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  std::copy(std::begin(c->by_kernel), std::end(c->by_kernel), counts);
  return TNCO_HIP_OK;
}

int tnco_hip_contract_row_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  std::copy(std::begin(c->by_row_kernel), std::end(c->by_row_kernel), counts);
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_exponents(tnco_hip_contract c, const int32_t* exps) {
  if (!c || (!exps && !c->leaf_numel.empty())) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (!c->scaling) return fail(TNCO_HIP_EINVAL, "the plan has no scaling.");
  c->leaf_exps.assign(exps, exps + c->leaf_numel.size());
  return TNCO_HIP_OK;
}

int tnco_hip_contract_exponents(tnco_hip_contract c, int32_t* exps) {
  if (!c || !exps) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (!c->scaling) return fail(TNCO_HIP_EINVAL, "the plan has no scaling.");
  CT_TRY(hipSetDevice(c->device));
  const size_t n = c->leaf_numel.size() + c->steps.size() / STEP_W;
  if (n) CT_TRY(hipMemcpyAsync(exps, c->d_exps + c->last_member * (int64_t)n, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  CT_TRY(hipStreamSynchronize(c->stream));
  return TNCO_HIP_OK;
}

int tnco_hip_contract_narrow_launches(tnco_hip_contract c, int64_t* count) {
  if (!c || !count) return fail(TNCO_HIP_EINVAL, "null argument.");
  *count = c->narrow_launches;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_slice_batch(tnco_hip_contract c, int64_t batch) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (batch < 1 || batch > MAX_SLICE_BATCH) return fail(TNCO_HIP_EINVAL, "'batch' must be from 1 to 64.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with a slice batch.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "a slice batch and a path kernel are exclusive.");
  if (c->sched.set == Schedule::REUSE) return fail(TNCO_HIP_EINVAL, "a slice batch is not supported with reuse periods.");
  const size_t n_steps = c->steps.size() / STEP_W, n_slots = c->leaf_numel.size() + n_steps;
  if (!n_steps) {  // a single leaf gathered into the output: runs as it does without a batch, nothing to reserve
    c->batch = batch;
    return TNCO_HIP_OK;
  }
  CT_TRY(hipSetDevice(c->device));
  CT_TRY(hipStreamSynchronize(c->stream));
  // B arenas, B blocks of the output's type, and with scaling the B-fold exponent slots and max words
  // (`bytes` counts arena_elems per member, as Plan.peak_device_bytes does; a plan whose steps need no arena keeps the
  // one element create allocated for it)
  const size_t arena = (size_t)c->arena_elems * c->elem, B = (size_t)batch;
  const size_t stage = B * (size_t)c->block_numel * c->out_elem;
  const size_t scale_b = c->scaling ? 4 * (n_slots + n_steps) : 0;
  const int64_t bytes = c->base_bytes + (int64_t)((B - 1) * (arena + scale_b) + stage);
  size_t free_b = 0, total_b = 0;
  CT_TRY(hipMemGetInfo(&free_b, &total_b));
  // what the batch adds to `bytes` must be free.  (The new buffers are allocated before the old ones are released, so
  // that a failure leaves the handle as it was: a device with the growth free but not the new buffers fails below.)
  const size_t need = (size_t)(bytes - c->bytes);
  if (bytes > c->bytes && need > free_b)
    return fail(TNCO_HIP_ERUNTIME, "the slice batch needs " + std::to_string(need) + " bytes of device memory, " +
                                       std::to_string(free_b) + " are free.");
  // the new buffers first: a handle that this call fails on stays as it was
  void *d_arena = nullptr, *d_stage = nullptr, *d_exps = nullptr;
  if (hipMalloc(&d_arena, std::max<size_t>(B * arena, c->elem)) != hipSuccess || hipMalloc(&d_stage, std::max<size_t>(stage, 4)) != hipSuccess ||
      (c->scaling && (hipMalloc(&d_exps, B * scale_b) != hipSuccess ||
                      hipMemsetAsync(d_exps, 0, B * scale_b, c->stream) != hipSuccess ||
                      hipStreamSynchronize(c->stream) != hipSuccess))) {
    for (void* p : {d_arena, d_stage, d_exps})
      if (p) (void)hipFree(p);
    return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  for (void* p : {c->d_arena, c->d_batch_out, c->scaling ? (void*)c->d_exps : nullptr})
    if (p) (void)hipFree(p);
  c->d_arena = d_arena, c->d_batch_out = d_stage;
  drop_accumulate_stage(c);
  if (c->scaling) c->d_exps = (int32_t*)d_exps, c->d_amax = (uint32_t*)(c->d_exps + B * n_slots);
  c->batch = batch, c->bytes = bytes;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_compute(tnco_hip_contract c, int32_t mode) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (mode != 0 && mode != 1) return fail(TNCO_HIP_EINVAL, "'mode' must be 0 (plain) or 1 (bf16x3).");
  if (c->dtype != 0 && c->dtype != 2) return fail(TNCO_HIP_EINVAL, "a compute mode needs a float32 or complex64 plan.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with a compute mode.");
  if (mode && c->path_group) return fail(TNCO_HIP_EINVAL, "a compute mode is not supported with a path kernel.");
  if (mode && c->matrix) return fail(TNCO_HIP_EINVAL, "a compute mode and matrix mode are exclusive.");
  if (mode && !c->ind_steps.empty()) return fail(TNCO_HIP_EINVAL, "a compute mode is not supported with indirect operands.");
  c->compute = mode;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_split_launches(tnco_hip_contract c, int64_t* count) {
  if (!c || !count) return fail(TNCO_HIP_EINVAL, "null argument.");
  *count = c->split_launches;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_matrix(tnco_hip_contract c, int32_t on) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (on != 0 && on != 1) return fail(TNCO_HIP_EINVAL, "'on' must be 0 or 1.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with matrix mode.");
  if (c->dtype > 3) return fail(TNCO_HIP_EINVAL, "matrix mode needs a plain dtype.");
  if (c->compute) return fail(TNCO_HIP_EINVAL, "a compute mode and matrix mode are exclusive.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "matrix mode is not supported with a path kernel.");
  if (!c->ind_steps.empty()) return fail(TNCO_HIP_EINVAL, "matrix mode is not supported with indirect operands.");
  c->matrix = on;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_matrix_launches(tnco_hip_contract c, int64_t* count) {
  if (!c || !count) return fail(TNCO_HIP_EINVAL, "null argument.");
  *count = c->matrix_launches;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_path_kernel(tnco_hip_contract c, int64_t group) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (group < 1 || group > MAX_PATH_GROUP) return fail(TNCO_HIP_EINVAL, "'group' must be from 1 to 1024.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with a path kernel.");
  if (c->dtype > 3) return fail(TNCO_HIP_EINVAL, "a path kernel needs a plain dtype.");
  if (c->batch) return fail(TNCO_HIP_EINVAL, "a slice batch and a path kernel are exclusive.");
  if (c->compute) return fail(TNCO_HIP_EINVAL, "a compute mode is not supported with a path kernel.");
  if (c->matrix) return fail(TNCO_HIP_EINVAL, "matrix mode is not supported with a path kernel.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "the path kernel is already set.");
  if (c->sched.set == Schedule::HOIST) return fail(TNCO_HIP_EINVAL, "hoisting is not supported with a path kernel.");
  if (c->sched.set == Schedule::REUSE) return fail(TNCO_HIP_EINVAL, "a path kernel is not supported with reuse periods.");
  if (!c->ind_steps.empty() || c->folded) return fail(TNCO_HIP_EINVAL, "a path kernel is not supported with indirect operands.");
  const int64_t S = (int64_t)c->steps.size() / STEP_W;
  for (int64_t k = 0; k < S; ++k) {
    const int64_t* st = &c->steps[k * STEP_W];
    int64_t macs = 1;  // H M N K, every factor checked before it enters the product
    bool over = false;
    for (int q = ST_H; q <= ST_K && !over; ++q) {
      over = st[q] > MAX_PATH_STEP_MACS / macs;
      macs *= over ? 1 : st[q];
    }
    if (over)
      return fail(TNCO_HIP_EINVAL, "step " + std::to_string(k) + " has more than 2^24 multiply-adds: too large for a path kernel.");
  }
  if (!S) {  // a single leaf gathered into the output: runs as it does without the call, nothing to reserve
    c->path_group = group;
    return TNCO_HIP_OK;
  }
  CT_TRY(hipSetDevice(c->device));
  CT_TRY(hipStreamSynchronize(c->stream));
  // the tables that are new on the device: the steps, the permute groups, and where every assignment of the run goes in
  // the output (the `visited` bookkeeping of the unfused loop, which does not depend on the data)
  std::vector<int64_t>& tab = c->path_image;
  tab.assign(c->steps.begin(), c->steps.end());
  for (int64_t g = 0; g <= S; ++g) tab.push_back(c->group_first[g]), tab.push_back(c->group_count[g]);
  std::vector<char> visited(c->n_blocks, 0);
  for (int64_t sid = c->start; sid < c->stop; ++sid) {
    int64_t blk = 0;
    for (int64_t b : c->block) blk = blk * c->slice_dims[b] + (sid / c->place[b]) % c->slice_dims[b];
    tab.push_back(blk * c->block_numel * 2 + visited[blk]);
    visited[blk] = 1;
  }
  // G arenas, G blocks of the output's type and the tables (`bytes` counts arena_elems per member, as
  // Plan.peak_device_bytes does)
  const size_t arena = (size_t)c->arena_elems * c->elem, G = (size_t)group;
  const size_t stage = G * (size_t)c->block_numel * c->out_elem, tables = tab.size() * sizeof(int64_t);
  const int64_t bytes = c->base_bytes + (int64_t)((G - 1) * arena + stage + tables);
  size_t free_b = 0, total_b = 0;
  CT_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t need = (size_t)(bytes - c->bytes);
  if (need > free_b) {
    tab.clear();
    return fail(TNCO_HIP_ERUNTIME, "the path kernel needs " + std::to_string(need) + " bytes of device memory, " +
                                       std::to_string(free_b) + " are free.");
  }
  // the new buffers first: a handle that this call fails on stays as it was
  void *d_arena = nullptr, *d_stage = nullptr, *d_tab = nullptr;
  if (hipMalloc(&d_arena, std::max<size_t>(G * arena, c->elem)) != hipSuccess || hipMalloc(&d_stage, std::max<size_t>(stage, 4)) != hipSuccess ||
      hipMalloc(&d_tab, tables) != hipSuccess ||
      hipMemcpyAsync(d_tab, tab.data(), tables, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    for (void* p : {d_arena, d_stage, d_tab})
      if (p) (void)hipFree(p);
    tab.clear();
    return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  if (c->d_arena) (void)hipFree(c->d_arena);
  c->d_arena = d_arena, c->d_path_stage = d_stage, c->d_path_tables = (int64_t*)d_tab;
  drop_accumulate_stage(c);
  c->path_group = c->path_cap = group, c->bytes = bytes;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_path_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  counts[0] = c->path_launches[0], counts[1] = c->path_launches[1];
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_hoist(tnco_hip_contract c, const int64_t* step_flags, const int64_t* perm_flags) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  const int64_t S = (int64_t)c->steps.size() / STEP_W, P = (int64_t)c->perms.size() / PERM_W;
  if ((S && !step_flags) || (P && !perm_flags)) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with hoisting.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "hoisting is not supported with a path kernel.");
  if (c->sched.set == Schedule::REUSE) return fail(TNCO_HIP_EINVAL, "hoisting is not supported with reuse periods: they include it.");
  // a flagged item: the period that is due at the first assignment of a run only (a single assignment: any above 1)
  const int64_t once = std::max<int64_t>(n_assignments(c), 2);
  std::vector<int64_t> step_period(S), perm_period(P);
  bool any = false;
  for (int64_t i = 0; i < S + P; ++i) {
    const int64_t f = i < S ? step_flags[i] : perm_flags[i - S];
    if (f != 0 && f != 1) return fail(TNCO_HIP_EINVAL, "a hoist flag must be 0 or 1.");
    (i < S ? step_period[i] : perm_period[i - S]) = f ? once : 1;
    any |= f == 1;
  }
  Schedule s;
  if (const char* e = make_schedule(c, step_period.data(), perm_period.data(), HOIST_RULES, &s)) return fail(TNCO_HIP_EINVAL, e);
  s.set = any ? Schedule::HOIST : Schedule::NEVER;  // (nothing to hoist: the handle runs as one on which this was never called)
  c->sched = std::move(s);
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_reuse(tnco_hip_contract c, const int64_t* step_period, const int64_t* perm_period) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  const int64_t S = (int64_t)c->steps.size() / STEP_W, P = (int64_t)c->perms.size() / PERM_W;
  if ((S && !step_period) || (P && !perm_period)) return fail(TNCO_HIP_EINVAL, "null argument.");
  // a period: the place of a sliced index, or the number of assignments (what no sliced index reaches)
  const int64_t n_slices = n_assignments(c);
  bool any = false;
  for (int64_t i = 0; i < S + P; ++i) {
    const int64_t v = i < S ? step_period[i] : perm_period[i - S];
    if (v != n_slices && std::find(c->place.begin(), c->place.end(), v) == c->place.end())
      return fail(TNCO_HIP_EINVAL, "a period must be the place of a sliced index or the number of assignments.");
    any |= v != 1;
  }
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with reuse periods.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "a path kernel is not supported with reuse periods.");
  if (c->batch) return fail(TNCO_HIP_EINVAL, "a slice batch is not supported with reuse periods.");
  if (c->sched.set == Schedule::HOIST) return fail(TNCO_HIP_EINVAL, "hoisting is not supported with reuse periods: they include it.");
  Schedule s;
  if (const char* e = make_schedule(c, step_period, perm_period, REUSE_RULES, &s)) return fail(TNCO_HIP_EINVAL, e);
  s.set = any ? Schedule::REUSE : Schedule::NEVER;  // (every period 1: the handle runs as one on which this was never called)
  c->sched = std::move(s);
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_indirect(tnco_hip_contract c, const int64_t* ind_steps, int64_t n_maps, const int64_t* maps) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  const int64_t S = (int64_t)c->steps.size() / STEP_W;
  if ((S && !ind_steps) || n_maps < 0 || (n_maps && !maps)) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with indirect operands.");
  if (c->dtype > 3) return fail(TNCO_HIP_EINVAL, "indirect operands need a plain dtype.");
  if (c->compute) return fail(TNCO_HIP_EINVAL, "a compute mode is not supported with indirect operands.");
  if (c->matrix) return fail(TNCO_HIP_EINVAL, "matrix mode is not supported with indirect operands.");
  if (c->path_group) return fail(TNCO_HIP_EINVAL, "a path kernel is not supported with indirect operands.");
  // Every table inside the pool, every entry >= 0, and the furthest element the three tables of an operand reach inside
  // the leaf (at the largest slice offset) or the arena: no table can send a lane outside its operand
  std::vector<char> fast(2 * S, 0);
  bool any = false;
  for (int64_t k = 0; k < S; ++k) {
    const int64_t* st = &c->steps[k * STEP_W];
    const auto [H, M, N, K] = step_shape(st);
    const std::string at = "step " + std::to_string(k) + ": ";
    for (int side = 0; side < 2; ++side) {
      const int64_t* o = ind_steps + k * IND_W + IX_SIDE * side;
      const int64_t ext[3] = {H, side ? K : M, side ? N : K};
      const int64_t s0 = st[ST_SIDE * side + ST_A_M], s1 = st[ST_SIDE * side + ST_A_K];
      if (o[0] == -1 && o[1] == -1 && o[2] == -1) {
        if (s0 == 0 && s1 == 0) return fail(TNCO_HIP_EINVAL, at + "an operand with both strides 0 needs its tables.");
        fast[2 * k + side] = s1 == 1;  // (direct: A contiguous along k, B along n, as the plain kernel stages them)
        continue;
      }
      if (s0 != 0 || s1 != 0) return fail(TNCO_HIP_EINVAL, at + "both stride columns of a folded operand must be 0.");
      const int64_t kind = st[ST_SIDE * side + ST_A_KIND], ref = st[ST_SIDE * side + ST_A_REF];
      const int64_t room = kind == K_LEAF ? c->leaf_numel[ref] - leaf_slice_reach(c, ref) : c->arena_elems - ref;
      int64_t reach = 0, step1[3];
      for (int q = 0; q < 3; ++q) {
        if (o[q] < 0 || o[q] > n_maps || ext[q] > n_maps - o[q]) return fail(TNCO_HIP_EINVAL, at + "an offset table lies outside the pool.");
        int64_t largest = 0;
        for (int64_t i = 0; i < ext[q]; ++i) {
          const int64_t v = maps[o[q] + i];
          if (v < 0) return fail(TNCO_HIP_EINVAL, at + "an offset table has a negative entry.");
          if (v >= room) return fail(TNCO_HIP_EINVAL, at + "an offset table reaches beyond its operand.");
          largest = std::max(largest, v);
        }
        reach += largest;
        step1[q] = ext[q] > 1 ? maps[o[q] + 1] - maps[o[q]] : INT64_MAX;
        if (step1[q] <= 0) step1[q] = INT64_MAX;
      }
      if (reach >= room) return fail(TNCO_HIP_EINVAL, at + "an offset table reaches beyond its operand.");
      // (the result of the step, in the arena, apart from everything a folded arena operand reaches)
      if (kind == K_ARENA && st[ST_C_KIND] == K_ARENA && st[ST_C_REF] <= ref + reach && ref < st[ST_C_REF] + H * M * N)
        return fail(TNCO_HIP_EINVAL, at + "step result overlaps a folded operand.");
      // tiled kernel: lanes along k of A (n of B) when that table has the smaller step, the source's innermost axis
      fast[2 * k + side] = step1[2] <= step1[1];  // (the tables of A: h, m, k; of B: h, k, n)
      any = true;
    }
  }
  if (!any) {  // nothing folded: the handle runs as one on which this was never called
    if (c->d_ind) (void)hipFree(c->d_ind);
    c->d_ind = nullptr, c->bytes -= c->ind_bytes, c->ind_bytes = 0;
    c->ind_steps.clear(), c->ind_fast.clear();
    return TNCO_HIP_OK;
  }
  CT_TRY(hipSetDevice(c->device));
  CT_TRY(hipStreamSynchronize(c->stream));
  std::vector<int64_t> image(ind_steps, ind_steps + S * IND_W);
  image.insert(image.end(), maps, maps + n_maps);
  const int64_t bytes = (int64_t)image.size() * 8;
  size_t free_b = 0, total_b = 0;
  CT_TRY(hipMemGetInfo(&free_b, &total_b));
  if ((size_t)bytes > free_b)
    return fail(TNCO_HIP_ERUNTIME, "the offset tables need " + std::to_string(bytes) + " bytes of device memory, " +
                                       std::to_string(free_b) + " are free.");
  // the new buffer first: a handle that this call fails on stays as it was
  int64_t* d_new = nullptr;
  if (hipMalloc((void**)&d_new, (size_t)bytes) != hipSuccess ||
      hipMemcpyAsync(d_new, image.data(), (size_t)bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    if (d_new) (void)hipFree(d_new);
    return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
  }
  if (c->d_ind) (void)hipFree(c->d_ind);
  c->d_ind = d_new, c->bytes += bytes - c->ind_bytes, c->ind_bytes = bytes;
  c->ind_steps.assign(ind_steps, ind_steps + S * IND_W), c->ind_fast = fast;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_indirect_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  std::copy(std::begin(c->by_ix), std::end(c->by_ix), counts);
  return TNCO_HIP_OK;
}

int tnco_hip_contract_set_accumulate(tnco_hip_contract c, int32_t mode) {
  if (!c) return fail(TNCO_HIP_EINVAL, "null argument.");
  if (mode != 0 && mode != 1) return fail(TNCO_HIP_EINVAL, "'mode' must be 0 (off) or 1 (float64).");
  if (c->dtype == 1 || c->dtype == 3) return fail(TNCO_HIP_EINVAL, "wide accumulation needs a float32 or complex64 output.");
  if (!c->row_steps.empty() || !c->row_maps.empty()) return fail(TNCO_HIP_EINVAL, "row axes are not supported with wide accumulation.");
  CT_TRY(hipSetDevice(c->device));
  CT_TRY(hipStreamSynchronize(c->stream));
  // the new buffers first: a handle that this call fails on stays as it was
  void *d_acc = nullptr, *d_stage = nullptr;
  if (const int64_t bytes = accumulate_bytes(c, mode)) {
    size_t free_b = 0, total_b = 0;
    CT_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t had = accumulate_bytes(c, c->accumulate);
    if (bytes > had && (size_t)(bytes - had) > free_b)
      return fail(TNCO_HIP_ERUNTIME, "the accumulator needs " + std::to_string(bytes - had) + " bytes of device memory, " +
                                         std::to_string(free_b) + " are free.");
    const size_t acc = (size_t)c->out_numel * 2 * c->out_elem, stage = (size_t)(bytes - (int64_t)acc);
    if (hipMalloc(&d_acc, acc) != hipSuccess || (stage && hipMalloc(&d_stage, stage) != hipSuccess)) {
      if (d_acc) (void)hipFree(d_acc);
      return fail(TNCO_HIP_ERUNTIME, "device allocation failed.");
    }
  }
  if (c->d_acc) (void)hipFree(c->d_acc);
  drop_accumulate_stage(c);
  c->d_acc = d_acc, c->d_acc_stage = d_stage, c->accumulate = mode;
  return TNCO_HIP_OK;
}

int tnco_hip_contract_accumulate_launches(tnco_hip_contract c, int64_t* counts) {
  if (!c || !counts) return fail(TNCO_HIP_EINVAL, "null argument.");
  counts[0] = c->acc_launches[0], counts[1] = c->acc_launches[1];
  return TNCO_HIP_OK;
}

int tnco_hip_contract_batch_launches(tnco_hip_contract c, int64_t* count) {
  if (!c || !count) return fail(TNCO_HIP_EINVAL, "null argument.");
  *count = c->batch_launches;
  return TNCO_HIP_OK;
}

void tnco_hip_contract_destroy(tnco_hip_contract c) {
  if (!c) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (void* p : {(void*)c->d_leaves, c->d_arena, c->d_out, (void*)c->d_tables, (void*)c->d_leaf_ptrs, (void*)c->d_row_maps,
                  (void*)c->d_exps, c->d_batch_out, c->d_path_stage, (void*)c->d_path_tables, (void*)c->d_ind, c->d_acc,
                  c->d_acc_stage, c->d_sets_out, (void*)c->d_sets_tables, (void*)c->d_walk_tables})
    if (p) (void)hipFree(p);
  for (const auto* bufs : {&c->d_stack, &c->d_versions})
    for (void* p : *bufs)
      if (p) (void)hipFree(p);
  for (hipEvent_t e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

}  // extern "C"
