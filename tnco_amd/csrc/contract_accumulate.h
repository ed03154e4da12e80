// contract_accumulate.h -- the sum over slice assignments in float64 (tnco_hip_contract_set_accumulate); included by
// contract.hip inside its anonymous namespace, after BatchPlace and contract_path.h.
// Every assignment computes its float32 / complex64 block of the output as the run without the call does, always with
// beta 0 and into a staging block: the batch staging buffer, the path kernel's, or unbatched a block of its own.  The fold
// then goes into an accumulator of float64 / complex128, one element per output element, instead of into the output:
//   ct_acc_reduce_kernel       the twin of ct_batch_reduce_kernel: stage [n][block] -> the accumulator, one lane per element
//                              of a block, the members in assignment order; the first block that reaches an output block is
//                              placed, widened exactly, every later one is added with one float64 addition per part
//                              (an unbatched assignment is a group of one);
//   ct_acc_path_reduce_kernel  the twin of ct_path_reduce_kernel, the placement from the path kernel's device table;
//   ct_acc_narrow_kernel       once per run, after the last assignment: the accumulator rounded to float32 / complex64, to
//                              nearest even, into the output.
// The accumulator is cleared at the start of a run, so a block that slice_range does not reach narrows to zero.  Pure
// streaming kernels: per lane and element one 4 / 8-byte read and one 8 / 16-byte read-modify-write, no LDS, no atomics,
// the order fixed.  float / cplx<float> only.
#pragma once

template <class T>
struct ct_wide;
template <>
struct ct_wide<float> {
  using type = double;
};
template <>
struct ct_wide<cplx<float>> {
  using type = cplx<double>;
};
template <class T>
using ct_wide_t = typename ct_wide<T>::type;

// exact: every float32 is a float64
__device__ inline double ct_widen64(float v) { return (double)v; }
__device__ inline cplx<double> ct_widen64(cplx<float> v) { return cplx<double>{(double)v.re, (double)v.im}; }
// one rounding to nearest even per part; beyond float32's range inf, below it a subnormal or zero
__device__ inline float ct_narrow32(double v) { return (float)v; }
__device__ inline cplx<float> ct_narrow32(cplx<double> v) { return cplx<float>{(float)v.re, (float)v.im}; }

template <class T>
__global__ __launch_bounds__(256) void ct_acc_reduce_kernel(ct_wide_t<T>* acc, const T* stage, int64_t numel, int n, BatchPlace pl) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    for (int b = 0; b < n; ++b) {
      ct_wide_t<T>* o = acc + pl.off[b] + e;
      const ct_wide_t<T> v = ct_widen64(stage[b * numel + e]);
      *o = (pl.beta >> b) & 1 ? ct_add(*o, v) : v;
    }
}

template <class T>
__global__ __launch_bounds__(256) void ct_acc_path_reduce_kernel(ct_wide_t<T>* acc, const T* stage, int64_t numel, int n,
                                                                 const int64_t* place) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    for (int b = 0; b < n; ++b) {
      const int64_t pl = place[b];
      ct_wide_t<T>* o = acc + (pl >> 1) + e;
      const ct_wide_t<T> v = ct_widen64(stage[b * numel + e]);
      *o = pl & 1 ? ct_add(*o, v) : v;
    }
}

template <class T>
__global__ __launch_bounds__(256) void ct_acc_narrow_kernel(T* out, const ct_wide_t<T>* acc, int64_t numel) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    out[e] = ct_narrow32(acc[e]);
}
