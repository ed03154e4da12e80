// contract_io.h -- leaves and results that live in a caller's device memory (included by contract.hip, inside its
// anonymous namespace; tnco_hip_contract_load_leaf, tnco_hip_contract_run_loaded).
//   ct_ingest_kernel<D, S>  a caller's leaf, any strides, into the handle's leaf buffer (C-contiguous), widened exactly;
//   ct_emit_kernel<T>       the handle's output buffer, [block axes][the other axes], into a caller's C-contiguous buffer in
//                           the result's own axis order.
// A caller's pointer may belong to another HIP runtime in the same process (PyTorch bundles its own): this library's
// runtime does not know such memory, so no API call of it ever gets the pointer -- no copy, no memset, no attribute query.
// The pointer is a kernel argument and nothing else; what it can reach is the caller's to check.
// Both kernels: a grid-stride loop, at most IO_MAX_BLOCKS blocks of 256, no LDS, the axis table a kernel argument (nothing
// is allocated for a launch).  An element's offset on the strided side is the sum of digit x stride over the axes, the
// digits taken from the linear index of the contiguous side, last axis fastest; int64 throughout (32-bit divisions where
// the element count allows).  Where both sides are C-contiguous in one order and of one type (IoAxes::nd < 0) the copy
// is io_copy: 16-byte loads and stores over the stretch where both addresses are 16-byte aligned, element by element
// before and after it, and element by element throughout when the two addresses are not congruent modulo 16.

constexpr int64_t IO_MAX_BLOCKS = 2048;

struct IoAxes {
  int nd;                          // axes; -1: the vector path
  int64_t dim[CT_MAX_AXES];
  int64_t stride[CT_MAX_AXES];     // in elements, of the strided side; >= 0
};

template <class T>
struct io_parts {
  using real = T;
  static constexpr bool complex = false;
};
template <class R>
struct io_parts<cplx<R>> {
  using real = R;
  static constexpr bool complex = true;
};

// the exact widenings: real to a wider real, real to complex (imaginary part +0), complex to a wider complex
template <class D, class S>
__device__ inline D io_widen(const S& s) {
  using R = typename io_parts<D>::real;
  if constexpr (std::is_same<D, S>::value) return s;
  else if constexpr (io_parts<S>::complex) return D{(R)s.re, (R)s.im};
  else if constexpr (io_parts<D>::complex) return D{(R)s, (R)0};
  else return (D)s;
}

template <class I>
__device__ inline int64_t io_digits(const IoAxes& ax, I rem) {
  int64_t off = 0;
  for (int k = ax.nd - 1; k > 0; --k) {
    const I d = (I)ax.dim[k], q = rem / d;
    off += (int64_t)(rem - q * d) * ax.stride[k];
    rem = q;
  }
  return off + (int64_t)rem * ax.stride[0];
}

// the offset of element e (linear on the contiguous side) on the strided side; small: the element count fits 32 bits
__device__ inline int64_t io_offset(const IoAxes& ax, int64_t e, bool small) {
  if (ax.nd <= 1) return ax.nd == 1 ? e * ax.stride[0] : 0;
  return small ? io_digits<uint32_t>(ax, (uint32_t)e) : io_digits<int64_t>(ax, e);
}

// n elements, both sides C-contiguous
template <class T>
__device__ inline void io_copy(T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  static_assert(16 % sizeof(T) == 0, "an element divides 16 bytes");
  constexpr int64_t PER = 16 / sizeof(T);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)gridDim.x * blockDim.x;
  const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
  int64_t head = n, body = 0;  // elements before the aligned stretch, 16-byte pieces of it
  if (((sa ^ da) & 15) == 0 && (sa & 15) % sizeof(T) == 0) {
    head = (int64_t)((16 - (sa & 15)) & 15) / (int64_t)sizeof(T);
    if (head > n) head = n;
    body = (n - head) / PER;
  }
  for (int64_t e = tid; e < head; e += lanes) dst[e] = src[e];
  const uint4* __restrict__ s4 = (const uint4*)(src + head);
  uint4* __restrict__ d4 = (uint4*)(dst + head);
#pragma unroll 4
  for (int64_t v = tid; v < body; v += lanes) d4[v] = s4[v];
  for (int64_t e = head + body * PER + tid; e < n; e += lanes) dst[e] = src[e];
}

template <class D, class S>
__global__ __launch_bounds__(256) void ct_ingest_kernel(D* __restrict__ dst, const S* __restrict__ src, int64_t numel, IoAxes ax) {
  if constexpr (std::is_same<D, S>::value) {
    if (ax.nd < 0) {
      io_copy(dst, src, numel);
      return;
    }
  }
  const bool small = numel <= (int64_t)UINT32_MAX;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    dst[e] = io_widen<D, S>(src[io_offset(ax, e, small)]);
}

template <class T>
__global__ __launch_bounds__(256) void ct_emit_kernel(T* __restrict__ dst, const T* __restrict__ src, int64_t numel, IoAxes ax) {
  if (ax.nd < 0) {
    io_copy(dst, src, numel);
    return;
  }
  const bool small = numel <= (int64_t)UINT32_MAX;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x)
    dst[io_offset(ax, e, small)] = src[e];
}

// blocks of 256 for `numel` elements of `elem` bytes: a lane per element, on the vector path a lane per 16 bytes
inline unsigned io_blocks(int64_t numel, size_t elem, bool vector) {
  const int64_t work = vector ? (numel * (int64_t)elem + 15) / 16 + 1 : numel;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, IO_MAX_BLOCKS));
}

// dims / strides as the entry points take them into an IoAxes.  The text of what is wrong, or nullptr.  `contiguous`: the
// strides are those of a C-contiguous array of these dims (strides == nullptr says so)
inline const char* io_axes(int64_t ndim, const int64_t* dims, const int64_t* strides, int64_t want, const char* what_numel,
                           IoAxes* ax, bool* contiguous) {
  if (ndim < 0 || ndim > CT_MAX_AXES) return "'ndim' must be from 0 to 32.";
  if (ndim && !dims) return "null argument.";
  int64_t prod = 1;
  for (int64_t k = 0; k < ndim; ++k) {
    if (dims[k] < 1) return "dims must be positive.";
    if (prod > want / dims[k]) return what_numel;  // (beyond the count already: no overflow)
    prod *= dims[k];
    if (strides && strides[k] < 0) return "a stride is negative.";
  }
  if (prod != want) return what_numel;
  *contiguous = true;
  int64_t dense = 1;
  for (int64_t k = ndim - 1; k >= 0; --k) {
    ax->dim[k] = dims[k];
    ax->stride[k] = strides ? strides[k] : dense;
    if (dims[k] > 1 && ax->stride[k] != dense) *contiguous = false;
    dense *= dims[k];
  }
  ax->nd = (int)ndim;
  return nullptr;
}
