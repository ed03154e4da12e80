// accept_probe.hip -- a TEST-ONLY device probe around the arithmetic shortcuts of the annealing kernels, compiled from
// the product headers with the product's flags (tests/test_gpu_accept.py; no part of libtnco_hip.so or its ABI):
//   * the Metropolis accept filter: tnco::accept_move (sa_sweep.h) and tnco::small_accept (sa_small.h) per element, with
//     the path each decision took (TNCO_ACCEPT_PATH), the device pow that tnco::accept_exact calls, and the error of the
//     bare v_log_f32 (__log2f) the filter's margin is derived from, over whole ranges of float bit patterns;
//   * tnco::small_mod (x % n through a double reciprocal) and fws_divmod (the parallel shuffle's float-reciprocal
//     quotient, fw_wave.h) against integer division, mismatches counted on the device.
// Every entry point allocates, launches and copies back itself and returns 0 or a hipError_t.
//
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -shared -fPIC -I tnco_amd/csrc
//         -o tests/csrc/libaccept_probe.so tests/csrc/accept_probe.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace accept_probe {
constexpr int PATH_BLOCKS = 1024, PATH_TPB = 256;
__device__ int g_path[PATH_BLOCKS * PATH_TPB];  // one slot per thread of probe_accept's launch
}  // namespace accept_probe
#define TNCO_ACCEPT_PATH(p) (accept_probe::g_path[blockIdx.x * blockDim.x + threadIdx.x] = (p))

#include "sa_small.h"
#include "fw_kernels.h"

namespace accept_probe {

// ---- v_log_f32 ----------------------------------------------------------------------------------------------------
constexpr int LOG_CHUNK_BITS = 16, LOG_TPB = 256;  // a block scans 2^16 consecutive bit patterns: one binade (2^23) holds whole chunks
struct LogChunk {
  double err, exc;      // max |v_log_f32(t) - log2 t|, max of |err| - 1.2e-7 |log2 t| (-1: the chunk holds nothing of the range)
  uint32_t err_at, exc_at;
};

__global__ __launch_bounds__(LOG_TPB) void log2_scan_kernel(uint32_t lo, uint32_t hi, uint32_t chunk0, LogChunk* out) {
  const uint32_t chunk = chunk0 + blockIdx.x;
  double e = -1.0, x = -1e300;
  uint32_t ea = 0, xa = 0;
  for (uint32_t k = threadIdx.x; k < (1u << LOG_CHUNK_BITS); k += LOG_TPB) {
    const uint32_t bits = (chunk << LOG_CHUNK_BITS) | k;
    if (bits < lo || bits > hi) continue;
    const float t = __uint_as_float(bits);
    const double ref = log2((double)t);
    const double err = fabs((double)__log2f(t) - ref);
    const double exc = err - 1.2e-7 * fabs(ref);
    if (!(err <= e)) { e = err; ea = bits; }  // (a NaN error wins: it must not pass)
    if (!(exc <= x)) { x = exc; xa = bits; }
  }
  __shared__ double se[LOG_TPB], sx[LOG_TPB];
  __shared__ uint32_t sea[LOG_TPB], sxa[LOG_TPB];
  se[threadIdx.x] = e; sx[threadIdx.x] = x; sea[threadIdx.x] = ea; sxa[threadIdx.x] = xa;
  __syncthreads();
  for (int s = LOG_TPB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      if (!(se[threadIdx.x + s] <= se[threadIdx.x])) { se[threadIdx.x] = se[threadIdx.x + s]; sea[threadIdx.x] = sea[threadIdx.x + s]; }
      if (!(sx[threadIdx.x + s] <= sx[threadIdx.x])) { sx[threadIdx.x] = sx[threadIdx.x + s]; sxa[threadIdx.x] = sxa[threadIdx.x + s]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[blockIdx.x].err = se[0]; out[blockIdx.x].exc = sx[0];
    out[blockIdx.x].err_at = sea[0]; out[blockIdx.x].exc_at = sxa[0];
  }
}

__global__ void log2_at_kernel(int64_t n, const uint32_t* bits, float* dev, double* ref) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float t = __uint_as_float(bits[i]);
    dev[i] = __log2f(t);
    ref[i] = log2((double)t);
  }
}

// ---- the accept rule ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PATH_TPB) void accept_kernel(int64_t n, const int* kind, const int* f32, const double* beta,
                                                          const double* delta, const double* total, const double* u,
                                                          uint8_t* out_move, uint8_t* out_small, uint8_t* path_move,
                                                          uint8_t* path_small) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = slot; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    g_path[slot] = 255;
    const bool a = tnco::accept_move(kind[i], beta[i], delta[i], total[i], u[i], f32[i]);
    const int pa = g_path[slot];
    g_path[slot] = 255;
    const bool b = tnco::small_accept(kind[i], beta[i], delta[i], total[i], u[i]);
    const int pb = g_path[slot];
    out_move[i] = a ? 1 : 0;
    out_small[i] = b ? 1 : 0;
    path_move[i] = (uint8_t)pa;
    path_small[i] = (uint8_t)pb;
  }
}

__global__ void pow_kernel(int64_t n, const double* x, const double* beta, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = pow(x[i], -beta[i]);
}

// ---- small_mod --------------------------------------------------------------------------------------------------------
constexpr int MOD_TPB = 256, MOD_PER_THREAD = 32, MOD_CHUNK = MOD_TPB * MOD_PER_THREAD;  // quotients per block

__device__ __forceinline__ void mod_check(uint32_t x, uint32_t n, double inv_n, unsigned long long& bad, uint32_t& bad_x) {
  if (tnco::small_mod(x, n, inv_n) != x % n) { ++bad; bad_x = x; }
}

// Block b of the launch serves chunk (first + b); prefix[j] = chunks of all n < n0 + j, so the block's n is found by bisection.
__global__ __launch_bounds__(MOD_TPB) void small_mod_kernel(uint32_t n0, uint32_t count, const unsigned long long* prefix,
                                                            unsigned long long first, unsigned long long* out) {
  const unsigned long long c = first + blockIdx.x;
  uint32_t lo = 0, hi = count;  // prefix[lo] <= c < prefix[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (prefix[mid] <= c) lo = mid; else hi = mid;
  }
  const uint32_t n = n0 + lo;
  const double inv_n = 1.0 / (double)n;  // (as small_sweeps computes it)
  const uint64_t qmax = 0xFFFFFFFFull / n;
  const uint64_t q0 = (c - prefix[lo]) * (uint64_t)MOD_CHUNK;
  unsigned long long bad = 0;
  uint32_t bad_x = 0;
  for (int k = 0; k < MOD_PER_THREAD; ++k) {
    const uint64_t q = q0 + (uint64_t)k * MOD_TPB + threadIdx.x;
    if (q > qmax) break;
    const uint64_t x = q * n;  // <= 2^32 - 1
    mod_check((uint32_t)x, n, inv_n, bad, bad_x);
    if (x >= 1) mod_check((uint32_t)(x - 1), n, inv_n, bad, bad_x);
    if (x + 1 <= 0xFFFFFFFFull) mod_check((uint32_t)(x + 1), n, inv_n, bad, bad_x);
  }
  if (q0 == 0 && threadIdx.x == 0) {
    mod_check(0x7FFFFFFFu, n, inv_n, bad, bad_x);
    mod_check(0x80000000u, n, inv_n, bad, bad_x);
    mod_check(0x80000001u, n, inv_n, bad, bad_x);
    mod_check(0xFFFFFFFFu, n, inv_n, bad, bad_x);
  }
  if (bad) {
    atomicAdd(&out[0], bad);
    out[1] = bad_x;
    out[2] = n;
  }
}

__global__ void fws_divmod_kernel(unsigned long long* out) {
  const uint32_t dv = 2u + blockIdx.x;  // 2 ... 129
  const uint32_t range = dv * (dv - 1u);
  unsigned long long bad = 0;
  uint32_t bad_x = 0;
  for (uint32_t x = threadIdx.x; x < range; x += blockDim.x) {
    uint32_t q, rem;
    tnco::fws_divmod(x, dv, q, rem);
    if (q != x / dv || rem != x % dv) { ++bad; bad_x = x; }
  }
  if (bad) {
    atomicAdd(&out[0], bad);
    out[1] = bad_x;
    out[2] = dv;
  }
}

struct DevBufs {  // every device allocation of a call, freed when the call returns
  std::vector<void*> p;
  ~DevBufs() { for (void* q : p) (void)hipFree(q); }
  template <class T> hipError_t get(T** out, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, count ? count * sizeof(T) : sizeof(T));
    if (e == hipSuccess) p.push_back(q);
    *out = static_cast<T*>(q);
    return e;
  }
};

}  // namespace accept_probe

using namespace accept_probe;
#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// Every float bit pattern in [lo_bits, hi_bits] (positive floats: hi_bits < 0x7F800000).  out[binade * 8 + ...], binade = the
// exponent field 0 ... 254: [0] max |v_log_f32(t) - log2 t| (-1: nothing of the binade in range), [1] the bits of the t that
// attains it, [2] v_log_f32 there, [3] the device's float64 log2 there, [4] max of |err| - 1.2e-7 |log2 t|, [5] [6] [7] the same
// three for it.  Per 2^16-pattern chunk on the device, the chunks of a binade folded here.
extern "C" int probe_log2_scan(int device, uint32_t lo_bits, uint32_t hi_bits, double* out) {
  for (int i = 0; i < 255 * 8; ++i) out[i] = (i & 3) == 0 ? -1.0 : 0.0;
  for (int b = 0; b < 255; ++b) out[b * 8 + 4] = -1e300;
  if (hi_bits >= 0x7F800000u || lo_bits > hi_bits) return (int)hipErrorInvalidValue;
  TRY(hipSetDevice(device));
  DevBufs bufs;
  const uint32_t c0 = lo_bits >> LOG_CHUNK_BITS, c1 = hi_bits >> LOG_CHUNK_BITS, nch = c1 - c0 + 1;
  LogChunk* d = nullptr;
  TRY(bufs.get(&d, nch));
  log2_scan_kernel<<<nch, LOG_TPB>>>(lo_bits, hi_bits, c0, d);
  TRY(hipGetLastError());
  std::vector<LogChunk> h(nch);
  TRY(hipMemcpy(h.data(), d, nch * sizeof(LogChunk), hipMemcpyDeviceToHost));
  std::vector<uint32_t> at(255 * 2, 0u);
  for (uint32_t c = 0; c < nch; ++c) {
    const int b = (int)(((c0 + c) << LOG_CHUNK_BITS) >> 23);
    if (h[c].err < 0 && h[c].err == h[c].err) continue;
    if (!(h[c].err <= out[b * 8 + 0])) { out[b * 8 + 0] = h[c].err; at[b * 2] = h[c].err_at; }
    if (!(h[c].exc <= out[b * 8 + 4])) { out[b * 8 + 4] = h[c].exc; at[b * 2 + 1] = h[c].exc_at; }
  }
  uint32_t* dbits = nullptr;
  float* ddev = nullptr;
  double* dref = nullptr;
  TRY(bufs.get(&dbits, 510));
  TRY(bufs.get(&ddev, 510));
  TRY(bufs.get(&dref, 510));
  TRY(hipMemcpy(dbits, at.data(), 510 * sizeof(uint32_t), hipMemcpyHostToDevice));
  log2_at_kernel<<<2, 256>>>(510, dbits, ddev, dref);
  TRY(hipGetLastError());
  std::vector<float> hdev(510);
  std::vector<double> href(510);
  TRY(hipMemcpy(hdev.data(), ddev, 510 * sizeof(float), hipMemcpyDeviceToHost));
  TRY(hipMemcpy(href.data(), dref, 510 * sizeof(double), hipMemcpyDeviceToHost));
  for (int b = 0; b < 255; ++b) {
    if (out[b * 8] < 0 && out[b * 8] == out[b * 8]) continue;
    for (int j = 0; j < 2; ++j) {
      out[b * 8 + 4 * j + 1] = (double)at[b * 2 + j];
      out[b * 8 + 4 * j + 2] = (double)hdev[b * 2 + j];
      out[b * 8 + 4 * j + 3] = href[b * 2 + j];
    }
  }
  return 0;
}

// v_log_f32 and the device's float64 log2 at n given float bit patterns (the host checks the latter against mpmath).
extern "C" int probe_log2_at(int device, int64_t n, const uint32_t* bits, float* out_dev, double* out_ref) {
  if (n <= 0) return 0;
  TRY(hipSetDevice(device));
  DevBufs bufs;
  uint32_t* dbits = nullptr;
  float* ddev = nullptr;
  double* dref = nullptr;
  TRY(bufs.get(&dbits, (size_t)n));
  TRY(bufs.get(&ddev, (size_t)n));
  TRY(bufs.get(&dref, (size_t)n));
  TRY(hipMemcpy(dbits, bits, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  log2_at_kernel<<<(unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096), 256>>>(n, dbits, ddev, dref);
  TRY(hipGetLastError());
  TRY(hipMemcpy(out_dev, ddev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  TRY(hipMemcpy(out_ref, dref, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// Both functions' decisions (0 / 1) and paths (0 early yes, 1 early zero, 2 filter yes, 3 filter no, 4 exact) per element.
// small_accept has no float32 mode: it is called with the same operands whatever f32[i] says.
extern "C" int probe_accept(int device, int64_t n, const int* kind, const int* f32, const double* beta, const double* delta,
                            const double* total, const double* u, uint8_t* out_move, uint8_t* out_small, uint8_t* path_move,
                            uint8_t* path_small) {
  if (n <= 0) return 0;
  TRY(hipSetDevice(device));
  DevBufs bufs;
  int *dk = nullptr, *df = nullptr;
  double* dd[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* dres[4] = {nullptr, nullptr, nullptr, nullptr};
  const double* hd[4] = {beta, delta, total, u};
  uint8_t* ho[4] = {out_move, out_small, path_move, path_small};
  const size_t N = (size_t)n;
  TRY(bufs.get(&dk, N));
  TRY(bufs.get(&df, N));
  TRY(hipMemcpy(dk, kind, N * sizeof(int), hipMemcpyHostToDevice));
  TRY(hipMemcpy(df, f32, N * sizeof(int), hipMemcpyHostToDevice));
  for (int j = 0; j < 4; ++j) {
    TRY(bufs.get(&dd[j], N));
    TRY(hipMemcpy(dd[j], hd[j], N * sizeof(double), hipMemcpyHostToDevice));
    TRY(bufs.get(&dres[j], N));
  }
  const int64_t want = (n + PATH_TPB - 1) / PATH_TPB;
  accept_kernel<<<(unsigned)(want < PATH_BLOCKS ? want : PATH_BLOCKS), PATH_TPB>>>(n, dk, df, dd[0], dd[1], dd[2], dd[3], dres[0], dres[1],
                                                                                  dres[2], dres[3]);
  TRY(hipGetLastError());
  for (int j = 0; j < 4; ++j) TRY(hipMemcpy(ho[j], dres[j], N, hipMemcpyDeviceToHost));
  return 0;
}

// The device's pow(x, -beta): the OCML pow that tnco::accept_exact calls, under the same compiler flags.
extern "C" int probe_pow(int device, int64_t n, const double* x, const double* beta, double* out) {
  if (n <= 0) return 0;
  TRY(hipSetDevice(device));
  DevBufs bufs;
  double *dx = nullptr, *db = nullptr, *dout = nullptr;
  const size_t N = (size_t)n;
  TRY(bufs.get(&dx, N));
  TRY(bufs.get(&db, N));
  TRY(bufs.get(&dout, N));
  TRY(hipMemcpy(dx, x, N * 8, hipMemcpyHostToDevice));
  TRY(hipMemcpy(db, beta, N * 8, hipMemcpyHostToDevice));
  pow_kernel<<<(unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096), 256>>>(n, dx, db, dout);
  TRY(hipGetLastError());
  TRY(hipMemcpy(out, dout, N * 8, hipMemcpyDeviceToHost));
  return 0;
}

// small_mod(x, n, 1.0 / n) against x % n for every n in [n_lo, n_hi] (2 <= n_lo <= n_hi < 2^16) and every x in
// {q n - 1, q n, q n + 1} of every quotient q with q n < 2^32, plus 0, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 1.
// mismatches_out[0] their number, [1] [2] the x and n of one of them.
extern "C" int probe_small_mod(int device, uint32_t n_lo, uint32_t n_hi, unsigned long long* mismatches_out) {
  mismatches_out[0] = mismatches_out[1] = mismatches_out[2] = 0;
  if (n_lo < 2 || n_hi < n_lo || n_hi > 0xFFFFu) return (int)hipErrorInvalidValue;
  TRY(hipSetDevice(device));
  const uint32_t count = n_hi - n_lo + 1;
  std::vector<unsigned long long> prefix(count + 1, 0ull);
  for (uint32_t j = 0; j < count; ++j) {
    const unsigned long long quotients = 0xFFFFFFFFull / (n_lo + j) + 1ull;
    prefix[j + 1] = prefix[j] + (quotients + MOD_CHUNK - 1) / MOD_CHUNK;
  }
  DevBufs bufs;
  unsigned long long *dprefix = nullptr, *dout = nullptr;
  TRY(bufs.get(&dprefix, count + 1));
  TRY(bufs.get(&dout, 3));
  TRY(hipMemcpy(dprefix, prefix.data(), (count + 1) * 8, hipMemcpyHostToDevice));
  TRY(hipMemset(dout, 0, 24));
  const unsigned long long per_launch = 1ull << 19;  // blocks: a launch stays well below a second
  for (unsigned long long first = 0; first < prefix[count]; first += per_launch) {
    const unsigned long long left = prefix[count] - first;
    small_mod_kernel<<<(unsigned)(left < per_launch ? left : per_launch), MOD_TPB>>>(n_lo, count, dprefix, first, dout);
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
  }
  TRY(hipMemcpy(mismatches_out, dout, 24, hipMemcpyDeviceToHost));
  return 0;
}

// fws_divmod(x, dv) against x / dv and x % dv over its whole domain: dv = 2 ... 129, every x < dv (dv - 1).
extern "C" int probe_fws_divmod(int device, unsigned long long* mismatches_out) {
  mismatches_out[0] = mismatches_out[1] = mismatches_out[2] = 0;
  TRY(hipSetDevice(device));
  DevBufs bufs;
  unsigned long long* dout = nullptr;
  TRY(bufs.get(&dout, 3));
  TRY(hipMemset(dout, 0, 24));
  fws_divmod_kernel<<<128, 256>>>(dout);
  TRY(hipGetLastError());
  TRY(hipMemcpy(mismatches_out, dout, 24, hipMemcpyDeviceToHost));
  return 0;
}
