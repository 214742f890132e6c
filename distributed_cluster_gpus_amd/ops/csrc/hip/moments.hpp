// Shared ensemble reduction: {n, mean, M2, min, max} of one row of
// per-replica figures over the replicas that contribute (gfx950).
//
// One workgroup of MOM_THREADS reduces one row, threads striding over the
// coalesced replica axis, in three passes in f64:
//   0. count the contributing replicas and find the first one; its value x0
//      is the shift of pass 1;
//   1. shifted sum -> mean = x0 + sum(x - x0) / n, so the sum runs over the
//      spread, not the magnitude, and a row whose values are all equal gets
//      exactly that value and M2 == 0;
//   2. sum (x - mean)^2 with min and max (the 32 KB row of a 4096-replica run
//      is re-read from cache) — a one-pass sum-of-squares loses everything
//      for energies ~1e9 with unit spread.
// Partials are combined in a fixed order (per-thread strided partial, shuffle
// tree inside the wave, waves 0..3 through LDS), so the result is bitwise
// reproducible for a given replica count.  reduce_series_kernel
// (pop_series.hpp) and lat_stats_kernel (lat_hist.hpp) are this function with
// their own "replica r contributes" predicate.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace dcg {

constexpr int MOM_STATS = 5;  // n, mean, M2, min, max
constexpr int MOM_THREADS = 256;
constexpr int MOM_WAVES = MOM_THREADS / 64;

// throw if the kernel launch just issued failed
inline void check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// fixed-order block reductions: shuffle tree in each wave, then every thread
// folds the wave results in wave order
__device__ __forceinline__ double block_sum(double v, double* l_buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // l_buf may still be read from the previous reduction
  if (lane == 0) l_buf[wave] = v;
  __syncthreads();
  double s = l_buf[0];
#pragma unroll
  for (int w = 1; w < MOM_WAVES; ++w) s += l_buf[w];
  return s;
}
__device__ __forceinline__ double block_min(double v, double* l_buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) l_buf[wave] = v;
  __syncthreads();
  double s = l_buf[0];
#pragma unroll
  for (int w = 1; w < MOM_WAVES; ++w) s = fmin(s, l_buf[w]);
  return s;
}

// row[n_rep] -> stats[cell][MOM_STATS], by the whole workgroup; has(r) says
// whether replica r contributes, l_buf is MOM_WAVES doubles of LDS.  An empty
// row gives n = 0, M2 = 0 and NaN mean / min / max.  ZERO_INF_SHIFT: an
// infinite shift would turn inf - inf into NaN, so it is replaced by 0; such
// a row's mean is infinite (or NaN) either way.
template <bool ZERO_INF_SHIFT, class Has>
__device__ __forceinline__ void block_moments(const double* __restrict__ row,
                                              int n_rep, double* l_buf,
                                              Has has,
                                              double* __restrict__ stats,
                                              int64_t cell) {
  double cnt = 0.0, first = (double)n_rep;
  for (int r = threadIdx.x; r < n_rep; r += MOM_THREADS) {
    if (has(r)) {
      cnt += 1.0;
      first = fmin(first, (double)r);
    }
  }
  const double n = block_sum(cnt, l_buf);  // exact: counts < 2^53
  const int r0 = (int)block_min(first, l_buf);
  double x0 = r0 < n_rep ? row[r0] : 0.0;
  if (ZERO_INF_SHIFT && isinf(x0)) x0 = 0.0;

  double sum = 0.0;
  for (int r = threadIdx.x; r < n_rep; r += MOM_THREADS)
    if (has(r)) sum += row[r] - x0;
  sum = block_sum(sum, l_buf);
  const double mean = x0 + sum / n;  // n == 0: overwritten below

  double m2 = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int r = threadIdx.x; r < n_rep; r += MOM_THREADS) {
    if (has(r)) {
      double x = row[r];
      double dx = x - mean;
      m2 += dx * dx;
      lo = fmin(lo, x);
      hi = fmax(hi, x);
    }
  }
  m2 = block_sum(m2, l_buf);
  lo = block_min(lo, l_buf);
  hi = -block_min(-hi, l_buf);
  if (threadIdx.x == 0) {
    double* out = stats + cell * MOM_STATS;
    const bool any = n > 0.0;
    const double qnan = __builtin_nan("");
    out[0] = n;
    out[1] = any ? mean : qnan;
    out[2] = any ? m2 : 0.0;
    out[3] = any ? lo : qnan;
    out[4] = any ? hi : qnan;
  }
}

}  // namespace dcg
