// Bin arithmetic of the per-replica latency histograms (lat_hist.hpp; the
// recording hook sits at the job-finish site of advance_kernel).
// Pure C++ (no HIP, no torch): it compiles for the host alone, and the
// kernels include it too.
//
// A bin is read off the f64 bit pattern: the exponent and the top
// LH_SUB_BITS mantissa bits, i.e. 8 bins per octave.  No transcendental is
// involved, so host and device agree exactly.  Bin b in 1..254 is
// [lower(b), upper(b)) with upper / lower <= 1.125; the bins run from
// 2^-14 s (61 us) to 2^18 s (about 3 days); bin 0 also takes everything
// below (0, denormals, NaN), bin 255 everything above (+inf included).
//
// The quantile q of a histogram of n > 0 samples is reported as the UPPER
// edge of the first bin whose cumulative count reaches lat_rank(q, n).  For
// the true k-th order statistic x_k, k = lat_rank(q, n), inside the exact
// range [2^-14, 1.875 * 2^17) that gives x_k < reported <= 1.125 * x_k.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCG_HD __host__ __device__
#else
#define DCG_HD
#endif

namespace dcg {

constexpr int LH_SUB_BITS = 3;
constexpr int LH_BINS = 256;
constexpr int LH_SHIFT = 52 - LH_SUB_BITS;  // 49
constexpr long long LH_KEY0 = (1023ll - 14) << LH_SUB_BITS;

DCG_HD inline uint64_t lat_bits_of(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}
DCG_HD inline double lat_double_of(uint64_t u) {
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

DCG_HD inline int lat_bin(double x) {
  x = x > 0.0 ? x : 0.0;  // negatives, -0 and NaN count as 0
  long long key = (long long)(lat_bits_of(x) >> LH_SHIFT) - LH_KEY0;
  return (int)(key < 0 ? 0 : key > LH_BINS - 1 ? LH_BINS - 1 : key);
}

DCG_HD inline double lat_bin_lower(int b) {
  return lat_double_of((uint64_t)(LH_KEY0 + b) << LH_SHIFT);
}
DCG_HD inline double lat_bin_upper(int b) {
  return b < LH_BINS - 1
             ? lat_double_of((uint64_t)(LH_KEY0 + b + 1) << LH_SHIFT)
             : std::numeric_limits<double>::infinity();
}

// 1-based rank of the order statistic that quantile q of n samples reports
DCG_HD inline long long lat_rank(double q, long long n) {
  return (long long)ceil(q * (double)n);
}

}  // namespace dcg
