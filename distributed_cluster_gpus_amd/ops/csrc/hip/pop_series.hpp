// Population time series: per-tick Monte-Carlo statistics over the replica
// ensemble (gfx950).
//
// With the feature on, EVERY replica records a snapshot of its per-DC state
// at every log tick (the sampling hook lives next to emit_cluster_rows in
// replica_engine.hip), into
//
//   samples[t_cap][n_dc + 1][PS_K][n_rep]      f64, replica-minor
//
// row n_dc is the fleet row ("ALL").  Launches are bounded by events, not by
// time, so replicas drift apart: the buffer covers the whole run and each
// replica indexes it by its own log-tick counter tick[r].
//
// reduce_series turns the raw samples into {n, mean, M2, min, max} per
// (tick, cell): one workgroup per cell, threads striding over the coalesced
// replica axis.  Two passes over the samples in f64 (shifted sum -> mean,
// then sum (x - mean)^2 with min/max; the 32 KB row of a 4096-replica run is
// re-read from cache) — a one-pass sum-of-squares loses everything for
// energies ~1e9 with unit spread.  Partials are combined in a fixed order
// (per-thread strided partial, shuffle tree inside the wave, waves 0..3
// through LDS), so the result is bitwise reproducible for a given replica
// count.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace dcg {

// sampled metrics per DC, in buffer order (cl_rows column in brackets):
// freq [2], busy [3], running [5], q_inf [8], q_trn [9], power_w [13],
// energy_j [14]
constexpr int PS_K = 7;
constexpr int PS_STATS = 5;  // n, mean, M2, min, max

struct PopSeriesDesc {
  double* samples;  // [t_cap][n_dc+1][PS_K][n_rep]
  double* time;     // [t_cap] tick times (local replica 0 writes them)
  int* tick;        // [n_rep] log ticks this replica has processed
  int t_cap;
  int every;        // sample when tick % every == 0, at index tick/every - 1
};

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;

// fixed-order block reductions: shuffle tree in each wave, then thread 0
// folds the wave results in wave order and every thread reads the total back
__device__ __forceinline__ double ps_block_sum(double v, double* l_buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // l_buf may still be read from the previous reduction
  if (lane == 0) l_buf[wave] = v;
  __syncthreads();
  double s = l_buf[0];
#pragma unroll
  for (int w = 1; w < PS_WAVES; ++w) s += l_buf[w];
  return s;
}
__device__ __forceinline__ double ps_block_min(double v, double* l_buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) l_buf[wave] = v;
  __syncthreads();
  double s = l_buf[0];
#pragma unroll
  for (int w = 1; w < PS_WAVES; ++w) s = fmin(s, l_buf[w]);
  return s;
}

// replica r has a sample at tick index t iff tick[r] / every > t, so an
// unfinished run yields a correct per-tick n
__global__ void __launch_bounds__(PS_THREADS)
reduce_series_kernel(const double* __restrict__ samples,
                     const int* __restrict__ tick, int every, int n_cells,
                     int n_rep, double* __restrict__ stats) {
  __shared__ double l_buf[PS_WAVES];
  const int64_t cell = blockIdx.x;         // t * n_cells + c
  const int t = (int)(cell / n_cells);
  const double* row = samples + cell * (int64_t)n_rep;

  // pass 0 (tick counters only): count, and the first contributing replica.
  // Its sample x0 is the shift of pass 1: the mean is x0 + sum(x - x0) / n,
  // so the sum runs over the spread, not the magnitude, and a cell whose
  // samples are all equal gets exactly that value and M2 == 0.
  double cnt = 0.0, first = (double)n_rep;
  for (int r = threadIdx.x; r < n_rep; r += PS_THREADS) {
    if (tick[r] / every > t) {
      cnt += 1.0;
      first = fmin(first, (double)r);
    }
  }
  const double n = ps_block_sum(cnt, l_buf);   // exact: counts < 2^53
  const int r0 = (int)ps_block_min(first, l_buf);
  const double x0 = r0 < n_rep ? row[r0] : 0.0;

  // pass 1: shifted sum -> mean
  double sum = 0.0;
  for (int r = threadIdx.x; r < n_rep; r += PS_THREADS)
    if (tick[r] / every > t) sum += row[r] - x0;
  sum = ps_block_sum(sum, l_buf);
  const double mean = x0 + sum / n;            // n == 0: overwritten below

  // pass 2: centred second moment, min, max
  double m2 = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int r = threadIdx.x; r < n_rep; r += PS_THREADS) {
    if (tick[r] / every > t) {
      double x = row[r];
      double dx = x - mean;
      m2 += dx * dx;
      lo = fmin(lo, x);
      hi = fmax(hi, x);
    }
  }
  m2 = ps_block_sum(m2, l_buf);
  lo = ps_block_min(lo, l_buf);
  hi = -ps_block_min(-hi, l_buf);
  if (threadIdx.x == 0) {
    double* out = stats + cell * PS_STATS;
    const bool any = n > 0.0;
    const double qnan = __builtin_nan("");
    out[0] = n;
    out[1] = any ? mean : qnan;
    out[2] = any ? m2 : 0.0;
    out[3] = any ? lo : qnan;
    out[4] = any ? hi : qnan;
  }
}

// (samples[T, C, R] f64, ticks[R] i32, every) -> stats[T, C, 5] f64
inline torch::Tensor reduce_series(torch::Tensor samples, torch::Tensor ticks,
                                   int64_t every) {
  TORCH_CHECK(samples.is_cuda() && ticks.is_cuda(),
              "reduce_series: tensors must live on the GPU");
  TORCH_CHECK(samples.dtype() == torch::kFloat64 && samples.dim() == 3,
              "reduce_series: samples must be f64 [T, C, R]");
  TORCH_CHECK(ticks.dtype() == torch::kInt32 && ticks.dim() == 1 &&
                  ticks.size(0) == samples.size(2),
              "reduce_series: ticks must be i32 [R]");
  TORCH_CHECK(every >= 1 && every <= INT32_MAX, "reduce_series: every >= 1");
  samples = samples.contiguous();
  ticks = ticks.contiguous();
  const int64_t T = samples.size(0), C = samples.size(1), R = samples.size(2);
  TORCH_CHECK(R >= 1 && R <= INT32_MAX && C <= INT32_MAX &&
                  T * C <= INT32_MAX,
              "reduce_series: shape out of range");
  auto stats = torch::empty({T, C, (int64_t)PS_STATS}, samples.options());
  if (T * C == 0) return stats;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(reduce_series_kernel, dim3((unsigned)(T * C)),
                     dim3(PS_THREADS), 0, stream, samples.data_ptr<double>(),
                     ticks.data_ptr<int>(), (int)every, (int)C, (int)R,
                     stats.data_ptr<double>());
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("reduce_series_kernel: ") +
                             hipGetErrorString(e));
  return stats;
}

}  // namespace dcg
