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
// (tick, cell): one workgroup per cell, by the shared ensemble reduction of
// moments.hpp (three passes in f64, fixed-order folds, bitwise reproducible
// for a given replica count).
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "moments.hpp"

namespace dcg {

// sampled metrics per DC, in buffer order (cl_rows column in brackets):
// freq [2], busy [3], running [5], q_inf [8], q_trn [9], power_w [13],
// energy_j [14]
constexpr int PS_K = 7;

struct PopSeriesDesc {
  double* samples;  // [t_cap][n_dc+1][PS_K][n_rep]
  double* time;     // [t_cap] tick times (local replica 0 writes them)
  int* tick;        // [n_rep] log ticks this replica has processed
  int t_cap;
  int every;        // sample when tick % every == 0, at index tick/every - 1
};

// replica r has a sample at tick index t iff tick[r] / every > t, so an
// unfinished run yields a correct per-tick n
__global__ void __launch_bounds__(MOM_THREADS)
reduce_series_kernel(const double* __restrict__ samples,
                     const int* __restrict__ tick, int every, int n_cells,
                     int n_rep, double* __restrict__ stats) {
  __shared__ double l_buf[MOM_WAVES];
  const int64_t cell = blockIdx.x;         // t * n_cells + c
  const int t = (int)(cell / n_cells);
  block_moments<false>(
      samples + cell * (int64_t)n_rep, n_rep, l_buf,
      [=](int r) { return tick[r] / every > t; }, stats, cell);
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
  auto stats = torch::empty({T, C, (int64_t)MOM_STATS}, samples.options());
  if (T * C == 0) return stats;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(reduce_series_kernel, dim3((unsigned)(T * C)),
                     dim3(MOM_THREADS), 0, stream, samples.data_ptr<double>(),
                     ticks.data_ptr<int>(), (int)every, (int)C, (int)R,
                     stats.data_ptr<double>());
  check_launch("reduce_series_kernel");
  return stats;
}

}  // namespace dcg
