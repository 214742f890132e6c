// Per-replica latency histograms: tail quantiles and SLA misses over the
// replica ensemble (gfx950).
//
// With the feature on, EVERY replica counts each of its job finishes (the
// hook sits in the lane-0 section of the job-finish block of advance_kernel,
// replica_engine.hip; one wave owns one replica, so plain loads and stores
// suffice) into
//
//   hist[n_rep][n_dc][2][LH_BINS]   i32, bins of lat_bins.hpp
//   over[n_rep][n_dc][2]            i32, finishes with sojourn > sla_s
//
// indexed (replica, DC, job type).  The histograms live in global memory:
// 2 KiB per (replica, DC) has no place in the advance kernel's LDS budget.
//
// latency_reduce turns them into
//   pop_hist[C', B]   i64  sum over replicas (integer: exact, order-free)
//   per_rep[C', K, R] f64  replica-minor; K = Q + 2: the Q quantiles by the
//                          rule of lat_bins.hpp, sla_miss_frac = over/count,
//                          jobs = count; quantiles and fraction are NaN where
//                          the replica's cell is empty
//   stats[C', K, 5]   f64  {n, mean, M2, min, max} over the replicas whose
//                          value is not NaN
// with C' = (n_dc + 1) * 2 cells (row, jt); row n_dc is the fleet row "ALL",
// the sum over DCs.
//
// lat_cell_kernel maps one wavefront to one (replica, cell): the 64 lanes
// load the 256 bins as one coalesced 1 KiB row, 4 bins (16 B) per lane, the
// fleet row adds the n_dc rows the same way; a shuffle scan gives every lane
// its cumulative counts, and for each rank a ballot finds the first lane that
// reaches it.  lat_stats_kernel is the shared ensemble reduction of
// moments.hpp over the replica axis with "is not NaN" as the mask, so it is
// bitwise reproducible for a given replica count.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <tuple>

#include "lat_bins.hpp"
#include "moments.hpp"
#include "sim_models.hpp"

namespace dcg {

struct LatHistDesc {
  int* hist;     // [n_rep][n_dc][2][LH_BINS]
  int* over;     // [n_rep][n_dc][2]
  double sla_s;  // a finish counts in `over` when its sojourn exceeds this
};

// the job-finish hook of advance_kernel<.., LAT = true>: lane 0 of the
// replica's lanes counts the sojourn x of a type-jt job finishing at DC d
__device__ __forceinline__ void lat_hist_record(const LatHistDesc& L,
                                                int64_t r, int n_dc, int d,
                                                int jt, double x) {
  const int64_t cell = (r * n_dc + d) * 2 + jt;
  // (64-lane build: the sojourn is the wave's, so the bin is scalar and the
  // whole address with it; with the bin in a VGPR more instantiations lost
  // a wave per SIMD, profiles/README.md)
  L.hist[cell * LH_BINS + sub_uniform_i32(lat_bin(x))] += 1;
  if (x > L.sla_s) L.over[cell] += 1;
}

constexpr int LH_MAX_Q = 8;
constexpr int LH_PER_LANE = LH_BINS / 64;  // 4 bins = one 16-byte load
constexpr int LH_THREADS = 256;
constexpr int LH_POP_CHUNK = 64;           // replicas per lat_pop_kernel block
static_assert(LH_PER_LANE == 4, "one int4 load per lane covers the row");
static_assert(LH_THREADS == LH_BINS && LH_THREADS == MOM_THREADS,
              "lat_pop_kernel: a thread per bin; lat_stats_kernel: block_moments");

struct LatQuantiles {
  double q[LH_MAX_Q];
  int n;
};

// one wavefront per (replica, cell)
__global__ void __launch_bounds__(LH_THREADS)
lat_cell_kernel(const int* __restrict__ hist, const int* __restrict__ over,
                int n_rep, int n_dc, LatQuantiles Q,
                double* __restrict__ per_rep) {
  const int lane = threadIdx.x & 63;
  const int n_cell = (n_dc + 1) * 2;
  const int64_t wave =
      (int64_t)blockIdx.x * (LH_THREADS / 64) + (threadIdx.x >> 6);
  if (wave >= (int64_t)n_rep * n_cell) return;  // whole waves leave together
  const int r = (int)(wave / n_cell);
  const int c = (int)(wave % n_cell);
  const int row = c >> 1, jt = c & 1;

  // this lane's 4 bins (and the cell's `over`), summed over DCs for the
  // fleet row
  const int d0 = row < n_dc ? row : 0;
  const int d1 = row < n_dc ? row + 1 : n_dc;
  long long v[LH_PER_LANE] = {0, 0, 0, 0};
  long long n_over = 0;
  for (int d = d0; d < d1; ++d) {
    const int64_t cell = ((int64_t)r * n_dc + d) * 2 + jt;
    const int4 h = *reinterpret_cast<const int4*>(hist + cell * LH_BINS +
                                                  lane * LH_PER_LANE);
    v[0] += h.x; v[1] += h.y; v[2] += h.z; v[3] += h.w;
    n_over += over[cell];
  }
  // inclusive cumulative counts: inside the lane, then a shuffle scan of the
  // lane totals
  long long cum[LH_PER_LANE];
  cum[0] = v[0];
#pragma unroll
  for (int i = 1; i < LH_PER_LANE; ++i) cum[i] = cum[i - 1] + v[i];
  long long incl = cum[LH_PER_LANE - 1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    long long up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const long long before = incl - cum[LH_PER_LANE - 1];
#pragma unroll
  for (int i = 0; i < LH_PER_LANE; ++i) cum[i] += before;
  const long long n = __shfl(incl, 63, 64);

  const int K = Q.n + 2;
  double* out = per_rep + (int64_t)c * K * n_rep + r;
  const double qnan = __builtin_nan("");
  for (int k = 0; k < Q.n; ++k) {
    const long long rank = lat_rank(Q.q[k], n);
    // first bin of this lane whose cumulative count reaches the rank
    int first = LH_PER_LANE;
#pragma unroll
    for (int i = LH_PER_LANE - 1; i >= 0; --i)
      if (cum[i] >= rank) first = i;
    const unsigned long long hit = __ballot(first < LH_PER_LANE);
    // n > 0 and q <= 1: rank <= n = cum of the last bin, so some lane hits
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;
    const int b = __shfl(src * LH_PER_LANE + min(first, LH_PER_LANE - 1), src,
                         64);
    if (lane == 0)
      out[(int64_t)k * n_rep] = n > 0 ? lat_bin_upper(b) : qnan;
  }
  if (lane == 0) {
    out[(int64_t)Q.n * n_rep] = n > 0 ? (double)n_over / (double)n : qnan;
    out[(int64_t)(Q.n + 1) * n_rep] = (double)n;
  }
}

// pop_hist[c][bin] += sum over a chunk of replicas; a thread per bin, the
// chunk partial added with one integer atomic (exact in any order)
__global__ void __launch_bounds__(LH_THREADS)
lat_pop_kernel(const int* __restrict__ hist, int n_rep, int n_dc,
               unsigned long long* __restrict__ pop_hist) {
  const int c = blockIdx.x;
  const int row = c >> 1, jt = c & 1;
  const int d0 = row < n_dc ? row : 0;
  const int d1 = row < n_dc ? row + 1 : n_dc;
  const int r0 = blockIdx.y * LH_POP_CHUNK;
  const int r1 = min(n_rep, r0 + LH_POP_CHUNK);
  unsigned long long acc = 0;
  for (int r = r0; r < r1; ++r)
    for (int d = d0; d < d1; ++d)
      acc += (unsigned long long)(long long)
          hist[(((int64_t)r * n_dc + d) * 2 + jt) * LH_BINS + threadIdx.x];
  if (acc) atomicAdd(&pop_hist[(int64_t)c * LH_BINS + threadIdx.x], acc);
}

// {n, mean, M2, min, max} of one per_rep row over the replicas whose value is
// not NaN
__global__ void __launch_bounds__(LH_THREADS)
lat_stats_kernel(const double* __restrict__ per_rep, int n_rep,
                 double* __restrict__ stats) {
  __shared__ double l_buf[MOM_WAVES];
  const int64_t cell = blockIdx.x;  // c * K + k
  const double* row = per_rep + cell * (int64_t)n_rep;
  block_moments<true>(
      row, n_rep, l_buf, [=](int r) { return row[r] == row[r]; },
      stats, cell);
}

// (hist[R, D, 2, B] i32, over[R, D, 2] i32, qs[Q] f64 on any device,
// 1 <= Q <= 8, each q in (0, 1]) -> (pop_hist[C', B] i64,
// per_rep[C', Q + 2, R] f64, stats[C', Q + 2, 5] f64), on the current stream
inline std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> latency_reduce(
    torch::Tensor hist, torch::Tensor over, torch::Tensor qs) {
  TORCH_CHECK(hist.is_cuda() && over.is_cuda() &&
                  hist.device() == over.device(),
              "latency_reduce: hist and over must live on one GPU");
  TORCH_CHECK(hist.dtype() == torch::kInt32 && hist.dim() == 4 &&
                  hist.size(2) == 2 && hist.size(3) == LH_BINS,
              "latency_reduce: hist must be i32 [R, D, 2, ", LH_BINS, "]");
  TORCH_CHECK(over.dtype() == torch::kInt32 && over.dim() == 3 &&
                  over.size(0) == hist.size(0) &&
                  over.size(1) == hist.size(1) && over.size(2) == 2,
              "latency_reduce: over must be i32 [R, D, 2]");
  TORCH_CHECK(qs.dtype() == torch::kFloat64 && qs.dim() == 1 &&
                  qs.size(0) >= 1 && qs.size(0) <= LH_MAX_Q,
              "latency_reduce: qs must be f64 [Q], 1 <= Q <= ", LH_MAX_Q);
  hist = hist.contiguous();
  over = over.contiguous();
  auto qh = qs.cpu().contiguous();
  LatQuantiles Q{};
  Q.n = (int)qh.size(0);
  for (int k = 0; k < Q.n; ++k) {
    Q.q[k] = qh.data_ptr<double>()[k];
    TORCH_CHECK(Q.q[k] > 0.0 && Q.q[k] <= 1.0,
                "latency_reduce: quantiles must lie in (0, 1]");
  }
  const int64_t R = hist.size(0), D = hist.size(1);
  const int64_t C = (D + 1) * 2, K = Q.n + 2;
  TORCH_CHECK(R >= 1 && R <= INT32_MAX && D >= 1 && D <= 1024 &&
                  R * C / (LH_THREADS / 64) + 1 <= INT32_MAX &&
                  (R + LH_POP_CHUNK - 1) / LH_POP_CHUNK <= 65535,
              "latency_reduce: shape out of range");
  auto pop = torch::zeros({C, (int64_t)LH_BINS},
                          hist.options().dtype(torch::kInt64));
  auto per_rep = torch::empty({C, K, R}, hist.options().dtype(torch::kFloat64));
  auto stats = torch::empty({C, K, (int64_t)MOM_STATS}, per_rep.options());
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const int64_t waves = R * C, per_block = LH_THREADS / 64;
  hipLaunchKernelGGL(lat_cell_kernel,
                     dim3((unsigned)((waves + per_block - 1) / per_block)),
                     dim3(LH_THREADS), 0, stream, hist.data_ptr<int>(),
                     over.data_ptr<int>(), (int)R, (int)D, Q,
                     per_rep.data_ptr<double>());
  hipLaunchKernelGGL(
      lat_pop_kernel,
      dim3((unsigned)C, (unsigned)((R + LH_POP_CHUNK - 1) / LH_POP_CHUNK)),
      dim3(LH_THREADS), 0, stream, hist.data_ptr<int>(), (int)R, (int)D,
      reinterpret_cast<unsigned long long*>(pop.data_ptr<int64_t>()));
  hipLaunchKernelGGL(lat_stats_kernel, dim3((unsigned)(C * K)),
                     dim3(LH_THREADS), 0, stream, per_rep.data_ptr<double>(),
                     (int)R, stats.data_ptr<double>());
  check_launch("latency_reduce");
  return {pop, per_rep, stats};
}

}  // namespace dcg
