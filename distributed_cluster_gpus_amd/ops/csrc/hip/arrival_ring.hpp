// The arrival ring: a replica's merged arrival sequence, produced ahead of
// the advance kernel.
//
// In every algorithm but chsac_af the arrival process is autonomous: an
// arrival's size, its random route and its stream's next arrival time depend
// only on the replica's Philox counter and on the stream's previous arrival
// time, and no other event draws a random number.  The advance kernel gives a
// replica a whole wavefront, so there this arithmetic (Philox blocks, log,
// pow, fmod, sin) runs 1 wide on a 64-wide vector unit.  pregen_arrivals_kernel
// runs it lane-parallel instead and appends the result to a per-replica ring
// of ARec records in global memory; the PRE instantiations of the advance
// kernel take the head record at an arrival event instead of drawing.
//
// Results are bitwise those of the inline draws: the generator walks the
// streams in the event select's order (earliest next arrival, lowest stream
// index on a tie), gives every draw the counter the advance kernel would have
// given it (size, route unless the algorithm routes itself, then two per
// thinning round), and evaluates the same map functions (philox.hpp,
// thinning_rate below) on the same uniforms.  Each record carries the
// counter after its arrival, so S.rng_ctr and S.arr_next keep meaning "after
// the last PROCESSED event" whatever the generator has run ahead.
//
// Lanes: a group of PG_GROUP = 8 lanes owns a replica.
//   * the 16 stream times live two per lane; the earliest is a 3-stage
//     butterfly inside the group;
//   * the serial chain of a replica is "time of arrival k -> inter-arrival
//     time -> time of arrival k+1".  Only the inter-arrival draw is on it, so
//     only that is computed in the walk: the group evaluates four thinning
//     rounds side by side (even lane = candidate waiting time and its
//     acceptance threshold, odd lane = the acceptance uniform), takes the
//     first accepted one and counts the draws up to it;
//   * size and route are off the chain: every eighth walk step each lane
//     finishes ONE of the group's last eight arrivals (one Philox block or
//     two, the size map, rbelow) and stores its record, so those maps run 64
//     wide and once per arrival.
// One lane per replica was not built: at 4096 replicas it leaves 64 waves on
// 1024 SIMDs, and the whole serial chain (profiles/README.md) on each.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "arrival_plan.hpp"
#include "engine_desc.hpp"
#include "philox.hpp"
#include "sim_models.hpp"

namespace dcg {

// arrival rate of the sinusoid process at time t + w (reference
// arrivals.py:35-48); the one expression both the inline thinning loop and
// the generator evaluate
__device__ __forceinline__ double thinning_rate(double rate, double amp,
                                                double period, double t,
                                                double w) {
  return fmax(0.0, rate * (1.0 + amp *
      sin(2.0 * M_PI * fmod(t + w, period) / period)));
}

// job size from the two uniforms of one Philox block: Pareto for inference
// (the first uniform), clamped lognormal for training (both) -- the maps
// behind rpareto_inf / rlognormal
__device__ __forceinline__ double job_size_map(int jt, double ua, double ub) {
  return jt == 0 ? rpareto_inf_map(ua)
                 : fmax(0.1, rlognormal_map(ua, ub, log(50000.0), 0.4));
}

#if DCG_SUBWAVE == 64
constexpr int PG_GROUP = 8;      // lanes per replica
constexpr int PG_THREADS = 256;  // 32 replicas per block, no LDS
static_assert(MAX_STREAMS == 2 * PG_GROUP, "two stream times per lane");

// a predicate's ballot over the caller's 8-lane group (bit i = group lane i)
__device__ __forceinline__ int pg_group_ballot(bool p, int lane64) {
  unsigned long long m = __ballot(p);
  return (int)((m >> (lane64 & ~(PG_GROUP - 1))) & 0xffull);
}

// Arrival mode 3, a piecewise-constant rate profile (ProfDesc): the gap g >= 0
// after an arrival at t with integral_t^{t+g} lambda = E, E a unit
// exponential, by exact inversion; no thinning.  models/arrivals.py
// profile_gap is the host twin, operation for operation: contraction is off,
// so a*b+c rounds twice here as it does there, and fmod, the division and
// floor are exact or correctly rounded on both sides.  Called by all eight
// lanes of a group with the same arguments; the lanes share the search for
// the landing segment (lane gl tests segments gl, gl + 8, ..., the group
// ballot picks the first), and all return the same value.  D_INF where the
// stream is off (rate 0 or a row of zeros); the caller then draws nothing.
__device__ __forceinline__ bool profile_on(double rate, const double* row) {
  const int K = min((int)row[0], PROF_MAX_SEG);
  return rate > 0 && row[1 + PROF_MAX_SEG + K] > 0;
}
__device__ __forceinline__ double profile_gap(double E, double t, double rate,
                                              double period, const double* row,
                                              int gl, int lane64) {
#pragma clang fp contract(off)
  const int K = min((int)row[0], PROF_MAX_SEG);
  const double* m = row + 1;
  const double* cum = row + 1 + PROF_MAX_SEG;
  const double M = cum[K];
  if (!(rate > 0 && M > 0)) return D_INF;
  const double x = fmod(t, period) / period;
  const int k0 = min(K - 1, (int)(x * (double)K));
  const double A = cum[k0] + (x - (double)k0 / (double)K) * m[k0];
  const double T = A + E / (rate * period);
  double n = floor(T / M);
  double Tp = T - n * M;
  if (Tp >= M) { Tp -= M; n += 1.0; }
  if (Tp < 0) Tp = 0.0;
  // the first k with cum[k + 1] > Tp: cum[k] <= Tp, hence m[k] > 0
  int k = K - 1;
  bool found = false;
  for (int j = 0; j < K && !found; j += PG_GROUP) {
    const int kk = j + gl;
    const bool p = kk < K && cum[kk + 1] > Tp;
    const int b = pg_group_ballot(p, lane64);
    if (b) { k = j + __ffs(b) - 1; found = true; }
  }
  const double xp = (double)k / (double)K + (Tp - cum[k]) / m[k];
  return fmax(0.0, (n + xp - x) * period);
}

// Tops every live replica's ring up to ring_topup_target(budget, cap)
// records, or to the last arrival not later than min(end_time, t_target),
// whichever comes first, continuing from the generator's frontier.  With an
// empty ring the frontier IS the consumed state, so it is re-read from
// S.arr_next / S.rng_ctr (which also covers the first launch of a run and a
// host that rewrote those tensors between runs).
//
// SWP: a parameter sweep is on (SweepDesc): rate, amplitude and period are
// the replica's own, loaded once per lane before the walk, instead of the
// EngineDesc scalars.  The modes are not swept.  SWP = false never looks at W.
//
// PROF: a job type is in mode 3 (rate profile): its gap is one draw inverted
// through the winning stream's row of P (profile_gap).  The other job type
// keeps its own mode.  PROF = false never looks at P and holds no code for it.
template <bool SWP, bool PROF>
__global__ void __launch_bounds__(PG_THREADS)
pregen_arrivals_kernel(EngineDesc S, ArrRing A, double t_target,
                       long long budget, SweepDesc W, ProfDesc P) {
  const int r = (int)((blockIdx.x * (unsigned)PG_THREADS + threadIdx.x) /
                      PG_GROUP);
  const int gl = threadIdx.x & (PG_GROUP - 1);
  const int lane64 = threadIdx.x & 63;
  const int NS = S.n_streams;
  const bool live = r < S.n_rep && !S.done[r];
  const long long target = ring_topup_target(budget, A.cap);
  const double t_lim = fmin(S.end_time, t_target);
  const int n_hdr = S.algo == A_ECO_ROUTE ? 1 : 2;  // size (+ route) draws

  int count = 0, head = 0;
  uint64_t ctr = 0, key = 0;
  double s0 = D_INF, s1 = D_INF;  // streams 2*gl (inference), 2*gl+1 (training)
  if (live) {
    count = A.count[r];
    head = A.head[r];
    const bool empty = count == 0;
    const double* an = (empty ? S.arr_next : A.gen_arr_next) + (int64_t)r * NS;
    ctr = empty ? S.rng_ctr[r] : A.gen_ctr[r];
    if (2 * gl < NS) s0 = an[2 * gl];
    if (2 * gl + 1 < NS) s1 = an[2 * gl + 1];
    key = S.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(S.rep_id_offset + r));
  }
  // SWP: the replica's own arrival parameters by job type, six registers
  // (a dead lane never walks)
  double rate0 = 0.0, rate1 = 0.0, amp0 = 0.0, amp1 = 0.0;
  double period0 = 1.0, period1 = 1.0;
  if (SWP && live) {
    const double* sw = W.arr + (int64_t)r * 6;
    rate0 = sw[0]; amp0 = sw[1]; period0 = sw[2];
    rate1 = sw[3]; amp1 = sw[4]; period1 = sw[5];
  }

  // the arrival this lane finishes at the next flush
  bool pend = false;
  uint64_t p_ctr = 0, p_after = 0;
  double p_tnext = 0.0;
  int p_stream = 0, p_slot = 0;
  auto flush = [&]() {
    if (pend) {
      uint32_t w[4];
      philox4x32(key, p_ctr, w);
      // the two uniforms of u01x2 (the first is u01's)
      double ua = u01_map(w[0], w[1]);
      double ub = ((w[2] >> 5) * 67108864.0 + (w[3] >> 6)) *
                  (1.0 / 9007199254740992.0);
      ARec rec;
      rec.size = job_size_map(p_stream & 1, ua, ub);
      rec.t_next = p_tnext;
      rec.ctr = p_after;
      rec.stream = p_stream;
      rec.dc = -1;
      if (n_hdr == 2) {
        philox4x32(key, p_ctr + 1, w);
        rec.dc = (int)rbelow_map(w[0], (uint32_t)S.n_dc);
      }
      A.ring[(int64_t)r * A.cap + p_slot] = rec;
      pend = false;
    }
  };

  bool act = live;
  for (int it = 0;; ++it) {
    if (act) act = count < target;
    // earliest stream of the group; the lower stream index wins a tie, as
    // the lower lane does in the advance kernel's event select
    double bv = s0;
    int bi = 2 * gl;
    if (act) {
      if (s1 < bv) { bv = s1; bi = 2 * gl + 1; }
#pragma unroll
      for (int off = 1; off < PG_GROUP; off <<= 1) {
        double ov = __shfl_xor(bv, off, 64);
        int oi = __shfl_xor(bi, off, 64);
        if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      // the advance kernel processes an event at t iff t <= end_time and
      // t <= t_target
      if (bv > t_lim) act = false;
    }
    if (!__any(act)) break;
    if (act) {
      const int jt = bi & 1;
      const uint64_t c_hdr = ctr;
      uint64_t c = ctr + n_hdr;
      // inter-arrival time: draw_interarrival's cases, its counters
      // (selects, not S.arr_*[jt]: jt differs between the groups of a wave,
      // and a lane-indexed kernel argument would be copied to scratch)
      // (SWP: the same selects between the replica's registers)
      const double rate = SWP ? (jt ? rate1 : rate0)
                              : (jt ? S.arr_rate[1] : S.arr_rate[0]);
      const int mode = jt ? S.arr_mode[1] : S.arr_mode[0];
      const double amp = SWP ? (jt ? amp1 : amp0)
                             : (jt ? S.arr_amp[1] : S.arr_amp[0]);
      const double period = SWP ? (jt ? period1 : period0)
                                : (jt ? S.arr_period[1] : S.arr_period[0]);
      const double lambd = mode == 1 ? rate * (1.0 + fabs(amp)) : rate;
      double ia = D_INF;
      bool prof = false;
      if constexpr (PROF) {
        prof = mode == 3;
        if (prof) {
          // one draw, the same in every lane, as in the Poisson case; rows
          // differ between the groups of a wave, a group reads one
          const double* row = P.tab + (int64_t)bi * PROF_W;
          if (profile_on(rate, row)) {
            uint32_t w[4];
            philox4x32(key, c, w);
            const double E = rexp_map(u01_map(w[0], w[1]), 1.0);
            ia = profile_gap(E, bv, rate, period, row, gl, lane64);
            c += 1;
          }
        }
      }
      if (!prof && (mode == 0 || mode == 1) && lambd > 0) {
        // Poisson: one draw, the same in every lane.  Sinusoid: lane pair
        // (2i, 2i+1) is round i of this pass, up to 4096 rounds in all
        for (int pass = 0; pass < 4096 / (PG_GROUP / 2); ++pass) {
          uint32_t w[4];
          philox4x32(key, c + (mode == 1 ? gl : 0), w);
          double u = u01_map(w[0], w[1]);
          double wv = rexp_map(u, lambd);
          if (mode == 0) { ia = wv; c += 1; break; }
          double thr = thinning_rate(rate, amp, period, bv, wv) / lambd;
          double un = __shfl_down(u, 1, 64);  // the pair's acceptance uniform
          int m = pg_group_ballot(!(gl & 1) && un <= thr, lane64);
          if (m) {
            int first = __ffs(m) - 1;  // an even group lane: round first / 2
            ia = __shfl(wv, (lane64 & ~(PG_GROUP - 1)) + first, 64);
            c += first + 2;
            break;
          }
          c += PG_GROUP;
        }
      }
      const double tn = bv + ia;
      if (bi == 2 * gl) s0 = tn;
      if (bi == 2 * gl + 1) s1 = tn;
      ctr = c;
      if ((it & (PG_GROUP - 1)) == gl) {
        pend = true;
        p_ctr = c_hdr;
        p_after = c;
        p_tnext = tn;
        p_stream = bi;
        p_slot = ring_slot(head, count, A.cap);
      }
      ++count;
    }
    if ((it & (PG_GROUP - 1)) == PG_GROUP - 1) flush();
  }
  flush();

  if (live) {
    if (2 * gl < NS) A.gen_arr_next[(int64_t)r * NS + 2 * gl] = s0;
    if (2 * gl + 1 < NS) A.gen_arr_next[(int64_t)r * NS + 2 * gl + 1] = s1;
    if (gl == 0) {
      A.gen_ctr[r] = ctr;
      A.count[r] = count;
    }
  }
}
#endif  // DCG_SUBWAVE == 64

}  // namespace dcg
