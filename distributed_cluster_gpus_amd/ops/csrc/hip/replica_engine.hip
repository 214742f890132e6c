// Batched Monte-Carlo replica engine for MI355X (gfx950, CDNA4).
//
// Architecture (SURVEY §7 "fixed-Δt lockstep engine with exact event times"):
// each CDNA4 wavefront (64 lanes) owns ONE replica of the multi-DC simulation
// and advances it event-by-event with exact event times; thousands of
// replicas run concurrently (256 CUs x 4 SIMDs x N waves).  All per-replica
// state lives in HBM3E as replica-major structure-of-arrays, so lane-strided
// scans (job-slot min-finish, empty-slot search, queue walks) are coalesced.
// Next-event selection is a wave argmin over {16 arrival streams, in-flight
// WAN transfers, per-DC cached min finish times, next log tick}.  The
// (n, f) grid search maps the full 8x8 candidate grid onto the 64 lanes of
// one wavefront (sim_models.hpp::wave_grid_argmin).
//
// Execution discipline: control flow is wave-uniform — every lane computes
// the same scalar values redundantly; global-memory writes are guarded to
// lane 0; cooperative phases (scans/argmins) use lane-strided reads + the
// subgroup reductions of sim_models.hpp (64-lane build: DPP on the VALU with
// the result in SGPRs, so the event dispatch is scalar branches; 8-lane
// build: shfl_xor butterflies).  Replicas are independent, so kernels need
// no inter-workgroup communication; multi-GPU scaling shards replicas per rank
// (parallel/sharding.py) with RCCL used only for metric reductions.
//
// Event semantics mirror the scalar engines (engine/oracle.py ==
// reference simulator simcore/simulator_paper_multi.py:412-480): per-event
// energy/util accrual using per-job f_used power, queue-drain on completion
// with inference priority, per-algorithm admission decisions, the
// finish%log_interval job-unit remainder quirk, the end-of-run baseline-model
// energy flush.  RNG is Philox (philox.hpp) — parity with the scalar engines
// is distributional, not bitwise (SURVEY §7 "RNG stream equivalence").
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "arrival_ring.hpp"
#include "engine_bind.hpp"
#include "engine_desc.hpp"
#include "engine_limits.hpp"
#include "lat_hist.hpp"
#include "launch_plan.hpp"
#include "moments.hpp"
#include "philox.hpp"
#include "pop_series.hpp"
#include "sim_models.hpp"

namespace dcg {

// ---------------- wave helpers ----------------
// (the subgroup reductions live in sim_models.hpp)
__device__ __forceinline__ void store_fence() {
  // make lane-0 stores (global AND LDS) visible to this wave's subsequent
  // loads: full hardware wait + compiler reordering barrier
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void lds_fence() {
  // lighter fence for sites that only wrote LDS: waiting lgkmcnt alone
  // avoids draining unrelated outstanding global loads (vmcnt)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---------------- hot per-replica state (LDS-resident) ----------------
// The fields every event touches live in LDS for the kernel's lifetime
// (~850 B per replica, ~3.4 KB per 4-replica workgroup of the CU's 160 KiB)
// and are written back to HBM at kernel exit.  This removes most of the
// dependent global-memory round trips per event (PMC before: waves waiting
// 63% of cycles on memory; see profiles/README.md).
constexpr int THREADS_PER_BLOCK = 128;
constexpr int REPLICAS_PER_BLOCK = THREADS_PER_BLOCK / DCG_SUBWAVE;
struct Hot {
  double arr_next[MAX_STREAMS];
  // per-replica scalars updated every arrival/finish — LDS-resident so the
  // hot path never does global read-modify-writes for them
  double sum_lat, sum_lat_inf, sum_wait;
  long long jobs_done, jobs_done_inf;
  int jid_ctr, seq_ctr;
  double dc_minf[MAX_DC];
  double p_active[MAX_DC];
  double sum_tpt[MAX_DC];
  double energy[MAX_DC];
  double util_time[MAX_DC];
  double acc_unit[MAX_DC];
  double util_begin[MAX_DC];
  double next_log;
  double cur_freq[MAX_DC];
  int dc_mins[MAX_DC];
  int busy[MAX_DC];
  int n_running[MAX_DC];
  int q_len[MAX_DC * 2];
  int q_head[MAX_DC * 2];
};

// actor-forward LDS scratch: obs, two activation buffers, head logits
constexpr size_t RL_LDS_BYTES =
    (RL_MAX_OBS + 2 * RL_MAX_HID + RL_MAX_LOG) * sizeof(float);

// Byte sizes of the parts of one replica's dynamic-LDS slice, in carve
// order: Hot, then (SUBW==64 only — at 8 replicas per wave they would exceed
// the LDS budget) the s_finish and x_time mirrors, then (chsac only) the
// actor-forward scratch.  The kernel carves by it, advance() sizes the
// launch by it.
struct LdsSizes {
  size_t hot, fin, xt, rl;
  __host__ __device__ size_t stride() const { return hot + fin + xt + rl; }
};
__host__ __device__ inline LdsSizes lds_sizes(int total_slots, int tcap,
                                              bool chsac) {
  return {(sizeof(Hot) + 15) & ~size_t(15),
          SUBW == 64 ? (size_t)total_slots * sizeof(double) : 0,
          SUBW == 64 ? (size_t)tcap * sizeof(double) : 0,
          chsac ? RL_LDS_BYTES : 0};
}

// ---------------- replica context ----------------
struct Ctx {
  const EngineDesc* S;
  Hot* hs;      // LDS-resident hot state of this wave's replica
  double* l_fin;  // LDS mirror of this replica's s_finish[total_slots]
  double* l_xt;   // LDS mirror of this replica's x_time[tcap]
  // chsac serve-device scratch (LDS): obs vector, two activation ping-pong
  // buffers, and the head logits (dc at +0, g at +8)
  float* l_obs;
  float* l_act_a;
  float* l_act_b;
  float* l_logits;
  int r;        // local replica index
  int lane;
  PhiloxState rng;
  double now;       // last processed event time (or -1)
  double t_first;   // first event time (-1 until known)
  // lane d < n_dc keeps DC d's capacity and per-idle-GPU power (already
  // resolved to power_gating ? p_sleep : p_idle) for the kernel's lifetime:
  // the per-event accrual reads no scenario table
  int my_total;
  double my_pidle;

  // launch-invariant tables (sim_models.hpp: scalar loads in the 64-lane
  // build when the index is wave-uniform)
  __device__ kc_f64 pc3(int d, int jt) const {
    return launch_const(S->pc) + (d * 2 + jt) * 3;
  }
  __device__ kc_f64 lc3(int d, int jt) const {
    return launch_const(S->lc) + (d * 2 + jt) * 3;
  }
  __device__ kc_f64 freq_levels() const { return launch_const(S->freq_levels); }
  __device__ int slot_off(int d) const { return launch_const(S->slot_off)[d]; }
  __device__ int slot_dc(int slot) const {
    return launch_const(S->slot_dc)[slot];
  }
  __device__ int total_gpus(int d) const {
    return launch_const(S->total_gpus)[d];
  }
  __device__ int free_gpus(int d) const {
    return total_gpus(d) - hs->busy[d];
  }
  __device__ double idle_gpu_power(int d) const {
    return launch_const(S->power_gating)[d] ? launch_const(S->p_sleep)[d]
                                            : launch_const(S->p_idle)[d];
  }
  __device__ double dc_power(int d) const {
    int idle = free_gpus(d);
    double pi = idle_gpu_power(d);
    return hs->p_active[d] + idle * pi;
  }
  // lane's own DC, from the registers (lane < n_dc)
  __device__ double my_dc_power() const {
    int idle = my_total - hs->busy[lane];
    return hs->p_active[lane] + idle * my_pidle;
  }
  __device__ double price_kwh(double t) const {
    int h = static_cast<int>(fmod(t, 86400.0) / 3600.0);
    return S->price24[h];
  }
};

// RL trace a chsac arrival carries into its WAN transfer; a null pointer
// stands for a plain (untraced) arrival
struct JobTrace {
  const float* s0;          // observation at decision time [obs_dim]
  int adc, ag, mdc, mg;     // action and mask bytes
  int n_rew;                // the RL-chosen n (unclamped g+1)
};

// recompute a DC's cached min finish (wave-cooperative)
__device__ void rescan_dc_min(Ctx& c, int d) {
  const EngineDesc& S = *c.S;
  int lo = c.slot_off(d), hi = c.slot_off(d + 1);
  double v = D_INF;
  int slot = -1;
  for (int k = lo + c.lane; k < hi; k += SUBW) {
    double f = c.l_fin[k];
    if (f < v) { v = f; slot = k; }
  }
  int wl;
  double best = wave_argmin_f64(v, wl);
  slot = sub_bcast_i32(slot, wl);
  if (c.lane == 0) {
    c.hs->dc_minf[d] = best;
    c.hs->dc_mins[d] = best < D_INF ? slot : -1;
  }
  lds_fence();
}

// start a job on DC d with (n, f); assumes free >= 1; wave-cooperative.
// Keeps the DC's cached min finish exact incrementally; returns true when the
// new finish time TIES the cached minimum — the one case where only a full
// rescan_dc_min reproduces the scan's slot tie-break.
__device__ bool start_job(Ctx& c, int d, int jt, double size, float netlat,
                          int jid, int ing, int n, double f, double now) {
  const EngineDesc& S = *c.S;
  int64_t base = (int64_t)c.r * S.total_slots;
  int lo = c.slot_off(d), hi = c.slot_off(d + 1);
  // find first empty slot (finish == INF <=> s_gpus == 0), from the LDS mirror
  int cand = sub_first_empty(c.l_fin, lo, hi);
  if (cand == INT_MAX) {  // cannot happen if capacities == total_gpus
    if (c.lane == 0) atomicOr(&S.err[c.r], ERR_SLOT_OVF);
    return false;
  }
  double T = d_unit_time(n, f, c.lc3(d, jt));
  double finish = now + (double)size * T;
  double minf = c.hs->dc_minf[d];
  if (c.lane == 0) {
    c.l_fin[cand] = finish;
    SRec* sr = &S.s_rec[base + cand];
    sr->start = now;
    sr->lastupd = now;
    sr->size = size;
    sr->fused = f;
    sr->netlat = netlat;
    sr->jid = jid;
    sr->done = 0.0;
    sr->pcount = 0;
    sr->ing = (unsigned char)ing;
    sr->seq = ++c.hs->seq_ctr;
    sr->has_rl = 0;
    S.s_gpus[base + cand] = (short)n;
    S.s_jtype[base + cand] = (char)jt;
    c.hs->busy[d] += n;
    c.hs->n_running[d] += 1;
    c.hs->p_active[d] += d_job_power(n, f, c.pc3(d, jt));
    c.hs->sum_tpt[d] += 1.0 / T;
    if (finish < minf) {
      c.hs->dc_minf[d] = finish;
      c.hs->dc_mins[d] = cand;
    }
  }
  store_fence();
  return finish == minf;
}

// heuristic allocator (policy.py:16-41 semantics); mutates cur_freq; returns g
__device__ int heuristic_alloc(Ctx& c, int d, int jt) {
  const EngineDesc& S = *c.S;
  int free = c.free_gpus(d);
  int g = free > 0 ? min(free, S.max_gpj) : 0;
  double cf = c.hs->cur_freq[d];
  double nf = cf;
  if (!S.energy_aware) {  // perf_first
    if (jt == 0) nf = S.dvfs_high;
    else {
      int qi = c.hs->q_len[d * 2 + 0];
      nf = fmax(cf, qi > 0 ? S.dvfs_high : launch_const(S.default_freq)[d]);
    }
  } else {
    if (jt == 0) nf = S.dvfs_high;
    else if (S.scale_out_low && free >= 2) {
      nf = S.dvfs_low;
      g = min(free, S.max_gpj);
    } else nf = fmax(cf, S.dvfs_low);
  }
  if (c.lane == 0) c.hs->cur_freq[d] = nf;
  lds_fence();
  return max(1, g);
}

// per-algorithm (n, f) decision at admission; returns chosen n, f
template <int ALGO>
__device__ void decide_nf(Ctx& c, int d, int jt, float size, double now,
                          int& n_out, double& f_out) {
  const EngineDesc& S = *c.S;
  int free = c.free_gpus(d);
  if (ALGO == A_JOINT_NF) {
    GridPick g = S.fp32_score
        ? wave_grid_argmin<float>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                               S.n_freq, S.max_gpj, 0, 0.0, 0.0, false, 0.0)
        : wave_grid_argmin<double>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                           S.n_freq, S.max_gpj, 0, 0.0, 0.0, false, 0.0);
    n_out = g.n; f_out = g.f;
  } else if (ALGO == A_BANDIT) {
    // UCB1 (learners.py:20-36): uniform-redundant serial loop over arms
    long long t = S.b_t[c.r] + 1;
    if (c.lane == 0) S.b_t[c.r] = t;
    int64_t ab = ((int64_t)c.r * S.n_dc + d) * 2 + jt;
    double bf = -1.0;
    for (int k = 0; k < S.n_freq; ++k)
      if (S.b_n[ab * S.n_freq + k] < 1) { bf = S.freq_levels[k]; break; }
    if (bf < 0) {
      double best_ucb = -1e9;
      for (int k = 0; k < S.n_freq; ++k) {
        int nn = S.b_n[ab * S.n_freq + k];
        double mean = S.b_s[ab * S.n_freq + k] / nn;
        double ucb = mean + sqrt(2.0 * log((double)t) / nn);
        if (ucb > best_ucb) { best_ucb = ucb; bf = S.freq_levels[k]; }
      }
    }
    n_out = min(free, S.max_gpj);
    f_out = bf;
  } else if (ALGO == A_CARBON_COST) {
    double price = c.price_kwh(now);
    int obj = price > 0.0 ? 2 : 1;
    double ci = price > 0.0 ? 0.0 : S.carbon[d];
    GridPick g = S.fp32_score
        ? wave_grid_argmin<float>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                               S.n_freq, S.max_gpj, obj, ci, price, false, 0.0)
        : wave_grid_argmin<double>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                           S.n_freq, S.max_gpj, obj, ci, price, false, 0.0);
    n_out = g.n; f_out = g.f;
  } else if (ALGO == A_DEBUG) {
    n_out = S.num_fixed;
    f_out = S.fixed_freq > 0 ? S.fixed_freq
            : (S.fp32_score
               ? wave_energy_freq<float>(c.pc3(d, jt), c.lc3(d, jt),
                                      c.freq_levels(), S.n_freq, S.num_fixed)
               : wave_energy_freq<double>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                                  S.n_freq, S.num_fixed));
  } else {  // heuristic family
    n_out = heuristic_alloc(c, d, jt);
    f_out = c.hs->cur_freq[d];
  }
}

// queue ops (wave-uniform; lane-0 writes).  `enq` is the job's enqueue time
// at this DC — carried per entry so pops can credit the queueing delay.
// `front` inserts ahead of the head (a popped job going back) instead of at
// the tail.
__device__ bool queue_push(Ctx& c, int d, int jt, double size, float netlat,
                           int jid, int ing, double enq, bool front = false) {
  const EngineDesc& S = *c.S;
  int ql = d * 2 + jt;
  int len = c.hs->q_len[ql];
  if (len >= S.qcap) {
    if (c.lane == 0) atomicOr(&S.err[c.r], ERR_QUEUE_OVF);
    return false;
  }
  int pos = front ? (c.hs->q_head[ql] - 1 + S.qcap) % S.qcap
                  : (c.hs->q_head[ql] + len) % S.qcap;
  if (c.lane == 0) {
    int64_t at = ((int64_t)(c.r * S.n_dc + d) * 2 + jt) * S.qcap + pos;
    S.q_pay[at * 2] = size;
    S.q_pay[at * 2 + 1] = enq;
    if (c.r == S.log_replica) {
      int64_t aux = ((int64_t)ql) * S.qcap + pos;
      S.q_netlat[aux] = netlat;
      S.q_jid[aux] = jid;
      S.q_ing[aux] = (char)ing;
    }
    if (front) c.hs->q_head[ql] = pos;
    c.hs->q_len[ql] = len + 1;
  }
  store_fence();
  return true;
}

__device__ bool queue_pop(Ctx& c, int d, int jt, double& size, float& netlat,
                          int& jid, int& ing, double& enq) {
  const EngineDesc& S = *c.S;
  int ql = d * 2 + jt;
  int len = c.hs->q_len[ql];
  if (len <= 0) return false;
  int pos = c.hs->q_head[ql];
  int64_t at = ((int64_t)(c.r * S.n_dc + d) * 2 + jt) * S.qcap + pos;
  size = S.q_pay[at * 2];
  enq = S.q_pay[at * 2 + 1];
  if (c.r == S.log_replica) {
    int64_t aux = ((int64_t)ql) * S.qcap + pos;
    netlat = S.q_netlat[aux];
    jid = S.q_jid[aux];
    ing = S.q_ing[aux];
  } else {
    netlat = 0.0f; jid = 0; ing = 0;
  }
  if (c.lane == 0) {
    c.hs->q_head[ql] = (pos + 1) % S.qcap;
    c.hs->q_len[ql] = len - 1;
  }
  store_fence();
  return true;
}

// pop the job a drain of DC d serves next: the inference queue first when
// inf_priority, else (or when that is empty) the training queue (the chsac
// one-job drain; drain_queues keeps the same three lines inline)
__device__ bool queue_pop_next(Ctx& c, int d, int& jt, double& size,
                               float& netlat, int& jid, int& ing,
                               double& enq) {
  if (c.S->inf_priority && queue_pop(c, d, 0, size, netlat, jid, ing, enq))
    jt = 0;
  else if (queue_pop(c, d, 1, size, netlat, jid, ing, enq)) jt = 1;
  else return false;
  return true;
}

// drain queues after a completion (inference first; reference :839-927);
// returns true if any started job tied the DC's cached min finish (see
// start_job) so the caller must rescan
template <int ALGO>
__device__ bool drain_queues(Ctx& c, int d, double now) {
  const EngineDesc& S = *c.S;
  bool tie = false;
  while (c.free_gpus(d) > 0) {
    double size, enq;
    float netlat;
    int jid, ing;
    int jt;
    // queue_pop_next, written out: every call form of it measured here
    // changed this hot loop's code generation (profiles/README.md)
    if (S.inf_priority && queue_pop(c, d, 0, size, netlat, jid, ing, enq)) jt = 0;
    else if (queue_pop(c, d, 1, size, netlat, jid, ing, enq)) jt = 1;
    else break;
    int n; double f;
    if (ALGO == A_CARBON_COST) {
      // the reference's drain path always uses the CARBON objective for
      // carbon_cost (simulator_paper_multi.py:909-920), unlike its admission
      // path which prefers cost when a price is set (:622-645)
      GridPick g = S.fp32_score
          ? wave_grid_argmin<float>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                                 S.n_freq, S.max_gpj, 1, S.carbon[d], 0.0,
                                 false, 0.0)
          : wave_grid_argmin<double>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                             S.n_freq, S.max_gpj, 1, S.carbon[d], 0.0,
                             false, 0.0);
      n = g.n; f = g.f;
    } else if (ALGO == A_JOINT_NF || ALGO == A_BANDIT) {
      // explicit drain branches in the reference (:892-907); everything else
      // drains through the heuristic allocator (:922-927) — including debug
      decide_nf<ALGO>(c, d, jt, size, now, n, f);
    } else {
      n = heuristic_alloc(c, d, jt);
      f = c.hs->cur_freq[d];
    }
    n = max(1, min(n, c.free_gpus(d)));
    tie |= start_job(c, d, jt, size, netlat, jid, ing, n, f, now);
    if (c.lane == 0) c.hs->sum_wait += fmax(0.0, now - enq);
  }
  return tie;
}

// inter-arrival time of the jtype-jt process after an arrival at time t:
// Poisson, or faithful non-accumulating sinusoid thinning (reference
// arrivals.py:35-48); D_INF when the process is off
__device__ double draw_interarrival(Ctx& c, int jt, double t) {
  const EngineDesc& S = *c.S;
  double rate = S.arr_rate[jt];
  int mode = S.arr_mode[jt];
  double amp = S.arr_amp[jt];
  double period = S.arr_period[jt];
  double ia = D_INF;
  if (mode == 0 && rate > 0) {
    ia = rexp(c.rng, rate);
  } else if (mode == 1) {
    double max_rate = rate * (1.0 + fabs(amp));
    if (max_rate > 0) {
      for (int it = 0; it < 4096; ++it) {
        double w = rexp(c.rng, max_rate);
        double lam = thinning_rate(rate, amp, period, t, w);
        if (u01(c.rng) <= lam / max_rate) { ia = w; break; }
      }
    }
  }
  return ia;
}

// push the WAN transfer of an arrival routed to DC d_sel into the first empty
// transfer slot; `tr` (chsac) rides along as the RL part of the record
// (reference :570-588), n_rew being the RL-chosen n
__device__ void push_transfer(Ctx& c, double now, int jt, int ing, double size,
                              int jid, int d_sel,
                              const JobTrace* tr = nullptr) {
  const EngineDesc& S = *c.S;
  double lnet = launch_const(S.wan_lat)[ing * S.n_dc + d_sel];
  double bw = launch_const(S.wan_bw)[ing * S.n_dc + d_sel];
  double xfer = bw > 0.0 ? S.payload_gb[jt] / bw : 0.0;
  int cand = sub_first_empty(c.l_xt, 0, S.tcap);
  if (tr && cand != INT_MAX)  // the s0 trace (lane-parallel over obs_dim)
    for (int k = c.lane; k < S.obs_dim; k += SUBW)
      S.x_s0[((int64_t)c.r * S.tcap + cand) * S.obs_dim + k] = tr->s0[k];
  if (cand == INT_MAX) {
    if (c.lane == 0) atomicOr(&S.err[c.r], ERR_XFER_OVF);
  } else if (c.lane == 0) {
    int64_t at = (int64_t)c.r * S.tcap + cand;
    c.l_xt[cand] = now + lnet + xfer;
    XRec* xr = &S.x_rec[at];
    xr->size = size;
    xr->netlat = (float)lnet;
    xr->jid = jid;
    xr->dc = (unsigned char)d_sel;
    xr->jtype = (unsigned char)jt;
    xr->ing = (unsigned char)ing;
    if (tr) {
      xr->nsel = (short)tr->n_rew;
      xr->adc = (unsigned char)tr->adc;
      xr->ag = (unsigned char)tr->ag;
      xr->mdc = (unsigned char)tr->mdc;
      xr->mg = (unsigned char)tr->mg;
    }
    xr->has_rl = tr != nullptr;
  }
  store_fence();
}

// accrue energy + util across DCs to time t (lanes 0..n_dc-1)
__device__ void accrue_to(Ctx& c, double t) {
  const EngineDesc& S = *c.S;
  if (c.lane < S.n_dc) {
    double last = c.now;
    if (last < 0.0) {
      c.hs->util_begin[c.lane] = t;
    } else {
      double dt = fmax(0.0, t - last);
      c.hs->util_time[c.lane] += c.hs->busy[c.lane] * dt;
      c.hs->energy[c.lane] += c.my_dc_power() * dt;
    }
  }
  lds_fence();
}

// emit one cluster-log row set (logging replica only; wave-cooperative counts)
__device__ void emit_cluster_rows(Ctx& c, double now) {
  const EngineDesc& S = *c.S;
  if (c.r != S.log_replica) return;
  int64_t base = (int64_t)c.r * S.total_slots;
  for (int d = 0; d < S.n_dc; ++d) {
    int lo = S.slot_off[d], hi = S.slot_off[d + 1];
    int cnt_inf = 0;
    for (int k = lo + c.lane; k < hi; k += SUBW)
      if (S.s_gpus[base + k] != 0 && S.s_jtype[base + k] == 0) cnt_inf++;
    cnt_inf = wave_sum_i32(cnt_inf);
    int run_total = c.hs->n_running[d];
    if (c.lane == 0) {
      int idx = *S.cl_count;
      if (idx < S.cl_cap) {
        double* row = &S.cl_rows[(int64_t)idx * 15];
        double begin = c.hs->util_begin[d];
        double elapsed = fmax(1e-9, now - (begin >= 0 ? begin : now));
        row[0] = now;
        row[1] = d;
        row[2] = c.hs->cur_freq[d];
        row[3] = c.hs->busy[d];
        row[4] = S.total_gpus[d] - c.hs->busy[d];
        row[5] = run_total;
        row[6] = cnt_inf;
        row[7] = run_total - cnt_inf;
        row[8] = c.hs->q_len[d * 2 + 0];
        row[9] = c.hs->q_len[d * 2 + 1];
        row[10] = S.total_gpus[d] ? (double)c.hs->busy[d] / S.total_gpus[d] : 0.0;
        row[11] = S.total_gpus[d]
            ? c.hs->util_time[d] / (S.total_gpus[d] * elapsed) : 0.0;
        row[12] = c.hs->acc_unit[d];
        row[13] = c.dc_power(d);
        row[14] = c.hs->energy[d];
        *S.cl_count = idx + 1;
      } else {
        atomicOr(&S.err[c.r], ERR_LOG_OVF);
      }
    }
    store_fence();
  }
}

// population time series: EVERY replica snapshots its per-DC state at the log
// tick (same place and same expressions as emit_cluster_rows, so a sample
// equals the matching cl_rows column bit for bit), plus one fleet row summed
// in DC order 0..n_dc-1 — per-DC variances do not combine into a fleet
// variance, so the total is sampled per replica.  The replica's own tick
// counter indexes the buffer (replicas drift apart within a launch).  Cold
// scattered 8-byte stores, replica-minor for the reduction's coalescing.
__device__ __forceinline__ void pop_series_sample(Ctx& c,
                                                  const PopSeriesDesc& P,
                                                  double now) {
  const EngineDesc& S = *c.S;
  int cnt = P.tick[c.r] + 1;
  if (c.lane == 0) P.tick[c.r] = cnt;
  if (cnt % P.every == 0) {
    int ti = cnt / P.every - 1;
    if (ti < P.t_cap) {
      const int64_t R = S.n_rep;
      double* cell = P.samples + (int64_t)ti * (S.n_dc + 1) * PS_K * R + c.r;
      double acc[PS_K];
#pragma unroll
      for (int k = 0; k < PS_K; ++k) acc[k] = 0.0;
      for (int d = 0; d < S.n_dc; ++d) {
        const double v[PS_K] = {
            c.hs->cur_freq[d],         (double)c.hs->busy[d],
            (double)c.hs->n_running[d], (double)c.hs->q_len[d * 2 + 0],
            (double)c.hs->q_len[d * 2 + 1], c.dc_power(d),
            c.hs->energy[d]};
#pragma unroll
        for (int k = 0; k < PS_K; ++k) {
          acc[k] += v[k];
          if (c.lane == 0) cell[(int64_t)(d * PS_K + k) * R] = v[k];
        }
      }
      acc[0] /= (double)S.n_dc;  // fleet frequency: mean over DCs
      if (c.lane == 0) {
#pragma unroll
        for (int k = 0; k < PS_K; ++k)
          cell[(int64_t)(S.n_dc * PS_K + k) * R] = acc[k];
        if (c.r == 0) P.time[ti] = now;
      }
    } else if (c.lane == 0) {
      atomicOr(&S.err[c.r], ERR_LOG_OVF);
    }
  }
  store_fence();
}

__device__ void emit_job_row(Ctx& c, int d, int jt, int jid, int ing,
                             double size, double fused, int n, float netlat,
                             double start, double finish, int pcount) {
  const EngineDesc& S = *c.S;
  if (c.r != S.log_replica) return;
  if (c.lane == 0) {
    int idx = *S.jl_count;
    if (idx < S.jl_cap) {
      double* row = &S.jl_rows[(int64_t)idx * 11];
      row[0] = jid; row[1] = ing; row[2] = jt; row[3] = size; row[4] = d;
      row[5] = fused; row[6] = n; row[7] = netlat; row[8] = start;
      row[9] = finish; row[10] = pcount;
      *S.jl_count = idx + 1;
    } else {
      atomicOr(&S.err[c.r], ERR_LOG_OVF);
    }
  }
  store_fence();
}

// cap_greedy controller step at log ticks — reference-exact sorted-snapshot
// semantics (freq_load_agg.py:44-80 + simulator_paper_multi.py:229-315):
//   outer pass: snapshot every running job's f; build the full DOWN-ladder
//   atom list from that snapshot (atom (slot, k) = step lv[k] -> lv[k-1] for
//   k <= i0, rho frozen at snapshot ladder values);
//   inner loop: apply atoms in ascending (rho, task-order, step-order) —
//   emulated as a selection walk so no materialized sort is needed; an atom
//   whose target f is not strictly below the job's LIVE f is skipped (a
//   cheaper deeper atom may already have jumped the job lower); each applied
//   atom reschedules the job with the reference's exact progress arithmetic
//   and re-estimates total power before the next deficit check.
// Task order = DC-major, then running_jobs insertion order (s_seq); step
// order = i0-k ascending — exactly the reference's stable rho sort.
__device__ __attribute__((noinline)) void cap_greedy_control(Ctx& c,
                                                             double now) {
  // noinline ON PURPOSE: this runs once per log tick (cold), but inlined
  // it inflates live ranges across the whole advance loop — the
  // cap_greedy kernel instantiation measured 233 M ev/s vs 426 M for the
  // identical trajectory under cap_uniform (round2_algo_sweep.jsonl).
  const EngineDesc& S = *c.S;
  // sorted ladder (atoms_for_task sorts freq_levels)
  double lv[MAX_FREQ];
  for (int i = 0; i < S.n_freq; ++i) lv[i] = S.freq_levels[i];
  for (int i = 1; i < S.n_freq; ++i) {
    double x = lv[i];
    int j = i - 1;
    while (j >= 0 && lv[j] > x) { lv[j + 1] = lv[j]; --j; }
    lv[j + 1] = x;
  }
  double f_min = lv[0];
  double totalP = 0;
  for (int d = 0; d < S.n_dc; ++d) totalP += c.dc_power(d);
  if (totalP <= S.power_cap - 5.0) return;  // hysteresis (reference :235-237)
  double deficit = fmax(0.0, totalP - S.power_cap);
  if (deficit <= 1e-6) return;
  int64_t base = (int64_t)c.r * S.total_slots;
  int guard = 10000;
  while (deficit > 1e-6 && guard-- > 0) {
    // ---- snapshot: freeze each cappable task's f for this pass ----
    int have = 0;
    for (int k = c.lane; k < S.total_slots; k += SUBW) {
      double sf = 0.0;
      if (c.l_fin[k] < D_INF) {
        double fu = S.s_rec[base + k].fused;
        if (fu > f_min + 1e-12) { sf = fu; have = 1; }
      }
      S.snap_f[base + k] = sf;
    }
    store_fence();
    if (wave_sum_i32(have) == 0) break;  // no tasks
    bool applied_any = false;
    bool exhausted = false;
    // frozen-order selection walk: strictly-after (last_rho, last_key)
    double last_rho = -D_INF;
    long long last_key = -1;
    while (deficit > 1e-6) {
      double best_rho = D_INF;
      long long best_key = LLONG_MAX;
      int best_slot = -1, best_k = -1;
      for (int k = c.lane; k < S.total_slots; k += SUBW) {
        double sf = S.snap_f[base + k];
        if (sf <= 0.0) continue;
        int i0 = 0;
        double bd = 1e300;
        for (int q = 0; q < S.n_freq; ++q) {
          double df = fabs(lv[q] - sf);
          if (df < bd) { bd = df; i0 = q; }
        }
        if (i0 == 0) continue;
        int d = S.slot_dc[k];
        int jt = S.s_jtype[base + k];
        int n = S.s_gpus[base + k];
        long long seq = S.s_rec[base + k].seq;
        double curV = 1.0 / d_unit_time(n, lv[i0], c.lc3(d, jt));
        double curP = d_job_power(n, lv[i0], c.pc3(d, jt));
        for (int kk = i0; kk >= 1; --kk) {
          double V2 = 1.0 / d_unit_time(n, lv[kk - 1], c.lc3(d, jt));
          double P2 = d_job_power(n, lv[kk - 1], c.pc3(d, jt));
          double dV = fmax(0.0, curV - V2), dP = fmax(0.0, curP - P2);
          if (dV > 0 && dP >= 0) {
            double rho = dP / dV;
            long long key = ((long long)d << 40) | (seq << 8) | (i0 - kk);
            bool after = rho > last_rho || (rho == last_rho && key > last_key);
            if (after && (rho < best_rho ||
                          (rho == best_rho && key < best_key))) {
              best_rho = rho; best_key = key; best_slot = k; best_k = kk;
            }
          }
          curV = V2;
          curP = P2;
        }
      }
      // subgroup reduction on (rho, key)
#pragma unroll
      for (int off = SUBW / 2; off > 0; off >>= 1) {
        double orho = __shfl_xor(best_rho, off, 64);
        long long okey = __shfl_xor(best_key, off, 64);
        int oslot = __shfl_xor(best_slot, off, 64);
        int ok = __shfl_xor(best_k, off, 64);
        if (orho < best_rho || (orho == best_rho && okey < best_key)) {
          best_rho = orho; best_key = okey; best_slot = oslot; best_k = ok;
        }
      }
      if (best_rho >= D_INF) { exhausted = true; break; }  // atom list done
      last_rho = best_rho;
      last_key = best_key;
      // skip unless the atom still goes strictly DOWN from the live f
      SRec* bs = &S.s_rec[base + best_slot];
      double cur_f = bs->fused;
      double f_to = lv[best_k - 1];
      if (f_to >= cur_f - 1e-12) continue;
      // ---- apply: the reference's exact reschedule arithmetic ----
      int d = S.slot_dc[best_slot];
      int jt = S.s_jtype[base + best_slot];
      int n = S.s_gpus[base + best_slot];
      double T_old = d_unit_time(n, cur_f, c.lc3(d, jt));
      double rate_old = 1.0 / fmax(T_old, 1e-9);
      double size = bs->size;
      double dt = fmax(0.0, now - bs->lastupd);
      double done = fmin(size, bs->done + rate_old * dt);
      double units_left = fmax(0.0, size - done);
      double T_new = d_unit_time(n, f_to, c.lc3(d, jt));
      double rate_new = 1.0 / fmax(T_new, 1e-9);
      double finish_new = now + units_left / fmax(rate_new, 1e-9);
      if (c.lane == 0) {
        bs->done = done;
        bs->lastupd = now;
        bs->fused = f_to;
        c.l_fin[best_slot] = finish_new;
        c.hs->p_active[d] += d_job_power(n, f_to, c.pc3(d, jt)) -
                             d_job_power(n, cur_f, c.pc3(d, jt));
        c.hs->sum_tpt[d] += rate_new - rate_old;
      }
      store_fence();
      rescan_dc_min(c, d);
      applied_any = true;
      // exact total-power re-estimate after each applied atom (:300-307)
      totalP = 0;
      for (int dd = 0; dd < S.n_dc; ++dd) totalP += c.dc_power(dd);
      deficit = fmax(0.0, totalP - S.power_cap);
    }
    if (!applied_any) break;
    if (exhausted && deficit > 1e-6) continue;  // rebuild snapshot, next pass
  }
}

// ---------------- CHSAC-AF (RL) device helpers ----------------
// obs vector [now] + per-DC [total, busy, free, current_f, q_inf, q_train]
// (reference _upgr_obs, simulator_paper_multi.py:1041-1053); lanes 0..n_dc-1
// write their DC's 6 features in parallel.
__device__ void rl_build_obs(Ctx& c, double now, float* out) {
  const EngineDesc& S = *c.S;
  if (c.lane == 0) out[0] = (float)now;
  if (c.lane < S.n_dc) {
    float total = (float)S.total_gpus[c.lane];
    float busy = (float)c.hs->busy[c.lane];
    out[1 + 6 * c.lane + 0] = total;
    out[1 + 6 * c.lane + 1] = busy;
    out[1 + 6 * c.lane + 2] = fmaxf(0.0f, total - busy);
    out[1 + 6 * c.lane + 3] = c.hs->cur_freq[c.lane];
    out[1 + 6 * c.lane + 4] = (float)c.hs->q_len[c.lane * 2 + 0];
    out[1 + 6 * c.lane + 5] = (float)c.hs->q_len[c.lane * 2 + 1];
  }
  store_fence();
}

// approximate p99 (ms) from the per-replica log-binned latency histogram.
// The reference computes an exact percentile over a 2048-sample sliding
// window (:728-737); the histogram form is the batched approximation
// (documented divergence; exact at the oracle).
__device__ double rl_p99_ms(Ctx& c, int jt) {
  const EngineDesc& S = *c.S;
  long long total = S.lat_count[c.r * 2 + jt];
  if (S.exact_p99) {
    // np.percentile(buf, 99) over the sorted window: linear interpolation
    // at virtual index 0.99*(n-1)
    long long n = total < S.p99_win ? total : S.p99_win;
    if (n < 5) return -1.0;
    const double* a = &S.p99_sorted[(int64_t)(c.r * 2 + jt) * S.p99_win];
    double vi = 0.99 * (double)(n - 1);
    long long lo = (long long)vi;
    double frac = vi - (double)lo;
    double v = a[lo];
    if (lo + 1 < n) v = v + (a[lo + 1] - v) * frac;
    return v * 1000.0;
  }
  if (total < 5) return -1.0;
  long long target = (long long)(0.99 * (double)total);
  long long cum = 0;
  const int* h = &S.lat_hist[(c.r * 2 + jt) * LAT_BINS];
  for (int b = 0; b < LAT_BINS; ++b) {
    cum += h[b];
    if (cum > target) {
      // upper edge of bin b: 10^(-4 + 8*(b+1)/LAT_BINS) seconds
      double s = pow(10.0, -4.0 + 8.0 * (b + 1) / LAT_BINS);
      return s * 1000.0;
    }
  }
  return 1e7;
}

__device__ void rl_record_latency(Ctx& c, int jt, double sojourn_s) {
  const EngineDesc& S = *c.S;
  if (c.lane != 0) return;
  double l = log10(fmax(sojourn_s, 1e-9));
  int b = (int)((l + 4.0) / 8.0 * LAT_BINS);
  b = max(0, min(LAT_BINS - 1, b));
  S.lat_hist[(c.r * 2 + jt) * LAT_BINS + b] += 1;
  long long cnt = S.lat_count[c.r * 2 + jt];
  S.lat_count[c.r * 2 + jt] = cnt + 1;
  S.lat_sum[c.r * 2 + jt] += sojourn_s;
  if (S.exact_p99) {
    // maintain the sorted window (serial on lane 0 — parity-mode only)
    const int W = S.p99_win;
    double* srt = &S.p99_sorted[(int64_t)(c.r * 2 + jt) * W];
    double* ring = &S.p99_ring[(int64_t)(c.r * 2 + jt) * W];
    long long n = cnt < W ? cnt : W;
    if (cnt >= W) {
      // evict the oldest: find its slot in the sorted array, close the gap
      double old = ring[cnt % W];
      int p = 0;
      while (p < n && srt[p] < old) ++p;   // first slot holding `old`
      for (int q = p; q + 1 < n; ++q) srt[q] = srt[q + 1];
      n -= 1;
    }
    int p = 0;
    while (p < n && srt[p] < sojourn_s) ++p;
    for (int q = (int)n; q > p; --q) srt[q] = srt[q - 1];
    srt[p] = sojourn_s;
    ring[cnt % W] = sojourn_s;
  }
}

// masks (reference _upgr_masks :1055-1082): DC valid if it has free GPUs;
// g in 1..N valid if <= max free anywhere; g capped to 1 when recent p99 is
// comfortably under the SLA (training window preferred).
__device__ void rl_build_masks(Ctx& c, int& mdc, int& mg) {
  const EngineDesc& S = *c.S;
  int m1 = 0, max_free = 0;
  for (int d = 0; d < S.n_dc; ++d) {
    int free = c.free_gpus(d);
    if (free > 0) m1 |= (1 << d);
    max_free = max(max_free, free);
  }
  int m2 = 0;
  for (int g = 1; g <= S.max_gpj; ++g)
    if (g <= max_free) m2 |= (1 << (g - 1));
  int jt_buf = S.lat_count[c.r * 2 + 1] > 0 ? 1 : 0;
  double p99 = rl_p99_ms(c, jt_buf);
  if (p99 >= 0.0 && p99 < 0.9 * S.sla_p99_ms) {
    m2 = 0;
    if (1 <= max_free) m2 = 1;  // cap at a single GPU
  }
  mdc = m1;
  mg = m2;
}

// write an action request and stash the paused-event context
__device__ void rl_request(Ctx& c, int kind, double now, int jt, int ing,
                           double size, float netlat, int jid, int src_dc,
                           int from_inf, double enq) {
  const EngineDesc& S = *c.S;
  rl_build_obs(c, now, &S.req_obs[(int64_t)c.r * S.obs_dim]);
  int mdc, mg;
  rl_build_masks(c, mdc, mg);
  if (c.lane == 0) {
    S.req_mdc[c.r] = mdc;
    S.req_mg[c.r] = mg;
    S.pend_kind[c.r] = kind;
    S.pend_size[c.r] = size;
    S.pend_netlat[c.r] = netlat;
    S.pend_jid[c.r] = jid;
    S.pend_ing[c.r] = ing;
    S.pend_jt[c.r] = jt;
    S.pend_dc[c.r] = src_dc;
    S.pend_from_inf[c.r] = from_inf;
    S.pend_enq[c.r] = enq;
    S.req_flag[c.r] = REQ_PENDING;
  }
  store_fence();
}

// min n meeting the SLA at fixed f (reference _min_n_for_sla :1091-1096)
__device__ int rl_min_n_for_sla(Ctx& c, int d, int jt, double size, double f) {
  const EngineDesc& S = *c.S;
  for (int n = 1; n <= S.max_gpj; ++n)
    if (size * d_unit_time(n, f, c.lc3(d, jt)) * 1000.0 <= S.sla_p99_ms)
      return n;
  return S.max_gpj;
}

// energy-optimal f at n over the sorted ladder (deadline guard is vacuous:
// reference jobs never carry deadlines — Job.deadline is always None)
__device__ double rl_energy_freq(Ctx& c, int d, int jt, int n) {
  const EngineDesc& S = *c.S;
  return wave_energy_freq<double>(c.pc3(d, jt), c.lc3(d, jt), c.freq_levels(),
                                  S.n_freq, n);
}

// ---------------- device-side actor forward + sampling ----------------
// One wave evaluates the full CHSAC actor for ONE observation:
// enc (obs->hid->hid->hid, ReLU) then the two categorical heads
// (hid->hid->n_dc / n_g).  Weights are [in][out]-major, so at every input
// index the SUBW lanes read consecutive floats (fully coalesced, L2-resident
// at ~1.1 MB total); activations live in LDS.  ~280k FMA per call.

__device__ void rl_dense(const float* x, int in, const float* Wt,
                         const float* b, int out, float* y, int lane,
                         bool relu) {
  for (int j = lane; j < out; j += SUBW) {
    float acc = 0.0f;
    for (int i = 0; i < in; ++i) acc = fmaf(x[i], Wt[i * out + j], acc);
    acc += b[j];
    y[j] = relu ? fmaxf(acc, 0.0f) : acc;
  }
  lds_fence();
}

// logits for both heads; obs in LDS, dc logits at L[0..n_dc), g at L[8..)
__device__ void rl_logits_impl(const float* pw, int D, int H, int n_dc,
                               int n_g, const float* obs, float* A, float* B,
                               float* L, int lane) {
  const float *w1 = pw, *b1 = w1 + D * H;
  const float *w2 = b1 + H, *b2 = w2 + H * H;
  const float *w3 = b2 + H, *b3 = w3 + H * H;
  const float *hdc1 = b3 + H, *hdc1b = hdc1 + H * H;
  const float *hdc2 = hdc1b + H, *hdc2b = hdc2 + H * n_dc;
  const float *hg1 = hdc2b + n_dc, *hg1b = hg1 + H * H;
  const float *hg2 = hg1b + H, *hg2b = hg2 + H * n_g;
  rl_dense(obs, D, w1, b1, H, A, lane, true);
  rl_dense(A, H, w2, b2, H, B, lane, true);
  rl_dense(B, H, w3, b3, H, A, lane, true);        // h3 stays in A
  rl_dense(A, H, hdc1, hdc1b, H, B, lane, true);
  rl_dense(B, H, hdc2, hdc2b, n_dc, L, lane, false);
  rl_dense(A, H, hg1, hg1b, H, B, lane, true);
  rl_dense(B, H, hg2, hg2b, n_g, L + 8, lane, false);
}

__device__ void rl_actor_logits(Ctx& c) {
  const EngineDesc& S = *c.S;
  rl_logits_impl(S.pw, S.obs_dim, S.hid, S.n_dc, S.n_g, c.l_obs,
                 c.l_act_a, c.l_act_b, c.l_logits, c.lane);
}

// direct (key, ctr) uniform — distinct per-category Gumbel draws without
// advancing the per-replica stream n times serially
__device__ __forceinline__ double u01_at(uint64_t key, uint64_t ctr) {
  uint32_t w[4];
  philox4x32(key, ctr, w);
  return ((w[0] >> 5) * 67108864.0 + (w[1] >> 6)) *
         (1.0 / 9007199254740992.0);
}

// masked Gumbel-max categorical pick (equivalent in distribution to the host
// path's log_softmax+Gumbel argmax: the log-softmax shift cancels in the
// argmax).  mask==0 falls back to all-valid, mirroring the host guard.
// Wave-uniform: every lane computes the same winner from the same draws.
__device__ int rl_pick(Ctx& c, const float* logits, int mask, int n) {
  const EngineDesc& S = *c.S;
  if (mask == 0) mask = (1 << n) - 1;
  double best = -D_INF;
  int arg = 0;
  if (S.rl_det) {
    for (int j = 0; j < n; ++j) {
      double z = logits[j];
      if ((mask >> j & 1) && z > best) { best = z; arg = j; }
    }
    return arg;
  }
  uint64_t ctr0 = c.rng.ctr;
  c.rng.ctr += n;
  for (int j = 0; j < n; ++j) {
    if (!(mask >> j & 1)) continue;
    double u = fmax(u01_at(c.rng.key, ctr0 + j), 1e-20);
    double z = (double)logits[j] - log(-log(u));
    if (z > best) { best = z; arg = j; }
  }
  return arg;
}

// build obs+masks into LDS, run the actor, sample (a_dc, a_g)
__device__ void rl_serve_inline(Ctx& c, double now, int& a_dc, int& a_g,
                                int& mdc, int& mg) {
  const EngineDesc& S = *c.S;
  rl_build_obs(c, now, c.l_obs);
  rl_build_masks(c, mdc, mg);
  rl_actor_logits(c);
  a_dc = rl_pick(c, c.l_logits, mdc, S.n_dc);
  a_g = rl_pick(c, c.l_logits + 8, mg, S.n_g);
}

// start a job carrying an RL trace (chsac).  Deliberately NOT folded into
// start_job: with the trace as an optional argument of one start_job the
// non-CHSAC kernels stayed identical, but the RL loop measured ~3% slower
// (profiles/README.md), so any change to slot allocation, SRec layout or the
// min-finish cache still has to be made in both.
__device__ void rl_start_job(Ctx& c, int d, int jt, double size, float netlat,
                             int jid, int ing, int n, double f, double now,
                             const float* s0, int a_dc, int a_g,
                             int mdc, int mg, int n_rew,
                             double units_done = 0.0, int pcount = 0,
                             int has_rl = 1, double orig_start = -1.0) {
  const EngineDesc& S = *c.S;
  int64_t base = (int64_t)c.r * S.total_slots;
  int lo = S.slot_off[d], hi = S.slot_off[d + 1];
  int cand = sub_first_empty(c.l_fin, lo, hi);
  if (cand == INT_MAX) {
    if (c.lane == 0) atomicOr(&S.err[c.r], ERR_SLOT_OVF);
    return;
  }
  double T = d_unit_time(n, f, c.lc3(d, jt));
  // fresh starts: finish = now + size*T (reference _start_job_with_nf);
  // resumes (orig_start >= 0): the reference's exact arithmetic
  // units_left / max(1/T, 1e-9) and the ORIGINAL start time preserved
  // (reference _resume_preempted_job :362-387 — start_time not reset)
  double finish;
  if (orig_start >= 0.0) {
    double units_left = fmax(0.0, size - units_done);
    finish = now + units_left / fmax(1.0 / T, 1e-9);
  } else {
    finish = now + size * T;
  }
  // copy s0 trace (lane-parallel over obs_dim)
  for (int k = c.lane; k < S.obs_dim; k += SUBW)
    S.slot_s0[(base + cand) * S.obs_dim + k] = s0[k];
  if (c.lane == 0) {
    c.l_fin[cand] = finish;
    SRec* sr = &S.s_rec[base + cand];
    sr->start = orig_start >= 0.0 ? orig_start : now;
    sr->lastupd = now;
    sr->size = size;
    sr->fused = f;
    sr->netlat = netlat;
    sr->jid = jid;
    sr->done = units_done;
    sr->pcount = (unsigned char)pcount;
    sr->ing = (unsigned char)ing;
    sr->seq = ++c.hs->seq_ctr;
    sr->adc = (unsigned char)a_dc;
    sr->ag = (unsigned char)a_g;
    sr->mdc = (unsigned char)mdc;
    sr->mg = (unsigned char)mg;
    sr->has_rl = (unsigned char)has_rl;
    sr->nrew = (unsigned char)max(1, n_rew);
    S.s_gpus[base + cand] = (short)n;
    S.s_jtype[base + cand] = (char)jt;
    c.hs->busy[d] += n;
    c.hs->n_running[d] += 1;
    c.hs->p_active[d] += d_job_power(n, f, c.pc3(d, jt));
    c.hs->sum_tpt[d] += 1.0 / T;
    if (finish < c.hs->dc_minf[d]) {
      c.hs->dc_minf[d] = finish;
      c.hs->dc_mins[d] = cand;
    }
  }
  store_fence();
}

// emit a CHSAC transition (s0, s1, a, r, costs, masks) into the global ring
__device__ void rl_emit_transition(Ctx& c, const float* s0, int a_dc, int a_g,
                                   float r, float c_lat, float c_pow,
                                   float c_over, int mdc, int mg, double now) {
  const EngineDesc& S = *c.S;
  // s1 = obs at completion time; build into a scratch row first (reuse the
  // replica's request-obs row as scratch — safe: no pending request coexists
  // with a finish emission in the same event)
  float* s1 = &S.req_obs[(int64_t)c.r * S.obs_dim];
  rl_build_obs(c, now, s1);
  int idx = 0;
  if (c.lane == 0) idx = atomicAdd(S.tr_count, 1);
  // broadcast from THIS subgroup's base lane (absolute in-wave index)
  idx = __shfl(idx, (threadIdx.x & 63) & ~(SUBW - 1), 64);
  if (idx >= S.tr_cap) {
    if (c.lane == 0) atomicOr(&S.err[c.r], ERR_LOG_OVF);
    return;
  }
  for (int k = c.lane; k < S.obs_dim; k += SUBW) {
    S.tr_s0[(int64_t)idx * S.obs_dim + k] = s0[k];
    S.tr_s1[(int64_t)idx * S.obs_dim + k] = s1[k];
  }
  if (c.lane == 0) {
    S.tr_adc[idx] = (unsigned char)a_dc;
    S.tr_ag[idx] = (unsigned char)a_g;
    S.tr_r[idx] = r;
    S.tr_costs[idx * 3 + 0] = c_lat;
    S.tr_costs[idx * 3 + 1] = c_pow;
    S.tr_costs[idx * 3 + 2] = c_over;
    S.tr_mdc[idx] = (unsigned char)mdc;
    S.tr_mg[idx] = (unsigned char)mg;
  }
  store_fence();
}

// ---- elastic scaling (chsac): preempt all training jobs of a DC into the
// replica's pool, then reallocate them one by one with fresh RL actions
// (reference _preempt_all_training_jobs :396-409 + _rl_reallocate_training_jobs
// :498-534; a failed resume re-queues instead of stranding — oracle fix) ----
__device__ __attribute__((noinline)) int rl_elastic_preempt_all(
    Ctx& c, int d, double now) {
  const EngineDesc& S = *c.S;
  int64_t base = (int64_t)c.r * S.total_slots;
  int lo = S.slot_off[d], hi = S.slot_off[d + 1];
  int count = 0;
  // preempt in running_jobs INSERTION order (ascending s_seq), matching the
  // reference's dict walk; pool order drives the reallocation sequence
  for (;;) {   // uniform selection loop (rare event)
    int k = -1, best_seq = INT_MAX;
    for (int q = lo; q < hi; ++q) {
      if (S.s_gpus[base + q] == 0 || S.s_jtype[base + q] != 1) continue;
      int sq = S.s_rec[base + q].seq;
      if (sq < best_seq) { best_seq = sq; k = q; }
    }
    if (k < 0) break;
    if (count >= S.pp_cap) {
      if (c.lane == 0) atomicOr(&S.err[c.r], ERR_SLOT_OVF);
      break;
    }
    int n = S.s_gpus[base + k];
    SRec* sk = &S.s_rec[base + k];
    double f = sk->fused;
    double T = d_unit_time(n, f, c.lc3(d, 1));
    double done = sk->done +
                  fmax(0.0, now - sk->lastupd) / fmax(T, 1e-300);
    double size = sk->size;
    done = fmin(size, done);
    int64_t pb = (int64_t)c.r * S.pp_cap + count;
    if (c.lane == 0) {
      S.pp_size[pb] = size;
      S.pp_done[pb] = done;
      S.pp_start[pb] = sk->start;
      S.pp_netlat[pb] = sk->netlat;
      S.pp_jid[pb] = sk->jid;
      S.pp_ing[pb] = sk->ing;
      S.pp_dc[pb] = (unsigned char)d;
      S.pp_pcount[pb] = (unsigned char)(sk->pcount + 1);
      S.pp_adc[pb] = sk->adc;
      S.pp_ag[pb] = sk->ag;
      S.pp_nrew[pb] = sk->nrew;
      S.pp_has_rl[pb] = sk->has_rl;
      // free the slot + caches
      S.s_gpus[base + k] = 0;
      c.l_fin[k] = D_INF;
      c.hs->busy[d] -= n;
      c.hs->n_running[d] -= 1;
      c.hs->p_active[d] -= d_job_power(n, f, c.pc3(d, 1));
      c.hs->sum_tpt[d] -= 1.0 / T;
    }
    store_fence();
    // carry the RL trace (lane-parallel)
    for (int q = c.lane; q < S.obs_dim; q += SUBW)
      S.pp_s0[pb * S.obs_dim + q] = S.slot_s0[(base + k) * S.obs_dim + q];
    store_fence();
    ++count;
  }
  if (c.lane == 0) {
    S.pp_count[c.r] = count;
    S.pp_cursor[c.r] = 0;
  }
  store_fence();
  rescan_dc_min(c, d);
  return count;
}

// request the RL action for the pool entry at the cursor
__device__ void rl_request_realloc(Ctx& c, double now) {
  const EngineDesc& S = *c.S;
  int cur = S.pp_cursor[c.r];
  int64_t pb = (int64_t)c.r * S.pp_cap + cur;
  rl_request(c, PEND_REALLOC, now, 1, S.pp_ing[pb], S.pp_size[pb],
             S.pp_netlat[pb], S.pp_jid[pb], S.pp_dc[pb], 0, now);
}

// ---- action EXECUTION bodies, shared by the host resume path and the
// in-kernel serving path (an RL-routed arrival is push_transfer with the
// trace) ----

// execute a drain action on the popped job: start on the RL's target DC, or
// push back at the FRONT of the source queue when the target has no free
// GPUs (reference :849-890)
__device__ void rl_do_drain_action(Ctx& c, double now, int src_d, int jt,
                                   int ing, double size, float netlat,
                                   int jid, double enq, int a_dc, int a_g,
                                   const float* s0, int mdc, int mg) {
  const EngineDesc& S = *c.S;
  int d_tgt = a_dc;
  if (c.free_gpus(d_tgt) <= 0) {
    queue_push(c, src_d, jt, size, netlat, jid, ing, enq, /*front=*/true);
  } else {
    int n_sel = max(1, min(min(a_g + 1, c.free_gpus(d_tgt)), S.max_gpj));
    double f = rl_energy_freq(c, d_tgt, jt, n_sel);
    rl_start_job(c, d_tgt, jt, size, netlat, jid, ing, n_sel, f, now,
                 s0, a_dc, a_g, mdc, mg, n_sel);
    if (c.lane == 0) c.hs->sum_wait += fmax(0.0, now - enq);
  }
}

// chsac drains AT MOST ONE queued job per finish via a fresh policy action
// (reference :849-890).  Host serving (`serve` false) requests the action and
// returns true (the replica pauses); device serving serves and executes it in
// place, so the replica continues its event loop with no host round-trip.
__device__ bool rl_drain_one(Ctx& c, int d, double now, bool serve) {
  const EngineDesc& S = *c.S;
  double size, enq;
  float netlat;
  int jid, ing, jt;
  if (c.free_gpus(d) <= 0 ||
      !queue_pop_next(c, d, jt, size, netlat, jid, ing, enq))
    return false;
  if (!serve) {
    rl_request(c, PEND_DRAIN, now, jt, ing, size, netlat, jid, d, jt == 0,
               enq);
    return true;
  }
  int a_dc, a_g, mdc, mg;
  rl_serve_inline(c, now, a_dc, a_g, mdc, mg);
  rl_do_drain_action(c, now, d, jt, ing, size, netlat, jid, enq, a_dc, a_g,
                     c.l_obs, mdc, mg);
  return false;
}

// one step of the elastic reallocation chain (reference
// _rl_reallocate_training_jobs :498-534): pool entry `cur` goes back on its
// DC — re-queued on the training queue when that has no free GPUs (oracle's
// fix of reference Appendix A.6 job-stranding), else resumed at the fresh
// action's n (clamped) and its energy-optimal f, keeping the trace it was
// preempted with.  Returns the entry's DC.
__device__ int rl_realloc_entry(Ctx& c, int cur, int a_g, int mdc, int mg,
                                double now) {
  const EngineDesc& S = *c.S;
  int64_t pb = (int64_t)c.r * S.pp_cap + cur;
  int d_src = S.pp_dc[pb];
  if (c.free_gpus(d_src) <= 0) {
    queue_push(c, d_src, 1, S.pp_size[pb], S.pp_netlat[pb],
               S.pp_jid[pb], S.pp_ing[pb], now);
  } else {
    int n_rl = max(1, min(min(a_g + 1, c.free_gpus(d_src)), S.max_gpj));
    double f = rl_energy_freq(c, d_src, 1, n_rl);
    rl_start_job(c, d_src, 1, S.pp_size[pb], S.pp_netlat[pb],
                 S.pp_jid[pb], S.pp_ing[pb], n_rl, f, now,
                 &S.pp_s0[pb * S.obs_dim], S.pp_adc[pb], S.pp_ag[pb],
                 mdc, mg, S.pp_nrew[pb], S.pp_done[pb], S.pp_pcount[pb],
                 S.pp_has_rl[pb], S.pp_start[pb]);
  }
  return d_src;
}

// in-kernel elastic reallocation chain (serve_device): fresh obs + actor
// forward per pool entry, all within this launch
__device__ __attribute__((noinline)) void rl_realloc_inline(Ctx& c,
                                                            double now) {
  const EngineDesc& S = *c.S;
  int cnt = S.pp_count[c.r];
  for (int cur = 0; cur < cnt; ++cur) {
    int a_dc, a_g, mdc, mg;
    rl_serve_inline(c, now, a_dc, a_g, mdc, mg);
    rl_realloc_entry(c, cur, a_g, mdc, mg, now);
  }
  if (c.lane == 0) {
    S.pp_count[c.r] = 0;
    S.pp_cursor[c.r] = 0;
  }
  store_fence();
}

// ---------------- the advance kernel ----------------
// PS: population-series sampling at the log tick, a compile-time flag so the
// <ALGO, false> kernels carry none of it.  Its descriptor P is a trailing
// kernel argument of its own, not a part of EngineDesc: the chsac and
// cap_greedy kernels keep a copy of EngineDesc in scratch for their
// out-of-line helpers, and growing it slowed the RL loop measurably
// (profiles/README.md).
// W: which replicas this launch serves and for how many events each
// (launch_plan.hpp); a trailing argument of its own for the same reason.
// WIN: the window arithmetic, a compile-time flag as well: a single launch of
// all replicas runs the <.., false> kernel, which never looks at W (with the
// arithmetic always in, the single-launch path measured 0.8 % slower than
// before; profiles/README.md).  max_ev is the budget of a single launch and
// W.ev_a of a windowed one.
// The 8-lane build sits at the 256-VGPR edge of 2 waves/SIMD, where its
// per-lane replica index and budget offset would tip single instantiations
// over: hold the register allocator to 2 waves/SIMD there.
#if DCG_SUBWAVE == 8
#define DCG_ADVANCE_BOUNDS __launch_bounds__(THREADS_PER_BLOCK, 2)
#else
#define DCG_ADVANCE_BOUNDS __launch_bounds__(THREADS_PER_BLOCK)
#endif
// PRE: arrivals come from the arrival ring (arrival_ring.hpp) instead of
// being drawn here; the PRE = false kernels are the ones from before the ring
// LAT: every job finish is counted into the replica's latency histogram
// (lat_hist.hpp); its descriptor L is one more trailing argument, and the
// LAT = false kernels never look at it
// SWP: a power_cap sweep (SweepDesc::cap): the log tick's cap control uses
// the replica's own cap as S.power_cap.  Instantiated for cap_greedy
// with PRE only; every kernel takes the trailing SW, the others ignore it
// (an arrival-rate sweep lives in the generator and runs the SWP = false
// kernels)
template <int ALGO, bool PS, bool WIN, bool PRE = false, bool LAT = false,
          bool SWP = false>
__global__ void DCG_ADVANCE_BOUNDS
advance_kernel(EngineDesc S, double t_target, long long max_ev,
               PopSeriesDesc P, LaunchWindow W, ArrRing A, LatHistDesc L,
               SweepDesc SW) {
  // SUBW lanes form one replica slot (64: wave-per-replica; 8: eight
  // replicas per wavefront)
  // (64-lane build: the slot, and with it the replica index and the event
  // budget, is wave-uniform; say so, so that everything indexed by it is
  // scalar address arithmetic)
  int slot_id = sub_uniform_i32((blockIdx.x * blockDim.x + threadIdx.x) / SUBW);
  int lane = threadIdx.x & (SUBW - 1);
  // chsac always gets the whole ensemble in one launch (its launch cadence
  // carries meaning)
  static_assert(!(WIN && ALGO == A_CHSAC), "chsac has no windowed kernel");
  static_assert(!(PRE && (ALGO == A_CHSAC || SUBW != 64)),
                "chsac draws at its arrivals; the 8-lane build has no ring");
  static_assert(!SWP || (PRE && ALGO == A_CAP_GREEDY),
                "only cap_greedy reads a swept cap, and only with the ring");
  if (slot_id >= (WIN ? W.count : S.n_rep)) return;
  // windowed: the event counter runs up to max_ev = W.ev_a for every slot, a
  // scalar bound in both builds; slots past the split start it at the
  // difference of the two budgets (the 8-lane build has no registers for a
  // per-lane bound)
  long long ev_skip = 0;
  if (WIN) {
    slot_id += W.first;
    if (slot_id >= S.n_rep) slot_id -= S.n_rep;
    slot_id = sub_uniform_i32(slot_id);
    ev_skip = sub_uniform_i64(
        (blockIdx.x * blockDim.x + threadIdx.x) / SUBW >= W.split
            ? W.ev_a - W.ev_b : 0ll);
  }

  Ctx c;
  c.S = &S;
  c.r = slot_id;
  c.lane = lane;
  if (S.done[c.r]) return;
  // CHSAC fast-path: a replica still waiting for its policy response must
  // not advance (and must not round-trip the hot state)
  if (ALGO == A_CHSAC && S.pend_kind[c.r] != PEND_NONE &&
      S.req_flag[c.r] != REQ_READY)
    return;
  c.now = S.now[c.r];
  {
    bool own = lane < S.n_dc;
    c.my_total = own ? S.total_gpus[lane] : 0;
    c.my_pidle = own ? (S.power_gating[lane] ? S.p_sleep[lane]
                                             : S.p_idle[lane]) : 0.0;
  }
  c.rng.key = S.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(S.rep_id_offset + c.r));
  c.rng.ctr = S.rng_ctr[c.r];
  // the replica's part of the arrival ring: next slot, records left
  int ring_head = 0, ring_left = 0;
  if (PRE) {
    ring_head = sub_uniform_i32(A.head[c.r]);
    ring_left = sub_uniform_i32(A.count[c.r]);
  }
  // A power_cap sweep: the replica's own cap (c.r is wave-uniform: one
  // scalar load) replaces power_cap in this kernel's by-value copy of the
  // descriptor, the copy c.S points to.  The gate at the log tick and the
  // out-of-line cap_greedy_control read it there as they always did, so that
  // function is the one the SWP = false kernels call, unchanged and noinline.
  if (SWP) S.power_cap = SW.cap[c.r];

  const int NS = S.n_streams;
  int64_t sbase = (int64_t)c.r * S.total_slots;
  long long n_events = ev_skip;
  bool paused = false;
  bool skip_loop = false;  // realloc chain pending: bypass the event loop

  // ---- carve the dynamic-LDS region (lds_sizes) ----
  // SUBW==8 has no mirrors: l_fin/l_xt alias the replica's global rows.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  {
    const LdsSizes z = lds_sizes(S.total_slots, S.tcap, ALGO == A_CHSAC);
    char* base = smem + (threadIdx.x / SUBW) * z.stride();
    c.hs = reinterpret_cast<Hot*>(base);
    if (SUBW == 64) {
      c.l_fin = reinterpret_cast<double*>(base + z.hot);
      c.l_xt = reinterpret_cast<double*>(base + z.hot + z.fin);
    } else {
      c.l_fin = S.s_finish + sbase;
      c.l_xt = S.x_time + (int64_t)c.r * S.tcap;
    }
    if (ALGO == A_CHSAC) {
      float* rb = reinterpret_cast<float*>(base + z.hot + z.fin + z.xt);
      c.l_obs = rb;
      c.l_act_a = rb + RL_MAX_OBS;
      c.l_act_b = c.l_act_a + RL_MAX_HID;
      c.l_logits = c.l_act_b + RL_MAX_HID;
    }
  }
  {
    Hot* h = c.hs;
    int nd = S.n_dc;
    if (SUBW == 64) {
      // slot finish times + transfer times into LDS (lane-strided)
      for (int k = lane; k < S.total_slots; k += SUBW)
        c.l_fin[k] = S.s_finish[sbase + k];
      for (int k = lane; k < S.tcap; k += SUBW)
        c.l_xt[k] = S.x_time[(int64_t)c.r * S.tcap + k];
    }
    for (int k = lane; k < NS; k += SUBW)
      h->arr_next[k] = S.arr_next[(int64_t)c.r * NS + k];
    if (lane < nd) {
      int rd = c.r * nd + lane;
      h->dc_minf[lane] = S.dc_min_finish[rd];
      h->dc_mins[lane] = S.dc_min_slot[rd];
      h->p_active[lane] = S.p_active[rd];
      h->sum_tpt[lane] = S.sum_tpt[rd];
      h->energy[lane] = S.energy_j[rd];
      h->util_time[lane] = S.util_time[rd];
      h->acc_unit[lane] = S.acc_unit[rd];
      h->util_begin[lane] = S.util_begin[rd];
      h->cur_freq[lane] = S.cur_freq[rd];
      h->busy[lane] = S.busy[rd];
      h->n_running[lane] = S.n_running[rd];
    }
    for (int k = lane; k < nd * 2; k += SUBW) {
      h->q_len[k] = S.q_len[c.r * nd * 2 + k];
      h->q_head[k] = S.q_head[c.r * nd * 2 + k];
    }
    if (lane == 0) {
      h->next_log = S.next_log[c.r];
      h->sum_lat = S.sum_lat[c.r];
      h->sum_lat_inf = S.sum_lat_inf[c.r];
      h->sum_wait = S.sum_wait[c.r];
      h->jobs_done = S.jobs_done[c.r];
      h->jobs_done_inf = S.jobs_done_inf[c.r];
      h->jid_ctr = S.jid_ctr[c.r];
      h->seq_ctr = S.seq_ctr[c.r];
    }
  }
  store_fence();  // global loads (vmcnt) AND the LDS writes (lgkmcnt)

  // ---- CHSAC: resume a paused action request ----
  if (ALGO == A_CHSAC && S.pend_kind[c.r] != PEND_NONE) {
    int a_dc = S.resp_dc[c.r];
    int a_g = S.resp_g[c.r];
    const float* s0 = &S.req_obs[(int64_t)c.r * S.obs_dim];
    int mdc = S.req_mdc[c.r], mg = S.req_mg[c.r];
    int pk = S.pend_kind[c.r];
    int jt = S.pend_jt[c.r];
    int ing = S.pend_ing[c.r];
    double size = S.pend_size[c.r];
    float netlat = S.pend_netlat[c.r];
    int jid = S.pend_jid[c.r];
    if (pk == PEND_ARRIVAL) {
      // complete the arrival: RL chose (dc, g); push the WAN transfer
      JobTrace tr{s0, a_dc, a_g, mdc, mg, a_g + 1};
      push_transfer(c, c.now, jt, ing, size, jid, a_dc, &tr);
    } else if (pk == PEND_DRAIN) {
      // one queued job (pend_jt names its queue), RL chose a target DC + g
      rl_do_drain_action(c, c.now, S.pend_dc[c.r], jt, ing, size, netlat, jid,
                         S.pend_enq[c.r], a_dc, a_g, s0, mdc, mg);
    } else {  // PEND_REALLOC: resume the pool entry at the cursor on its DC
      int cur = S.pp_cursor[c.r];
      int d_src = rl_realloc_entry(c, cur, a_g, mdc, mg, c.now);
      int nxt = cur + 1;
      if (nxt < S.pp_count[c.r]) {
        if (lane == 0) S.pp_cursor[c.r] = nxt;
        store_fence();
        // request the NEXT pool entry and skip straight to the hot-state
        // writeback (skip_loop empties the event loop; an early
        // return here would LOSE the LDS-resident bookkeeping updates)
        rl_request_realloc(c, c.now);
        skip_loop = true;
        paused = true;
      } else {
        if (lane == 0) {
          S.pp_count[c.r] = 0;
          S.pp_cursor[c.r] = 0;
        }
        store_fence();
        // reallocation finished -> the deferred one-job queue drain
        // (a paused request exists only under host serving)
        if (rl_drain_one(c, d_src, c.now, false)) {
          skip_loop = true;
          paused = true;
        }
      }
    }
    if (!paused && lane == 0) {
      S.pend_kind[c.r] = PEND_NONE;
      S.req_flag[c.r] = REQ_IDLE;
    }
    store_fence();
  }

  while (!skip_loop && n_events < max_ev) {
    // serve-device staleness bound: yield the launch once the transition
    // ring is full enough for a host train round (checked every 32 events;
    // the read races benignly with other replicas' atomicAdds)
    if (ALGO == A_CHSAC && S.serve_device && S.tr_limit > 0 &&
        (n_events & 31) == 0 && *S.tr_count >= S.tr_limit)
      break;
    // ---- 1. next event: wave argmin over candidate sources ----
    // per-lane candidate: value + kind/idx
    double v = D_INF;
    int kind = -1, idx = -1;
    if (SUBW == 64) {
      // NS <= 16 and n_dc <= 8 fit one pass, and so does the first 64 of the
      // transfer mirror: issue all the LDS reads unconditionally (index
      // clamped; out-of-range lanes are masked in the selects below) so they
      // go out back to back under one wait, then pick in the same source
      // order as the strided scans
      double ta = c.hs->arr_next[max(0, min(lane, NS - 1))];
      double tl = c.hs->next_log;
      int kd = max(0, min(lane, S.n_dc - 1));
      double td = c.hs->dc_minf[kd];
      int sd = c.hs->dc_mins[kd];
      double tx = c.l_xt[max(0, min(lane, S.tcap - 1))];
      if ((lane < NS) & (ta < v)) { v = ta; kind = 0; idx = lane; }
      if ((lane == 0) & (tl < v)) { v = tl; kind = 3; idx = 0; }
      if ((lane < S.n_dc) & (td < v)) { v = td; kind = 2; idx = sd; }
      if ((lane < S.tcap) & (tx < v)) { v = tx; kind = 1; idx = lane; }
      // larger tcap: the rest of the mirror, strided
      for (int k = lane + 64; k < S.tcap; k += 64) {
        double t = c.l_xt[k];
        if (t < v) { v = t; kind = 1; idx = k; }
      }
    } else {
      // arrival streams (strided)
      for (int k = lane; k < NS; k += SUBW) {
        double t = c.hs->arr_next[k];
        if (t < v) { v = t; kind = 0; idx = k; }
      }
      // log tick (one candidate)
      if (lane == 0) {
        double t = c.hs->next_log;
        if (t < v) { v = t; kind = 3; idx = 0; }
      }
      // dc min finishes (strided; n_dc <= 8 <= SUBW so one pass)
      for (int k = lane; k < S.n_dc; k += SUBW) {
        double t = c.hs->dc_minf[k];
        if (t < v) { v = t; kind = 2; idx = c.hs->dc_mins[k]; }
      }
      // transfers (strided over the mirror)
      for (int k = lane; k < S.tcap; k += SUBW) {
        double t = c.l_xt[k];
        if (t < v) { v = t; kind = 1; idx = k; }
      }
    }
    // 64-lane build: t_min, kind and idx come back in SGPRs, so the
    // dispatch below is scalar branches
    int wl;
    double t_min = wave_argmin_f64(v, wl);
    kind = sub_bcast_i32(kind, wl);
    idx = sub_bcast_i32(idx, wl);

    if (t_min > S.end_time) {
      // ---- end of simulation for this replica: final flush ----
      if (lane < S.n_dc) {
        double last = c.now;
        if (last >= 0.0 && last < S.end_time) {
          c.hs->util_time[lane] += c.hs->busy[lane] * (S.end_time - last);
          // reference quirk: the final accrue_energy(end) uses the BASELINE
          // idle/sleep + p_peak*f^alpha model (models.py:82-91)
          double f = c.hs->cur_freq[lane];
          int active = c.hs->busy[lane];
          int idlec = S.total_gpus[lane] - active;
          double pa = active * (S.p_idle[lane] +
                                S.p_peak[lane] * pow(f, S.pow_alpha[lane]));
          double pi = idlec * (S.power_gating[lane] ? S.p_sleep[lane] : S.p_idle[lane]);
          c.hs->energy[lane] += (pa + pi) * (S.end_time - last);
        }
      }
      if (lane == 0) S.done[c.r] = 1;
      store_fence();
      break;
    }
    if (t_min > t_target) break;  // chunk boundary

    // ---- 2. accrue energy + util to t_min ----
    accrue_to(c, t_min);
    c.now = t_min;
    n_events++;

    // ---- 3. dispatch ----
    if (kind == 0) {
      // ===== arrival at ingress stream idx =====
      int ing = idx >> 1;
      int jt = idx & 1;
      int jid = c.hs->jid_ctr + 1;
      if (lane == 0) c.hs->jid_ctr = jid;
      double size;
      int trace_d = -1;
      if (PRE) {
        // this arrival's size, random route, the stream's next time and the
        // counter after its draws, as pregen_arrivals_kernel recorded them
        ARec rec = A.ring[(int64_t)c.r * A.cap + ring_head];
        if (ring_left <= 0 || sub_uniform_i32(rec.stream) != idx) {
          if (lane == 0) atomicOr(&S.err[c.r], ERR_ARR_RING);
        }
        size = rec.size;
        trace_d = sub_uniform_i32(rec.dc);
        c.rng.ctr = (uint64_t)sub_uniform_i64((long long)rec.ctr);
        ring_head = ring_slot(ring_head, 1, A.cap);
        --ring_left;
        if (lane == 0) c.hs->arr_next[idx] = rec.t_next;
        lds_fence();
      } else if (S.trace_mode) {
        // replay mode: this arrival's size, routed DC and the stream's next
        // time come from the recorded trace
        int64_t tb = ((int64_t)c.r * S.n_streams + idx) * S.trace_cap;
        int posn = S.trace_pos[(int64_t)c.r * S.n_streams + idx];
        size = S.trace_size[tb + posn];
        trace_d = S.trace_dc[tb + posn];
        int nxt = posn + 1;
        double t_next = nxt < S.trace_cap ? S.trace_time[tb + nxt] : D_INF;
        if (lane == 0) {
          S.trace_pos[(int64_t)c.r * S.n_streams + idx] = nxt;
          c.hs->arr_next[idx] = t_next;
        }
        lds_fence();
      } else {
        size = jt == 0 ? rpareto_inf(c.rng)
                       : fmax(0.1, rlognormal(c.rng, log(50000.0), 0.4));
      }
      if (ALGO == A_CHSAC) {
        // schedule the next arrival first (RNG order differs from the scalar
        // engines; distributionally identical), then pause for the policy
        double ia_rl = D_INF;
        if (!S.trace_mode) ia_rl = draw_interarrival(c, jt, t_min);
        if (lane == 0 && !S.trace_mode) c.hs->arr_next[idx] = t_min + ia_rl;
        lds_fence();
        if (S.serve_device) {
          // in-kernel policy: forward + sample + execute, no pause
          int a_dc, a_g, mdc, mg;
          rl_serve_inline(c, t_min, a_dc, a_g, mdc, mg);
          JobTrace tr{c.l_obs, a_dc, a_g, mdc, mg, a_g + 1};
          push_transfer(c, t_min, jt, ing, size, jid, a_dc, &tr);
        } else {
          rl_request(c, PEND_ARRIVAL, t_min, jt, ing, size, 0.0f, jid,
                     -1, 0, t_min);
          paused = true;
          break;
        }
      } else {
      // routing
      int d_sel;
      if ((PRE || S.trace_mode) && trace_d >= 0) {
        d_sel = trace_d;
      } else if (ALGO == A_ECO_ROUTE) {
        double price = S.eco_obj == 2 ? c.price_kwh(t_min) : 0.0;
        if (SUBW == 64) {
          // all 64 lanes score: lane = d*8 + (n-1) covers (DC, n); each lane
          // reduces over the frequency ladder, then an 8-lane subgroup min
          // per DC and a wave argmin pick the DC (first-minimum = lowest DC
          // index, matching the scalar scan order).
          double score = D_INF;
          {
            int d = lane >> 3;
            int n = (lane & 7) + 1;
            if (d < S.n_dc && n <= S.max_gpj) {
              kc_f64 pcf = c.pc3(d, jt);
              kc_f64 tcf = c.lc3(d, jt);
              double best = D_INF;
              for (int q = 0; q < S.n_freq; ++q) {
                double f = S.freq_levels[q];
                double T = d_unit_time(n, f, tcf);
                double E = d_job_power(n, f, pcf) * T;
                double sc;
                if (S.eco_obj == 1) sc = E * S.carbon[d];
                else if (S.eco_obj == 2) sc = (E / 3.6e6) * price;
                else sc = E;
                if (sc < best) best = sc;
              }
              score = best * size;  // relative order preserved per objective
            }
          }
#pragma unroll
          for (int off = 1; off < 8; off <<= 1)
            score = fmin(score, __shfl_xor(score, off, 64));
          if (lane & 7) score = D_INF;
          int dl;
          wave_argmin_f64(score, dl);
          d_sel = dl >> 3;
        } else {
          // SUBW==8: lane d scores DC d serially over the grid
          double score = D_INF;
          if (lane < S.n_dc) {
            int d = lane;
            kc_f64 pcf = c.pc3(d, jt);
            kc_f64 tcf = c.lc3(d, jt);
            double best = D_INF;
            for (int n = 1; n <= S.max_gpj; ++n)
              for (int q = 0; q < S.n_freq; ++q) {
                double f = S.freq_levels[q];
                double T = d_unit_time(n, f, tcf);
                double E = d_job_power(n, f, pcf) * T;
                double sc;
                if (S.eco_obj == 1) sc = E * S.carbon[d];
                else if (S.eco_obj == 2) sc = (E / 3.6e6) * price;
                else sc = E;
                if (sc < best) best = sc;
              }
            score = best * size;
          }
          int dl;
          wave_argmin_f64(score, dl);
          d_sel = dl & (SUBW - 1);
        }
      } else {
        d_sel = (int)rbelow(c.rng, (uint32_t)S.n_dc);
      }
      d_sel = sub_uniform_i32(d_sel);
      push_transfer(c, t_min, jt, ing, size, jid, d_sel);
      // next arrival for this stream; in replay mode it was already set
      if (!PRE) {
      double ia = D_INF;
      if (!S.trace_mode) ia = draw_interarrival(c, jt, t_min);
      if (lane == 0 && !S.trace_mode) c.hs->arr_next[idx] = t_min + ia;
      lds_fence();
      }
      }  // end non-chsac arrival path

    } else if (kind == 1) {
      // ===== WAN transfer complete: admission =====
      int64_t at = (int64_t)c.r * S.tcap + idx;
      XRec xr = S.x_rec[at];
      int d = sub_uniform_i32(xr.dc);
      int jt = sub_uniform_i32(xr.jtype);
      double size = xr.size;
      float netlat = xr.netlat;
      int jid = xr.jid;
      int ing = xr.ing;
      if (lane == 0) c.l_xt[idx] = D_INF;
      lds_fence();
      if (c.free_gpus(d) > 0) {
        if (ALGO == A_CHSAC && xr.has_rl) {
          // RL-chosen n (clamped), energy-optimal f (reference :646-667)
          int n = max(1, min(min((int)xr.nsel, c.free_gpus(d)), S.max_gpj));
          double f = rl_energy_freq(c, d, jt, n);
          rl_start_job(c, d, jt, size, netlat, jid, ing, n, f, t_min,
                       &S.x_s0[at * S.obs_dim], xr.adc, xr.ag,
                       xr.mdc, xr.mg, (int)xr.nsel);
        } else {
          int n; double f;
          decide_nf<ALGO>(c, d, jt, size, t_min, n, f);
          n = max(1, min(n, c.free_gpus(d)));
          start_job(c, d, jt, size, netlat, jid, ing, n, f, t_min);
        }
      } else {
        // queueing drops the RL trace: a later chsac drain assigns a fresh
        // observation/action (reference :849-889 overwrites them)
        queue_push(c, d, jt, size, netlat, jid, ing, t_min);
      }

    } else if (kind == 2) {
      // ===== job finish =====
      int slot = idx;
      int d = sub_uniform_i32(c.slot_dc(slot));
      int64_t at = sbase + slot;
      int jt = sub_uniform_i32(S.s_jtype[at]);
      int n = sub_uniform_i32(S.s_gpus[at]);
      SRec srv = S.s_rec[at];
      double size = srv.size;
      double fused = srv.fused;
      double start = srv.start;
      float netlat = srv.netlat;
      int jid = srv.jid;
      int ingr = srv.ing;
      int pcount = srv.pcount;
      double T = d_unit_time(n, fused, c.lc3(d, jt));
      if (lane == 0) {
        c.l_fin[slot] = D_INF;
        S.s_gpus[at] = 0;
        c.hs->busy[d] = max(0, c.hs->busy[d] - n);
        c.hs->n_running[d] -= 1;
        c.hs->p_active[d] -= d_job_power(n, fused, c.pc3(d, jt));
        c.hs->sum_tpt[d] -= 1.0 / T;
        // remainder job-units: window = finish mod log_interval (quirk)
        c.hs->acc_unit[d] += (1.0 / T) * fmod(t_min, S.log_interval);
        // metrics
        c.hs->jobs_done += 1;
        c.hs->sum_lat += t_min - start;
        if (jt == 0) {
          c.hs->jobs_done_inf += 1;
          c.hs->sum_lat_inf += t_min - start;
        }
        // the sojourn of the job row emitted below, counted for every replica
        if (LAT)
          lat_hist_record(L, c.r, S.n_dc, d, jt, fmax(0.0, t_min - start));
        if (ALGO == A_BANDIT) {
          // reward = -E_pred (energy per unit at the used f); match the arm
          // by NEAREST ladder frequency (f_used is stored f32, so exact f64
          // comparison would never hit)
          double E = d_job_power(n, fused, c.pc3(d, jt)) * T;
          int64_t ab = ((int64_t)c.r * S.n_dc + d) * 2 + jt;
          int bk = 0;
          double bd = 1e300;
          for (int k = 0; k < S.n_freq; ++k) {
            double diff = fabs(S.freq_levels[k] - fused);
            if (diff < bd) { bd = diff; bk = k; }
          }
          S.b_n[ab * S.n_freq + bk] += 1;
          S.b_s[ab * S.n_freq + bk] += -E;
        }
      }
      store_fence();
      emit_job_row(c, d, jt, jid, ingr, size, fused, n, netlat, start, t_min,
                   pcount);
      rescan_dc_min(c, d);
      if (ALGO == A_CHSAC) {
        // record latency, then build the transition (reference :718-800)
        double sojourn = fmax(0.0, t_min - start);
        rl_record_latency(c, jt, sojourn);
        store_fence();
        if (srv.has_rl) {
          double E_pred = d_job_power(n, fused, c.pc3(d, jt)) * T;  // J/unit
          double E_unit_kwh = (E_pred * (double)size / 3.6e6) /
                              ((double)size + 1e-9);
          int n_rew = max(1, (int)srv.nrew);
          float r = (float)(-E_unit_kwh + 0.05 * (1.0 / n_rew));
          double p99 = rl_p99_ms(c, jt);
          if (p99 < 0.0) p99 = sojourn * 1000.0;  // <5 samples fallback
          double P_now = c.dc_power(d);
          int n_min = rl_min_n_for_sla(c, d, jt, size, fused);
          float c_over = (float)max(0, n - n_min);
          int mdc, mg;
          rl_build_masks(c, mdc, mg);  // masks at completion (reference :793)
          rl_emit_transition(c, &S.slot_s0[at * S.obs_dim],
                             srv.adc, srv.ag, r,
                             (float)p99, (float)P_now, c_over, mdc, mg, t_min);
          if (lane == 0) S.s_rec[at].has_rl = 0;
          store_fence();
        }
        // elastic scaling: on a training completion with other training jobs
        // still running in this DC, preempt them all and reallocate via
        // fresh RL actions (reference :829-837; gated to chsac + flag)
        if (S.elastic && jt == 1) {
          int n_train = 0;
          for (int k = S.slot_off[d]; k < S.slot_off[d + 1]; ++k)
            if (S.s_gpus[sbase + k] != 0 && S.s_jtype[sbase + k] == 1)
              ++n_train;
          if (n_train > 1) {
            int cnt = rl_elastic_preempt_all(c, d, t_min);
            if (cnt > 0) {
              if (S.serve_device) {
                rl_realloc_inline(c, t_min);  // whole chain, this launch
              } else {
                rl_request_realloc(c, t_min);
                paused = true;
                break;
              }
            }
          }
        }
        if (rl_drain_one(c, d, t_min, S.serve_device)) {
          paused = true;
          break;
        }
      } else {
        // the rescan above left the cache exact and start_job keeps it
        // exact, except when a started job ties the minimum: then only the
        // full scan's lane-order tie-break gives the slot.  The 8-lane
        // build always rescans (it stays the reference for the skip).
        bool tie = drain_queues<ALGO>(c, d, t_min);
        if (tie || SUBW != 64) rescan_dc_min(c, d);
      }

    } else {
      // ===== log tick =====
      // power-cap control first (reference :463-465 order)
      if (S.power_cap > 0) {
        if (ALGO == A_CAP_GREEDY) {
          cap_greedy_control(c, t_min);
        } else if (ALGO == A_ECO_ROUTE || ALGO == A_CARBON_COST) {
          if (lane < S.n_dc) {
            if (c.hs->busy[lane] == 0) {
              double fm = S.freq_levels[0];
              for (int k = 1; k < S.n_freq; ++k) fm = fmin(fm, S.freq_levels[k]);
              c.hs->cur_freq[lane] = fm;
            }
          }
          store_fence();
        }
        // cap_uniform: exact no-op (per-job f_used power model; see oracle)
      }
      // acc_job_unit for running jobs: cached sum_tpt * interval
      if (lane < S.n_dc) {
        c.hs->acc_unit[lane] += c.hs->sum_tpt[lane] * S.log_interval;
      }
      lds_fence();
      emit_cluster_rows(c, t_min);
      if (PS) pop_series_sample(c, P, t_min);
      if (lane == 0) c.hs->next_log = t_min + S.log_interval;
      lds_fence();
    }
  }

  // ---- write the hot state back to HBM ----
  {
    Hot* h = c.hs;
    int nd = S.n_dc;
    if (SUBW == 64) {
      for (int k = lane; k < S.total_slots; k += SUBW)
        S.s_finish[sbase + k] = c.l_fin[k];
      for (int k = lane; k < S.tcap; k += SUBW)
        S.x_time[(int64_t)c.r * S.tcap + k] = c.l_xt[k];
    }
    for (int k = lane; k < NS; k += SUBW)
      S.arr_next[(int64_t)c.r * NS + k] = h->arr_next[k];
    if (lane < nd) {
      int rd = c.r * nd + lane;
      S.dc_min_finish[rd] = h->dc_minf[lane];
      S.dc_min_slot[rd] = h->dc_mins[lane];
      S.p_active[rd] = h->p_active[lane];
      S.sum_tpt[rd] = h->sum_tpt[lane];
      S.energy_j[rd] = h->energy[lane];
      S.util_time[rd] = h->util_time[lane];
      S.acc_unit[rd] = h->acc_unit[lane];
      S.util_begin[rd] = h->util_begin[lane];
      S.cur_freq[rd] = h->cur_freq[lane];
      S.busy[rd] = h->busy[lane];
      S.n_running[rd] = h->n_running[lane];
    }
    for (int k = lane; k < nd * 2; k += SUBW) {
      S.q_len[c.r * nd * 2 + k] = h->q_len[k];
      S.q_head[c.r * nd * 2 + k] = h->q_head[k];
    }
  }
  if (lane == 0) {
    S.next_log[c.r] = c.hs->next_log;
    S.now[c.r] = c.now;
    S.rng_ctr[c.r] = c.rng.ctr;
    if (PRE) {
      A.head[c.r] = ring_head;
      A.count[c.r] = max(ring_left, 0);
      if (n_events >= max_ev) *A.more = 1;
    }
    S.ev_count[c.r] += n_events - ev_skip;
    S.sum_lat[c.r] = c.hs->sum_lat;
    S.sum_lat_inf[c.r] = c.hs->sum_lat_inf;
    S.sum_wait[c.r] = c.hs->sum_wait;
    S.jobs_done[c.r] = c.hs->jobs_done;
    S.jobs_done_inf[c.r] = c.hs->jobs_done_inf;
    S.jid_ctr[c.r] = c.hs->jid_ctr;
    S.seq_ctr[c.r] = c.hs->seq_ctr;
  }
}

// NEGATIVE RESULT (kept out): a grid-stride launcher over an extracted
// advance_one device function, with the chsac grid capped at resident
// capacity to free the workgroup dispatcher for concurrent train kernels.
// The restructure tanked the flagship 400 -> 247 M ev/s (65 k replicas:
// 551 -> 302 M) with OR without always_inline — the loop-wrapped body
// spills the wave-uniform scalars, the same failure mode as round 1's
// noinline experiment.  Train/sim concurrency remains bounded by
// dispatch behavior; the update-rate controller owns that tradeoff.
// What the resident-capacity idea was after for the non-chsac engines, a
// launch that never ends in a thin tail, is done from the host instead:
// launch_plan.hpp cuts a step into several full launches of this unchanged
// kernel (BatchedSimHip::advance), which costs the kernel one trailing
// argument and no loop around its body.

// ---------------- MFMA batched actor forward ----------------
// Matrix-core path for BATCHED policy evaluation (host-side serving /
// offline eval / act-batch): Y = relu(X W^T + b) chained through the whole
// actor on fp32 MFMA tiles (v_mfma_f32_16x16x4_f32 — exact f32, so results
// match the fmaf-chain serving path modulo accumulation order).  One
// workgroup of 16 waves owns 16 batch rows; each wave produces one 16-wide
// column tile per layer; activations ping-pong through padded LDS.
// Fragment maps (cdna4_isa.md §10): A[i=l&15][k=l>>4], B[k=l>>4][j=l&15],
// C/D col=l&15, row=(l>>4)*4+reg.
constexpr int MF_STRIDE = 257;  // 16-row LDS activation stride (bank-spread)
using mf_acc = __attribute__((ext_vector_type(4))) float;

__device__ void mfma_layer(const float* Wt, const float* b, int in, int out,
                           const float* X, float* Y, int wave, int lane,
                           bool relu, int rows) {
  int jt = wave * 16;
  if (jt < out) {
    mf_acc acc = {0.f, 0.f, 0.f, 0.f};
    int i = lane & 15, kw = lane >> 4, j = jt + (lane & 15);
    for (int k0 = 0; k0 < in; k0 += 4) {
      int k = k0 + kw;
      float a = (k < in) ? X[i * MF_STRIDE + k] : 0.0f;
      float w = (k < in && j < out) ? Wt[k * out + j] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int row = (lane >> 4) * 4 + r;
      if (j < out && row < rows) {
        float y = acc[r] + b[j];
        Y[row * MF_STRIDE + j] = relu ? fmaxf(y, 0.0f) : y;
      }
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(1024)
rl_forward_mfma_kernel(const float* pw, const float* obs, int B, int obs_dim,
                       int hid, int n_dc, int n_g, float* out_dc,
                       float* out_g) {
  __shared__ float bufA[16 * MF_STRIDE];
  __shared__ float bufB[16 * MF_STRIDE];
  int wave = threadIdx.x / 64;
  int lane = threadIdx.x & 63;
  int row0 = blockIdx.x * 16;
  int rows = min(16, B - row0);
  if (rows <= 0) return;
  // stage the obs tile (zero-padded)
  for (int idx = threadIdx.x; idx < 16 * MF_STRIDE; idx += blockDim.x)
    bufA[idx] = 0.0f;
  __syncthreads();
  for (int idx = threadIdx.x; idx < rows * obs_dim; idx += blockDim.x) {
    int r = idx / obs_dim, k = idx % obs_dim;
    bufA[r * MF_STRIDE + k] = obs[(int64_t)(row0 + r) * obs_dim + k];
  }
  __syncthreads();
  const int H = hid, D = obs_dim;
  const float *w1 = pw, *b1 = w1 + D * H;
  const float *w2 = b1 + H, *b2 = w2 + H * H;
  const float *w3 = b2 + H, *b3 = w3 + H * H;
  const float *hdc1 = b3 + H, *hdc1b = hdc1 + H * H;
  const float *hdc2 = hdc1b + H, *hdc2b = hdc2 + H * n_dc;
  const float *hg1 = hdc2b + n_dc, *hg1b = hg1 + H * H;
  const float *hg2 = hg1b + H, *hg2b = hg2 + H * n_g;
  mfma_layer(w1, b1, D, H, bufA, bufB, wave, lane, true, rows);
  mfma_layer(w2, b2, H, H, bufB, bufA, wave, lane, true, rows);
  mfma_layer(w3, b3, H, H, bufA, bufB, wave, lane, true, rows);  // h3 in B
  mfma_layer(hdc1, hdc1b, H, H, bufB, bufA, wave, lane, true, rows);
  // dc logits land in the first n_dc columns of a fresh LDS row set; reuse
  // bufA's upper half is unsafe (still holding hdc1 output) — write the
  // small head outputs straight to global from the accumulator instead:
  {
    int jt = wave * 16;
    if (jt < n_dc) {
      mf_acc acc = {0.f, 0.f, 0.f, 0.f};
      int i = lane & 15, kw = lane >> 4, j = jt + (lane & 15);
      for (int k0 = 0; k0 < H; k0 += 4) {
        int k = k0 + kw;
        float a = bufA[i * MF_STRIDE + k];
        float w = (j < n_dc) ? hdc2[k * n_dc + j] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = (lane >> 4) * 4 + r;
        if (j < n_dc && row < rows)
          out_dc[(int64_t)(row0 + row) * n_dc + j] = acc[r] + hdc2b[j];
      }
    }
    __syncthreads();
  }
  mfma_layer(hg1, hg1b, H, H, bufB, bufA, wave, lane, true, rows);
  {
    int jt = wave * 16;
    if (jt < n_g) {
      mf_acc acc = {0.f, 0.f, 0.f, 0.f};
      int i = lane & 15, kw = lane >> 4, j = jt + (lane & 15);
      for (int k0 = 0; k0 < H; k0 += 4) {
        int k = k0 + kw;
        float a = bufA[i * MF_STRIDE + k];
        float w = (j < n_g) ? hg2[k * n_g + j] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = (lane >> 4) * 4 + r;
        if (j < n_g && row < rows)
          out_g[(int64_t)(row0 + row) * n_g + j] = acc[r] + hg2b[j];
      }
    }
  }
}

std::vector<torch::Tensor> rl_forward_mfma(torch::Tensor pw,
                                           torch::Tensor obs,
                                           int64_t hid, int64_t n_dc,
                                           int64_t n_g) {
  TORCH_CHECK(pw.is_cuda() && obs.is_cuda() && pw.dtype() == torch::kFloat32
              && obs.dtype() == torch::kFloat32 && obs.is_contiguous());
  TORCH_CHECK(hid % 16 == 0 && hid <= 256 && n_dc <= 16 && n_g <= 16);
  int B = obs.size(0), D = obs.size(1);
  auto out_dc = torch::empty({B, n_dc}, obs.options());
  auto out_g = torch::empty({B, n_g}, obs.options());
  int blocks = (B + 15) / 16;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(rl_forward_mfma_kernel, dim3(blocks), dim3(1024), 0,
                     stream, pw.data_ptr<float>(), obs.data_ptr<float>(), B,
                     D, (int)hid, (int)n_dc, (int)n_g,
                     out_dc.data_ptr<float>(), out_g.data_ptr<float>());
  check_launch("rl_forward_mfma_kernel");
  return {out_dc, out_g};
}

}  // namespace dcg

// test-only entry points (their kernels and bindings)
#include "debug_entries.hpp"

namespace dcg {

// ---------------- host side ----------------
class BatchedSimHip {
 public:
  BatchedSimHip(py::dict tensors, py::dict cfg) {
    // keep tensor refs alive
    for (auto item : tensors)
      t_[py::cast<std::string>(item.first)] = py::cast<torch::Tensor>(item.second);
    // optional config key with a default
    auto opt = [&cfg](const char* key, auto dflt) {
      return cfg.contains(key) ? cfg[key].cast<decltype(dflt)>() : dflt;
    };

    S_.n_rep = cfg["n_rep"].cast<int>();
    S_.n_dc = cfg["n_dc"].cast<int>();
    S_.n_ing = cfg["n_ing"].cast<int>();
    S_.n_freq = cfg["n_freq"].cast<int>();
    S_.n_streams = S_.n_ing * 2;
    S_.total_slots = cfg["total_slots"].cast<int>();
    S_.tcap = cfg["tcap"].cast<int>();
    S_.qcap = cfg["qcap"].cast<int>();
    S_.end_time = cfg["end_time"].cast<double>();
    S_.log_interval = cfg["log_interval"].cast<double>();
    S_.algo = cfg["algo"].cast<int>();
    S_.max_gpj = cfg["max_gpj"].cast<int>();
    S_.inf_priority = cfg["inf_priority"].cast<int>();
    S_.scale_out_low = cfg["scale_out_low"].cast<int>();
    S_.energy_aware = cfg["energy_aware"].cast<int>();
    S_.dvfs_low = cfg["dvfs_low"].cast<double>();
    S_.dvfs_high = cfg["dvfs_high"].cast<double>();
    S_.power_cap = cfg["power_cap"].cast<double>();
    S_.eco_obj = cfg["eco_obj"].cast<int>();
    S_.fp32_score = opt("fp32_score", 0);
    S_.num_fixed = cfg["num_fixed"].cast<int>();
    S_.fixed_freq = cfg["fixed_freq"].cast<double>();
    S_.payload_gb[0] = cfg["payload_inf_gb"].cast<double>();
    S_.payload_gb[1] = cfg["payload_trn_gb"].cast<double>();
    auto am = cfg["arr_mode"].cast<std::vector<int>>();
    auto ar = cfg["arr_rate"].cast<std::vector<double>>();
    auto aa = cfg["arr_amp"].cast<std::vector<double>>();
    auto ap = cfg["arr_period"].cast<std::vector<double>>();
    for (int j = 0; j < 2; ++j) {
      S_.arr_mode[j] = am[j]; S_.arr_rate[j] = ar[j];
      S_.arr_amp[j] = aa[j]; S_.arr_period[j] = ap[j];
    }
    S_.seed = cfg["seed"].cast<uint64_t>();
    S_.rep_id_offset = cfg["rep_id_offset"].cast<int64_t>();
    S_.log_replica = cfg["log_replica"].cast<int>();
    S_.cl_cap = cfg["cl_cap"].cast<int>();
    S_.jl_cap = cfg["jl_cap"].cast<int>();

    // arrival-trace replay mode
    S_.trace_mode = opt("trace_mode", 0);
    S_.trace_cap = opt("trace_cap", 0);
    // arrival ring (0 = arrivals drawn inside the advance kernel)
    ar_.cap = opt("arr_cap", 0);
    if (ar_.cap != 0) {
      if (!arr_cap_valid(ar_.cap))
        throw std::invalid_argument(
            "engine limits: arr_cap = " + std::to_string(ar_.cap) +
            ", required a power of two");
      if (S_.algo == A_CHSAC || S_.trace_mode)
        throw std::invalid_argument(
            "arr_cap = " + std::to_string(ar_.cap) + ": chsac_af and "
            "trace mode have no pre-generated arrivals, required arr_cap = 0");
    }
    // CHSAC-AF extras
    S_.obs_dim = opt("obs_dim", 0);
    S_.sla_p99_ms = opt("sla_p99_ms", 500.0);
    S_.tr_cap = opt("tr_cap", 0);
    S_.elastic = opt("elastic", 0);
    S_.pp_cap = opt("pp_cap", 0);
    S_.serve_device = opt("serve_device", 0);
    S_.hid = opt("rl_hid", 256);
    S_.n_g = S_.max_gpj;
    S_.rl_det = opt("rl_det", 0);
    S_.tr_limit = opt("tr_limit", 0);
    if (S_.algo == A_CHSAC) {
      S_.exact_p99 = opt("exact_p99", 0);
      S_.p99_win = opt("p99_win", 2048);
    }
    // population time series (off unless the host allocated its buffers)
    ps_.every = opt("pop_series_every", 0);
    // latency histograms (off unless the host allocated them)
    const bool lat_on = t_.count("lh_hist") != 0;
    lh_.sla_s = opt("lat_sla_s", S_.sla_p99_ms / 1000.0);

    check_engine_limits(S_);
    shmem_bytes();  // an oversized scenario fails here, not at the first launch

    // The contract: every pointer this configuration's kernel may dereference,
    // with the extent the kernel indexes it to (in elements of the field).
    const int64_t R = S_.n_rep, D = S_.n_dc, I = S_.n_ing, NS = S_.n_streams,
                  F = S_.n_freq, TS = S_.total_slots, TC = S_.tcap,
                  Q = S_.qcap, O = S_.obs_dim;
    Binder bind(t_);
    // scenario constants
    bind(S_.freq_levels, "freq_levels", F);
    bind(S_.pc, "pc", D * 6);
    bind(S_.lc, "lc", D * 6);
    bind(S_.wan_lat, "wan_lat", I * D);
    bind(S_.wan_bw, "wan_bw", I * D);
    bind(S_.carbon, "carbon", D);
    bind(S_.price24, "price24", 24);
    bind(S_.total_gpus, "total_gpus", D);
    bind(S_.p_idle, "p_idle", D);
    bind(S_.p_sleep, "p_sleep", D);
    bind(S_.p_peak, "p_peak", D);
    bind(S_.pow_alpha, "pow_alpha", D);
    bind(S_.power_gating, "power_gating", D);
    bind(S_.default_freq, "default_freq", D);
    bind(S_.slot_off, "slot_off", D + 1);
    bind(S_.slot_dc, "slot_dc", TS);
    // per-replica scalars
    bind(S_.now, "now", R);
    bind(S_.next_log, "next_log", R);
    bind(S_.rng_ctr, "rng_ctr", R);
    bind(S_.jid_ctr, "jid_ctr", R);
    bind(S_.done, "done", R);
    bind(S_.err, "err", R);
    bind(S_.arr_next, "arr_next", R * NS);
    // per (r, dc)
    bind(S_.busy, "busy", R * D);
    bind(S_.cur_freq, "cur_freq", R * D);
    bind(S_.energy_j, "energy_j", R * D);
    bind(S_.util_time, "util_time", R * D);
    bind(S_.util_begin, "util_begin", R * D);
    bind(S_.acc_unit, "acc_unit", R * D);
    bind(S_.p_active, "p_active", R * D);
    bind(S_.sum_tpt, "sum_tpt", R * D);
    bind(S_.n_running, "n_running", R * D);
    bind(S_.dc_min_finish, "dc_min_finish", R * D);
    bind(S_.dc_min_slot, "dc_min_slot", R * D);
    // job slots, transfers, queues
    bind(S_.s_finish, "s_finish", R * TS);
    bind(S_.seq_ctr, "seq_ctr", R);
    bind(S_.s_rec, "s_rec", R * TS);
    bind(S_.s_gpus, "s_gpus", R * TS);
    bind(S_.s_jtype, "s_jtype", R * TS);
    bind(S_.x_time, "x_time", R * TC);
    bind(S_.x_rec, "x_rec", R * TC);
    bind(S_.q_head, "q_head", R * D * 2);
    bind(S_.q_len, "q_len", R * D * 2);
    bind(S_.q_pay, "q_pay", R * D * 2 * Q * 2);
    bind(S_.q_netlat, "q_netlat", D * 2 * Q);
    bind(S_.q_jid, "q_jid", D * 2 * Q);
    bind(S_.q_ing, "q_ing", D * 2 * Q);
    // only the cap_greedy / bandit kernels touch these; elsewhere the host
    // passes placeholders, which are neither bound nor checked
    if (S_.algo == A_CAP_GREEDY) bind(S_.snap_f, "snap_f", R * TS);
    else bind.unused("snap_f");
    if (S_.algo == A_BANDIT) {
      bind(S_.b_n, "b_n", R * D * 2 * F);
      bind(S_.b_s, "b_s", R * D * 2 * F);
    } else {
      bind.unused("b_n");
      bind.unused("b_s");
    }
    bind(S_.b_t, "b_t", R);
    // metrics
    bind(S_.ev_count, "ev_count", R);
    bind(S_.jobs_done, "jobs_done", R);
    bind(S_.jobs_done_inf, "jobs_done_inf", R);
    bind(S_.sum_lat, "sum_lat", R);
    bind(S_.sum_lat_inf, "sum_lat_inf", R);
    bind(S_.sum_wait, "sum_wait", R);
    // logging
    bind(S_.cl_count, "cl_count", 1);
    bind(S_.cl_rows, "cl_rows", (int64_t)S_.cl_cap * 15);
    bind(S_.jl_count, "jl_count", 1);
    bind(S_.jl_rows, "jl_rows", (int64_t)S_.jl_cap * 11);
    if (S_.trace_mode) {
      bind(S_.trace_time, "trace_time", R * NS * S_.trace_cap);
      bind(S_.trace_size, "trace_size", R * NS * S_.trace_cap);
      bind(S_.trace_dc, "trace_dc", R * NS * S_.trace_cap);
      bind(S_.trace_pos, "trace_pos", R * NS);
    }
    if (ar_.cap > 0) {
#if DCG_SUBWAVE == 64
      bind(ar_.ring, "arr_ring", R * ar_.cap);
      bind(ar_.head, "arr_head", R);
      bind(ar_.count, "arr_count", R);
      bind(ar_.gen_arr_next, "gen_arr_next", R * NS);
      bind(ar_.gen_ctr, "gen_ctr", R);
      bind(ar_.more, "arr_more", 1);
#else
      // the 8-lane build draws inline: it stays the independent reference
      for (const char* n : {"arr_ring", "arr_head", "arr_count",
                            "gen_arr_next", "gen_ctr", "arr_more"})
        bind.unused(n);
      ar_.cap = 0;
#endif
    }
    if (S_.serve_device) {
      // the seven layers of EngineDesc::pw
      const int64_t H = S_.hid, G = S_.n_g;
      bind(S_.pw, "policy_weights",
           (O * H + H) + 2 * (H * H + H) + (H * H + H) + (H * D + D) +
               (H * H + H) + (H * G + G));
    }
    if (S_.algo == A_CHSAC) {
      const int64_t PP = S_.pp_cap, TR = S_.tr_cap;
      bind(S_.req_flag, "req_flag", R);
      bind(S_.req_obs, "req_obs", R * O);
      bind(S_.req_mdc, "req_mdc", R);
      bind(S_.req_mg, "req_mg", R);
      bind(S_.resp_dc, "resp_dc", R);
      bind(S_.resp_g, "resp_g", R);
      bind(S_.pend_kind, "pend_kind", R);
      bind(S_.pend_size, "pend_size", R);
      bind(S_.pend_netlat, "pend_netlat", R);
      bind(S_.pend_jid, "pend_jid", R);
      bind(S_.pend_ing, "pend_ing", R);
      bind(S_.pend_jt, "pend_jt", R);
      bind(S_.pend_dc, "pend_dc", R);
      bind(S_.pend_from_inf, "pend_from_inf", R);
      bind(S_.pend_enq, "pend_enq", R);
      bind(S_.slot_s0, "slot_s0", R * TS * O);
      bind(S_.x_s0, "x_s0", R * TC * O);
      bind(S_.pp_count, "pp_count", R);
      bind(S_.pp_cursor, "pp_cursor", R);
      bind(S_.pp_size, "pp_size", R * PP);
      bind(S_.pp_done, "pp_done", R * PP);
      bind(S_.pp_start, "pp_start", R * PP);
      bind(S_.pp_netlat, "pp_netlat", R * PP);
      bind(S_.pp_jid, "pp_jid", R * PP);
      bind(S_.pp_s0, "pp_s0", R * PP * O);
      bind(S_.pp_ing, "pp_ing", R * PP);
      bind(S_.pp_dc, "pp_dc", R * PP);
      bind(S_.pp_pcount, "pp_pcount", R * PP);
      bind(S_.pp_adc, "pp_adc", R * PP);
      bind(S_.pp_ag, "pp_ag", R * PP);
      bind(S_.pp_nrew, "pp_nrew", R * PP);
      bind(S_.pp_has_rl, "pp_has_rl", R * PP);
      bind(S_.lat_hist, "lat_hist", R * 2 * LAT_BINS);
      bind(S_.lat_count, "lat_count", R * 2);
      bind(S_.lat_sum, "lat_sum", R * 2);
      if (S_.exact_p99) {
        bind(S_.p99_sorted, "p99_sorted", R * 2 * S_.p99_win);
        bind(S_.p99_ring, "p99_ring", R * 2 * S_.p99_win);
      } else {
        bind.unused("p99_sorted");
        bind.unused("p99_ring");
      }
      bind(S_.tr_count, "tr_count", 1);
      bind(S_.tr_s0, "tr_s0", TR * O);
      bind(S_.tr_s1, "tr_s1", TR * O);
      bind(S_.tr_r, "tr_r", TR);
      bind(S_.tr_costs, "tr_costs", TR * 3);
      bind(S_.tr_adc, "tr_adc", TR);
      bind(S_.tr_ag, "tr_ag", TR);
      bind(S_.tr_mdc, "tr_mdc", TR);
      bind(S_.tr_mg, "tr_mg", TR);
    }

    if (ps_.every > 0) {
      auto smp = t_.find("ps_samples");
      TORCH_CHECK(smp != t_.end() && smp->second.dim() == 4 &&
                      smp->second.size(1) == S_.n_dc + 1 &&
                      smp->second.size(2) == PS_K &&
                      smp->second.size(3) == S_.n_rep,
                  "ps_samples must be [t_cap][n_dc+1][", PS_K, "][n_rep]");
      ps_.t_cap = (int)smp->second.size(0);
      TORCH_CHECK(t_.count("ps_time") && t_.count("ps_tick") &&
                      t_["ps_time"].numel() == ps_.t_cap &&
                      t_["ps_tick"].numel() == S_.n_rep,
                  "ps_time must be [t_cap], ps_tick [n_rep]");
      bind(ps_.samples, "ps_samples", (int64_t)ps_.t_cap * (D + 1) * PS_K * R);
      bind(ps_.time, "ps_time", ps_.t_cap);
      bind(ps_.tick, "ps_tick", R);
    }
    if (lat_on) {
      bind(lh_.hist, "lh_hist", R * D * 2 * LH_BINS);
      bind(lh_.over, "lh_over", R * D * 2);
    }
    // parameter sweep (on where the host allocated its tensors): sw_arr is
    // the generator's; sw_cap is the cap_greedy kernel's and dereferenced
    // only where the sweep has a power_cap axis (cfg sweep_cap)
    if (t_.count("sw_arr") != 0 || t_.count("sw_cap") != 0) {
      const bool cap_axis = opt("sweep_cap", 0) != 0;
      if (ar_.cap == 0)
        throw std::invalid_argument(
            "engine tensor 'sw_arr': a sweep lives in the arrival-ring "
            "generator, required arr_cap > 0 in the 64-lane build");
      if (cap_axis && S_.algo != A_CAP_GREEDY)
        throw std::invalid_argument(
            "engine tensor 'sw_cap': only cap_greedy reads a swept cap");
      bind(sw_.arr, "sw_arr", R * 6);
      if (cap_axis) bind(sw_.cap, "sw_cap", R);
      else bind.unused("sw_cap");
    }
    // rate profiles (arrival mode 3): the table is the generator's, bound
    // exactly where a job type is in that mode
    const bool prof_mode = S_.arr_mode[0] == 3 || S_.arr_mode[1] == 3;
    if (prof_mode || t_.count("arr_prof") != 0) {
      if (!prof_mode)
        throw std::invalid_argument(
            "engine tensor 'arr_prof': no job type is in arrival mode 3 "
            "(profile), required no such tensor");
      if (ar_.cap == 0)
        throw std::invalid_argument(
            "engine tensor 'arr_prof': arrival mode 3 (profile) lives in the "
            "arrival-ring generator, required arr_cap > 0 in the 64-lane "
            "build");
      auto it = t_.find("arr_prof");
      if (it != t_.end() &&
          (it->second.dim() != 2 || it->second.size(1) != PROF_W))
        throw std::invalid_argument(
            "engine tensor 'arr_prof': required rows of " +
            std::to_string(PROF_W) + " (K, m[64], cum[65]), found " +
            std::to_string(it->second.dim()) + " dims, last of " +
            std::to_string(it->second.dim() ? it->second.size(-1) : 0));
      bind(pf_.tab, "arr_prof", NS * PROF_W);
    }
    contract_ = bind.rows();
    on_gpu_ = bind.on_gpu();
    device_ = bind.device_str();

    // DCG_ADVANCE_PASSES: unset or 0 = plan automatically, 1 = always a
    // single launch, k = at most k passes
    if (const char* ev = std::getenv("DCG_ADVANCE_PASSES")) {
      int k = std::atoi(ev);
      if (k > 0) max_passes_ = k;
    }
  }

  // the tensors this engine bound, in bind order: (field, dtype, required
  // numel); a field its kernel never dereferences has numel -1
  const std::vector<Binder::Row>& contract() const { return contract_; }

  // Create a CU-masked stream for the advance kernel, excluding the LAST
  // `n_reserved` CUs.  The advance kernel's blocks are persistent for a
  // whole cycle (each wave loops until its replica yields), so without a
  // mask they occupy every wave slot on the device and concurrent work
  // (the overlapped SAC train kernels) starves behind them — stream
  // priorities cannot help because no slot ever frees.  Masking carves a
  // small CU island the advance never touches; kernels on ordinary streams
  // land there immediately.  (A resident-grid cap on top of the mask was
  // tried and did not help — see NEGATIVE RESULT above; the uncapped full
  // grid measured ~20% more events/s.)
  void enable_masked_stream(int n_reserved) {
    require_gpu("enable_masked_stream");
    if (masked_stream_) return;
    hipDeviceProp_t prop;
    int dev;
    (void)hipGetDevice(&dev);
    (void)hipGetDeviceProperties(&prop, dev);
    int n_cu = prop.multiProcessorCount;
    int words = (n_cu + 31) / 32;
    std::vector<uint32_t> mask(words, 0u);
    int usable = n_cu - n_reserved;
    if (usable < 1) usable = 1;
    for (int i = 0; i < usable; ++i) mask[i / 32] |= (1u << (i % 32));
    hipError_t e = hipExtStreamCreateWithCUMask(&masked_stream_,
                                                (uint32_t)words, mask.data());
    if (e != hipSuccess) {
      masked_stream_ = nullptr;  // fall back to the torch stream
      throw std::runtime_error(std::string("CU-mask stream: ") +
                               hipGetErrorString(e));
    }
  }

  bool masked_active() const { return masked_stream_ != nullptr; }

  bool advance_done() { return hipStreamQuery(stream()) == hipSuccess; }

  void advance_sync() {
    hipError_t e = hipStreamSynchronize(stream());
    if (e != hipSuccess)
      throw std::runtime_error(std::string("advance_sync: ") +
                               hipGetErrorString(e));
  }

  // Launch-plan controls.  resident_capacity 0: ask the runtime (cached);
  // max_passes 1: always one launch of all replicas, the behaviour before
  // the planner; min_quantum / launch_cost < 0: the planner's defaults (tests
  // lower them to cut small budgets too).
  void set_launch_plan(int resident_capacity, int max_passes,
                       int64_t min_quantum, int64_t launch_cost) {
    if (resident_capacity < 0 || max_passes < 1)
      throw std::runtime_error("set_launch_plan: capacity >= 0, passes >= 1");
    forced_capacity_ = resident_capacity;
    max_passes_ = max_passes;
    min_quantum_ = min_quantum < 0 ? PLAN_MIN_QUANTUM : (long long)min_quantum;
    launch_cost_ = launch_cost < 0 ? PLAN_LAUNCH_COST : (long long)launch_cost;
  }

  // replicas the device holds at once: resident blocks per CU at the real
  // dynamic-LDS size, times CUs, times replicas per block.  Kernel and LDS
  // size are fixed for the engine's lifetime, so one query serves it.
  int resident_capacity() {
    require_gpu("resident_capacity");
    if (forced_capacity_ > 0) return forced_capacity_;
    if (queried_capacity_ == 0) {
      int per_cu = 0, dev = 0, n_cu = 0;
      hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu,
          reinterpret_cast<const void*>(kernel(S_.algo != A_CHSAC)),
          THREADS_PER_BLOCK,
          shmem_bytes());
      if (e == hipSuccess) e = hipGetDevice(&dev);
      if (e == hipSuccess)
        e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount,
                                  dev);
      if (e != hipSuccess || per_cu < 1 || n_cu < 1)
        throw std::runtime_error(std::string("advance occupancy query: ") +
                                 hipGetErrorString(e));
      queried_capacity_ = per_cu * n_cu * REPLICAS_PER_BLOCK;
    }
    return queried_capacity_;
  }

  // Sub-steps of advance(., max_ev): with the arrival ring, consecutive
  // budgets of at most arr_cap events (arrival_plan.hpp), each topped up and
  // planned on its own; without it, the whole call.
  std::vector<long long> substeps(long long max_ev) const {
    std::vector<long long> out;
    const int n = ar_.cap > 0 ? substep_count(max_ev, ar_.cap) : 1;
    for (int i = 0; i < n; ++i) out.push_back(substep_budget(max_ev, n, i));
    return out;
  }

  // The launches advance(., max_ev) issues.  One launch of everything for
  // chsac (its launch cadence carries meaning: tr_limit, pending requests)
  // and on the CU-masked stream (its capacity is not the device's).
  LaunchPlan plan_for(long long max_ev) {
    if (max_passes_ <= 1 || S_.algo == A_CHSAC || masked_stream_) {
      LaunchPlan p;
      p.windows.push_back(single_window(S_.n_rep, max_ev));
      return p;
    }
    return make_launch_plan(S_.n_rep, resident_capacity(), max_ev,
                            max_passes_, min_quantum_, launch_cost_);
  }

  std::vector<std::tuple<int, int, int, int64_t, int64_t>> launch_plan(
      int64_t max_ev) {
    std::vector<std::tuple<int, int, int, int64_t, int64_t>> out;
    for (long long ev : substeps(max_ev))
      for (const LaunchWindow& w : plan_for(ev).windows)
        out.emplace_back(w.first, w.count, w.split, (int64_t)w.ev_a,
                         (int64_t)w.ev_b);
    return out;
  }

  // enqueue one advance chunk; returns immediately (stream-async)
  void advance(double t_target, int64_t max_ev) {
    require_gpu("advance");
    const int rpb = REPLICAS_PER_BLOCK;
    size_t shmem = shmem_bytes();
    dim3 block(THREADS_PER_BLOCK);
    const std::vector<long long> subs = substeps(max_ev);
    for (size_t i = 0; i < subs.size(); ++i) {
      const long long ev = subs[i];
      // A call of many sub-steps (a budget far above what t_target allows)
      // asks the device every SUBSTEP_CHECK of them whether any replica
      // still ran into its event budget; if none did, every later sub-step
      // would find all replicas at t_target or done and change nothing.
      if (subs.size() > SUBSTEP_CHECK && i % SUBSTEP_CHECK == 0) {
        if (i > 0 && !budget_limited()) break;
        hipError_t e = hipMemsetAsync(ar_.more, 0, sizeof(int), stream());
        if (e != hipSuccess)
          throw std::runtime_error(std::string("advance: ") +
                                   hipGetErrorString(e));
      }
#if DCG_SUBWAVE == 64
      if (ar_.cap > 0) {
        // same stream, so the ring is topped up before the windows read it
        const int per_block = PG_THREADS / PG_GROUP;
        // a sweep's generator reads the replica's own arrival parameters
        // and a rate profile's the per-stream table
        auto gen = pf_.tab ? (sw_.arr ? pregen_arrivals_kernel<true, true>
                                      : pregen_arrivals_kernel<false, true>)
                           : (sw_.arr ? pregen_arrivals_kernel<true, false>
                                      : pregen_arrivals_kernel<false, false>);
        hipLaunchKernelGGL(gen, dim3((S_.n_rep + per_block - 1) / per_block),
                           dim3(PG_THREADS), 0, stream(), S_, ar_, t_target,
                           ev, sw_, pf_);
        check_launch("pregen_arrivals_kernel launch failed");
      }
#endif
      const LaunchPlan plan = plan_for(ev);
      AdvanceFn fn = kernel(plan.windows.size() > 1);
      for (const LaunchWindow& w : plan.windows) {
        dim3 grid((w.count + rpb - 1) / rpb);
        hipLaunchKernelGGL(fn, grid, block, shmem, stream(), S_, t_target,
                           w.ev_a, ps_, w, ar_, lh_, sw_);
        check_launch("advance_kernel launch failed");
      }
    }
  }

  // did any replica use up its event budget since arr_more was cleared
  // (waits for the stream)
  bool budget_limited() {
    int more = 1;
    hipError_t e = hipMemcpyAsync(&more, ar_.more, sizeof(int),
                                  hipMemcpyDeviceToHost, stream());
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    if (e != hipSuccess)
      throw std::runtime_error(std::string("advance: ") +
                               hipGetErrorString(e));
    return more != 0;
  }

  // arrivals come from the ring (false: drawn inside the advance kernel)
  bool arrival_pregen() const { return ar_.cap > 0; }

 private:
  // The constructor binds tensors on any device without a HIP call, so the
  // contract can be checked on CPU tensors; nothing is launched on them.
  void require_gpu(const char* what) const {
    if (!on_gpu_)
      throw std::runtime_error(std::string(what) + ": the engine's tensors "
                               "are on " + device_ + ", not on a GPU");
  }

  // the advance kernel's stream: the CU-masked one once enabled
  hipStream_t stream() const {
    return masked_stream_ ? masked_stream_
                          : (hipStream_t)at::hip::getCurrentHIPStream();
  }

  using AdvanceFn = void (*)(EngineDesc, double, long long, PopSeriesDesc,
                             LaunchWindow, ArrRing, LatHistDesc, SweepDesc);

  // this engine's instantiation: one per Algo, in enum order, without and
  // with the population-series sampling, without and with the window
  // arithmetic (chsac: never windowed), without and with the arrival ring
  // (64-lane build only; chsac: never), without and with the latency
  // histograms
  AdvanceFn kernel(bool windowed) const {
#define DCG_ADVANCE_ROW(PS, WIN, PRE, LAT, CHSAC)                              \
  {advance_kernel<A_DEFAULT, PS, WIN, PRE, LAT>,                               \
   advance_kernel<A_CAP_UNIFORM, PS, WIN, PRE, LAT>,                           \
   advance_kernel<A_CAP_GREEDY, PS, WIN, PRE, LAT>,                            \
   advance_kernel<A_JOINT_NF, PS, WIN, PRE, LAT>,                              \
   advance_kernel<A_BANDIT, PS, WIN, PRE, LAT>,                                \
   advance_kernel<A_CARBON_COST, PS, WIN, PRE, LAT>,                           \
   advance_kernel<A_ECO_ROUTE, PS, WIN, PRE, LAT>,                             \
   advance_kernel<A_DEBUG, PS, WIN, PRE, LAT>,                                 \
   CHSAC}
#define DCG_ADVANCE_TABLE(PRE, LAT, CHSAC, CHSAC_PS)                           \
  {{DCG_ADVANCE_ROW(false, false, PRE, LAT, CHSAC),                            \
    DCG_ADVANCE_ROW(true, false, PRE, LAT, CHSAC_PS)},                         \
   {DCG_ADVANCE_ROW(false, true, PRE, LAT, nullptr),                           \
    DCG_ADVANCE_ROW(true, true, PRE, LAT, nullptr)}}
    // [LAT][windowed][PS][algo]
    static const AdvanceFn kernels[2][2][2][A_CHSAC + 1] = {
        DCG_ADVANCE_TABLE(false, false,
                          (advance_kernel<A_CHSAC, false, false>),
                          (advance_kernel<A_CHSAC, true, false>)),
        DCG_ADVANCE_TABLE(false, true,
                          (advance_kernel<A_CHSAC, false, false, false, true>),
                          (advance_kernel<A_CHSAC, true, false, false, true>))};
    if (S_.algo < 0 || S_.algo > A_CHSAC)
      throw std::runtime_error("unsupported algo for HIP engine");
    const bool lat = lh_.hist != nullptr, ps = ps_.samples != nullptr;
    AdvanceFn fn = kernels[lat][windowed][ps][S_.algo];
#if DCG_SUBWAVE == 64
    static const AdvanceFn pre_kernels[2][2][2][A_CHSAC + 1] = {
        DCG_ADVANCE_TABLE(true, false, nullptr, nullptr),
        DCG_ADVANCE_TABLE(true, true, nullptr, nullptr)};
    if (ar_.cap > 0) fn = pre_kernels[lat][windowed][ps][S_.algo];
    // a power_cap sweep: cap_greedy with the replica's own cap
    // [LAT][windowed][PS]
#define DCG_SWEPT_CAP(PS, WIN, LAT)                                            \
  advance_kernel<A_CAP_GREEDY, PS, WIN, true, LAT, true>
    static const AdvanceFn swept_cap_kernels[2][2][2] = {
        {{DCG_SWEPT_CAP(false, false, false), DCG_SWEPT_CAP(true, false, false)},
         {DCG_SWEPT_CAP(false, true, false), DCG_SWEPT_CAP(true, true, false)}},
        {{DCG_SWEPT_CAP(false, false, true), DCG_SWEPT_CAP(true, false, true)},
         {DCG_SWEPT_CAP(false, true, true), DCG_SWEPT_CAP(true, true, true)}}};
#undef DCG_SWEPT_CAP
    if (sw_.cap != nullptr) fn = swept_cap_kernels[lat][windowed][ps];
#endif
#undef DCG_ADVANCE_TABLE
#undef DCG_ADVANCE_ROW
    if (!fn) throw std::runtime_error("chsac has no windowed advance kernel");
    return fn;
  }

  // dynamic LDS of one block
  size_t shmem_bytes() const {
    size_t shmem = REPLICAS_PER_BLOCK *
                   lds_sizes(S_.total_slots, S_.tcap,
                             S_.algo == A_CHSAC).stride();
    if (shmem > 64 * 1024)
      throw std::runtime_error(
          "scenario too large for the LDS-mirrored engine (total_slots = " +
          std::to_string(S_.total_slots) + " + tcap = " +
          std::to_string(S_.tcap) + " need " + std::to_string(shmem) +
          " B, above the 64 KiB dynamic-LDS budget per block)");
    return shmem;
  }

  static constexpr size_t SUBSTEP_CHECK = 8;
  EngineDesc S_{};
  PopSeriesDesc ps_{};            // samples == nullptr: feature off
  ArrRing ar_{};                  // cap == 0: arrivals drawn in the kernel
  LatHistDesc lh_{};              // hist == nullptr: feature off
  SweepDesc sw_{};                // arr == nullptr: no parameter sweep
  ProfDesc pf_{};                 // tab == nullptr: no rate profile
  // launch plan (launch_plan.hpp)
  int forced_capacity_ = 0;       // 0: the runtime's occupancy answer
  int queried_capacity_ = 0;      // cache of that answer
  int max_passes_ = PLAN_MAX_PASSES;
  long long min_quantum_ = PLAN_MIN_QUANTUM;
  long long launch_cost_ = PLAN_LAUNCH_COST;
  std::unordered_map<std::string, torch::Tensor> t_;
  std::vector<Binder::Row> contract_;
  bool on_gpu_ = false;           // the bound tensors' device is a GPU
  std::string device_;            // ... and its name, for messages
  hipStream_t masked_stream_ = nullptr;
};

}  // namespace dcg

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "Batched MI355X (gfx950) Monte-Carlo replica engine";
  // module_local: the 64-wide and 8-wide extensions register the
  // same C++ type in one process
  py::class_<dcg::BatchedSimHip>(m, "BatchedSimHip", py::module_local())
      .def(py::init<py::dict, py::dict>())
      .def("advance", &dcg::BatchedSimHip::advance,
           py::arg("t_target"), py::arg("max_events"))
      .def("set_launch_plan", &dcg::BatchedSimHip::set_launch_plan,
           "resident_capacity 0 = query the runtime; max_passes 1 = single "
           "launch; min_quantum, launch_cost (events) < 0 = defaults",
           py::arg("resident_capacity"), py::arg("max_passes"),
           py::arg("min_quantum") = -1, py::arg("launch_cost") = -1)
      .def("launch_plan", &dcg::BatchedSimHip::launch_plan,
           "windows (first, count, split, ev_a, ev_b) advance() would launch",
           py::arg("max_events"))
      .def("contract", &dcg::BatchedSimHip::contract,
           "bound tensors in bind order: (field, dtype, required numel; -1 = "
           "never dereferenced in this configuration)")
      .def("resident_capacity", &dcg::BatchedSimHip::resident_capacity)
      .def("arrival_pregen", &dcg::BatchedSimHip::arrival_pregen,
           "arrivals come from the pre-generated ring (false: drawn inside "
           "the advance kernel)")
      .def("enable_masked_stream", &dcg::BatchedSimHip::enable_masked_stream,
           py::arg("n_reserved_cus"))
      .def("masked_active", &dcg::BatchedSimHip::masked_active)
      .def("advance_done", &dcg::BatchedSimHip::advance_done)
      .def("advance_sync", &dcg::BatchedSimHip::advance_sync);
  m.def("reduce_series", &dcg::reduce_series,
        "population time-series reduction (samples[T,C,R] f64, ticks[R] i32, "
        "every) -> stats[T,C,5] f64 = {n, mean, M2, min, max}; replica r "
        "counts at tick t iff ticks[r] / every > t",
        py::arg("samples"), py::arg("ticks"), py::arg("every"));
  m.def("latency_reduce", &dcg::latency_reduce,
        "latency-histogram reduction (hist[R,D,2,256] i32, over[R,D,2] i32, "
        "qs[Q] f64, 1 <= Q <= 8) -> (pop_hist[C',256] i64, "
        "per_rep[C',Q+2,R] f64 = {quantiles, sla_miss_frac, jobs}, "
        "stats[C',Q+2,5] f64 = {n, mean, M2, min, max} over non-NaN "
        "replicas); C' = (D + 1) * 2, row D = sum over DCs",
        py::arg("hist"), py::arg("over"), py::arg("qs"));
  m.def("rl_forward_mfma", &dcg::rl_forward_mfma,
        "MFMA (matrix-core) batched actor forward "
        "(pw, obs[B,D], hid, n_dc, n_g) -> (logits_dc, logits_g)",
        py::arg("pw"), py::arg("obs"), py::arg("hid"), py::arg("n_dc"),
        py::arg("n_g"));
  dcg::bind_debug_entries(m);
}
