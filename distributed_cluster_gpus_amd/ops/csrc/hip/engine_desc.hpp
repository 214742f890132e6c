// The replica engine's host <-> device contract: the packed records, the
// enums, the kernel's compile-time limits and EngineDesc, the by-value kernel
// argument that names every device tensor.  Pure C++ (no HIP, no torch), so a
// host-only program can include it; engine_limits.hpp checks the scalar dims
// against the limits here, engine_bind.hpp binds and checks the pointers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dcg {

constexpr int MAX_DC = 8;
constexpr int MAX_FREQ = 8;

// Packed per-object payload records: everything a job start/finish (or a
// WAN-transfer push/admission) touches lands in ONE cache line instead of
// 6-12 scattered SoA arrays — the engine is memory-LATENCY-chain bound
// (profiles/README.md PMC analysis), so dependent line count per event is
// the cost that matters.  Scan-heavy fields (finish times, gpus, jtype)
// stay SoA/LDS.
struct XRec {            // 32 B: in-flight WAN transfer payload
  double size;
  float netlat;
  int jid;
  short nsel;            // RL-chosen n (chsac; unclamped g+1)
  unsigned char dc, jtype, ing, adc, ag, mdc;
  unsigned char mg, has_rl, pad0, pad1;
};
static_assert(sizeof(XRec) == 32, "XRec must be one 32B record");

struct SRec {            // 64 B: cold job-slot payload
  double start, lastupd, size, fused, done;
  float netlat;
  int jid;
  int seq;
  unsigned char ing, pcount, nrew, adc, ag, mdc, mg, has_rl;
  unsigned char pad[4];
};
static_assert(sizeof(SRec) == 64, "SRec must be one 64B record");

struct ARec {            // 32 B: one pre-generated arrival (arrival ring)
  double size;           // job size
  double t_next;         // the stream's next arrival time (arr_next[stream])
  uint64_t ctr;          // the replica's Philox counter after this arrival
  int stream;            // ing * 2 + jtype
  int dc;                // routed DC (rbelow); -1 where the kernel routes
};
static_assert(sizeof(ARec) == 32, "ARec must be one 32B record");

enum Algo { A_DEFAULT = 0, A_CAP_UNIFORM, A_CAP_GREEDY, A_JOINT_NF, A_BANDIT,
            A_CARBON_COST, A_ECO_ROUTE, A_DEBUG, A_CHSAC };

// CHSAC-AF action-request state machine kinds
enum PendKind : int { PEND_NONE = 0, PEND_ARRIVAL = 1, PEND_DRAIN = 2,
                      PEND_REALLOC = 3 };
// request flags
enum ReqFlag : int { REQ_IDLE = 0, REQ_PENDING = 1, REQ_READY = 2 };

constexpr int LAT_BINS = 64;  // log10 bins over sojourn [1e-4 s, 1e4 s)

enum Err : int { ERR_NONE = 0, ERR_QUEUE_OVF = 1, ERR_XFER_OVF = 2,
                 ERR_SLOT_OVF = 4, ERR_LOG_OVF = 8,
                 // an arrival found the ring empty, or its head record is for
                 // another stream (must never fire)
                 ERR_ARR_RING = 16 };

// compile-time limits of the advance kernel's LDS-resident state and of
// the in-kernel actor forward (checked by engine_limits.hpp)
constexpr int MAX_STREAMS = 16;
constexpr int RL_MAX_HID = 256;
constexpr int RL_MAX_OBS = 64;
constexpr int RL_MAX_LOG = 16;

struct EngineDesc {
  // sizes
  int n_rep, n_dc, n_ing, n_freq, n_streams, total_slots, tcap, qcap;
  double end_time, log_interval;
  // scenario constants (device)
  const double* freq_levels;      // [n_freq]
  const double* pc;               // [dc][2][3]
  const double* lc;               // [dc][2][3]
  const double* wan_lat;          // [ing][dc]
  const double* wan_bw;           // [ing][dc]
  const double* carbon;           // [dc]
  const double* price24;          // [24]
  const int* total_gpus;          // [dc]
  const double* p_idle;           // [dc]
  const double* p_sleep;          // [dc]
  const double* p_peak;           // [dc] (baseline end-flush model)
  const double* pow_alpha;        // [dc]
  const int* power_gating;        // [dc]
  const double* default_freq;     // [dc]
  const int* slot_off;            // [dc+1]
  const int* slot_dc;             // [total_slots] slot -> dc
  // policy / run params
  int algo, max_gpj, inf_priority, scale_out_low, energy_aware;
  double dvfs_low, dvfs_high, power_cap;
  int eco_obj, num_fixed;
  int fp32_score;                 // opt-in fp32 decision-score eval (grid /
                                  //   energy-freq argmins; times stay f64)
  double fixed_freq;
  double payload_gb[2];
  // arrival processes by jtype: mode 0=poisson 1=sinusoid 2=off 3=profile
  // (profile: the arrival-ring generator's only, with ProfDesc below)
  int arr_mode[2];
  double arr_rate[2], arr_amp[2], arr_period[2];
  uint64_t seed;
  int64_t rep_id_offset;          // global replica id of local replica 0
  // per-replica scalars
  double* now;                    // [r] (last event time; <0 = no event yet)
  double* next_log;               // [r]
  uint64_t* rng_ctr;              // [r]
  int* jid_ctr;                   // [r]
  int* done;                      // [r]
  int* err;                       // [r]
  double* arr_next;               // [r][n_streams]  (stream = ing*2 + jtype)
  // per (r, dc)
  int* busy;
  double* cur_freq;
  double* energy_j;
  double* util_time;
  double* util_begin;             // [r][dc] first-event stamp (<0 unset)
  double* acc_unit;
  double* p_active;               // cached sum of running-job powers
  double* sum_tpt;                // cached sum of running-job throughputs
  int* n_running;
  double* dc_min_finish;          // cached min finish time (INF if none)
  int* dc_min_slot;
  // job slots [r][total_slots]: finish times + scan fields SoA, the cold
  // payload as one SRec per slot (f64 values bitwise-exact as before)
  double* s_finish;               // INF = empty
  SRec* s_rec;                    // packed payload
  short* s_gpus;                  // 0 = empty (dense busy/log scans)
  char* s_jtype;                  // dense scans (log rows, elastic, cap)
  // in-flight transfers [r][tcap]: time SoA (LDS-mirrored), payload packed
  double* x_time;                 // INF = empty
  XRec* x_rec;
  // queues [r][dc][2] ring of capacity qcap; per-entry payload = (size,
  // enqueue-time) f64 pair; aux fields (netlat/jid/ing) exist only for the
  // logging replica ([dc][2][qcap], no replica dim)
  int* q_head;
  int* q_len;
  double* q_pay;                  // [r][dc][2][qcap][2] (f64 exact parity)
  float* q_netlat;                // [dc][2][qcap] (log replica only)
  int* q_jid;                     // [dc][2][qcap] (log replica only)
  char* q_ing;                    // [dc][2][qcap] (log replica only)
  // bandit state [r][dc][2][n_freq]
  int* b_n;
  double* b_s;
  long long* b_t;                 // [r]
  // metrics [r]
  long long* ev_count;
  long long* jobs_done;
  long long* jobs_done_inf;
  double* sum_lat;
  double* sum_lat_inf;
  double* sum_wait;               // summed queueing delay (job start minus
                                  //   its enqueue at the DC; 0 for jobs that
                                  //   start straight off the WAN transfer)
  int* seq_ctr;                   // [r] job-start sequence counter
  double* snap_f;                 // [r][total_slots] cap_greedy pass snapshot
                                  //   (allocated only for algo==cap_greedy)
  // logging (one designated replica); the host drains both buffers
  // chunk-wise between launches, so caps bound one launch's production only
  int log_replica;                // -1 = off
  int cl_cap, jl_cap;
  int* cl_count;                  // [1]
  double* cl_rows;                // [cl_cap][15]
  int* jl_count;                  // [1]
  double* jl_rows;                // [jl_cap][11]
  // ===== arrival-trace replay mode (single-replica exact-parity testing:
  // arrivals come from a host-recorded (time, size) FIFO per stream instead
  // of the Philox draws) =====
  int trace_mode;                 // 0 off, 1 on
  int trace_cap;                  // entries per stream
  const double* trace_time;       // [r][n_streams][cap] absolute times
  const double* trace_size;       // [r][n_streams][cap]
  const char* trace_dc;           // [r][n_streams][cap] routed DC (-1 = use
                                  //   the algorithm's own routing)
  int* trace_pos;                 // [r][n_streams] cursor
  // ===== CHSAC-AF (RL-in-the-loop) state; null unless algo == A_CHSAC =====
  int obs_dim;                    // 1 + 6*n_dc
  double sla_p99_ms;
  // --- device-side policy serving (serve_device=1): the actor MLP runs
  // INSIDE the advance kernel from a flat weights buffer the host refreshes
  // after each SAC train round, so replicas never pause for a host policy
  // round-trip (round-1 bottleneck: 206k ev/s host-loop-bound).  Layout of
  // pw (all fp32, [in][out]-major so the out index is lane-coalesced):
  //   enc1 Wt[obs_dim][hid] b[hid] | enc2 Wt[hid][hid] b | enc3 Wt[hid][hid] b
  //   | hdc1 Wt[hid][hid] b | hdc2 Wt[hid][n_dc] b[n_dc]
  //   | hg1 Wt[hid][hid] b | hg2 Wt[hid][n_g] b[n_g]
  int serve_device;               // 0 = host pause/resume, 1 = in-kernel
  int hid;                        // encoder/head hidden width (<= RL_MAX_HID)
  int n_g;                        // g-head size (max_gpj)
  int rl_det;                     // 1 = greedy argmax (no Gumbel draw)
  int tr_limit;                   // yield the launch when the transition ring
                                  //   reaches this (bounds policy staleness)
  const float* pw;                // flat policy weights
  // action request/response, one slot per replica
  int* req_flag;                  // [r] ReqFlag
  float* req_obs;                 // [r][obs_dim]
  int* req_mdc;                   // [r] bitmask of valid DCs
  int* req_mg;                    // [r] bitmask of valid g choices
  int* resp_dc;                   // [r]
  int* resp_g;                    // [r]
  int* pend_kind;                 // [r] PendKind
  // stashed context for the paused event
  double* pend_size;              // [r]
  float* pend_netlat;             // [r]
  int* pend_jid;                  // [r]
  int* pend_ing;                  // [r]
  int* pend_jt;                   // [r]
  int* pend_dc;                   // [r] (drain: source DC)
  int* pend_from_inf;             // [r] (drain: 1 = popped from the inference
                                  //   queue; kept for the host-side state
                                  //   layout — the resume reads pend_jt)
  double* pend_enq;               // [r] (drain: the popped job's enqueue time)
  // per-job RL obs traces (the action/mask bytes live in SRec/XRec;
  // arrival path keeps nrew = g_idx+1 unclamped, drain path clamped —
  // reference :571 vs :889)
  float* slot_s0;                 // [r][total_slots][obs_dim]
  float* x_s0;                    // [r][tcap][obs_dim]
  // elastic scaling (chsac only): preempted-training-job pool per replica
  int elastic;                    // 0 off, 1 on
  int pp_cap;                     // pool capacity
  int* pp_count;                  // [r] entries in pool
  int* pp_cursor;                 // [r] next entry to reallocate
  double* pp_size;                // [r][cap] original size
  double* pp_done;                // [r][cap] units completed at preemption
  double* pp_start;               // [r][cap] ORIGINAL start time (resume
                                  //   keeps it: latency spans preemptions)
  float* pp_netlat;               // [r][cap]
  int* pp_jid;                    // [r][cap]
  unsigned char* pp_ing;          // [r][cap]
  unsigned char* pp_dc;           // [r][cap]
  unsigned char* pp_pcount;       // [r][cap] job's preempt count
  float* pp_s0;                   // [r][cap][obs_dim] carried RL trace
  unsigned char* pp_adc;          // [r][cap]
  unsigned char* pp_ag;           // [r][cap]
  unsigned char* pp_nrew;         // [r][cap]
  unsigned char* pp_has_rl;       // [r][cap]
  // latency histograms per (r, jtype): counts in log10 bins
  int* lat_hist;                  // [r][2][LAT_BINS]
  long long* lat_count;           // [r][2]
  double* lat_sum;                // [r][2]
  // exact sliding-window p99 (parity mode): the reference computes an exact
  // percentile over the last 2048 sojourns (simulator_paper_multi.py:728-737)
  // where the fast path approximates from the log histogram.  exact_p99=1
  // maintains a SORTED window + an insertion-order ring per (r, jtype) and
  // reproduces np.percentile(buf, 99) bit-for-bit.
  int exact_p99;
  int p99_win;                    // window size (2048)
  double* p99_sorted;             // [r][2][win]
  double* p99_ring;               // [r][2][win]
  // transition ring (global across replicas; host drains between launches)
  int tr_cap;
  int* tr_count;                  // [1] atomicAdd cursor
  float* tr_s0;                   // [cap][obs_dim]
  float* tr_s1;                   // [cap][obs_dim]
  unsigned char* tr_adc;          // [cap]
  unsigned char* tr_ag;           // [cap]
  float* tr_r;                    // [cap]
  float* tr_costs;                // [cap][3]: latency_p99_ms, power_W, gpu_over
  unsigned char* tr_mdc;          // [cap]
  unsigned char* tr_mg;           // [cap]
};

// The arrival ring (arrival_ring.hpp): arrivals pre-generated by
// pregen_arrivals_kernel, consumed in order by the PRE advance kernels.  A
// trailing kernel argument of its own, as PopSeriesDesc is, so that EngineDesc
// and with it the PRE = false kernels stay what they were.  cap == 0: off
// (chsac, trace mode, the 8-lane build).
struct ArrRing {
  int cap;                        // records per replica, a power of two
  ARec* ring;                     // [r][cap]
  int* head;                      // [r] slot of the next record to consume
  int* count;                     // [r] records generated, not yet consumed
  // the generator's frontier: stream times and counter after the LAST
  // GENERATED record (arr_next / rng_ctr: after the last CONSUMED one)
  double* gen_arr_next;           // [r][n_streams]
  uint64_t* gen_ctr;              // [r]
  int* more;                      // [1] set by a replica that used up its
                                  //   event budget: a later sub-step of the
                                  //   same call may still have work
};

// A parameter sweep (engine/sweep.py): per-replica arrival parameters and
// power cap in place of the EngineDesc scalars of the same names.  Per
// replica, not per group plus an index: one load, no second indirection.
// Read by pregen_arrivals_kernel<true> (arr) and by the SWP instantiations
// of the cap_greedy advance kernel (cap); written by nobody on the device.
// A trailing kernel argument of its own, as ArrRing is.  null: off.
struct SweepDesc {
  const double* arr;              // [r][2][3] (jtype; rate, amp, period)
  const double* cap;              // [r] power cap; null: no power_cap axis
};

// Per-stream rate profiles (arrival mode 3; models/arrivals.py): stream s =
// ing * 2 + jtype runs at rate * m[floor(K * frac(t / period))], rate and
// period being the job type's (EngineDesc, or the replica's own under a
// sweep).  One row of PROF_W doubles per stream:
//   [0]        K, the number of segments (1..PROF_MAX_SEG; 0 in the rows of
//              a job type that is not in profile mode, which nobody reads)
//   [1..64]    m[0..K-1], the multipliers (>= 0), zero-padded
//   [65..129]  cum[0..K], cum[k] = (m[0] + ... + m[k-1]) / K, zero-padded
// m and cum are contiguous so that the eight lanes of a generator group read
// eight adjacent cum entries per step of the segment search.  Read by
// pregen_arrivals_kernel<*, true> only and written by nobody on the device;
// a trailing argument of the GENERATOR alone, so that neither EngineDesc nor
// ArrRing, which the advance kernels take, changes.  null: off.
constexpr int PROF_MAX_SEG = 64;
constexpr int PROF_W = 2 * PROF_MAX_SEG + 2;
struct ProfDesc {
  const double* tab;              // [n_streams][PROF_W]
};

// the Python side allocates the records as float64 rows (s_rec [.., 8],
// x_rec and arr_ring [.., 4]); the binder casts those rows to the record types
static_assert(sizeof(SRec) == 8 * sizeof(double), "s_rec rows are 8 f64 wide");
static_assert(sizeof(XRec) == 4 * sizeof(double), "x_rec rows are 4 f64 wide");
static_assert(sizeof(ARec) == 4 * sizeof(double), "arr_ring rows are 4 f64 wide");

}  // namespace dcg
