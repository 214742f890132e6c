// Launch planner for BatchedSimHip::advance(): balance a step over the
// device's resident capacity so that no launch ends in a thinly occupied
// tail.  Pure host C++ (no HIP, no torch), so it is testable on its own.
//
// Every wave of the advance kernel runs exactly its event budget, and the
// kernel is bound by per-wave latency: a wave alone on its SIMD is only
// about 1.6x faster than with its full complement of neighbours (measured,
// profiles/README.md).  One launch of R replicas on a device that holds C of
// them therefore costs close to ceil(R/C) full rounds of E events, however
// empty the last round is (4096 replicas on C = 3072: 1.62 rounds of time
// for 1.33 rounds of work; the cost model below rounds that up to 2).  The
// kernel saves and restores a replica's complete state at any event
// boundary, so the same step can be cut differently:
//
//   * every replica gets n passes with budgets E/n + (p < E%n), summing to E;
//   * the R*n replica-passes are laid out pass-major, replica-minor;
//   * that sequence is cut into consecutive windows of at most C, one launch
//     each: L = ceil(R*n/C) launches, all but the last exactly full.
//
// A window is a contiguous run of the sequence shorter than R, so it crosses
// at most one pass boundary (hence `split` and two budgets) and never holds a
// replica twice; launches on one stream run in order, which keeps a
// replica's passes in order.
#pragma once
#include <cstdint>
#include <vector>

namespace dcg {

// One launch.  Slot s in [0, count) serves replica (first + s) mod R with
// budget ev_a if s < split, else ev_b.  Passed to the kernel by value.
struct LaunchWindow {
  int first;
  int count;
  int split;
  long long ev_a;
  long long ev_b;
};

// The constants of the cost model.  Costs are in events.  One event costs a
// wave about 3.8 us (65,536 replicas run 818 M events/s over 3072 resident
// waves: 1 / (818e6 / 3072)).
//
// PLAN_MIN_QUANTUM: shortest pass a replica may be given once a step is
// split.  At 256 events a pass lasts ~1 ms, so a gap of tens of us between
// consecutive launches stays below about 3 % of it.
constexpr long long PLAN_MIN_QUANTUM = 256;
// PLAN_LAUNCH_COST: fixed cost of one more launch: the launch gap plus the
// kernel's load and write-back of the replica's hot state.  Measured 50 to
// 150 us per launch (profiles/README.md), 10 to 33 events; the upper end.  It
// also breaks the tie between n and its multiples (n = 3 and n = 6 cut the
// flagship equally well) in favour of fewer launches.
constexpr long long PLAN_LAUNCH_COST = 32;
constexpr int PLAN_MAX_PASSES = 8;
// PLAN_SINGLE_*: what ONE launch of R > C replicas costs, in rounds of E
// events.  Not ceil(R/C): once a grid is larger than the device, finished
// waves are replaced one by one, the waves of a SIMD drift out of step and
// run about 1.25x faster than a full launch in lockstep does, and the launch
// pays a fixed drain at its end instead.  Measured on the flagship kernel
// from 4096 to 65,536 replicas (profiles/README.md): 0.8 * R/C + 0.6 rounds,
// within 3 %.  Planned launches are full lockstep rounds (1.0 * R/C plus the
// launch costs), so they win below about 2.7 * C and lose above; without
// this term the planner cut 65,536 replicas into 64 launches and lost 18 %.
constexpr long long PLAN_SINGLE_SLOPE_NUM = 4, PLAN_SINGLE_TAIL_NUM = 3,
                    PLAN_SINGLE_DEN = 5;

struct LaunchPlan {
  int n_passes = 1;
  std::vector<LaunchWindow> windows;
};

inline LaunchWindow single_window(int R, long long E) {
  return LaunchWindow{0, R, R, E, E};
}

// Number of passes: n in 1..max_passes minimising the cost, smallest n on a
// tie.  n passes cost L(n) * (E/n + o), L(n) = ceil(R*n/C) launches, with
// E/n >= min_quantum for every n > 1; the single launch costs
// min(L(1), 0.8 * R/C + 0.6) * E + o (PLAN_SINGLE_*).  n = 1 (one launch of
// all R, as before) whenever splitting cannot help: everything is resident
// at once (R <= C), the rounds are all full (R % C == 0), or E is too small.
inline int plan_passes(long long R, long long C, long long E, int max_passes,
                       long long min_quantum = PLAN_MIN_QUANTUM,
                       long long launch_cost = PLAN_LAUNCH_COST) {
  if (R <= 0 || C <= 0 || E <= 0 || max_passes <= 1) return 1;
  if (R <= C || R % C == 0) return 1;
  if (min_quantum < 1) min_quantum = 1;
  typedef unsigned __int128 u128;
  // best n > 1: cost(n) = L * (E + o*n) / n, compared exactly by
  // cross-multiplication
  int best_n = 0;
  u128 best_num = 0;
  for (int n = 2; n <= max_passes; ++n) {
    if (E / n < min_quantum) break;
    u128 L = (u128)((R * n + C - 1) / C);
    u128 num = L * (u128)(E + launch_cost * n);
    if (best_n == 0 || num * (u128)best_n < best_num * (u128)n) {
      best_n = n;
      best_num = num;
    }
  }
  if (best_n == 0) return 1;
  // the single launch: s_num / s_den
  const long long L1 = (R + C - 1) / C;
  const long long lin = PLAN_SINGLE_SLOPE_NUM * R + PLAN_SINGLE_TAIL_NUM * C;
  const long long den = PLAN_SINGLE_DEN * C;
  u128 s_num, s_den;
  if (lin < L1 * den) {
    s_num = (u128)E * (u128)lin + (u128)launch_cost * (u128)den;
    s_den = (u128)den;
  } else {
    s_num = (u128)L1 * (u128)(E + launch_cost);
    s_den = 1;
  }
  return best_num * s_den < s_num * (u128)best_n ? best_n : 1;
}

inline LaunchPlan make_launch_plan(int R, int C, long long E, int max_passes,
                                   long long min_quantum = PLAN_MIN_QUANTUM,
                                   long long launch_cost = PLAN_LAUNCH_COST) {
  LaunchPlan plan;
  plan.n_passes = plan_passes(R, C, E, max_passes, min_quantum, launch_cost);
  const long long n = plan.n_passes;
  if (n == 1) {
    plan.windows.push_back(single_window(R, E));
    return plan;
  }
  // n > 1 implies C < R, so a window spans at most two passes
  const long long total = (long long)R * n;
  auto budget = [&](long long p) { return E / n + (p < E % n ? 1 : 0); };
  for (long long k = 0; k < total; k += C) {
    long long cnt = total - k < C ? total - k : C;
    long long pass = k / R, first = k % R;
    long long in_pass = R - first < cnt ? R - first : cnt;
    LaunchWindow w;
    w.first = (int)first;
    w.count = (int)cnt;
    w.split = (int)in_pass;
    w.ev_a = budget(pass);
    w.ev_b = in_pass < cnt ? budget(pass + 1) : w.ev_a;
    plan.windows.push_back(w);
  }
  return plan;
}

}  // namespace dcg
