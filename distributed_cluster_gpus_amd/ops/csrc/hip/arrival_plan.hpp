// Index arithmetic of the arrival ring (arrival_ring.hpp) and of the way
// BatchedSimHip::advance() cuts a call so that the ring can never run dry.
// Pure C++ (no HIP, no torch): it compiles for the host alone, and the
// kernels include it too.
//
// The ring of one replica holds arr_cap records, arr_cap a power of two.
// `head` is the slot of the oldest record, `count` the number of records, so
// record i (0 = oldest) sits in slot (head + i) & (arr_cap - 1).  One event
// consumes at most one record, so a launch sequence that gives every replica
// E events is safe once the ring holds min(E, arr_cap) records, and a call of
// more than arr_cap events is cut into sub-steps of at most arr_cap events,
// each topped up on its own.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCG_HD __host__ __device__
#else
#define DCG_HD
#endif

namespace dcg {

DCG_HD inline bool arr_cap_valid(long long cap) {
  return cap >= 1 && cap <= (1ll << 30) && (cap & (cap - 1)) == 0;
}

// slot of record i (0 = oldest); head in [0, cap), 0 <= i <= cap
DCG_HD inline int ring_slot(int head, int i, int cap) {
  return (int)(((long long)head + i) & (cap - 1));
}

// records the ring must hold before a launch sequence of `budget` events
DCG_HD inline long long ring_topup_target(long long budget, long long cap) {
  if (budget < 0) budget = 0;
  return budget < cap ? budget : cap;
}

// A call of E events runs as n consecutive sub-steps with budgets
// E/n + (i < E%n), n = ceil(E / cap): they sum to E, none exceeds cap, and
// they differ by at most one event (a short last sub-step would cost the
// launch planner its minimum quantum).  E <= 0: one sub-step of E, the
// launch the call made before.
DCG_HD inline int substep_count(long long E, long long cap) {
  return E <= 0 ? 1 : (int)((E + cap - 1) / cap);
}
DCG_HD inline long long substep_budget(long long E, int n, int i) {
  return E <= 0 ? E : E / n + (i < E % n ? 1 : 0);
}

}  // namespace dcg
