// The scalar dims of an EngineDesc against the advance kernel's compile-time
// limits, checked once at construction.  The kernel holds per-DC, per-stream
// and per-frequency state in fixed LDS arrays and registers (Hot, the 8x8
// grid search, cap_greedy_control's level table), so a dim past its limit is
// an out-of-bounds device write, not an error.  Pure C++ (no HIP, no torch).
#pragma once
#include <stdexcept>
#include <string>

#include "engine_desc.hpp"

namespace dcg {

constexpr int MAX_GPJ = 8;  // GPUs per job: one row of the 8x8 (n, f) grid

// Throws std::invalid_argument naming the first offending value.  Reads the
// scalar fields of S only; the pointers may still be null.
inline void check_engine_limits(const EngineDesc& S) {
  auto fail = [](const std::string& what, long long v, const std::string& want) {
    throw std::invalid_argument("engine limits: " + what + " = " +
                                std::to_string(v) + ", required " + want);
  };
  auto in_range = [&](const char* what, long long v, long long lo,
                      long long hi) {
    if (v < lo || v > hi)
      fail(what, v, std::to_string(lo) + " <= " + what + " <= " +
                        std::to_string(hi));
  };
  auto at_least_1 = [&](const char* what, long long v) {
    if (v < 1) fail(what, v, std::string(what) + " >= 1");
  };
  in_range("n_dc", S.n_dc, 1, MAX_DC);
  at_least_1("n_ing", S.n_ing);
  if (S.n_streams != 2 * S.n_ing || S.n_streams > MAX_STREAMS)
    fail("n_ing", S.n_ing,
         "n_streams = 2 * n_ing <= " + std::to_string(MAX_STREAMS) +
             " (n_streams = " + std::to_string(S.n_streams) + ")");
  in_range("n_freq", S.n_freq, 1, MAX_FREQ);
  in_range("max_gpj", S.max_gpj, 1, MAX_GPJ);
  at_least_1("tcap", S.tcap);
  at_least_1("qcap", S.qcap);
  at_least_1("total_slots", S.total_slots);
  at_least_1("n_rep", S.n_rep);
  in_range("log_replica", S.log_replica, -1, (long long)S.n_rep - 1);
  at_least_1("cl_cap", S.cl_cap);
  at_least_1("jl_cap", S.jl_cap);
  in_range("algo", S.algo, A_DEFAULT, A_CHSAC);
  if (S.algo == A_CHSAC) {
    at_least_1("obs_dim", S.obs_dim);
    if (S.elastic) at_least_1("pp_cap", S.pp_cap);
    at_least_1("p99_win", S.p99_win);
  }
  if (S.serve_device) {
    // the in-kernel actor forward: activations and logits in fixed LDS rows
    // (dc logits at +0, g logits at +8 of RL_MAX_LOG)
    in_range("hid", S.hid, 1, RL_MAX_HID);
    in_range("obs_dim", S.obs_dim, 1, RL_MAX_OBS);
    in_range("n_g", S.n_g, 1, 8);
  }
}

}  // namespace dcg
