// Device-side analytic models for the batched replica engine (gfx950).
//
// The DVFS power polynomial and T(n,f) latency model are fused into every
// step kernel as inlined device functions ("HIP device
// function, fused").  f64 forms are used on the simulation path (event times
// must track the scalar engines to rounding; energy integrals need the
// precision).  They are NOT bitwise-equal to the scalar engines' unfused
// arithmetic: the extension is compiled with floating-point contraction on,
// so c0*f*f*f + c1*f + c2 and the c2*n term become FMAs.  Measured through
// models_debug (tests/test_gpu_models.py): P differs from the unfused f64
// evaluation on 20 of 500 rows by at most 2 ulp, T on 4 of 500 by 1 ulp; both
// stay within their rounding depth (6 resp. 4) x 2^-53 of the exact value.
// Exact score ties between candidates are therefore resolved in DEVICE
// arithmetic: a contracted score can break a tie the scalar scan sees, or the
// reverse, whenever two candidates score within that rounding of each other.
// The (n,f) grid search is candidate-strided over the replica's
// subgroup: at the default 64-lane width the 8x8 candidate grid maps exactly
// one-candidate-per-lane onto a CDNA4 wavefront; the
// 8-lane multi-replica build strides 8 candidates per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

namespace dcg {

constexpr double D_INF = 1e300;

#ifndef DCG_SUBWAVE
#define DCG_SUBWAVE 64
#endif

// ---- launch-invariant scenario tables ----
// The coefficient / topology tables (pc, lc, wan_*, freq_levels, slot_off,
// slot_dc, total_gpus, ...) are written by the host before a launch and never
// by a kernel.  The 64-lane build reads them through the CONSTANT address
// space: with a wave-uniform index such a load is a scalar load (s_load, SGPR
// result, scalar cache) that the compiler may place across the engine's
// memory-clobbering fences, instead of a vector global load stuck behind
// them on the per-event dependent chain.  The 8-lane build keeps plain
// global pointers (its indices are uniform per subgroup only).
#if DCG_SUBWAVE == 64
typedef __attribute__((address_space(4))) const double* kc_f64;
typedef __attribute__((address_space(4))) const int* kc_i32;
__device__ __forceinline__ kc_f64 launch_const(const double* p) {
  return (kc_f64)p;
}
__device__ __forceinline__ kc_i32 launch_const(const int* p) {
  return (kc_i32)p;
}
#else
typedef const double* kc_f64;
typedef const int* kc_i32;
__device__ __forceinline__ kc_f64 launch_const(const double* p) { return p; }
__device__ __forceinline__ kc_i32 launch_const(const int* p) { return p; }
#endif

// The models are templated on the value type F of the frequency argument:
// double on the simulation path, float for the opt-in fp32 decision scores
// (coefficients are read as f64 and narrowed).  Coefficient-triple pointers
// are templated too: kc_f64 from the engine, plain pointers from anything
// else.  The narrowed literals are the ones the fp32 scores always used.
static_assert((float)1e-9 == 1e-9f && (float)3.6e6 == 3.6e6f,
              "fp32 score literals");
template <class F, class P3>
__device__ __forceinline__ F d_gpu_power(F f, P3 c3) {
  f = fmax((F)0.0, f);
  return (F)c3[0] * f * f * f + (F)c3[1] * f + (F)c3[2];
}
template <class F, class P3>
__device__ __forceinline__ F d_job_power(int n, F f, P3 c3) {
  return (F)max(0, n) * d_gpu_power(f, c3);
}
template <class F, class P3>
__device__ __forceinline__ F d_unit_time(int n, F f, P3 c3) {
  n = max(1, n);
  f = fmax((F)1e-9, f);
  if (n == 1) return (F)c3[0] + (F)c3[1] / f;
  return ((F)c3[0] + (F)c3[1] / f + (F)c3[2] * n) / n;
}

// ---- subwave reductions ----
// DCG_SUBWAVE lanes cooperate on one replica (64 = classic wave-per-replica;
// 8 = eight replicas per wavefront, amortizing the wave-uniform scalar work
// across subgroups).
//
// The two widths reduce differently.  The 8-lane build uses an xor butterfly
// of __shfl_xor (offsets < 8 stay inside an aligned subgroup); every lane of
// the subgroup ends up with the result in a VGPR.  The 64-lane build reduces
// with DPP row shifts/broadcasts on the VALU (no LDS-pipe permutes): the full
// result lands in lane 63 and is handed back through v_readlane, i.e. in
// SGPRs, so the compiler knows it is wave-uniform and callers branch on it
// with scalar branches.  Both order (value, tie-break key) pairs by the same
// strict total order, so they pick the same winner bit for bit; the 8-lane
// build doubles as the independent reference for the DPP code.
//
// All reductions must be called with every lane of the subgroup active.
constexpr int SUBW = DCG_SUBWAVE;
static_assert(SUBW == 64 || SUBW == 8, "supported subwave widths: 64, 8");

__device__ __forceinline__ int sub_lane() { return threadIdx.x & (SUBW - 1); }

#if DCG_SUBWAVE == 64
// ---- DPP building blocks (gfx9 dpp_ctrl encodings) ----
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114,
              DPP_ROW_SHR8 = 0x118, DPP_ROW_BCAST15 = 0x142,
              DPP_ROW_BCAST31 = 0x143;

// lane i reads `v` from the lane the control selects; a lane with no valid
// source (shifted in from outside its 16-lane row, or in a row the mask
// disables) gets `keep` instead
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int keep, int v) {
  return __builtin_amdgcn_update_dpp(keep, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double keep, double v) {
  int lo = dpp_i32<CTRL, ROW_MASK>(__double2loint(keep), __double2loint(v));
  int hi = dpp_i32<CTRL, ROW_MASK>(__double2hiint(keep), __double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}

// one stage of the (value, key) lexicographic min: a lane without a source
// compares against its own pair and keeps it.  Branch-free on purpose
// (v_cmp / v_cndmask, no EXEC-mask branches).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_argmin_stage(double& bv, int& bk) {
  double ov = dpp_f64<CTRL, ROW_MASK>(bv, bv);
  int ok = dpp_i32<CTRL, ROW_MASK>(bk, bk);
  bool take = (ov < bv) | ((ov == bv) & (ok < bk));
  bv = take ? ov : bv;
  bk = take ? ok : bk;
}
// full 64-lane reduction: after row_shr 1/2/4/8 lane 15 of each row holds its
// row's result; row_bcast:15 folds row 0 into row 1 and row 2 into row 3,
// row_bcast:31 folds lane 31 into rows 2-3; lane 63 holds the wave's result
__device__ __forceinline__ void dpp_argmin_wave(double& bv, int& bk) {
  dpp_argmin_stage<DPP_ROW_SHR1, 0xf>(bv, bk);
  dpp_argmin_stage<DPP_ROW_SHR2, 0xf>(bv, bk);
  dpp_argmin_stage<DPP_ROW_SHR4, 0xf>(bv, bk);
  dpp_argmin_stage<DPP_ROW_SHR8, 0xf>(bv, bk);
  dpp_argmin_stage<DPP_ROW_BCAST15, 0xa>(bv, bk);
  dpp_argmin_stage<DPP_ROW_BCAST31, 0xc>(bv, bk);
  bv = readlane_f64(bv, 63);
  bk = __builtin_amdgcn_readlane(bk, 63);
}
#endif  // DCG_SUBWAVE == 64

// broadcast lane `src`'s x to the subgroup; `src` is a lane index returned
// by wave_argmin_f64 (64-lane build: an SGPR, so this is one v_readlane)
__device__ __forceinline__ int sub_bcast_i32(int x, int src) {
#if DCG_SUBWAVE == 64
  return __builtin_amdgcn_readlane(x, src);
#else
  return __shfl(x, src, 64);
#endif
}

// mark a value the code keeps identical across the replica's lanes as
// wave-uniform (64-lane build only: in the 8-lane build it is uniform per
// subgroup, not per wave, and must stay a VGPR)
__device__ __forceinline__ int sub_uniform_i32(int x) {
#if DCG_SUBWAVE == 64
  return __builtin_amdgcn_readfirstlane(x);
#else
  return x;
#endif
}
// the same for a 64-bit value: two scalar halves
__device__ __forceinline__ long long sub_uniform_i64(long long x) {
#if DCG_SUBWAVE == 64
  unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)x);
  unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
#else
  return x;
#endif
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#if DCG_SUBWAVE == 64
  // lanes without a source add 0
  v += dpp_i32<DPP_ROW_SHR1, 0xf>(0, v);
  v += dpp_i32<DPP_ROW_SHR2, 0xf>(0, v);
  v += dpp_i32<DPP_ROW_SHR4, 0xf>(0, v);
  v += dpp_i32<DPP_ROW_SHR8, 0xf>(0, v);
  v += dpp_i32<DPP_ROW_BCAST15, 0xa>(0, v);
  v += dpp_i32<DPP_ROW_BCAST31, 0xc>(0, v);
  return __builtin_amdgcn_readlane(v, 63);
#else
#pragma unroll
  for (int off = SUBW / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
#endif
}

__device__ __forceinline__ double wave_min_f64(double v) {
#if DCG_SUBWAVE == 64
  v = fmin(v, dpp_f64<DPP_ROW_SHR1, 0xf>(v, v));
  v = fmin(v, dpp_f64<DPP_ROW_SHR2, 0xf>(v, v));
  v = fmin(v, dpp_f64<DPP_ROW_SHR4, 0xf>(v, v));
  v = fmin(v, dpp_f64<DPP_ROW_SHR8, 0xf>(v, v));
  v = fmin(v, dpp_f64<DPP_ROW_BCAST15, 0xa>(v, v));
  v = fmin(v, dpp_f64<DPP_ROW_BCAST31, 0xc>(v, v));
  return readlane_f64(v, 63);
#else
#pragma unroll
  for (int off = SUBW / 2; off > 0; off >>= 1)
    v = fmin(v, __shfl_xor(v, off, 64));
  return v;
#endif
}

// argmin with lowest-absolute-lane tie-break within the subgroup: returns the
// min value; lane_out = the winning lane's ABSOLUTE in-wave index (valid as
// a sub_bcast_i32 source for the subgroup).  Ties are `==` on the doubles.
__device__ __forceinline__ double wave_argmin_f64(double v, int& lane_out) {
  int lane = threadIdx.x & 63;
  double bv = v;
  int bl = lane;
#if DCG_SUBWAVE == 64
  dpp_argmin_wave(bv, bl);
#else
#pragma unroll
  for (int off = SUBW / 2; off > 0; off >>= 1) {
    double ov = __shfl_xor(bv, off, 64);
    int ol = __shfl_xor(bl, off, 64);
    if (ov < bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
  }
#endif
  lane_out = bl;
  return bv;
}

// generic (value, index) argmin: FIRST minimum in candidate-index order,
// matching the scalar engines' scan-order tie-break exactly.
__device__ __forceinline__ void wave_argmin_idx_f64(double v, int idx,
                                                    double& v_out, int& i_out) {
  double bv = v;
  int bi = idx;
#if DCG_SUBWAVE == 64
  dpp_argmin_wave(bv, bi);
#else
#pragma unroll
  for (int off = SUBW / 2; off > 0; off >>= 1) {
    double ov = __shfl_xor(bv, off, 64);
    int oi = __shfl_xor(bi, off, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
#endif
  v_out = bv;
  i_out = bi;
}

// lowest index k in [lo, hi) with row[k] >= D_INF (an empty slot), INT_MAX if
// none.  64-lane build: one ballot per 64-wide chunk and a find-first-set on
// the first non-zero mask; 8-lane build: per-lane first hit + butterfly min.
__device__ __forceinline__ int sub_first_empty(const double* row, int lo,
                                               int hi) {
#if DCG_SUBWAVE == 64
  int lane = threadIdx.x & 63;
  for (int k0 = lo; k0 < hi; k0 += 64) {
    int k = k0 + lane;
    // out-of-range lanes re-read the last valid element and vote "full"
    double f = row[min(k, hi - 1)];
    unsigned long long m = __ballot((k < hi) & (f >= D_INF));
    if (m) return k0 + __builtin_ctzll(m);
  }
  return INT_MAX;
#else
  int cand = INT_MAX;
  for (int k = lo + sub_lane(); k < hi; k += SUBW) {
    if (row[k] >= D_INF) { cand = k; break; }
  }
#pragma unroll
  for (int off = SUBW / 2; off > 0; off >>= 1)
    cand = min(cand, __shfl_xor(cand, off, 64));
  return cand;
#endif
}

// (n, f) grid argmin over n_max*n_freq candidates, candidate-strided over the
// subgroup's lanes; candidate index ci = (n-1)*n_freq + f_idx reproduces the
// scalar scan order (n-major, frequency-minor, first-minimum tie-break) of
// policies/gridsearch.py::best_nf_grid.
// objective: 0 energy, 1 carbon (score=E*ci), 2 cost (score=E/3.6e6*price).
//
// F is the type the candidates are RANKED in.  float is the opt-in fp32
// decision score (BASELINE config 5's "fp16/fp32 coeff eval"): only the
// ranking drops to fp32; the chosen (n, f) feeds the usual f64 time/energy
// models, so event times and energy integrals keep full precision.  A
// decision can differ from the f64 path only when two candidates score
// within fp32 rounding of each other (documented, measurable divergence —
// off by default).
struct GridPick { int n; double f, T, P, E; bool found; };

// "no candidate" score per ranking type, and the bound a found score is below
template <class F> struct ScoreLim;
template <> struct ScoreLim<double> {
  static constexpr double none = D_INF, found_below = D_INF;
};
template <> struct ScoreLim<float> {
  static constexpr float none = 3.0e38f;
  static constexpr double found_below = 3.0e38;
};

template <class F, class P3, class PF>
__device__ __forceinline__ GridPick wave_grid_argmin(
    P3 pc3, P3 lc3, PF freq_levels,
    int n_freq, int n_max, int objective, double ci, double price,
    bool has_ddl, double ddl) {
  int lane = sub_lane();
  int n_cand = n_max * n_freq;
  F best_sc = ScoreLim<F>::none;
  int best_ci = INT_MAX;
  for (int cand = lane; cand < n_cand; cand += SUBW) {
    int n = cand / n_freq + 1;
    F f = (F)freq_levels[cand % n_freq];
    F T = d_unit_time(n, f, lc3);
    F E = d_job_power(n, f, pc3) * T;
    if (has_ddl && T > (F)ddl) continue;
    F sc = E;
    if (objective == 1) sc = E * (F)ci;
    else if (objective == 2) sc = (E / (F)3.6e6) * (F)price;
    if (sc < best_sc) { best_sc = sc; best_ci = cand; }
  }
  double v;
  int wi;
  wave_argmin_idx_f64((double)best_sc, best_ci, v, wi);
  GridPick out;
  out.found = v < ScoreLim<F>::found_below;
  if (!out.found) {
    out.n = 1; out.f = 0; out.T = 0; out.P = 0; out.E = 0;
    return out;
  }
  // full-precision models on the CHOSEN candidate
  out.n = wi / n_freq + 1;
  out.f = freq_levels[wi % n_freq];
  out.T = d_unit_time(out.n, out.f, lc3);
  out.P = d_job_power(out.n, out.f, pc3);
  out.E = out.P * out.T;
  return out;
}

// energy-argmin over frequencies at fixed n (best_energy_freq),
// candidate-strided, first-minimum tie-break; ranked in F as above.
template <class F, class P3, class PF>
__device__ __forceinline__ double wave_energy_freq(
    P3 pc3, P3 lc3, PF freq_levels,
    int n_freq, int n) {
  int lane = sub_lane();
  F best_sc = ScoreLim<F>::none;
  int best_k = INT_MAX;
  for (int k = lane; k < n_freq; k += SUBW) {
    F f = (F)freq_levels[k];
    F sc = d_job_power(n, f, pc3) * d_unit_time(n, f, lc3);
    if (sc < best_sc) { best_sc = sc; best_k = k; }
  }
  double v;
  int wk;
  wave_argmin_idx_f64((double)best_sc, best_k, v, wk);
  return freq_levels[wk];
}

}  // namespace dcg
