// Test-only entry points of the replica-engine extensions: stand-alone
// drivers that run the production device functions (in-kernel actor forward,
// subgroup reductions, Philox draws, analytic models, grid searches) on given
// inputs, with their kernels, host wrappers and bindings.  Not a stand-alone
// header: replica_engine.hip includes it after the device code it drives.
#pragma once

namespace dcg {

// standalone batched actor forward (test/verification path): one subwave
// slot per observation row, same device math as the in-engine serving
__global__ void __launch_bounds__(THREADS_PER_BLOCK)
rl_forward_kernel(const float* pw, const float* obs, int B, int obs_dim,
                  int hid, int n_dc, int n_g, float* out_dc, float* out_g) {
  int slot = (blockIdx.x * blockDim.x + threadIdx.x) / SUBW;
  int lane = threadIdx.x & (SUBW - 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rb =
      reinterpret_cast<float*>(smem + (threadIdx.x / SUBW) * RL_LDS_BYTES);
  if (slot >= B) return;
  float* l_obs = rb;
  float* A = rb + RL_MAX_OBS;
  float* Bv = A + RL_MAX_HID;
  float* L = Bv + RL_MAX_HID;
  for (int k = lane; k < obs_dim; k += SUBW)
    l_obs[k] = obs[(int64_t)slot * obs_dim + k];
  lds_fence();
  rl_logits_impl(pw, obs_dim, hid, n_dc, n_g, l_obs, A, Bv, L, lane);
  for (int k = lane; k < n_dc; k += SUBW)
    out_dc[(int64_t)slot * n_dc + k] = L[k];
  for (int k = lane; k < n_g; k += SUBW)
    out_g[(int64_t)slot * n_g + k] = L[8 + k];
}

std::vector<torch::Tensor> rl_forward_debug(torch::Tensor pw,
                                            torch::Tensor obs,
                                            int64_t hid, int64_t n_dc,
                                            int64_t n_g) {
  TORCH_CHECK(pw.is_cuda() && obs.is_cuda() && pw.dtype() == torch::kFloat32);
  int B = obs.size(0), D = obs.size(1);
  auto out_dc = torch::empty({B, n_dc}, obs.options());
  auto out_g = torch::empty({B, n_g}, obs.options());
  int rpb = REPLICAS_PER_BLOCK;
  int blocks = (B + rpb - 1) / rpb;
  size_t shmem = (size_t)rpb * RL_LDS_BYTES;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(rl_forward_kernel, dim3(blocks), dim3(THREADS_PER_BLOCK),
                     shmem, stream, pw.data_ptr<float>(),
                     obs.data_ptr<float>(), B, D, (int)hid, (int)n_dc,
                     (int)n_g, out_dc.data_ptr<float>(),
                     out_g.data_ptr<float>());
  check_launch("rl_forward_kernel");
  return {out_dc, out_g};
}

// standalone drivers for the subgroup reduction helpers (test/verification
// path): one wavefront per row runs the production device functions
__global__ void __launch_bounds__(64)
wave_reduce_debug_kernel(const double* vals, const int* idx, double* v_lane,
                         int* o_lane, double* v_idx, int* o_idx) {
  int64_t row = blockIdx.x;
  int lane = threadIdx.x;
  double x = vals[row * 64 + lane];
  int ix = idx[row * 64 + lane];
  int wl;
  double a = wave_argmin_f64(x, wl);
  double b;
  int bi;
  wave_argmin_idx_f64(x, ix, b, bi);
  if (lane == 0) {
    v_lane[row] = a;
    o_lane[row] = wl;
    v_idx[row] = b;
    o_idx[row] = bi;
  }
}

std::vector<torch::Tensor> wave_reduce_debug(torch::Tensor vals,
                                             torch::Tensor idx) {
  TORCH_CHECK(SUBW == 64, "wave_reduce_debug drives the 64-lane reductions");
  TORCH_CHECK(vals.is_cuda() && idx.is_cuda() &&
              vals.dtype() == torch::kFloat64 && idx.dtype() == torch::kInt32);
  TORCH_CHECK(vals.dim() == 2 && vals.size(1) == 64 &&
              idx.sizes() == vals.sizes());
  vals = vals.contiguous();
  idx = idx.contiguous();
  int64_t B = vals.size(0);
  auto v_lane = torch::empty({B}, vals.options());
  auto o_lane = torch::empty({B}, idx.options());
  auto v_idx = torch::empty({B}, vals.options());
  auto o_idx = torch::empty({B}, idx.options());
  if (B == 0) return {v_lane, o_lane, v_idx, o_idx};
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(wave_reduce_debug_kernel, dim3((unsigned)B), dim3(64), 0,
                     stream, vals.data_ptr<double>(), idx.data_ptr<int>(),
                     v_lane.data_ptr<double>(), o_lane.data_ptr<int>(),
                     v_idx.data_ptr<double>(), o_idx.data_ptr<int>());
  check_launch("wave_reduce_debug_kernel");
  return {v_lane, o_lane, v_idx, o_idx};
}

__global__ void __launch_bounds__(64)
first_empty_debug_kernel(const double* rows, int L, int* out) {
  int64_t row = blockIdx.x;
  int k = sub_first_empty(rows + row * L, 0, L);
  if (threadIdx.x == 0) out[row] = k;
}

torch::Tensor first_empty_debug(torch::Tensor rows) {
  TORCH_CHECK(rows.is_cuda() && rows.dtype() == torch::kFloat64 &&
              rows.dim() == 2 && rows.size(1) >= 1 &&
              rows.size(1) < (1 << 30));
  rows = rows.contiguous();
  int64_t B = rows.size(0);
  auto out = torch::empty({B}, rows.options().dtype(torch::kInt32));
  if (B == 0) return out;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(first_empty_debug_kernel, dim3((unsigned)B), dim3(64), 0,
                     stream, rows.data_ptr<double>(), (int)rows.size(1),
                     out.data_ptr<int>());
  check_launch("first_empty_debug_kernel");
  return out;
}

// standalone drivers for the RNG (philox.hpp) and the analytic models / grid
// searches (sim_models.hpp), same test/verification path.  The RNG and model
// drivers run one thread per row; the grid drivers one 64-thread block per
// row (8-lane build: every subgroup solves the same row, subgroup 0 writes).
constexpr int RNG_DRAW_COLS = 7;  // u01, u01x2 a, u01x2 b, rexp, rnormal,
                                  // rlognormal, rpareto_inf
constexpr int RNG_CTR_COLS = 7;   // u01, u01x2, rexp, rbelow, rnormal,
                                  // rlognormal, rpareto_inf

__global__ void __launch_bounds__(64)
philox_debug_kernel(const int64_t* keys, const int64_t* ctrs, int64_t B,
                    int64_t* words) {
  int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  uint32_t w[4];
  philox4x32((uint64_t)keys[row], (uint64_t)ctrs[row], w);
  for (int k = 0; k < 4; ++k) words[row * 4 + k] = (int64_t)w[k];
}

torch::Tensor philox_debug(torch::Tensor keys, torch::Tensor ctrs) {
  TORCH_CHECK(keys.is_cuda() && ctrs.is_cuda() &&
              keys.dtype() == torch::kInt64 && ctrs.dtype() == torch::kInt64);
  TORCH_CHECK(keys.dim() == 1 && ctrs.sizes() == keys.sizes());
  keys = keys.contiguous();
  ctrs = ctrs.contiguous();
  int64_t B = keys.size(0);
  auto words = torch::empty({B, 4}, keys.options());
  if (B == 0) return words;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(philox_debug_kernel, dim3((unsigned)((B + 63) / 64)),
                     dim3(64), 0, stream, keys.data_ptr<int64_t>(),
                     ctrs.data_ptr<int64_t>(), B, words.data_ptr<int64_t>());
  check_launch("philox_debug_kernel");
  return words;
}

// every production draw from a fresh state at (key, ctr): the value and the
// counter the draw leaves behind
__global__ void __launch_bounds__(64)
rng_draws_debug_kernel(const int64_t* keys, const int64_t* ctrs,
                       const int64_t* n_below, int64_t B, double lambd,
                       double mu, double sigma, double* vals, int64_t* below,
                       int64_t* ctr_after) {
  int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  double* v = vals + row * RNG_DRAW_COLS;
  int64_t* ca = ctr_after + row * RNG_CTR_COLS;
  auto fresh = [&]() {
    return PhiloxState{(uint64_t)keys[row], (uint64_t)ctrs[row]};
  };
  PhiloxState st = fresh();
  v[0] = u01(st);
  ca[0] = (int64_t)st.ctr;
  st = fresh();
  u01x2(st, v[1], v[2]);
  ca[1] = (int64_t)st.ctr;
  st = fresh();
  v[3] = rexp(st, lambd);
  ca[2] = (int64_t)st.ctr;
  st = fresh();
  below[row] = (int64_t)rbelow(st, (uint32_t)n_below[row]);
  ca[3] = (int64_t)st.ctr;
  st = fresh();
  v[4] = rnormal(st, mu, sigma);
  ca[4] = (int64_t)st.ctr;
  st = fresh();
  v[5] = rlognormal(st, mu, sigma);
  ca[5] = (int64_t)st.ctr;
  st = fresh();
  v[6] = rpareto_inf(st);
  ca[6] = (int64_t)st.ctr;
}

std::vector<torch::Tensor> rng_draws_debug(torch::Tensor keys,
                                           torch::Tensor ctrs,
                                           torch::Tensor n_below, double lambd,
                                           double mu, double sigma) {
  TORCH_CHECK(keys.is_cuda() && ctrs.is_cuda() && n_below.is_cuda() &&
              keys.dtype() == torch::kInt64 && ctrs.dtype() == torch::kInt64 &&
              n_below.dtype() == torch::kInt64);
  TORCH_CHECK(keys.dim() == 1 && ctrs.sizes() == keys.sizes() &&
              n_below.sizes() == keys.sizes());
  keys = keys.contiguous();
  ctrs = ctrs.contiguous();
  n_below = n_below.contiguous();
  int64_t B = keys.size(0);
  auto vals = torch::empty({B, RNG_DRAW_COLS},
                           keys.options().dtype(torch::kFloat64));
  auto below = torch::empty({B}, keys.options());
  auto ctr_after = torch::empty({B, RNG_CTR_COLS}, keys.options());
  if (B == 0) return {vals, below, ctr_after};
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(rng_draws_debug_kernel, dim3((unsigned)((B + 63) / 64)),
                     dim3(64), 0, stream, keys.data_ptr<int64_t>(),
                     ctrs.data_ptr<int64_t>(), n_below.data_ptr<int64_t>(), B,
                     lambd, mu, sigma, vals.data_ptr<double>(),
                     below.data_ptr<int64_t>(), ctr_after.data_ptr<int64_t>());
  check_launch("rng_draws_debug_kernel");
  return {vals, below, ctr_after};
}

// the word -> value halves of the same recipes at given words
__global__ void __launch_bounds__(64)
rng_maps_debug_kernel(const int64_t* words, const int64_t* n_below, int64_t B,
                      double lambd, double mu, double sigma, double* vals,
                      int64_t* below) {
  int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  uint32_t w[4];
  for (int k = 0; k < 4; ++k) w[k] = (uint32_t)words[row * 4 + k];
  double* v = vals + row * RNG_DRAW_COLS;
  double ua = u01_map(w[0], w[1]), ub = u01_map(w[2], w[3]);
  v[0] = ua;
  v[1] = ua;
  v[2] = ub;
  v[3] = rexp_map(ua, lambd);
  v[4] = rnormal_map(ua, ub, mu, sigma);
  v[5] = rlognormal_map(ua, ub, mu, sigma);
  v[6] = rpareto_inf_map(ua);
  below[row] = (int64_t)rbelow_map(w[0], (uint32_t)n_below[row]);
}

std::vector<torch::Tensor> rng_maps_debug(torch::Tensor words,
                                          torch::Tensor n_below, double lambd,
                                          double mu, double sigma) {
  TORCH_CHECK(words.is_cuda() && n_below.is_cuda() &&
              words.dtype() == torch::kInt64 &&
              n_below.dtype() == torch::kInt64);
  TORCH_CHECK(words.dim() == 2 && words.size(1) == 4 && n_below.dim() == 1 &&
              n_below.size(0) == words.size(0));
  words = words.contiguous();
  n_below = n_below.contiguous();
  int64_t B = words.size(0);
  auto vals = torch::empty({B, RNG_DRAW_COLS},
                           words.options().dtype(torch::kFloat64));
  auto below = torch::empty({B}, words.options());
  if (B == 0) return {vals, below};
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(rng_maps_debug_kernel, dim3((unsigned)((B + 63) / 64)),
                     dim3(64), 0, stream, words.data_ptr<int64_t>(),
                     n_below.data_ptr<int64_t>(), B, lambd, mu, sigma,
                     vals.data_ptr<double>(), below.data_ptr<int64_t>());
  check_launch("rng_maps_debug_kernel");
  return {vals, below};
}

__global__ void __launch_bounds__(64)
models_debug_kernel(const double* pc, const double* lc, const int* n,
                    const double* f, int64_t B, double* P, double* T) {
  int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  P[row] = d_job_power<double>(n[row], f[row], pc + row * 3);
  T[row] = d_unit_time<double>(n[row], f[row], lc + row * 3);
}

// (pc, lc) coefficient rows as the model drivers take them: f64[B,3] on the
// GPU, bounded so that no score can reach the searches' "no candidate" value
static void check_coeff_rows(const torch::Tensor& pc, const torch::Tensor& lc) {
  TORCH_CHECK(pc.is_cuda() && lc.is_cuda() && pc.dtype() == torch::kFloat64 &&
              lc.dtype() == torch::kFloat64);
  TORCH_CHECK(pc.dim() == 2 && pc.size(1) == 3 && lc.sizes() == pc.sizes());
  TORCH_CHECK(pc.numel() == 0 ||
                  ((pc.abs() <= 1e6).all().item<bool>() &&
                   (lc.abs() <= 1e6).all().item<bool>()),
              "coefficients must be finite and within +-1e6");
}
static void check_freq_ladder(const torch::Tensor& freq) {
  TORCH_CHECK(freq.is_cuda() && freq.dtype() == torch::kFloat64 &&
              freq.dim() == 1 && freq.size(0) >= 1 && freq.size(0) <= 4096);
  TORCH_CHECK((freq.abs() <= 1e3).all().item<bool>(),
              "frequencies must be finite and within +-1e3");
}

std::vector<torch::Tensor> models_debug(torch::Tensor pc, torch::Tensor lc,
                                        torch::Tensor n, torch::Tensor f) {
  check_coeff_rows(pc, lc);
  int64_t B = pc.size(0);
  TORCH_CHECK(n.is_cuda() && f.is_cuda() && n.dtype() == torch::kInt32 &&
              f.dtype() == torch::kFloat64 && n.dim() == 1 && f.dim() == 1 &&
              n.size(0) == B && f.size(0) == B);
  pc = pc.contiguous();
  lc = lc.contiguous();
  n = n.contiguous();
  f = f.contiguous();
  auto P = torch::empty({B}, f.options());
  auto T = torch::empty({B}, f.options());
  if (B == 0) return {P, T};
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(models_debug_kernel, dim3((unsigned)((B + 63) / 64)),
                     dim3(64), 0, stream, pc.data_ptr<double>(),
                     lc.data_ptr<double>(), n.data_ptr<int>(),
                     f.data_ptr<double>(), B, P.data_ptr<double>(),
                     T.data_ptr<double>());
  check_launch("models_debug_kernel");
  return {P, T};
}

template <class F>
__global__ void __launch_bounds__(64)
grid_argmin_debug_kernel(const double* pc, const double* lc,
                         const double* freq, int n_freq, int n_max,
                         int objective, const double* ci, const double* price,
                         bool has_ddl, const double* ddl, int* found, int* n,
                         double* f, double* T, double* P, double* E) {
  int64_t row = blockIdx.x;
  GridPick g = wave_grid_argmin<F>(pc + row * 3, lc + row * 3, freq, n_freq,
                                   n_max, objective, ci[row], price[row],
                                   has_ddl, ddl[row]);
  if (threadIdx.x == 0) {
    found[row] = g.found ? 1 : 0;
    n[row] = g.n;
    f[row] = g.f;
    T[row] = g.T;
    P[row] = g.P;
    E[row] = g.E;
  }
}

std::vector<torch::Tensor> grid_argmin_debug(
    torch::Tensor pc, torch::Tensor lc, torch::Tensor freq, int64_t n_max,
    int64_t objective, torch::Tensor ci, torch::Tensor price, bool has_ddl,
    torch::Tensor ddl, bool fp32) {
  check_coeff_rows(pc, lc);
  check_freq_ladder(freq);
  int64_t B = pc.size(0);
  TORCH_CHECK(n_max >= 1 && n_max <= 4096 && objective >= 0 && objective <= 2);
  for (const torch::Tensor* t : {&ci, &price, &ddl})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kFloat64 &&
                t->dim() == 1 && t->size(0) == B);
  TORCH_CHECK(B == 0 || ((ci.abs() <= 1e3).all().item<bool>() &&
                         (price.abs() <= 1e3).all().item<bool>()),
              "ci and price must be finite and within +-1e3");
  pc = pc.contiguous();
  lc = lc.contiguous();
  freq = freq.contiguous();
  ci = ci.contiguous();
  price = price.contiguous();
  ddl = ddl.contiguous();
  auto i32 = pc.options().dtype(torch::kInt32);
  auto found = torch::empty({B}, i32);
  auto n = torch::empty({B}, i32);
  auto f = torch::empty({B}, pc.options());
  auto T = torch::empty({B}, pc.options());
  auto P = torch::empty({B}, pc.options());
  auto E = torch::empty({B}, pc.options());
  if (B == 0) return {found, n, f, T, P, E};
  hipStream_t stream = at::hip::getCurrentHIPStream();
  auto kern = fp32 ? grid_argmin_debug_kernel<float>
                   : grid_argmin_debug_kernel<double>;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), 0, stream,
                     pc.data_ptr<double>(), lc.data_ptr<double>(),
                     freq.data_ptr<double>(), (int)freq.size(0), (int)n_max,
                     (int)objective, ci.data_ptr<double>(),
                     price.data_ptr<double>(), has_ddl, ddl.data_ptr<double>(),
                     found.data_ptr<int>(), n.data_ptr<int>(),
                     f.data_ptr<double>(), T.data_ptr<double>(),
                     P.data_ptr<double>(), E.data_ptr<double>());
  check_launch("grid_argmin_debug_kernel");
  return {found, n, f, T, P, E};
}

template <class F>
__global__ void __launch_bounds__(64)
energy_freq_debug_kernel(const double* pc, const double* lc,
                         const double* freq, int n_freq, const int* n,
                         double* f) {
  int64_t row = blockIdx.x;
  double best = wave_energy_freq<F>(pc + row * 3, lc + row * 3, freq, n_freq,
                                    n[row]);
  if (threadIdx.x == 0) f[row] = best;
}

torch::Tensor energy_freq_debug(torch::Tensor pc, torch::Tensor lc,
                                torch::Tensor freq, torch::Tensor n,
                                bool fp32) {
  check_coeff_rows(pc, lc);
  check_freq_ladder(freq);
  int64_t B = pc.size(0);
  TORCH_CHECK(n.is_cuda() && n.dtype() == torch::kInt32 && n.dim() == 1 &&
              n.size(0) == B);
  TORCH_CHECK(B == 0 || (n.abs() <= 4096).all().item<bool>());
  pc = pc.contiguous();
  lc = lc.contiguous();
  freq = freq.contiguous();
  n = n.contiguous();
  auto f = torch::empty({B}, pc.options());
  if (B == 0) return f;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  auto kern = fp32 ? energy_freq_debug_kernel<float>
                   : energy_freq_debug_kernel<double>;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), 0, stream,
                     pc.data_ptr<double>(), lc.data_ptr<double>(),
                     freq.data_ptr<double>(), (int)freq.size(0),
                     n.data_ptr<int>(), f.data_ptr<double>());
  check_launch("energy_freq_debug_kernel");
  return f;
}

#if DCG_SUBWAVE == 64
// standalone driver for the rate-profile inversion (arrival_ring.hpp): one
// 8-lane group per row runs the production profile_gap on (E, t) through the
// row's stream of the table, as the generator's groups do
__global__ void __launch_bounds__(PG_THREADS)
profile_gap_debug_kernel(const double* E, const double* t, const int* stream,
                         int64_t B, double rate, double period,
                         const double* tab, double* out) {
  const int64_t row = ((int64_t)blockIdx.x * PG_THREADS + threadIdx.x) /
                      PG_GROUP;
  const int gl = threadIdx.x & (PG_GROUP - 1);
  const int lane64 = threadIdx.x & 63;
  if (row >= B) return;  // whole groups leave together
  const double g = profile_gap(E[row], t[row], rate, period,
                               tab + (int64_t)stream[row] * PROF_W, gl,
                               lane64);
  if (gl == 0) out[row] = g;
}

torch::Tensor profile_gap_debug(torch::Tensor E, torch::Tensor t,
                                torch::Tensor stream, double rate,
                                double period, torch::Tensor tab) {
  TORCH_CHECK(E.is_cuda() && t.is_cuda() && stream.is_cuda() &&
              tab.is_cuda() && E.dtype() == torch::kFloat64 &&
              t.dtype() == torch::kFloat64 &&
              stream.dtype() == torch::kInt32 &&
              tab.dtype() == torch::kFloat64);
  TORCH_CHECK(E.dim() == 1 && t.sizes() == E.sizes() &&
              stream.sizes() == E.sizes());
  TORCH_CHECK(tab.dim() == 2 && tab.size(1) == PROF_W && tab.size(0) >= 1,
              "tab must be [n_streams][", PROF_W, "]");
  E = E.contiguous();
  t = t.contiguous();
  stream = stream.contiguous();
  tab = tab.contiguous();
  int64_t B = E.size(0);
  auto out = torch::empty({B}, E.options());
  if (B == 0) return out;
  TORCH_CHECK(B < (1 << 24));
  TORCH_CHECK((stream >= 0).all().item<bool>() &&
                  (stream < tab.size(0)).all().item<bool>(),
              "stream outside [0, n_streams)");
  auto Kcol = tab.select(1, 0);
  TORCH_CHECK((Kcol >= 0).all().item<bool>() &&
                  (Kcol <= PROF_MAX_SEG).all().item<bool>(),
              "K outside [0, ", PROF_MAX_SEG, "]");
  hipStream_t hs = at::hip::getCurrentHIPStream();
  const int64_t per_block = PG_THREADS / PG_GROUP;
  hipLaunchKernelGGL(profile_gap_debug_kernel,
                     dim3((unsigned)((B + per_block - 1) / per_block)),
                     dim3(PG_THREADS), 0, hs, E.data_ptr<double>(),
                     t.data_ptr<double>(), stream.data_ptr<int>(), B, rate,
                     period, tab.data_ptr<double>(), out.data_ptr<double>());
  check_launch("profile_gap_debug_kernel");
  return out;
}
#endif  // DCG_SUBWAVE == 64

inline void bind_debug_entries(py::module_& m) {
#if DCG_SUBWAVE == 64
  m.def("profile_gap_debug", &dcg::profile_gap_debug,
        "production profile_gap, one 8-lane group per row of (E[B] f64, "
        "t[B] f64, stream[B] i32) through tab[n_streams, PROF_W] -> gap[B]",
        py::arg("E"), py::arg("t"), py::arg("stream"), py::arg("rate"),
        py::arg("period"), py::arg("tab"));
#endif
  m.def("rl_forward_debug", &dcg::rl_forward_debug,
        "batched actor forward via the in-kernel serving math "
        "(pw, obs[B,D], hid, n_dc, n_g) -> (logits_dc, logits_g)",
        py::arg("pw"), py::arg("obs"), py::arg("hid"), py::arg("n_dc"),
        py::arg("n_g"));
  m.def("wave_reduce_debug", &dcg::wave_reduce_debug,
        "production wave_argmin_f64 / wave_argmin_idx_f64 over each row of "
        "(vals[B,64] f64, idx[B,64] i32) -> (value, lane, value, index)",
        py::arg("vals"), py::arg("idx"));
  m.def("first_empty_debug", &dcg::first_empty_debug,
        "production first-empty-slot search over each row of rows[B,L] f64 "
        "-> lowest k with rows[k] >= 1e300, INT_MAX if none",
        py::arg("rows"));
  m.def("philox_debug", &dcg::philox_debug,
        "production philox4x32 per row of (keys[B] i64, ctrs[B] i64) -> "
        "words[B,4] i64",
        py::arg("keys"), py::arg("ctrs"));
  m.def("rng_draws_debug", &dcg::rng_draws_debug,
        "every production draw from a fresh state at (keys[B], ctrs[B]) -> "
        "(vals[B,7] f64 = u01, u01x2 a, u01x2 b, rexp, rnormal, rlognormal, "
        "rpareto_inf; rbelow[B] i64; ctr_after[B,7] i64 = u01, u01x2, rexp, "
        "rbelow, rnormal, rlognormal, rpareto_inf)",
        py::arg("keys"), py::arg("ctrs"), py::arg("n_below"),
        py::arg("lambd"), py::arg("mu"), py::arg("sigma"));
  m.def("rng_maps_debug", &dcg::rng_maps_debug,
        "the word -> value halves of the draws at words[B,4] i64 -> "
        "(vals[B,7] f64 as rng_draws_debug, rbelow[B] i64)",
        py::arg("words"), py::arg("n_below"), py::arg("lambd"),
        py::arg("mu"), py::arg("sigma"));
  m.def("models_debug", &dcg::models_debug,
        "production d_job_power<double> / d_unit_time<double> per row of "
        "(pc[B,3], lc[B,3], n[B] i32, f[B]) -> (P, T)",
        py::arg("pc"), py::arg("lc"), py::arg("n"), py::arg("f"));
  m.def("grid_argmin_debug", &dcg::grid_argmin_debug,
        "production wave_grid_argmin, one 64-thread block per row -> "
        "(found i32, n i32, f, T, P, E)",
        py::arg("pc"), py::arg("lc"), py::arg("freq"), py::arg("n_max"),
        py::arg("objective"), py::arg("ci"), py::arg("price"),
        py::arg("has_ddl"), py::arg("ddl"), py::arg("fp32"));
  m.def("energy_freq_debug", &dcg::energy_freq_debug,
        "production wave_energy_freq, one 64-thread block per row -> f[B]",
        py::arg("pc"), py::arg("lc"), py::arg("freq"), py::arg("n"),
        py::arg("fp32"));
}

}  // namespace dcg
