// Fused kernels for the SAC critic phase (gfx950): the whole TD-target chain
// in one kernel, and the twin quantile-Huber loss with its gradient in one
// pass.  Opt-in (rl/fused.py); the torch path in rl/sac.py is the
// specification of both.
//
// sac_td_target_kernel
// --------------------
//   target = r_eff + (1 - done) * gamma *
//            (min(Q1', Q2')(h', a') - alpha * logp(a'))
// with h' = encoder(s_next), a' ~ masked Gumbel-max over the two actor heads
// and Q' the twin target critic: 13 linear layers, all fp32 on
// v_mfma_f32_16x16x4_f32 (exact f32 products and sums).
//
// Work split.  One workgroup of 16 waves owns TD_ROWS = 16 batch rows; wave w
// owns the output columns [16 w, 16 w + 16) of every layer, so one MFMA
// accumulator (4 VGPRs) is a wave's whole result.  16 rows rather than 32:
// the production batch of 256 then fills 16 CUs instead of 8, and the chain
// is latency-bound (13 dependent layers) — the 2.4 MB of weights are read
// from L2 by every workgroup either way, and halving that traffic buys less
// than halving the number of CUs that share the latency costs.
//
// Weights are read where nn.Linear keeps them, W[out][in] row-major, through
// the parameters' own pointers: no packed or transposed copy.  A lane
// (j = lane & 15, q = lane >> 4) loads the 16 bytes W[j][k0 + 4q .. k0 + 4q + 3]
// and feeds them to four consecutive MFMAs; MFMA t of the group therefore
// multiplies logical k = k0 + 4q + t in its k slot q.  The A fragment is read
// from LDS with the same permutation — one 16-byte read X[i][k0 + 4q ..] per
// four MFMAs — and the sum over k does not care about the order.  A weight
// matrix whose rows are not 16-byte aligned (the first layer: obs_dim is
// arbitrary) takes clamped scalar loads into the same register layout.  A
// wave fetches its whole slice of a layer (<= 16 x 16 B per lane) in one
// burst, one layer ahead: before the barrier that ends the previous layer.
//
// LDS plan (TD_STRIDE = 260 floats per row: 16-byte aligned rows, and the
// 16 rows of a fragment read spread over the banks):
//   bufA, bufB  ping-pong activations          2 x 16 x 260 x 4 B
//   bufH        the latent h', live from the encoder's last layer through
//               both actor heads and both critics      16 x 260 x 4 B
//   per-row action, log-prob                            ~0.3 KB
// The two actor output layers run side by side (wave 0: dc, wave 1: g); the
// logits never leave the accumulator: a row's 16 columns sit in the 16 lanes
// of one quarter-wave, so log-softmax, the Gumbel scores and the argmax are
// xor-shuffles inside that quarter.  The critics' first layer multiplies only
// the latent part of its input; the one-hot part is W[:, latent + a_dc] +
// W[:, latent + n_dc + a_g], added per row in the epilogue.  Q1' stays in
// registers while Q2' is computed: the same lane holds the same (row,
// quantile) of both.
//
// qr_huber_twin_kernel
// --------------------
// One wave per sample; a lane owns one (critic, predicted quantile) pair and
// loops over the N target quantiles in LDS, accumulating the loss and the
// closed-form gradient (pinball held constant) in registers.  The scalar loss
// is folded in a fixed order — lane sum, shuffle tree, waves in order,
// per-block partials, one final single-wave pass — in f64 and without float
// atomics, so it is bitwise reproducible.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <vector>

#include "moments.hpp"

namespace dcg {

constexpr int TD_ROWS = 16;
constexpr int TD_WAVES = 16;
constexpr int TD_THREADS = TD_WAVES * 64;
constexpr int TD_MAXW = 256;       // widest layer
constexpr int TD_STRIDE = 260;     // LDS floats per activation row
constexpr int TD_MAX_ACT = 16;     // actor head width limit (one column tile)
constexpr int TD_MAX_Q = 64;       // quantile limit (four column tiles)
constexpr int TD_LINEARS = 13;

// scalar f32 VALU ops only in these kernels (no packed-f32 forms): every
// product and sum outside the MFMAs is the plain f32 op the torch path does
#if defined(__HIP_DEVICE_COMPILE__)
#define TD_FN __attribute__((target("no-packed-fp32-ops")))
#else
#define TD_FN
#endif

using td_acc = __attribute__((ext_vector_type(4))) float;
using td_f4 = __attribute__((ext_vector_type(4))) float;

// the few cross-lane and barrier primitives these kernels use, on the
// builtins: functions that carry TD_FN cannot inline the HIP header's
// wrappers, which are compiled for the default feature set
TD_FN __device__ __forceinline__ int td_lane_read(int v, int src_lane) {
  return __builtin_amdgcn_ds_bpermute(src_lane << 2, v);
}
TD_FN __device__ __forceinline__ float td_lane_read(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}
TD_FN __device__ __forceinline__ double td_lane_read(double v, int src_lane) {
  using i2 = __attribute__((ext_vector_type(2))) int;
  i2 x = __builtin_bit_cast(i2, v);
  x[0] = __builtin_amdgcn_ds_bpermute(src_lane << 2, x[0]);
  x[1] = __builtin_amdgcn_ds_bpermute(src_lane << 2, x[1]);
  return __builtin_bit_cast(double, x);
}
// sum over the wave, valid in lane 0; fixed order (the __shfl_down tree)
TD_FN __device__ __forceinline__ double td_wave_sum(double v, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += td_lane_read(v, (lane + off) & 63);
  return v;
}
TD_FN __device__ __forceinline__ void td_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct TdLinear {
  const float* w;  // [out][ld]
  const float* b;  // [out]
};

struct TdArgs {
  TdLinear lin[TD_LINEARS];  // enc x3, head_dc x2, head_g x2, q1 x3, q2 x3
  const float* s_next;       // [B][obs_dim]
  const bool* mask_dc;       // [B][n_dc] or nullptr
  const bool* mask_g;        // [B][n_g] or nullptr
  const float* u_dc;         // [B][n_dc]
  const float* u_g;          // [B][n_g]
  const float* r_eff;        // [B]
  const float* done;         // [B]
  const float* log_alpha;    // scalar, on the device
  float gamma;
  int B, obs_dim, hid, n_dc, n_g, nq;
  float* target;             // [B][nq]
  int64_t* a_dc;             // [B]
  int64_t* a_g;              // [B]
  float* logp;               // [B]
};

// One wave's slice of a weight matrix, in registers: the 16 rows of column
// tile `tile`, all of k (<= 256), as up to 16 x 16 bytes per lane.  Fetched in
// one burst, and for the NEXT layer before the barrier that ends the current
// one: weights do not depend on activations, so their L2 latency hides behind
// the epilogue and the barrier wait instead of heading every layer.
struct TdW {
  td_f4 v[TD_MAXW / 16];
};

struct TdLayer {
  const float* w;  // [out][ld]
  int ld, in, out, tile;
};

// columns >= out read a clamped row of W and are discarded by the caller; a
// matrix whose rows are not 16-byte aligned, or whose k has a tail, takes
// scalar loads into the same register layout
TD_FN __device__ __forceinline__ void td_fetch(TdW& R, const TdLayer& L,
                                               int lane) {
  if (L.tile * 16 >= L.out) return;
  const int q = lane >> 4;
  const int j = min(L.tile * 16 + (lane & 15), L.out - 1);
  const float* wrow = L.w + (int64_t)j * L.ld + 4 * q;
  const bool vec = ((L.ld & 3) == 0) && ((L.in & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(L.w) & 15) == 0);
  if (vec) {
#pragma unroll
    for (int c = 0; c < TD_MAXW / 16; ++c)
      if (c * 16 < L.in)
        R.v[c] = *reinterpret_cast<const td_f4*>(wrow + c * 16);
  } else {
    // every load is in bounds (k clamped to the row), the tail is selected
    // to zero afterwards: no branch per element
    const float* w0 = L.w + (int64_t)j * L.ld;
#pragma unroll
    for (int c = 0; c < TD_MAXW / 16; ++c)
      if (c * 16 < L.in) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = c * 16 + 4 * q + t;
          const float x = w0[min(k, L.in - 1)];
          R.v[c][t] = k < L.in ? x : 0.0f;
        }
      }
  }
}

// acc[r] = sum_k X[row(r)][k] * W[col][k], row(r) = 4 (lane >> 4) + r; X is
// zero past `in` up to the next multiple of 16
TD_FN __device__ __forceinline__ td_acc td_mma(const TdW& R, int in,
                                               const float* X, int lane) {
  td_acc acc = {0.f, 0.f, 0.f, 0.f};
  const float* xrow = X + (lane & 15) * TD_STRIDE + 4 * (lane >> 4);
  // the A fragment is read one chunk ahead of its MFMAs and no further: a
  // scheduler free to hoist all 16 reads would need 64 more registers
  td_f4 a = *reinterpret_cast<const td_f4*>(xrow);
#pragma unroll
  for (int c = 0; c < TD_MAXW / 16; ++c)
    if (c * 16 < in) {
      td_f4 an = a;
      if ((c + 1) * 16 < in)
        an = *reinterpret_cast<const td_f4*>(xrow + (c + 1) * 16);
      const td_f4 w = R.v[c];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], w[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], w[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], w[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], w[3], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      a = an;
    }
  return acc;
}

// Y = relu(X W^T + b) for a hidden layer (out == hid) whose weights are in R;
// then R <- the next layer's weights, the epilogue, and a barrier.
// ONEHOT: W is a critic's first layer [hid][in + n_dc + n_g]; the one-hot part
// of its input is the two selected columns, added per row.
template <bool ONEHOT>
TD_FN __device__ __forceinline__ void td_hidden(
    TdW& R, const TdLayer& L, const float* bias, const TdLayer& next,
    const float* X, float* Y, int lane, int n_dc, const int* s_adc,
    const int* s_ag) {
  const bool active = L.tile * 16 < L.out;
  td_acc acc = {0.f, 0.f, 0.f, 0.f};
  if (active) acc = td_mma(R, L.in, X, lane);
  td_fetch(R, next, lane);
  if (active) {
    const int j = L.tile * 16 + (lane & 15);  // out % 16 == 0: always a column
    const float bj = bias[j];
    const float* wrow = L.w + (int64_t)j * L.ld + L.in;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
      float y = acc[r] + bj;
      if (ONEHOT) y += wrow[s_adc[row]] + wrow[n_dc + s_ag[row]];
      Y[row * TD_STRIDE + j] = fmaxf(y, 0.0f);
    }
  }
  td_barrier();
}

// One actor head's sampling, by the wave whose accumulator holds its logits:
// masked log-softmax, Gumbel scores, argmax (lowest index wins ties) and the
// chosen log-prob, per row, inside each quarter-wave.
TD_FN __device__ __forceinline__ void td_sample(td_acc acc, const float* bias, int n,
                                          const bool* mask, const float* u,
                                          int row0, int rows, int lane,
                                          int* s_a, float* s_lp) {
  const int j = lane & 15;
  const bool col = j < n;
  const float bj = col ? bias[j] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = (lane >> 4) * 4 + r;
    const bool live = col && row < rows;
    const int64_t g = (int64_t)(row0 + row) * n + j;
    float x = acc[r] + bj;
    if (live && mask != nullptr && !mask[g]) x = -FLT_MAX;  // finfo.min
    const float xm = col ? x : -INFINITY;
    float m = xm;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, td_lane_read(m, lane ^ off));
    float s = col ? expf(x - m) : 0.0f;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) s += td_lane_read(s, lane ^ off);
    const float lp = x - m - logf(s);
    const float uu = live ? u[g] : 0.5f;
    const float gum = -logf(-logf(fmaxf(uu, 1e-20f)));
    float best = col ? lp + gum : -INFINITY;
    int arg = j;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const float ob = td_lane_read(best, lane ^ off);
      const int oa = td_lane_read(arg, lane ^ off);
      if (ob > best || (ob == best && oa < arg)) {
        best = ob;
        arg = oa;
      }
    }
    arg = min(arg, n - 1);  // only a row of NaNs could leave the head
    const float lp_a = td_lane_read(lp, (lane & 48) + arg);
    if (j == 0) {
      s_a[row] = arg;
      s_lp[row] = lp_a;
    }
  }
}

TD_FN __global__ void __launch_bounds__(TD_THREADS)
sac_td_target_kernel(TdArgs A) {
  __shared__ __attribute__((aligned(16))) float bufA[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufB[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufH[TD_ROWS * TD_STRIDE];
  __shared__ int s_adc[TD_ROWS], s_ag[TD_ROWS];
  __shared__ float s_lpdc[TD_ROWS], s_lpg[TD_ROWS];
  // the wave index in an SGPR: every branch on it is a scalar branch
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * TD_ROWS;
  const int rows = min(TD_ROWS, A.B - row0);
  const int H = A.hid, D = A.obs_dim;

  const int ldc = H + A.n_dc + A.n_g;
  const TdLayer enc0 = {A.lin[0].w, D, D, H, wave};
  const TdLayer enc1 = {A.lin[1].w, H, H, H, wave};
  const TdLayer enc2 = {A.lin[2].w, H, H, H, wave};
  const TdLayer dc0 = {A.lin[3].w, H, H, H, wave};
  const TdLayer g0 = {A.lin[5].w, H, H, H, wave};
  const TdLayer dc1 = {A.lin[4].w, H, H, A.n_dc, 0};
  const TdLayer g1 = {A.lin[6].w, H, H, A.n_g, 0};
  const TdLayer c10 = {A.lin[7].w, ldc, H, H, wave};
  const TdLayer c11 = {A.lin[8].w, H, H, H, wave};
  const TdLayer c12 = {A.lin[9].w, H, H, A.nq, wave};
  const TdLayer c20 = {A.lin[10].w, ldc, H, H, wave};
  const TdLayer c21 = {A.lin[11].w, H, H, H, wave};
  const TdLayer c22 = {A.lin[12].w, H, H, A.nq, wave};
  TdW R;
  td_fetch(R, enc0, lane);

  // stage the s_next tile, zero-padded: rows past the batch and the k tail
  // of the first layer multiply zeros
  for (int idx = threadIdx.x; idx < TD_ROWS * TD_STRIDE; idx += TD_THREADS) {
    const int r = idx / TD_STRIDE, k = idx - r * TD_STRIDE;
    bufA[idx] = (r < rows && k < D)
                    ? A.s_next[(int64_t)(row0 + r) * D + k] : 0.0f;
  }
  td_barrier();

  // encoder: A -> B -> A -> H
  td_hidden<false>(R, enc0, A.lin[0].b, enc1, bufA, bufB, lane, 0, nullptr, nullptr);
  td_hidden<false>(R, enc1, A.lin[1].b, enc2, bufB, bufA, lane, 0, nullptr, nullptr);
  td_hidden<false>(R, enc2, A.lin[2].b, dc0, bufA, bufH, lane, 0, nullptr, nullptr);
  // actor hidden layers: H -> A (dc), H -> B (g); then wave 0 and wave 1 run
  // the two output layers and their sampling side by side, while the other
  // waves already hold the first critic layer's weights
  td_hidden<false>(R, dc0, A.lin[3].b, g0, bufH, bufA, lane, 0, nullptr, nullptr);
  td_hidden<false>(R, g0, A.lin[5].b, wave == 0 ? dc1 : wave == 1 ? g1 : c10,
                   bufH, bufB, lane, 0, nullptr, nullptr);
  if (wave == 0) {
    const td_acc acc = td_mma(R, H, bufA, lane);
    td_fetch(R, c10, lane);
    td_sample(acc, A.lin[4].b, A.n_dc, A.mask_dc, A.u_dc, row0, rows, lane,
              s_adc, s_lpdc);
  } else if (wave == 1) {
    const td_acc acc = td_mma(R, H, bufB, lane);
    td_fetch(R, c10, lane);
    td_sample(acc, A.lin[6].b, A.n_g, A.mask_g, A.u_g, row0, rows, lane,
              s_ag, s_lpg);
  }
  td_barrier();
  if (threadIdx.x < rows) {
    const int r = threadIdx.x;
    A.a_dc[row0 + r] = s_adc[r];
    A.a_g[row0 + r] = s_ag[r];
    A.logp[row0 + r] = s_lpdc[r] + s_lpg[r];
  }

  // twin target critic; Q1' waits in registers for Q2'
  const bool qwave = wave * 16 < A.nq;
  td_acc q1 = {0.f, 0.f, 0.f, 0.f};
  td_hidden<true>(R, c10, A.lin[7].b, c11, bufH, bufA, lane, A.n_dc, s_adc, s_ag);
  td_hidden<false>(R, c11, A.lin[8].b, c12, bufA, bufB, lane, 0, nullptr, nullptr);
  // (q1's reads of bufB are ordered by the next layer's closing barrier)
  if (qwave) q1 = td_mma(R, H, bufB, lane);
  td_fetch(R, c20, lane);
  td_hidden<true>(R, c20, A.lin[10].b, c21, bufH, bufA, lane, A.n_dc, s_adc, s_ag);
  td_hidden<false>(R, c21, A.lin[11].b, c22, bufA, bufB, lane, 0, nullptr, nullptr);
  if (qwave) {
    const td_acc q2 = td_mma(R, H, bufB, lane);
    const int j = wave * 16 + (lane & 15);
    if (j < A.nq) {
      const float alpha = expf(*A.log_alpha);
      const float b1 = A.lin[9].b[j], b2 = A.lin[12].b[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;
        if (row < rows) {
          const float lp = s_lpdc[row] + s_lpg[row];
          const float qm = fminf(q1[r] + b1, q2[r] + b2) - alpha * lp;
          const float keep = (1.0f - A.done[row0 + row]) * A.gamma;
          A.target[(int64_t)(row0 + row) * A.nq + j] =
              A.r_eff[row0 + row] + keep * qm;
        }
      }
    }
  }
}

// (weights[26], s_next[B,D], mask_dc, mask_g (bool or None), u_dc, u_g,
//  r_eff[B], done[B], log_alpha (0-dim, device), gamma)
//   -> (target[B,N] f32, a_dc[B] i64, a_g[B] i64, logp[B] f32)
inline std::vector<torch::Tensor> sac_td_target(
    std::vector<torch::Tensor> weights, torch::Tensor s_next,
    c10::optional<torch::Tensor> mask_dc, c10::optional<torch::Tensor> mask_g,
    torch::Tensor u_dc, torch::Tensor u_g, torch::Tensor r_eff,
    torch::Tensor done, torch::Tensor log_alpha, double gamma) {
  auto f32 = [](const torch::Tensor& t) {
    return t.is_cuda() && t.dtype() == torch::kFloat32 && t.is_contiguous();
  };
  TORCH_CHECK(weights.size() == 2 * TD_LINEARS,
              "sac_td_target: 26 tensors, (weight, bias) of 13 linears");
  TORCH_CHECK(f32(s_next) && s_next.dim() == 2,
              "sac_td_target: s_next must be a contiguous f32 [B, obs_dim] "
              "GPU tensor");
  for (auto& w : weights)
    TORCH_CHECK(f32(w) && w.device() == s_next.device(),
                "sac_td_target: weights must be contiguous f32 on s_next's GPU");
  const int64_t B = s_next.size(0), D = s_next.size(1);
  TORCH_CHECK(weights[0].dim() == 2 && weights[8].dim() == 2 &&
                  weights[12].dim() == 2 && weights[18].dim() == 2,
              "sac_td_target: weights must be 2-d");
  const int64_t H = weights[0].size(0);
  const int64_t n_dc = weights[8].size(0), n_g = weights[12].size(0);
  const int64_t N = weights[18].size(0);
  TORCH_CHECK(H >= 16 && H % 16 == 0 && H <= TD_MAXW,
              "sac_td_target: hid = latent must be a multiple of 16, <= 256 "
              "(got ", H, ")");
  TORCH_CHECK(D >= 1 && D <= TD_MAXW, "sac_td_target: 1 <= obs_dim <= 256 "
              "(got ", D, ")");
  TORCH_CHECK(n_dc >= 1 && n_dc <= TD_MAX_ACT && n_g >= 1 && n_g <= TD_MAX_ACT,
              "sac_td_target: n_dc, n_g <= 16 (got ", n_dc, ", ", n_g, ")");
  TORCH_CHECK(N >= 1 && N <= TD_MAX_Q, "sac_td_target: N <= 64 (got ", N, ")");
  TORCH_CHECK(B >= 1 && B * std::max<int64_t>(D, N) <= INT32_MAX,
              "sac_td_target: B >= 1");
  const int64_t C = H + n_dc + n_g;
  const int64_t want[TD_LINEARS][2] = {
      {H, D}, {H, H}, {H, H}, {H, H}, {n_dc, H}, {H, H}, {n_g, H},
      {H, C}, {H, H}, {N, H}, {H, C}, {H, H}, {N, H}};
  TdArgs A;
  for (int l = 0; l < TD_LINEARS; ++l) {
    const auto &w = weights[2 * l], &b = weights[2 * l + 1];
    TORCH_CHECK(w.dim() == 2 && w.size(0) == want[l][0] &&
                    w.size(1) == want[l][1] && b.dim() == 1 &&
                    b.size(0) == want[l][0],
                "sac_td_target: linear ", l, " has shape ", w.sizes(),
                ", expected [", want[l][0], ", ", want[l][1], "]");
    A.lin[l] = {w.data_ptr<float>(), b.data_ptr<float>()};
  }
  auto on_dev = [&](const torch::Tensor& t) {
    return t.device() == s_next.device();
  };
  auto mask_ptr = [&](const c10::optional<torch::Tensor>& m, int64_t n,
                      const char* name) -> const bool* {
    if (!m.has_value()) return nullptr;
    TORCH_CHECK(m->is_cuda() && on_dev(*m) && m->dtype() == torch::kBool &&
                    m->is_contiguous() && m->dim() == 2 && m->size(0) == B &&
                    m->size(1) == n,
                "sac_td_target: ", name, " must be a contiguous bool [B, n]");
    return m->data_ptr<bool>();
  };
  A.mask_dc = mask_ptr(mask_dc, n_dc, "mask_dc");
  A.mask_g = mask_ptr(mask_g, n_g, "mask_g");
  TORCH_CHECK(f32(u_dc) && on_dev(u_dc) && u_dc.dim() == 2 &&
                  u_dc.size(0) == B && u_dc.size(1) == n_dc && f32(u_g) &&
                  on_dev(u_g) && u_g.dim() == 2 && u_g.size(0) == B &&
                  u_g.size(1) == n_g,
              "sac_td_target: u_dc / u_g must be f32 [B, n_dc] / [B, n_g]");
  TORCH_CHECK(f32(r_eff) && on_dev(r_eff) && r_eff.numel() == B &&
                  f32(done) && on_dev(done) && done.numel() == B,
              "sac_td_target: r_eff and done must be f32 with B elements");
  TORCH_CHECK(f32(log_alpha) && on_dev(log_alpha) && log_alpha.numel() == 1,
              "sac_td_target: log_alpha must be a one-element f32 GPU tensor");
  auto target = torch::empty({B, N}, s_next.options());
  auto a_dc = torch::empty({B}, s_next.options().dtype(torch::kInt64));
  auto a_g = torch::empty({B}, s_next.options().dtype(torch::kInt64));
  auto logp = torch::empty({B}, s_next.options());
  A.s_next = s_next.data_ptr<float>();
  A.u_dc = u_dc.data_ptr<float>();
  A.u_g = u_g.data_ptr<float>();
  A.r_eff = r_eff.data_ptr<float>();
  A.done = done.data_ptr<float>();
  A.log_alpha = log_alpha.data_ptr<float>();
  A.gamma = (float)gamma;
  A.B = (int)B, A.obs_dim = (int)D, A.hid = (int)H;
  A.n_dc = (int)n_dc, A.n_g = (int)n_g, A.nq = (int)N;
  A.target = target.data_ptr<float>();
  A.a_dc = a_dc.data_ptr<int64_t>();
  A.a_g = a_g.data_ptr<int64_t>();
  A.logp = logp.data_ptr<float>();
  const unsigned blocks = (unsigned)((B + TD_ROWS - 1) / TD_ROWS);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(sac_td_target_kernel, dim3(blocks), dim3(TD_THREADS), 0,
                     stream, A);
  check_launch("sac_td_target_kernel");
  return {target, a_dc, a_g, logp};
}

// ---------------- twin quantile-Huber loss + gradient ----------------
constexpr int QH_WAVES = 4;  // samples per workgroup
constexpr int QH_THREADS = QH_WAVES * 64;

// loss pair terms follow rl/sac.py::quantile_huber_loss: pair (j, i) is
// (target_j, pred_i), weighted by |tau_j - 1{target_j < pred_i}|
TD_FN __global__ void __launch_bounds__(QH_THREADS)
qr_huber_twin_kernel(const float* __restrict__ q1, const float* __restrict__ q2,
                     const float* __restrict__ target,
                     const float* __restrict__ taus, int B, int N, float inv,
                     float* __restrict__ dq1, float* __restrict__ dq2,
                     double* __restrict__ partials) {
  __shared__ float s_tgt[QH_WAVES][TD_MAX_Q];
  __shared__ float s_tau[TD_MAX_Q];
  __shared__ double s_part[QH_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * QH_WAVES + wave;
  if (threadIdx.x < N) s_tau[threadIdx.x] = taus[threadIdx.x];
  if (b < B && lane < N) s_tgt[wave][lane] = target[(int64_t)b * N + lane];
  td_barrier();
  double lsum = 0.0;
  if (b < B) {
    for (int e = lane; e < 2 * N; e += 64) {
      const bool second = e >= N;
      const int i = second ? e - N : e;
      const float p = (second ? q2 : q1)[(int64_t)b * N + i];
      float loss = 0.0f, grad = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float t = s_tgt[wave][j];
        const float d = p - t, ad = fabsf(d);
        const float pin = fabsf(s_tau[j] - (t < p ? 1.0f : 0.0f));
        loss += pin * (ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
        grad += pin * fminf(fmaxf(d, -1.0f), 1.0f);
      }
      (second ? dq2 : dq1)[(int64_t)b * N + i] = grad * inv;
      lsum += (double)loss;
    }
  }
  lsum = td_wave_sum(lsum, lane);
  if (lane == 0) s_part[wave] = lsum;
  td_barrier();
  if (threadIdx.x == 0) {
    double s = s_part[0];
#pragma unroll
    for (int w = 1; w < QH_WAVES; ++w) s += s_part[w];
    partials[blockIdx.x] = s;
  }
}

// one wave: strided partial per lane, shuffle tree, scale
TD_FN __global__ void __launch_bounds__(64)
qr_huber_final_kernel(const double* __restrict__ partials, int n, double inv,
                      float* __restrict__ loss) {
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += 64) s += partials[k];
  s = td_wave_sum(s, threadIdx.x);
  if (threadIdx.x == 0) *loss = (float)(s * inv);
}

// (q1, q2, target [B,N] f32, taus [N] f32) -> (loss 0-dim, dq1, dq2 [B,N]):
// loss = mean-QR-Huber(q1) + mean-QR-Huber(q2), dq* = d loss / d q*
inline std::vector<torch::Tensor> qr_huber_twin(torch::Tensor q1,
                                                torch::Tensor q2,
                                                torch::Tensor target,
                                                torch::Tensor taus) {
  auto f32 = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == q1.device() &&
           t.dtype() == torch::kFloat32;
  };
  TORCH_CHECK(f32(q1) && f32(q2) && f32(target) && f32(taus),
              "qr_huber_twin: f32 tensors on one GPU");
  TORCH_CHECK(q1.dim() == 2 && q2.sizes() == q1.sizes() &&
                  target.sizes() == q1.sizes() && taus.dim() == 1 &&
                  taus.size(0) == q1.size(1),
              "qr_huber_twin: q1, q2, target [B, N] and taus [N]");
  const int64_t B = q1.size(0), N = q1.size(1);
  TORCH_CHECK(N >= 1 && N <= TD_MAX_Q, "qr_huber_twin: N <= 64 (got ", N, ")");
  TORCH_CHECK(B >= 1 && B * N <= INT32_MAX, "qr_huber_twin: B >= 1");
  q1 = q1.contiguous();
  q2 = q2.contiguous();
  target = target.contiguous();
  taus = taus.contiguous();
  const unsigned blocks = (unsigned)((B + QH_WAVES - 1) / QH_WAVES);
  auto dq1 = torch::empty({B, N}, q1.options());
  auto dq2 = torch::empty({B, N}, q1.options());
  auto loss = torch::empty({}, q1.options());
  auto partials =
      torch::empty({(int64_t)blocks}, q1.options().dtype(torch::kFloat64));
  const double inv = 1.0 / ((double)B * (double)N * (double)N);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(qr_huber_twin_kernel, dim3(blocks), dim3(QH_THREADS), 0,
                     stream, q1.data_ptr<float>(), q2.data_ptr<float>(),
                     target.data_ptr<float>(), taus.data_ptr<float>(), (int)B,
                     (int)N, (float)inv, dq1.data_ptr<float>(),
                     dq2.data_ptr<float>(), partials.data_ptr<double>());
  check_launch("qr_huber_twin_kernel");
  hipLaunchKernelGGL(qr_huber_final_kernel, dim3(1), dim3(64), 0, stream,
                     partials.data_ptr<double>(), (int)blocks, inv,
                     loss.data_ptr<float>());
  check_launch("qr_huber_final_kernel");
  return {loss, dq1, dq2};
}

}  // namespace dcg
