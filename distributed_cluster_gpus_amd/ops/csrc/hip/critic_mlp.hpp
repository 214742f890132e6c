// A twin quantile critic that can be trained in HIP (gfx950): a forward that
// keeps its activations and a backward that produces dh, dW and db.  Opt-in
// (rl/fused.py::twin_critic); TwinQuantileCritic under torch autograd is the
// specification.  All products and sums are fp32: v_mfma_f32_16x16x4_f32 plus
// plain f32 VALU (TD_FN), no float atomics, every sum in a fixed order, so two
// calls on the same inputs are bitwise equal.  The tile, the weight fetch and
// the one-hot epilogue are sac_target.hpp's, unchanged.
//
// twin_critic_fwd_kernel
// ----------------------
// One workgroup of 16 waves owns TD_ROWS = 16 batch rows of ONE critic
// (grid.y): the twins share nothing but h here, so B = 256 fills 32 CUs.  Wave
// w owns output columns [16 w, 16 w + 16); weights are fetched one layer ahead
// (td_hidden).  The first layer multiplies the latent part only, the one-hot
// part is W1[:, H + a_dc] + W1[:, H + n_dc + a_g] in the epilogue.  After each
// hidden layer's barrier the post-ReLU tile is copied LDS -> act, coalesced,
// while the next layer already runs.
//
// twin_critic_bwd_dx_kernel
// -------------------------
// Same split.  In LDS from dq down:
//   dz3 = dq (zero-padded to 16 columns), dz2 = (dz3 W3) . [a2 > 0],
//   dz1 = (dz2 W2) . [a1 > 0], and when asked dh_c = dz1 W1[:, :H];
// dz2 and dz1 also go to global for the weight-gradient kernel.
// These are products with the UNtransposed weight: the B operand W[k][n] is
// contiguous along n, so the forward's 16-byte load along k does not apply.
// Data path taken: dword loads straight from global into the forward's own
// register layout, R.v[c][t] = W[16 c + 4 q + t][n0 + j].  Each load
// instruction reads, per quarter-wave, 16 consecutive floats of one W row: a
// fully used 64-byte segment.  Staging W slabs through LDS was the
// alternative and was not taken: a wave owns its 16 columns for all of k, so
// no element of W is used by two waves of a workgroup and LDS would add a
// write, a read and a barrier per slab without saving a single global load.
// With this layout td_mma serves all three products as it stands (the A
// fragment is the same 16-byte LDS read per four MFMAs), and the fetch for
// the next product is issued before the epilogue and barrier of the current.
// dh is the sum over the two critics: each critic's workgroup writes its
// part, dh_part [2, B, H], and the host adds the two with one elementwise op.
// (One workgroup carrying the accumulator over both critics would halve the
// CUs used by a chain that is latency-bound.)
//
// twin_critic_bwd_dw_kernel
// -------------------------
// dW_l = dZ_l^T X_l and db_l = sum_b dZ_l[b], K = B.  One wave owns one 16x16
// tile of one dW; the grid is the flat list of tiles over (critic, layer,
// out-tile, in-tile), in-tile fastest so that the four waves of a workgroup
// mostly share their dZ slab in L1.  Both operands are dword loads of 16
// consecutive floats per quarter-wave: MFMA slot q of step s holds batch row
// 16 s' + 4 t + q, and the loop over B is sequential, hence reproducible.
// Rows past B are selected to zero (loads clamped in bounds).  X_1's columns
// past H are the one-hots, generated from a_dc / a_g in the fragment load;
// H % 16 == 0, so a tile is all latent or all one-hot and the choice is a
// scalar branch.  Stores are dword stores predicated on (row < out, col < in):
// no alignment is asked of dW1's rows.  db comes from the in-tile 0 wave of
// each out-tile: a lane sums the dZ values it loaded anyway, in loop order,
// and the four quarters are added in the order 0, 1, 2, 3.
//
// Actions outside [0, n) are clamped (forward and backward alike) so that no
// index can leave W1; torch's one_hot raises on them instead.
#pragma once
#include "sac_target.hpp"

#include <tuple>

namespace dcg {

constexpr int CM_DW_WAVES = 4;  // tiles per workgroup of the dW kernel

struct CmNet {
  TdLinear lin[2][3];  // [critic][layer]
};

struct CmArgs {
  CmNet net;
  const float* h;       // [B][hid]
  const int64_t* a_dc;  // [B]
  const int64_t* a_g;   // [B]
  int B, hid, n_dc, n_g, nq;
  float* q[2];          // fwd out: [B][nq] per critic
  float* act;           // fwd out, bwd in: [2][2][B][hid] post-ReLU a1, a2
  const float* dq[2];   // bwd in: [B][nq] per critic
  float* dz;            // bwd: [2][2][B][hid] dz1, dz2 per critic
  float* dh;            // bwd out: [2][B][hid] per-critic parts, or nullptr
  float* dw[2][3];      // bwd out: [out][in]
  float* db[2][3];      // bwd out: [out]
};

TD_FN __device__ __forceinline__ int cm_action(const int64_t* a, int b, int n) {
  return max(0, min((int)a[b], n - 1));
}

// rows [0, rows) of an LDS activation tile -> global [rows][H], coalesced
TD_FN __device__ __forceinline__ void cm_store_tile(const float* buf,
                                                    float* dst, int rows,
                                                    int H) {
  for (int idx = threadIdx.x; idx < rows * H; idx += TD_THREADS) {
    const int r = idx / H, k = idx - r * H;
    dst[idx] = buf[r * TD_STRIDE + k];
  }
}

TD_FN __global__ void __launch_bounds__(TD_THREADS)
twin_critic_fwd_kernel(CmArgs A) {
  __shared__ __attribute__((aligned(16))) float bufH[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufA[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufB[TD_ROWS * TD_STRIDE];
  __shared__ int s_adc[TD_ROWS], s_ag[TD_ROWS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.y;
  const int row0 = blockIdx.x * TD_ROWS;
  const int rows = min(TD_ROWS, A.B - row0);
  const int H = A.hid;
  const TdLinear* lin = A.net.lin[c];
  const TdLayer l0 = {lin[0].w, H + A.n_dc + A.n_g, H, H, wave};
  const TdLayer l1 = {lin[1].w, H, H, H, wave};
  const TdLayer l2 = {lin[2].w, H, H, A.nq, wave};
  TdW R;
  td_fetch(R, l0, lane);

  // the h tile, zero-padded: rows past the batch multiply zeros
  for (int idx = threadIdx.x; idx < TD_ROWS * TD_STRIDE; idx += TD_THREADS) {
    const int r = idx / TD_STRIDE, k = idx - r * TD_STRIDE;
    bufH[idx] = (r < rows && k < H) ? A.h[(int64_t)(row0 + r) * H + k] : 0.0f;
  }
  if (threadIdx.x < TD_ROWS) {
    const int r = threadIdx.x, b = row0 + min(r, rows - 1);
    s_adc[r] = cm_action(A.a_dc, b, A.n_dc);
    s_ag[r] = cm_action(A.a_g, b, A.n_g);
  }
  td_barrier();

  float* act1 = A.act + ((int64_t)(c * 2 + 0) * A.B + row0) * H;
  float* act2 = A.act + ((int64_t)(c * 2 + 1) * A.B + row0) * H;
  td_hidden<true>(R, l0, lin[0].b, l1, bufH, bufA, lane, A.n_dc, s_adc, s_ag);
  cm_store_tile(bufA, act1, rows, H);
  td_hidden<false>(R, l1, lin[1].b, l2, bufA, bufB, lane, 0, nullptr, nullptr);
  cm_store_tile(bufB, act2, rows, H);
  if (wave * 16 < A.nq) {
    const td_acc acc = td_mma(R, H, bufB, lane);
    const int j = wave * 16 + (lane & 15);
    if (j < A.nq) {
      const float bj = lin[2].b[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;
        if (row < rows)
          A.q[c][(int64_t)(row0 + row) * A.nq + j] = acc[r] + bj;
      }
    }
  }
}

// One wave's slice of an UNtransposed weight, as the B operand of X W:
// R.v[c][t] = W[16 c + 4 q + t][16 tile + j] for k < K, zero past K (loads
// clamped to the last row).  ncols % 16 == 0.  Same register layout as
// td_fetch, so td_mma multiplies it as it stands.
TD_FN __device__ __forceinline__ void cm_fetch_t(TdW& R, const float* w,
                                                 int ld, int K, int ncols,
                                                 int tile, int lane) {
  if (tile * 16 >= ncols) return;
  const int q = lane >> 4;
  const float* wc = w + tile * 16 + (lane & 15);
#pragma unroll
  for (int c = 0; c < TD_MAXW / 16; ++c)
    if (c * 16 < K) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = c * 16 + 4 * q + t;
        const float x = wc[(int64_t)min(k, K - 1) * ld];
        R.v[c][t] = k < K ? x : 0.0f;
      }
    }
}

// Y = (X W) . [act > 0] for one hidden layer going down, W (K rows) in R; then
// R <- the next product's weights (wn: [H][ldn], first H columns), the
// epilogue to LDS and to dz, and a barrier.  Rows past the batch become zero.
TD_FN __device__ __forceinline__ void cm_back(TdW& R, int K, const float* X,
                                              float* Y, const float* act,
                                              float* dz, const float* wn,
                                              int ldn, int H, int rows,
                                              int wave, int lane) {
  const bool active = wave * 16 < H;
  const int j = wave * 16 + (lane & 15);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  td_acc acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
      a[r] = act[min(row, rows - 1) * H + j];
    }
    acc = td_mma(R, K, X, lane);
  }
  if (wn != nullptr) cm_fetch_t(R, wn, ldn, H, H, wave, lane);
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
      const float y = (row < rows && a[r] > 0.0f) ? acc[r] : 0.0f;
      Y[row * TD_STRIDE + j] = y;
      if (row < rows) dz[row * H + j] = y;
    }
  }
  td_barrier();
}

TD_FN __global__ void __launch_bounds__(TD_THREADS)
twin_critic_bwd_dx_kernel(CmArgs A) {
  __shared__ __attribute__((aligned(16))) float bufA[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufB[TD_ROWS * TD_STRIDE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.y;
  const int row0 = blockIdx.x * TD_ROWS;
  const int rows = min(TD_ROWS, A.B - row0);
  const int H = A.hid, N = A.nq;
  const TdLinear* lin = A.net.lin[c];
  TdW R;
  cm_fetch_t(R, lin[2].w, H, N, H, wave, lane);

  // dz3 = dq, zero-padded (columns up to the next multiple of 16, rows past
  // the batch)
  const float* dq = A.dq[c];
  for (int idx = threadIdx.x; idx < TD_ROWS * TD_STRIDE; idx += TD_THREADS) {
    const int r = idx / TD_STRIDE, k = idx - r * TD_STRIDE;
    bufA[idx] = (r < rows && k < N) ? dq[(int64_t)(row0 + r) * N + k] : 0.0f;
  }
  td_barrier();

  const int64_t t1 = ((int64_t)(c * 2 + 0) * A.B + row0) * H;
  const int64_t t2 = ((int64_t)(c * 2 + 1) * A.B + row0) * H;
  cm_back(R, (N + 15) & ~15, bufA, bufB, A.act + t2, A.dz + t2, lin[1].w, H, H,
          rows, wave, lane);
  cm_back(R, H, bufB, bufA, A.act + t1, A.dz + t1,
          A.dh != nullptr ? lin[0].w : nullptr, H + A.n_dc + A.n_g, H, rows,
          wave, lane);
  if (A.dh != nullptr && wave * 16 < H) {
    const td_acc acc = td_mma(R, H, bufA, lane);
    const int j = wave * 16 + (lane & 15);
    float* dh = A.dh + ((int64_t)c * A.B + row0) * H;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
      if (row < rows) dh[row * H + j] = acc[r];
    }
  }
}

TD_FN __global__ void __launch_bounds__(CM_DW_WAVES * 64)
twin_critic_bwd_dw_kernel(CmArgs A, int tiles_per_critic) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  int t = blockIdx.x * CM_DW_WAVES + wave;
  if (t >= 2 * tiles_per_critic) return;
  const int B = A.B, H = A.hid, C = H + A.n_dc + A.n_g;
  const int hT = H / 16, cT = (C + 15) / 16;
  const int c = t / tiles_per_critic;
  t -= c * tiles_per_critic;
  // (layer, out-tile, in-tile) of this wave, in-tile fastest
  int layer = 0, inT = cT;
  if (t >= hT * cT) {
    t -= hT * cT, layer = 1, inT = hT;
    if (t >= hT * hT) t -= hT * hT, layer = 2;
  }
  const int ot = t / inT, it = t - ot * inT;
  // dZ_l [B][out] and X_l [B][in]
  const int64_t t1 = (int64_t)(c * 2 + 0) * B * H, t2 = t1 + (int64_t)B * H;
  const float* Z = layer == 0 ? A.dz + t1 : layer == 1 ? A.dz + t2 : A.dq[c];
  const float* X = layer == 0 ? A.h : layer == 1 ? A.act + t1 : A.act + t2;
  const int out = layer == 2 ? A.nq : H;
  const int in = layer == 0 ? C : H;
  const bool onehot = it * 16 >= H;  // layer 0's columns past the latent

  const int q = lane >> 4, m = lane & 15;
  const int o = ot * 16 + m, i = it * 16 + m;
  const bool o_ok = o < out;
  const int oc = min(o, out - 1);
  const int e = i - H;  // one-hot column: [0, n_dc) dc, [n_dc, n_dc + n_g) g
  td_acc acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.0f;
#pragma unroll 2
  for (int b0 = 0; b0 < B; b0 += 16) {
    float z[4], x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int b = b0 + 4 * s + q;
      const int bb = min(b, B - 1);
      const float zv = Z[(int64_t)bb * out + oc];
      float xv;
      if (onehot) {
        const int hot = e < A.n_dc ? cm_action(A.a_dc, bb, A.n_dc)
                                   : A.n_dc + cm_action(A.a_g, bb, A.n_g);
        xv = e == hot ? 1.0f : 0.0f;
      } else {
        xv = X[(int64_t)bb * H + i];
      }
      z[s] = (b < B && o_ok) ? zv : 0.0f;
      x[s] = b < B ? xv : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(z[s], x[s], acc, 0, 0, 0);
      bsum += z[s];
    }
  }
  float* dw = A.dw[c][layer];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oo = ot * 16 + 4 * q + r;
    if (oo < out && i < in) dw[(int64_t)oo * in + i] = acc[r];
  }
  if (it == 0) {
    float s = td_lane_read(bsum, m);
    s += td_lane_read(bsum, m + 16);
    s += td_lane_read(bsum, m + 32);
    s += td_lane_read(bsum, m + 48);
    if (q == 0 && o_ok) A.db[c][layer][o] = s;
  }
}

// shared checks of both entries; fills the pointers and sizes of A
inline void cm_check(const std::vector<torch::Tensor>& weights,
                     const torch::Tensor& h, const torch::Tensor& a_dc,
                     const torch::Tensor& a_g, int64_t n_dc, int64_t n_g,
                     CmArgs& A) {
  auto f32 = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == h.device() &&
           t.dtype() == torch::kFloat32 && t.is_contiguous();
  };
  TORCH_CHECK(weights.size() == 12,
              "twin_critic: 12 tensors, (weight, bias) of q1 x3 and q2 x3");
  TORCH_CHECK(h.is_cuda() && f32(h) && h.dim() == 2,
              "twin_critic: h must be a contiguous f32 [B, H] GPU tensor");
  for (auto& w : weights)
    TORCH_CHECK(f32(w), "twin_critic: weights must be contiguous f32 on h's GPU");
  const int64_t B = h.size(0), H = h.size(1);
  TORCH_CHECK(H >= 16 && H % 16 == 0 && H <= TD_MAXW,
              "twin_critic: hid = latent must be a multiple of 16, <= 256 "
              "(got ", H, ")");
  TORCH_CHECK(n_dc >= 1 && n_dc <= TD_MAX_ACT && n_g >= 1 && n_g <= TD_MAX_ACT,
              "twin_critic: n_dc, n_g <= 16 (got ", n_dc, ", ", n_g, ")");
  TORCH_CHECK(weights[4].dim() == 2, "twin_critic: weights must be 2-d");
  const int64_t N = weights[4].size(0);
  TORCH_CHECK(N >= 1 && N <= TD_MAX_Q, "twin_critic: N <= 64 (got ", N, ")");
  TORCH_CHECK(B >= 1 && B * (H + n_dc + n_g) <= INT32_MAX / 4,
              "twin_critic: B >= 1");
  const int64_t C = H + n_dc + n_g;
  const int64_t want[3][2] = {{H, C}, {H, H}, {N, H}};
  for (int l = 0; l < 6; ++l) {
    const auto &w = weights[2 * l], &b = weights[2 * l + 1];
    const int64_t* s = want[l % 3];
    TORCH_CHECK(w.dim() == 2 && w.size(0) == s[0] && w.size(1) == s[1] &&
                    b.dim() == 1 && b.size(0) == s[0],
                "twin_critic: linear ", l, " has shape ", w.sizes(),
                ", expected [", s[0], ", ", s[1], "]");
    A.net.lin[l / 3][l % 3] = {w.data_ptr<float>(), b.data_ptr<float>()};
  }
  auto i64 = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == h.device() &&
           t.dtype() == torch::kInt64 && t.is_contiguous() && t.dim() == 1 &&
           t.size(0) == B;
  };
  TORCH_CHECK(i64(a_dc) && i64(a_g),
              "twin_critic: a_dc, a_g must be contiguous int64 [B] on h's GPU");
  A.h = h.data_ptr<float>();
  A.a_dc = a_dc.data_ptr<int64_t>();
  A.a_g = a_g.data_ptr<int64_t>();
  A.B = (int)B, A.hid = (int)H, A.n_dc = (int)n_dc, A.n_g = (int)n_g;
  A.nq = (int)N;
  A.q[0] = A.q[1] = A.act = A.dz = A.dh = nullptr;
  A.dq[0] = A.dq[1] = nullptr;
  for (int l = 0; l < 6; ++l) A.dw[l / 3][l % 3] = A.db[l / 3][l % 3] = nullptr;
}

// (weights[12] = (weight, bias) of q1 x3, q2 x3; h [B,H] f32; a_dc, a_g [B]
//  i64; n_dc, n_g) -> (q1 [B,N], q2 [B,N], act [2,2,B,H])
inline std::vector<torch::Tensor> twin_critic_fwd(
    std::vector<torch::Tensor> weights, torch::Tensor h, torch::Tensor a_dc,
    torch::Tensor a_g, int64_t n_dc, int64_t n_g) {
  CmArgs A;
  cm_check(weights, h, a_dc, a_g, n_dc, n_g, A);
  const int64_t B = A.B, H = A.hid, N = A.nq;
  auto q1 = torch::empty({B, N}, h.options());
  auto q2 = torch::empty({B, N}, h.options());
  auto act = torch::empty({2, 2, B, H}, h.options());
  A.q[0] = q1.data_ptr<float>();
  A.q[1] = q2.data_ptr<float>();
  A.act = act.data_ptr<float>();
  const unsigned blocks = (unsigned)((B + TD_ROWS - 1) / TD_ROWS);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(twin_critic_fwd_kernel, dim3(blocks, 2), dim3(TD_THREADS),
                     0, stream, A);
  check_launch("twin_critic_fwd_kernel");
  return {q1, q2, act};
}

// (weights[12], h, a_dc, a_g, n_dc, n_g, act, dq1, dq2, want_dh, want_dw)
//   -> (dh [B,H] or undefined, grads[12] in the order of weights or empty)
inline std::tuple<torch::Tensor, std::vector<torch::Tensor>> twin_critic_bwd(
    std::vector<torch::Tensor> weights, torch::Tensor h, torch::Tensor a_dc,
    torch::Tensor a_g, int64_t n_dc, int64_t n_g, torch::Tensor act,
    torch::Tensor dq1, torch::Tensor dq2, bool want_dh, bool want_dw) {
  CmArgs A;
  cm_check(weights, h, a_dc, a_g, n_dc, n_g, A);
  const int64_t B = A.B, H = A.hid, N = A.nq;
  auto f32 = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == h.device() &&
           t.dtype() == torch::kFloat32 && t.is_contiguous();
  };
  TORCH_CHECK(f32(act) && act.dim() == 4 && act.size(0) == 2 &&
                  act.size(1) == 2 && act.size(2) == B && act.size(3) == H,
              "twin_critic: act must be the forward's f32 [2, 2, B, H]");
  TORCH_CHECK(f32(dq1) && f32(dq2) && dq1.dim() == 2 && dq1.size(0) == B &&
                  dq1.size(1) == N && dq2.sizes() == dq1.sizes(),
              "twin_critic: dq1, dq2 must be contiguous f32 [B, N]");
  auto dz = torch::empty({2, 2, B, H}, h.options());
  torch::Tensor parts, dh;
  A.act = act.data_ptr<float>();
  A.dq[0] = dq1.data_ptr<float>();
  A.dq[1] = dq2.data_ptr<float>();
  A.dz = dz.data_ptr<float>();
  if (want_dh) {
    parts = torch::empty({2, B, H}, h.options());
    A.dh = parts.data_ptr<float>();
  }
  const unsigned blocks = (unsigned)((B + TD_ROWS - 1) / TD_ROWS);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(twin_critic_bwd_dx_kernel, dim3(blocks, 2),
                     dim3(TD_THREADS), 0, stream, A);
  check_launch("twin_critic_bwd_dx_kernel");
  if (want_dh) dh = parts[0] + parts[1];
  std::vector<torch::Tensor> grads;
  if (want_dw) {
    for (int l = 0; l < 6; ++l) {
      grads.push_back(torch::empty_like(weights[2 * l]));
      grads.push_back(torch::empty_like(weights[2 * l + 1]));
      A.dw[l / 3][l % 3] = grads[2 * l].data_ptr<float>();
      A.db[l / 3][l % 3] = grads[2 * l + 1].data_ptr<float>();
    }
    const int64_t C = H + n_dc + n_g, hT = H / 16;
    const int tiles = (int)(hT * ((C + 15) / 16) + hT * hT +
                            ((N + 15) / 16) * hT);
    const unsigned wg = (unsigned)((2 * tiles + CM_DW_WAVES - 1) / CM_DW_WAVES);
    hipLaunchKernelGGL(twin_critic_bwd_dw_kernel, dim3(wg),
                       dim3(CM_DW_WAVES * 64), 0, stream, A, tiles);
    check_launch("twin_critic_bwd_dw_kernel");
  }
  return {dh, grads};
}

}  // namespace dcg
