// The two policy heads of HybridActor, trainable in HIP (gfx950): a forward
// that draws the actions and keeps what the backward needs, and a backward
// that produces dh, dW and db.  Opt-in (rl/fused.py::actor_heads); HybridActor
// under torch autograd with rl/masking.py::sample_categorical is the
// specification.  All products and sums are fp32: v_mfma_f32_16x16x4_f32 plus
// plain f32 VALU (TD_FN), no float atomics, every sum in a fixed order, so two
// calls on the same inputs are bitwise equal.  The tile, the weight fetch and
// the hidden layer are sac_target.hpp's, the transposed fetch and the downward
// layer are critic_mlp.hpp's, all unchanged.
//
// Head k is 0 for dc and 1 for g.  Per head
//   z1 = h W1^T + b1, a1 = relu(z1), logits = a1 W2^T + b2,
//   x = mask ? logits : -FLT_MAX, lp = log_softmax(x),
//   a = argmax(lp - log(-log(max(u, 1e-20)))), lowest index winning ties,
//   logp_k = lp[a].
// A row whose mask allows nothing is not supported: torch draws uniformly
// over its dtype-min logits there, and these kernels make no such promise.
//
// actor_heads_fwd_kernel
// ----------------------
// One workgroup of 16 waves owns TD_ROWS = 16 batch rows of ONE head (grid.y):
// the heads share nothing but h.  Wave w owns hidden columns [16 w, 16 w + 16)
// (td_hidden), and the post-ReLU tile goes LDS -> act, coalesced.
// The output layer is one 16-column tile with K = H.  It is split over k:
// wave w multiplies k in [16 w, 16 w + 16), the very columns of a1 that it
// wrote itself, with 4 MFMAs and one 16-byte weight load per lane (fetched
// before the hidden layer's epilogue), and writes its 16x16 partial to LDS —
// into the h tile, which nobody reads any more.  After one barrier wave 0 adds
// the H/16 partials in wave order: a fixed order, hence reproducible.  The
// alternative, one wave running the whole K = H as sac_td_target_kernel does,
// is a chain of up to 64 dependent MFMAs behind a 16 x 16 B fetch per lane
// while 15 waves idle; here the chain is 4 MFMAs, a barrier and up to 16
// LDS reads and adds.
// The draw is td_sample's: a row's 16 columns sit in one quarter-wave, so the
// max, the sum, the argmax and the pick are xor-shuffles.  The variant here
// also stores the masked log-softmax, lp_all [2, B, 16] (-inf past n), and
// writes actions and log-probs straight to global memory.
//
// actor_heads_bwd_dx_kernel
// -------------------------
// Same split.  From the upstream g [B] = dL/dlogp (both heads receive it):
//   dlogits[b][j] = g[b] * (1{j == a[b]} - exp(lp_all[b][j])),
// exactly 0 for j >= n, for masked entries (exp of about -FLT_MAX) and in
// rows past the batch; to LDS and to global [2, B, 16] for the dW kernel.
//   dz1 = (dlogits W2) . [a1 > 0]   K = 16: 4 MFMAs per wave (cm_back),
// to LDS and to global [2, B, H]; and when asked dh_part[k] = dz1 W1, the two
// parts added by the host with one elementwise op.
//
// actor_heads_bwd_dw_kernel
// -------------------------
// dW1 = dz1^T h (H x H), dW2 = dlogits^T a1 (n x H), db = column sums, K = B.
// One wave per 16x16 tile over (head, layer, out-tile, in-tile), in-tile
// fastest, the loop over B sequential.  Rows past B are selected to zero
// (loads clamped in bounds), stores are predicated on (row < out, col < in),
// db comes from the in-tile 0 wave with the quarters added in order 0..3.
#pragma once
#include "critic_mlp.hpp"
#include "sac_target.hpp"

#include <tuple>

namespace dcg {

constexpr int AH_DW_WAVES = 4;   // tiles per workgroup of the dW kernel
constexpr int AH_LP = TD_MAX_ACT;  // row length of lp_all and dlogits

struct AhArgs {
  TdLinear lin[2][2];   // [head][layer]
  const float* h;       // [B][hid]
  const bool* mask[2];  // [B][n] or nullptr
  const float* u[2];    // [B][n]
  int n[2];
  int B, hid;
  int64_t* a[2];        // fwd out, bwd in: [B]
  float* logp;          // fwd out: [2][B]
  float* act;           // fwd out, bwd in: [2][B][hid] post-ReLU a1
  float* lp_all;        // fwd out, bwd in: [2][B][16] masked log-softmax
  const float* g;       // bwd in: [B] dL/dlogp
  float* dlogits;       // bwd: [2][B][16]
  float* dz;            // bwd: [2][B][hid] dz1
  float* dh;            // bwd out: [2][B][hid] per-head parts, or nullptr
  float* dw[2][2];      // bwd out: [out][hid]
  float* db[2][2];      // bwd out: [out]
};

// td_sample, storing to global memory: the action, the chosen log-prob and
// the whole masked log-softmax row (columns past n as -inf)
TD_FN __device__ __forceinline__ void ah_sample(td_acc acc, const float* bias,
                                                int n, const bool* mask,
                                                const float* u, int row0,
                                                int rows, int lane,
                                                int64_t* a_out, float* lp_out,
                                                float* lp_all) {
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
    if (row < rows) {
      lp_all[(int64_t)(row0 + row) * AH_LP + j] = col ? lp : -INFINITY;
      if (j == 0) {
        a_out[row0 + row] = arg;
        lp_out[row0 + row] = lp_a;
      }
    }
  }
}

TD_FN __global__ void __launch_bounds__(TD_THREADS)
actor_heads_fwd_kernel(AhArgs A) {
  __shared__ __attribute__((aligned(16))) float bufH[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufA[TD_ROWS * TD_STRIDE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.y;
  const int row0 = blockIdx.x * TD_ROWS;
  const int rows = min(TD_ROWS, A.B - row0);
  const int H = A.hid, n = A.n[k];
  const TdLinear* lin = A.lin[k];
  const bool active = wave * 16 < H;
  const TdLayer l0 = {lin[0].w, H, H, H, wave};
  // this wave's k slab of the output layer: W2[j][16 w .. 16 w + 16) as a
  // 16-wide layer of its own; a wave past H fetches nothing
  const TdLayer l1 = {lin[1].w + (active ? 16 * wave : 0), H, 16,
                      active ? n : 0, 0};
  TdW R;
  td_fetch(R, l0, lane);

  // the h tile, zero-padded: rows past the batch multiply zeros
  for (int idx = threadIdx.x; idx < TD_ROWS * TD_STRIDE; idx += TD_THREADS) {
    const int r = idx / TD_STRIDE, c = idx - r * TD_STRIDE;
    bufH[idx] = (r < rows && c < H) ? A.h[(int64_t)(row0 + r) * H + c] : 0.0f;
  }
  td_barrier();

  td_hidden<false>(R, l0, lin[0].b, l1, bufH, bufA, lane, 0, nullptr, nullptr);
  cm_store_tile(bufA, A.act + ((int64_t)k * A.B + row0) * H, rows, H);
  // split-K partials, [wave][row][col], over the h tile: every read of it
  // lies before td_hidden's barrier
  float* part = bufH;
  if (active) {
    const td_acc acc = td_mma(R, 16, bufA + 16 * wave, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[wave * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
  }
  td_barrier();
  if (wave == 0) {
    td_acc acc;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      acc[r] = part[((lane >> 4) * 4 + r) * 16 + (lane & 15)];
    for (int p = 1; p < H / 16; ++p) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[r] += part[p * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)];
    }
    ah_sample(acc, lin[1].b, n, A.mask[k], A.u[k], row0, rows, lane, A.a[k],
              A.logp + (int64_t)k * A.B, A.lp_all + (int64_t)k * A.B * AH_LP);
  }
}

TD_FN __global__ void __launch_bounds__(TD_THREADS)
actor_heads_bwd_dx_kernel(AhArgs A) {
  __shared__ __attribute__((aligned(16))) float bufA[TD_ROWS * TD_STRIDE];
  __shared__ __attribute__((aligned(16))) float bufB[TD_ROWS * TD_STRIDE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.y;
  const int row0 = blockIdx.x * TD_ROWS;
  const int rows = min(TD_ROWS, A.B - row0);
  const int H = A.hid, n = A.n[k];
  const TdLinear* lin = A.lin[k];
  TdW R;
  cm_fetch_t(R, lin[1].w, H, n, H, wave, lane);

  // dlogits, 16 columns wide: zero past n, where masked and past the batch
  if (threadIdx.x < TD_ROWS * AH_LP) {
    const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
    float d = 0.0f;
    if (r < rows) {
      const int64_t e = ((int64_t)k * A.B + row0 + r) * AH_LP + j;
      if (j < n) {
        const float p = expf(A.lp_all[e]);
        const float hot = (int)A.a[k][row0 + r] == j ? 1.0f : 0.0f;
        d = A.g[row0 + r] * (hot - p);
      }
      A.dlogits[e] = d;
    }
    bufA[r * TD_STRIDE + j] = d;
  }
  td_barrier();

  const int64_t t = ((int64_t)k * A.B + row0) * H;
  cm_back(R, 16, bufA, bufB, A.act + t, A.dz + t,
          A.dh != nullptr ? lin[0].w : nullptr, H, H, rows, wave, lane);
  if (A.dh != nullptr && wave * 16 < H) {
    const td_acc acc = td_mma(R, H, bufB, lane);
    const int j = wave * 16 + (lane & 15);
    float* dh = A.dh + t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
      if (row < rows) dh[row * H + j] = acc[r];
    }
  }
}

TD_FN __global__ void __launch_bounds__(AH_DW_WAVES * 64)
actor_heads_bwd_dw_kernel(AhArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int B = A.B, H = A.hid, hT = H / 16;
  const int tiles_per_head = hT * hT + hT;
  int t = blockIdx.x * AH_DW_WAVES + wave;
  if (t >= 2 * tiles_per_head) return;
  const int k = t / tiles_per_head;
  t -= k * tiles_per_head;
  // (layer, out-tile, in-tile) of this wave, in-tile fastest; the output
  // layer has one out-tile
  const int layer = t >= hT * hT ? 1 : 0;
  if (layer == 1) t -= hT * hT;
  const int ot = t / hT, it = t - ot * hT;
  // dZ [B][zld], of which `out` columns count, and X [B][H]
  const int64_t th = (int64_t)k * B * H;
  const float* Z = layer == 0 ? A.dz + th
                              : A.dlogits + (int64_t)k * B * AH_LP;
  const float* X = layer == 0 ? A.h : A.act + th;
  const int out = layer == 0 ? H : A.n[k];
  const int zld = layer == 0 ? H : AH_LP;

  const int q = lane >> 4, m = lane & 15;
  const int o = ot * 16 + m, i = it * 16 + m;
  const bool o_ok = o < out;
  const int oc = min(o, out - 1);
  td_acc acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.0f;
#pragma unroll 2
  for (int b0 = 0; b0 < B; b0 += 16) {
    float z[4], x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int b = b0 + 4 * s + q;
      const int bb = min(b, B - 1);
      const float zv = Z[(int64_t)bb * zld + oc];
      const float xv = X[(int64_t)bb * H + i];
      z[s] = (b < B && o_ok) ? zv : 0.0f;
      x[s] = b < B ? xv : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(z[s], x[s], acc, 0, 0, 0);
      bsum += z[s];
    }
  }
  float* dw = A.dw[k][layer];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oo = ot * 16 + 4 * q + r;
    if (oo < out && i < H) dw[(int64_t)oo * H + i] = acc[r];
  }
  if (it == 0) {
    float s = td_lane_read(bsum, m);
    s += td_lane_read(bsum, m + 16);
    s += td_lane_read(bsum, m + 32);
    s += td_lane_read(bsum, m + 48);
    if (q == 0 && o_ok) A.db[k][layer][o] = s;
  }
}

// shared checks of both entries; fills the weights, h and the sizes of A
inline void ah_check(const std::vector<torch::Tensor>& weights,
                     const torch::Tensor& h, AhArgs& A) {
  auto f32 = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == h.device() &&
           t.dtype() == torch::kFloat32 && t.is_contiguous();
  };
  TORCH_CHECK(weights.size() == 8,
              "actor_heads: 8 tensors, (weight, bias) of head_dc x2, head_g x2");
  TORCH_CHECK(h.is_cuda() && f32(h) && h.dim() == 2,
              "actor_heads: h must be a contiguous f32 [B, H] GPU tensor");
  for (auto& w : weights)
    TORCH_CHECK(f32(w), "actor_heads: weights must be contiguous f32 on h's GPU");
  const int64_t B = h.size(0), H = h.size(1);
  TORCH_CHECK(H >= 16 && H % 16 == 0 && H <= TD_MAXW,
              "actor_heads: hid = latent must be a multiple of 16, <= 256 "
              "(got ", H, ")");
  TORCH_CHECK(weights[2].dim() == 2 && weights[6].dim() == 2,
              "actor_heads: weights must be 2-d");
  const int64_t n[2] = {weights[2].size(0), weights[6].size(0)};
  TORCH_CHECK(n[0] >= 1 && n[0] <= TD_MAX_ACT && n[1] >= 1 &&
                  n[1] <= TD_MAX_ACT,
              "actor_heads: n_dc, n_g <= 16 (got ", n[0], ", ", n[1], ")");
  TORCH_CHECK(B >= 1 && B * H <= INT32_MAX / 4, "actor_heads: B >= 1");
  for (int l = 0; l < 4; ++l) {
    const auto &w = weights[2 * l], &b = weights[2 * l + 1];
    const int64_t out = l % 2 == 0 ? H : n[l / 2];
    TORCH_CHECK(w.dim() == 2 && w.size(0) == out && w.size(1) == H &&
                    b.dim() == 1 && b.size(0) == out,
                "actor_heads: linear ", l, " has shape ", w.sizes(),
                ", expected [", out, ", ", H, "]");
    A.lin[l / 2][l % 2] = {w.data_ptr<float>(), b.data_ptr<float>()};
  }
  A.h = h.data_ptr<float>();
  A.B = (int)B, A.hid = (int)H, A.n[0] = (int)n[0], A.n[1] = (int)n[1];
  A.logp = A.act = A.lp_all = A.dlogits = A.dz = A.dh = nullptr;
  A.g = nullptr;
  for (int k = 0; k < 2; ++k) {
    A.mask[k] = nullptr, A.u[k] = nullptr, A.a[k] = nullptr;
    for (int l = 0; l < 2; ++l) A.dw[k][l] = A.db[k][l] = nullptr;
  }
}

// (weights[8] = (weight, bias) of head_dc x2, head_g x2; h [B,H] f32; mask_dc,
//  mask_g bool [B,n] or None; u_dc, u_g f32 [B,n])
//   -> (a_dc [B] i64, a_g [B] i64, logp [2,B], act [2,B,H], lp_all [2,B,16])
inline std::vector<torch::Tensor> actor_heads_fwd(
    std::vector<torch::Tensor> weights, torch::Tensor h,
    c10::optional<torch::Tensor> mask_dc, c10::optional<torch::Tensor> mask_g,
    torch::Tensor u_dc, torch::Tensor u_g) {
  AhArgs A;
  ah_check(weights, h, A);
  const int64_t B = A.B, H = A.hid;
  const c10::optional<torch::Tensor>* masks[2] = {&mask_dc, &mask_g};
  const torch::Tensor* us[2] = {&u_dc, &u_g};
  for (int k = 0; k < 2; ++k) {
    const auto& u = *us[k];
    TORCH_CHECK(u.is_cuda() && u.device() == h.device() &&
                    u.dtype() == torch::kFloat32 && u.is_contiguous() &&
                    u.dim() == 2 && u.size(0) == B && u.size(1) == A.n[k],
                "actor_heads: u_dc / u_g must be contiguous f32 [B, n_dc] / "
                "[B, n_g] on h's GPU");
    A.u[k] = u.data_ptr<float>();
    const auto& m = *masks[k];
    if (!m.has_value()) continue;
    TORCH_CHECK(m->is_cuda() && m->device() == h.device() &&
                    m->dtype() == torch::kBool && m->is_contiguous() &&
                    m->dim() == 2 && m->size(0) == B && m->size(1) == A.n[k],
                "actor_heads: mask_dc / mask_g must be contiguous bool "
                "[B, n_dc] / [B, n_g] on h's GPU");
    A.mask[k] = m->data_ptr<bool>();
  }
  auto a_dc = torch::empty({B}, h.options().dtype(torch::kInt64));
  auto a_g = torch::empty({B}, h.options().dtype(torch::kInt64));
  auto logp = torch::empty({2, B}, h.options());
  auto act = torch::empty({2, B, H}, h.options());
  auto lp_all = torch::empty({2, B, AH_LP}, h.options());
  A.a[0] = a_dc.data_ptr<int64_t>();
  A.a[1] = a_g.data_ptr<int64_t>();
  A.logp = logp.data_ptr<float>();
  A.act = act.data_ptr<float>();
  A.lp_all = lp_all.data_ptr<float>();
  const unsigned blocks = (unsigned)((B + TD_ROWS - 1) / TD_ROWS);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(actor_heads_fwd_kernel, dim3(blocks, 2), dim3(TD_THREADS),
                     0, stream, A);
  check_launch("actor_heads_fwd_kernel");
  return {a_dc, a_g, logp, act, lp_all};
}

// (weights[8], h, a_dc, a_g, act, lp_all, g [B] = dL/dlogp, want_dh, want_dw)
//   -> (dh [B,H] or undefined, grads[8] in the order of weights or empty,
//       dlogits [2,B,16])
inline std::tuple<torch::Tensor, std::vector<torch::Tensor>, torch::Tensor>
actor_heads_bwd(std::vector<torch::Tensor> weights, torch::Tensor h,
                torch::Tensor a_dc, torch::Tensor a_g, torch::Tensor act,
                torch::Tensor lp_all, torch::Tensor g, bool want_dh,
                bool want_dw) {
  AhArgs A;
  ah_check(weights, h, A);
  const int64_t B = A.B, H = A.hid;
  auto on_dev = [&](const torch::Tensor& t, c10::ScalarType ty) {
    return t.is_cuda() && t.device() == h.device() && t.dtype() == ty &&
           t.is_contiguous();
  };
  TORCH_CHECK(on_dev(a_dc, torch::kInt64) && on_dev(a_g, torch::kInt64) &&
                  a_dc.dim() == 1 && a_dc.size(0) == B && a_g.dim() == 1 &&
                  a_g.size(0) == B,
              "actor_heads: a_dc, a_g must be contiguous int64 [B] on h's GPU");
  TORCH_CHECK(on_dev(act, torch::kFloat32) && act.dim() == 3 &&
                  act.size(0) == 2 && act.size(1) == B && act.size(2) == H,
              "actor_heads: act must be the forward's f32 [2, B, H]");
  TORCH_CHECK(on_dev(lp_all, torch::kFloat32) && lp_all.dim() == 3 &&
                  lp_all.size(0) == 2 && lp_all.size(1) == B &&
                  lp_all.size(2) == AH_LP,
              "actor_heads: lp_all must be the forward's f32 [2, B, 16]");
  TORCH_CHECK(on_dev(g, torch::kFloat32) && g.dim() == 1 && g.size(0) == B,
              "actor_heads: g must be a contiguous f32 [B]");
  auto dlogits = torch::empty({2, B, AH_LP}, h.options());
  auto dz = torch::empty({2, B, H}, h.options());
  torch::Tensor parts, dh;
  A.a[0] = a_dc.data_ptr<int64_t>();
  A.a[1] = a_g.data_ptr<int64_t>();
  A.act = act.data_ptr<float>();
  A.lp_all = lp_all.data_ptr<float>();
  A.g = g.data_ptr<float>();
  A.dlogits = dlogits.data_ptr<float>();
  A.dz = dz.data_ptr<float>();
  if (want_dh) {
    parts = torch::empty({2, B, H}, h.options());
    A.dh = parts.data_ptr<float>();
  }
  const unsigned blocks = (unsigned)((B + TD_ROWS - 1) / TD_ROWS);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(actor_heads_bwd_dx_kernel, dim3(blocks, 2),
                     dim3(TD_THREADS), 0, stream, A);
  check_launch("actor_heads_bwd_dx_kernel");
  if (want_dh) dh = parts[0] + parts[1];
  std::vector<torch::Tensor> grads;
  if (want_dw) {
    for (int l = 0; l < 4; ++l) {
      grads.push_back(torch::empty_like(weights[2 * l]));
      grads.push_back(torch::empty_like(weights[2 * l + 1]));
      A.dw[l / 2][l % 2] = grads[2 * l].data_ptr<float>();
      A.db[l / 2][l % 2] = grads[2 * l + 1].data_ptr<float>();
    }
    const int64_t hT = H / 16;
    const int64_t tiles = 2 * (hT * hT + hT);
    const unsigned wg = (unsigned)((tiles + AH_DW_WAVES - 1) / AH_DW_WAVES);
    hipLaunchKernelGGL(actor_heads_bwd_dw_kernel, dim3(wg),
                       dim3(AH_DW_WAVES * 64), 0, stream, A);
    check_launch("actor_heads_bwd_dw_kernel");
  }
  return {dh, grads, dlogits};
}

}  // namespace dcg
