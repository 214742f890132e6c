// Fused optimizer tail of one SAC optimizer step (gfx950): the gradient clip
// of clip_grad_norm_, the Adam step and the polyak average of the target
// network, over a whole parameter list in two launches.
//
// The list (up to OT_MAX_TENSORS tensors) is described by an OtTable that is
// passed to both kernels BY VALUE: 56 B per tensor in the kernel-argument
// segment, so a step needs no host-to-device copy and can be recorded into a
// hipGraph (the addresses are those of the capture and stay valid on replay).
//
// Work split: the flat element space is cut into chunks of OT_CHUNK elements
// (OT_THREADS threads x OT_PASSES x one 16-byte access).  A chunk never
// crosses a tensor boundary: tensor k owns max(1, ceil(numel / OT_CHUNK))
// chunks starting at its `chunk0`, and one workgroup serves one chunk.  It
// finds its tensor by scanning the chunk prefix of the table (wave-uniform,
// from the kernel-argument segment).  Thread t of a chunk owns the elements
// 4 * (t + OT_THREADS * pass) + {0..3} on the vector path and on the scalar
// path alike, so a tensor's result does not depend on its alignment.
//
// optim_sumsq_kernel   partials[chunk] = f64 sum of squares of the chunk's
//                      gradients (0 for tensors outside the clip set), folded
//                      in a fixed order: per-thread strided partial, shuffle
//                      tree, waves 0..3 through LDS.  Thread 0 of a tensor's
//                      first chunk adds 1 to the tensor's Adam step counter;
//                      it is done here so that no workgroup of the second
//                      launch races with it.
// optim_apply_kernel   every workgroup folds all partials in the same fixed
//                      order (the same total, bit for bit, in every one),
//                      forms the clip coefficient and the bias corrections
//                      in f64 and applies, per element in f32,
//                        g = grad * (clipped ? c : 1)
//                        m = beta1 * m + (1 - beta1) * g
//                        v = beta2 * v + (1 - beta2) * g * g
//                        p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//                        target = (1 - tau) * target + tau * p   (if any)
//                      grad itself is not scaled in place.
// No float atomics, no grid sync: two calls on the same inputs are bit-equal.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "moments.hpp"
#include "sac_target.hpp"

namespace dcg {

constexpr int OT_THREADS = 256;
constexpr int OT_WAVES = OT_THREADS / 64;
constexpr int OT_PASSES = 4;
constexpr int OT_CHUNK = OT_THREADS * 4 * OT_PASSES;  // 4096 elements
constexpr int OT_MAX_TENSORS = 32;
constexpr int64_t OT_MAX_NUMEL = (int64_t)1 << 30;

struct OtTensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;    // Adam's f32 device scalar
  float* target;  // polyak target, or null
  int32_t numel;
  uint32_t meta;  // first chunk index << 1 | clipped
};
struct OtTable {
  OtTensor t[OT_MAX_TENSORS];
  int32_t n;
};
static_assert(sizeof(OtTensor) == 56, "OtTensor is 56 B of kernel argument");
static_assert(sizeof(OtTable) + 64 <= 4096,
              "the table and the scalars fit the 4 KB kernel-argument limit");

// the tensor that owns `chunk`: the last entry whose first chunk is <= chunk
TD_FN __device__ __forceinline__ int ot_find(const OtTable& T, unsigned chunk) {
  int k = 0;
  for (int i = 1; i < T.n; ++i)
    if ((T.t[i].meta >> 1) <= chunk) k = i;
  return k;
}

TD_FN __device__ __forceinline__ bool ot_aligned(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// elements i .. i+3 of p[0 .. n), zero past the end; one 16-byte access when
// the base is aligned (i is a multiple of 4) and all four exist
TD_FN __device__ __forceinline__ td_f4 ot_load(const float* p, int i, int n,
                                               bool vec) {
  td_f4 x = {0.f, 0.f, 0.f, 0.f};
  if (vec && i + 4 <= n) {
    x = *reinterpret_cast<const td_f4*>(p + i);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) x[j] = p[i + j];
  }
  return x;
}
TD_FN __device__ __forceinline__ void ot_store(float* p, int i, int n, bool vec,
                                               td_f4 x) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<td_f4*>(p + i) = x;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = x[j];
  }
}

// fixed-order workgroup sum (moments.hpp::block_sum on the TD_FN primitives)
TD_FN __device__ __forceinline__ double ot_block_sum(double v, double* l_buf) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = td_wave_sum(v, lane);
  if (lane == 0) l_buf[wave] = v;
  td_barrier();
  double s = l_buf[0];
#pragma unroll
  for (int w = 1; w < OT_WAVES; ++w) s += l_buf[w];
  return s;
}

// b^n by squaring, n a step count
TD_FN __device__ __forceinline__ double ot_ipow(double b, unsigned n) {
  double r = 1.0;
  for (; n; n >>= 1, b *= b)
    if (n & 1) r *= b;
  return r;
}

TD_FN __global__ void __launch_bounds__(OT_THREADS)
optim_sumsq_kernel(OtTable T, double* __restrict__ partials) {
  __shared__ double s_part[OT_WAVES];
  const OtTensor& t = T.t[ot_find(T, blockIdx.x)];
  const int base = (int)(blockIdx.x - (t.meta >> 1)) * OT_CHUNK;
  double s = 0.0;
  if (t.meta & 1) {
    const bool vec = ot_aligned(t.grad);
#pragma unroll
    for (int pass = 0; pass < OT_PASSES; ++pass) {
      const int i = base + 4 * ((int)threadIdx.x + OT_THREADS * pass);
      const td_f4 g = ot_load(t.grad, i, t.numel, vec);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += (double)g[j] * (double)g[j];
    }
  }
  s = ot_block_sum(s, s_part);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    if (base == 0) *t.step += 1.0f;
  }
}

TD_FN __global__ void __launch_bounds__(OT_THREADS)
optim_apply_kernel(OtTable T, const double* __restrict__ partials, int n_part,
                   double lr, double beta1, double beta2, double eps,
                   double max_norm, double tau) {
  __shared__ double s_part[OT_WAVES];
  double total = 0.0;
  for (int k = threadIdx.x; k < n_part; k += OT_THREADS) total += partials[k];
  total = ot_block_sum(total, s_part);

  const OtTensor& t = T.t[ot_find(T, blockIdx.x)];
  const int base = (int)(blockIdx.x - (t.meta >> 1)) * OT_CHUNK;
  // per-tensor scalars in f64, rounded once
  const double c =
      __builtin_fmin(1.0, max_norm / (__builtin_sqrt(total) + 1e-6));
  const float clip = (t.meta & 1) ? (float)c : 1.0f;
  const unsigned step = (unsigned)*t.step;
  const double bc1 = 1.0 - ot_ipow(beta1, step);
  const double bc2 = 1.0 - ot_ipow(beta2, step);
  const float step_size = (float)(lr / bc1);
  const float sqrt_bc2 = (float)__builtin_sqrt(bc2);
  const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1);
  const float b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  const float epsf = (float)eps;
  const float tauf = (float)tau, omtau = (float)(1.0 - tau);
  const bool polyak = t.target != nullptr;
  const bool vec = ot_aligned(t.param) && ot_aligned(t.grad) &&
                   ot_aligned(t.exp_avg) && ot_aligned(t.exp_avg_sq) &&
                   ot_aligned(t.target);
  const int n = t.numel;
#pragma unroll
  for (int pass = 0; pass < OT_PASSES; ++pass) {
    const int i = base + 4 * ((int)threadIdx.x + OT_THREADS * pass);
    if (i >= n) break;
    const td_f4 g = ot_load(t.grad, i, n, vec);
    td_f4 p = ot_load(t.param, i, n, vec);
    td_f4 m = ot_load(t.exp_avg, i, n, vec);
    td_f4 v = ot_load(t.exp_avg_sq, i, n, vec);
    td_f4 tg = {0.f, 0.f, 0.f, 0.f};
    if (polyak) tg = ot_load(t.target, i, n, vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = g[j] * clip;
      m[j] = __builtin_fmaf(b1, m[j], omb1 * gj);
      v[j] = __builtin_fmaf(b2, v[j], omb2 * gj * gj);
      const float denom = __builtin_sqrtf(v[j]) / sqrt_bc2 + epsf;
      p[j] = __builtin_fmaf(-step_size, m[j] / denom, p[j]);
      tg[j] = __builtin_fmaf(tauf, p[j], omtau * tg[j]);
    }
    ot_store(t.param, i, n, vec, p);
    ot_store(t.exp_avg, i, n, vec, m);
    ot_store(t.exp_avg_sq, i, n, vec, v);
    if (polyak) ot_store(t.target, i, n, vec, tg);
  }
}

// One optimizer step over the listed tensors, on the current stream.  targets
// is empty (no polyak) or as long as params, with None where a parameter has
// no target.  Everything is checked before the first launch.
inline void optim_tail(std::vector<torch::Tensor> params,
                       std::vector<torch::Tensor> grads,
                       std::vector<torch::Tensor> exp_avgs,
                       std::vector<torch::Tensor> exp_avg_sqs,
                       std::vector<torch::Tensor> steps,
                       std::vector<c10::optional<torch::Tensor>> targets,
                       std::vector<bool> clipped, double lr, double beta1,
                       double beta2, double eps, double max_norm, double tau) {
  const size_t n = params.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)OT_MAX_TENSORS, "optim_tail: 1 to ",
              OT_MAX_TENSORS, " tensors per call (got ", n, ")");
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_sqs.size() == n && steps.size() == n &&
                  clipped.size() == n &&
                  (targets.empty() || targets.size() == n),
              "optim_tail: the lists differ in length");
  const auto dev = params[0].device();
  auto f32 = [&](const torch::Tensor& t) {
    return t.defined() && t.is_cuda() && t.device() == dev &&
           t.dtype() == torch::kFloat32 && t.is_contiguous() &&
           (reinterpret_cast<uintptr_t>(t.data_ptr()) & 3) == 0;
  };
  OtTable T{};  // unused entries zeroed: the argument is deterministic
  T.n = (int32_t)n;
  int64_t chunks = 0;
  for (size_t k = 0; k < n; ++k) {
    const int64_t numel = params[k].numel();
    TORCH_CHECK(f32(params[k]) && f32(grads[k]) && f32(exp_avgs[k]) &&
                    f32(exp_avg_sqs[k]) && f32(steps[k]),
                "optim_tail: tensor ", k, ": param, grad, exp_avg, exp_avg_sq "
                "and step must be contiguous f32 on one GPU");
    TORCH_CHECK(steps[k].dim() == 0, "optim_tail: tensor ", k,
                ": step must be 0-dim");
    TORCH_CHECK(numel <= OT_MAX_NUMEL && grads[k].numel() == numel &&
                    exp_avgs[k].numel() == numel &&
                    exp_avg_sqs[k].numel() == numel,
                "optim_tail: tensor ", k, ": numels differ or exceed 2^30");
    OtTensor& t = T.t[k];
    t.target = nullptr;
    if (!targets.empty() && targets[k].has_value()) {
      TORCH_CHECK(f32(*targets[k]) && targets[k]->numel() == numel,
                  "optim_tail: tensor ", k, ": target must be contiguous f32 "
                  "of the parameter's numel on its GPU");
      t.target = targets[k]->data_ptr<float>();
    }
    t.param = params[k].data_ptr<float>();
    t.grad = grads[k].data_ptr<float>();
    t.exp_avg = exp_avgs[k].data_ptr<float>();
    t.exp_avg_sq = exp_avg_sqs[k].data_ptr<float>();
    t.step = steps[k].data_ptr<float>();
    t.numel = (int32_t)numel;
    t.meta = ((uint32_t)chunks << 1) | (clipped[k] ? 1u : 0u);
    chunks += numel == 0 ? 1 : (numel + OT_CHUNK - 1) / OT_CHUNK;
  }
  TORCH_CHECK(chunks < ((int64_t)1 << 30), "optim_tail: too many chunks");
  auto partials = torch::empty(
      {chunks}, params[0].options().dtype(torch::kFloat64));
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)chunks),
                     dim3(OT_THREADS), 0, stream, T,
                     partials.data_ptr<double>());
  check_launch("optim_sumsq_kernel");
  hipLaunchKernelGGL(optim_apply_kernel, dim3((unsigned)chunks),
                     dim3(OT_THREADS), 0, stream, T,
                     partials.data_ptr<double>(), (int)chunks, lr, beta1,
                     beta2, eps, max_norm, tau);
  check_launch("optim_apply_kernel");
}

}  // namespace dcg
