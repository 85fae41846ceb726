// Hand-written CDNA4 (gfx950 / MI355X) kernels for the IMPALA hot path.
//
// Design notes (see /root/repo/SURVEY.md §2.4 for the op inventory):
// - Shapes are small ([T=80, B=8..32, A~6..18], H≈256..520): on MI355X these
//   ops are LAUNCH- and LATENCY-bound, not FLOP-bound. The win over stock
//   PyTorch is fusing each algorithmic stage (V-trace: ~15 eager kernels +
//   an 80-iteration Python loop; LSTM: ~5 kernels × T steps × layers) into
//   ONE kernel, keeping every intermediate in registers/LDS.
// - V-trace's reverse-time scan is sequential per batch column: one
//   workgroup per column, wave-parallel over T for the log-prob phase
//   (ref math: torchbeast/core/vtrace.py:91-139).
// - The LSTM unroll is a persistent cooperative kernel: the T-step
//   recurrence runs inside one launch with grid.sync() between the gate
//   GEMV phase and the state-update phase, with the input GEMM
//   (x @ W_ih^T, the parallelizable 90% of the FLOPs) hoisted out to one
//   rocBLAS GEMM over all T (ref behavior: monobeast.py:599-611 —
//   done-masked state resets between steps).
// - All block sizes are multiples of the 64-wide wavefront.

#include <hip/hip_runtime.h>
#include <hip/hip_cooperative_groups.h>
#include <hiprand/hiprand_kernel.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>

#include <climits>
#include <vector>

#include "atari_trunk.h"
#include "conv_mfma.h"

namespace tbamd {
std::vector<double> barrier_probe(int64_t variant, int64_t wgs, int64_t iters);
double launch_probe(int64_t iters);
}  // namespace tbamd (probes.hip)

namespace cg = cooperative_groups;

#define DEVCHECK(x) TORCH_CHECK(x == hipSuccess, "HIP error: ", hipGetErrorString(x))

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---------------------------------------------------------------------------
// V-trace: log-probs + rho/c clip + reverse scan + pg advantages, one launch.
// ---------------------------------------------------------------------------

// The per-element arithmetic shared by vtrace_kernel (from logits) and
// vtrace_iw_kernel (from log_rhos): both call these, so the two entry points
// cannot drift. A clip threshold of +inf means "do not clip": fminf(rho, inf)
// is rho exactly. c is clipped at 1 regardless, then scaled by lambda
// (arXiv:1802.01561 Remark 2); lambda = 1 multiplies exactly.
__device__ __forceinline__ void vtrace_clip(float log_rho, float clip_rho,
                                            float lambda, float* crho,
                                            float* c) {
  const float rho = __expf(log_rho);
  *crho = fminf(rho, clip_rho);
  *c = lambda * fminf(rho, 1.f);
}

__device__ __forceinline__ float vtrace_delta(float crho, float r, float disc,
                                              float v_next, float v) {
  return crho * (r + disc * v_next - v);
}

__device__ __forceinline__ float vtrace_scan_step(float delta, float disc,
                                                  float c, float acc) {
  return delta + disc * c * acc;
}

__device__ __forceinline__ float vtrace_advantage(float log_rho, float clip_pg,
                                                  float r, float disc,
                                                  float vs_next, float v) {
  const float rho = __expf(log_rho);
  return fminf(rho, clip_pg) * (r + disc * vs_next - v);
}

// Phases 2 and 3 of both kernels, entered after phase 1 has filled s_cs and
// s_delta: the reverse recurrence on one thread, then vs and pg_adv
// thread-strided over T. log_rhos is read back from global memory (written
// by this workgroup's phase 1 in vtrace_kernel, an input in vtrace_iw_kernel)
// and exp'd again rather than kept in LDS.
__device__ __forceinline__ void vtrace_scan_and_outputs(
    const float* s_cs, const float* s_delta, float* s_vmv,
    const float* log_rhos, const float* discounts, const float* rewards,
    const float* values, const float* bootstrap, float clip_pg, int T, int B,
    int b, float* vs, float* pg_adv) {
  __syncthreads();

  if (threadIdx.x == 0) {
    // The inherently sequential reverse recurrence over T.
    float acc = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      acc = vtrace_scan_step(s_delta[t], discounts[(int64_t)t * B + b],
                             s_cs[t], acc);
      s_vmv[t] = acc;
    }
  }
  __syncthreads();

  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const int64_t idx = (int64_t)t * B + b;
    const float v = values[idx];
    vs[idx] = s_vmv[t] + v;
    const float vs_next =
        (t + 1 < T) ? (s_vmv[t + 1] + values[idx + B]) : bootstrap[b];
    pg_adv[idx] = vtrace_advantage(log_rhos[idx], clip_pg, rewards[idx],
                                   discounts[idx], vs_next, v);
  }
}

// One workgroup per batch column b. Dynamic LDS: [3*T] floats
// (cs, deltas, vs_minus_v).
__global__ void vtrace_kernel(
    const float* __restrict__ behavior_logits,  // [T,B,A]
    const float* __restrict__ target_logits,    // [T,B,A]
    const int64_t* __restrict__ actions,        // [T,B]
    const float* __restrict__ discounts,        // [T,B]
    const float* __restrict__ rewards,          // [T,B]
    const float* __restrict__ values,           // [T,B]
    const float* __restrict__ bootstrap,        // [B]
    float clip_rho, float clip_pg, float lambda, int T, int B, int A,
    float* __restrict__ vs,        // [T,B]
    float* __restrict__ pg_adv,    // [T,B]
    float* __restrict__ log_rhos,  // [T,B]
    float* __restrict__ blp,       // [T,B]
    float* __restrict__ tlp) {     // [T,B]
  extern __shared__ float smem[];
  float* s_cs = smem;           // [T]
  float* s_delta = smem + T;    // [T]
  float* s_vmv = smem + 2 * T;  // [T]

  const int b = blockIdx.x;

  auto log_prob = [&](const float* logits, int t, int64_t a) {
    const float* row = logits + ((int64_t)t * B + b) * A;
    float m = row[0];
    for (int j = 1; j < A; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j < A; ++j) s += __expf(row[j] - m);
    return row[a] - m - __logf(s);
  };

  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const int64_t idx = (int64_t)t * B + b;
    const int64_t a = actions[idx];
    const float t_lp = log_prob(target_logits, t, a);
    const float b_lp = log_prob(behavior_logits, t, a);
    const float lr = t_lp - b_lp;
    tlp[idx] = t_lp;
    blp[idx] = b_lp;
    log_rhos[idx] = lr;

    float crho, c;
    vtrace_clip(lr, clip_rho, lambda, &crho, &c);
    s_cs[t] = c;
    const float v_next = (t + 1 < T) ? values[idx + B] : bootstrap[b];
    s_delta[t] = vtrace_delta(crho, rewards[idx], discounts[idx], v_next,
                              values[idx]);
  }
  vtrace_scan_and_outputs(s_cs, s_delta, s_vmv, log_rhos, discounts, rewards,
                          values, bootstrap, clip_pg, T, B, b, vs, pg_adv);
}

// vtrace_kernel without the log-prob phase: log_rhos is an input (any policy
// head, not only one softmax). Same grid, LDS layout and arithmetic.
__global__ void vtrace_iw_kernel(
    const float* __restrict__ log_rhos,   // [T,B]
    const float* __restrict__ discounts,  // [T,B]
    const float* __restrict__ rewards,    // [T,B]
    const float* __restrict__ values,     // [T,B]
    const float* __restrict__ bootstrap,  // [B]
    float clip_rho, float clip_pg, float lambda, int T, int B,
    float* __restrict__ vs,        // [T,B]
    float* __restrict__ pg_adv) {  // [T,B]
  extern __shared__ float smem[];
  float* s_cs = smem;           // [T]
  float* s_delta = smem + T;    // [T]
  float* s_vmv = smem + 2 * T;  // [T]

  const int b = blockIdx.x;

  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const int64_t idx = (int64_t)t * B + b;
    float crho, c;
    vtrace_clip(log_rhos[idx], clip_rho, lambda, &crho, &c);
    s_cs[t] = c;
    const float v_next = (t + 1 < T) ? values[idx + B] : bootstrap[b];
    s_delta[t] = vtrace_delta(crho, rewards[idx], discounts[idx], v_next,
                              values[idx]);
  }
  vtrace_scan_and_outputs(s_cs, s_delta, s_vmv, log_rhos, discounts, rewards,
                          values, bootstrap, clip_pg, T, B, b, vs, pg_adv);
}

// A tensor of the wrong shape, dtype or device would be an out-of-bounds or
// misread access on the device; reject it on the host instead. `first` is
// the entry point's first tensor, which fixes the GPU and T, B (and A).
static void check_vtrace_tensor(const torch::Tensor& t,
                                const torch::Tensor& first,
                                at::IntArrayRef shape, const char* name,
                                bool integral = false) {
  TORCH_CHECK(t.device() == first.device(), "vtrace: ", name, " is on ",
              t.device(), ", expected ", first.device());
  if (integral) {
    TORCH_CHECK(at::isIntegralType(t.scalar_type(), /*includeBool=*/false),
                "vtrace: ", name, " must be an integer tensor, got ",
                t.scalar_type());
  } else {
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "vtrace: ", name,
                " must be float32, got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), "vtrace: ", name, " must be contiguous");
  }
  TORCH_CHECK(t.sizes() == shape, "vtrace: ", name, " has shape ", t.sizes(),
              ", expected ", shape);
}

// Scalars and sizes common to both entry points. Returns the dynamic LDS
// request, which has to fit the device's per-workgroup limit: the kernels
// keep three [T] float rows in LDS.
static size_t check_vtrace_launch(const torch::Tensor& first, int64_t T,
                                  int64_t B, int64_t A, double lambda) {
  TORCH_CHECK(T >= 1 && B >= 1 && A >= 1,
              "vtrace: T, B and A must be >= 1, got T=", T, " B=", B,
              " A=", A);
  TORCH_CHECK(B <= INT_MAX && A <= INT_MAX, "vtrace: B=", B, " or A=", A,
              " exceeds the kernel's 32-bit sizes");
  TORCH_CHECK(lambda >= 0.0 && lambda <= 1.0,
              "vtrace: lambda must be in [0, 1], got ", lambda);
  const size_t limit =
      at::cuda::getDeviceProperties(first.get_device())->sharedMemPerBlock;
  TORCH_CHECK((uint64_t)T <= limit / (3 * sizeof(float)),
              "vtrace: unroll length T=", T, " needs ", 3 * sizeof(float),
              "*T bytes of LDS, the device allows ", limit,
              " per workgroup (T <= ", limit / (3 * sizeof(float)), ")");
  return 3 * (size_t)T * sizeof(float);
}

// Actions are not range-checked: that needs a device-side reduction and a
// host sync, which the learner step (and hipGraph capture) cannot afford.
// An action outside [0, A) reads a neighbouring logit or past the buffer.
std::vector<torch::Tensor> vtrace_from_logits(
    torch::Tensor behavior_logits, torch::Tensor target_logits,
    torch::Tensor actions, torch::Tensor discounts, torch::Tensor rewards,
    torch::Tensor values, torch::Tensor bootstrap, double clip_rho,
    double clip_pg, double lambda = 1.0) {
  TORCH_CHECK(behavior_logits.is_cuda() && behavior_logits.dim() == 3,
              "vtrace: behavior_logits must be a [T,B,A] GPU tensor");
  const int64_t T = behavior_logits.size(0);
  const int64_t B = behavior_logits.size(1);
  const int64_t A = behavior_logits.size(2);
  check_vtrace_tensor(behavior_logits, behavior_logits, {T, B, A},
                      "behavior_logits");
  check_vtrace_tensor(target_logits, behavior_logits, {T, B, A},
                      "target_logits");
  check_vtrace_tensor(actions, behavior_logits, {T, B}, "actions",
                      /*integral=*/true);
  check_vtrace_tensor(discounts, behavior_logits, {T, B}, "discounts");
  check_vtrace_tensor(rewards, behavior_logits, {T, B}, "rewards");
  check_vtrace_tensor(values, behavior_logits, {T, B}, "values");
  check_vtrace_tensor(bootstrap, behavior_logits, {B}, "bootstrap");
  const size_t lds = check_vtrace_launch(behavior_logits, T, B, A, lambda);

  const at::cuda::CUDAGuard device_guard(behavior_logits.device());
  auto opts = behavior_logits.options();
  auto vs = torch::empty({T, B}, opts);
  auto pg_adv = torch::empty({T, B}, opts);
  auto log_rhos = torch::empty({T, B}, opts);
  auto blp = torch::empty({T, B}, opts);
  auto tlp = torch::empty({T, B}, opts);
  auto actions_i64 = actions.to(torch::kInt64).contiguous();

  const int threads = 256;
  hipLaunchKernelGGL(vtrace_kernel, dim3(B), dim3(threads), lds,
                     at::cuda::getCurrentCUDAStream(),
                     behavior_logits.data_ptr<float>(),
                     target_logits.data_ptr<float>(),
                     actions_i64.data_ptr<int64_t>(),
                     discounts.data_ptr<float>(), rewards.data_ptr<float>(),
                     values.data_ptr<float>(), bootstrap.data_ptr<float>(),
                     (float)clip_rho, (float)clip_pg, (float)lambda, (int)T,
                     (int)B, (int)A, vs.data_ptr<float>(),
                     pg_adv.data_ptr<float>(), log_rhos.data_ptr<float>(),
                     blp.data_ptr<float>(), tlp.data_ptr<float>());
  DEVCHECK(hipGetLastError());
  return {vs, pg_adv, log_rhos, blp, tlp};
}

std::vector<torch::Tensor> vtrace_from_importance_weights(
    torch::Tensor log_rhos, torch::Tensor discounts, torch::Tensor rewards,
    torch::Tensor values, torch::Tensor bootstrap, double clip_rho,
    double clip_pg, double lambda = 1.0) {
  TORCH_CHECK(log_rhos.is_cuda() && log_rhos.dim() == 2,
              "vtrace: log_rhos must be a [T,B] GPU tensor");
  const int64_t T = log_rhos.size(0);
  const int64_t B = log_rhos.size(1);
  check_vtrace_tensor(log_rhos, log_rhos, {T, B}, "log_rhos");
  check_vtrace_tensor(discounts, log_rhos, {T, B}, "discounts");
  check_vtrace_tensor(rewards, log_rhos, {T, B}, "rewards");
  check_vtrace_tensor(values, log_rhos, {T, B}, "values");
  check_vtrace_tensor(bootstrap, log_rhos, {B}, "bootstrap");
  const size_t lds = check_vtrace_launch(log_rhos, T, B, /*A=*/1, lambda);

  const at::cuda::CUDAGuard device_guard(log_rhos.device());
  auto opts = log_rhos.options();
  auto vs = torch::empty({T, B}, opts);
  auto pg_adv = torch::empty({T, B}, opts);

  const int threads = 256;
  hipLaunchKernelGGL(vtrace_iw_kernel, dim3(B), dim3(threads), lds,
                     at::cuda::getCurrentCUDAStream(),
                     log_rhos.data_ptr<float>(), discounts.data_ptr<float>(),
                     rewards.data_ptr<float>(), values.data_ptr<float>(),
                     bootstrap.data_ptr<float>(), (float)clip_rho,
                     (float)clip_pg, (float)lambda, (int)T, (int)B,
                     vs.data_ptr<float>(), pg_adv.data_ptr<float>());
  DEVCHECK(hipGetLastError());
  return {vs, pg_adv};
}

// ---------------------------------------------------------------------------
// Fused IMPALA loss: pg + baseline + entropy values AND gradients, one pass.
// ---------------------------------------------------------------------------

// One thread per (t, b) row; block-reduced partial sums -> atomicAdd.
__global__ void impala_loss_kernel(
    const float* __restrict__ logits,     // [R, A], R = T*B
    const float* __restrict__ baseline,   // [R]
    const int64_t* __restrict__ actions,  // [R]
    const float* __restrict__ pg_advantages,  // [R]
    const float* __restrict__ vs,             // [R]
    int64_t R, int A,
    float* __restrict__ losses,        // [3]: pg, baseline, entropy
    float* __restrict__ d_logits_pg,   // [R, A]
    float* __restrict__ d_logits_ent,  // [R, A]
    float* __restrict__ d_baseline) {  // [R]
  __shared__ float red[3][256];

  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  float pg_sum = 0.f, bl_sum = 0.f, ent_sum = 0.f;

  if (row < R) {
    const float* z = logits + row * A;
    float m = z[0];
    for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
    float s = 0.f;
    for (int j = 0; j < A; ++j) s += __expf(z[j] - m);
    const float lse = m + __logf(s);
    const float inv_s = 1.f / s;

    // neg-entropy of this row: sum p*logp.
    float neg_ent = 0.f;
    for (int j = 0; j < A; ++j) {
      const float lp = z[j] - lse;
      neg_ent += __expf(z[j] - m) * inv_s * lp;
    }

    const int64_t a = actions[row];
    const float adv = pg_advantages[row];
    const float ce = lse - z[a];  // -log p[a]
    pg_sum = ce * adv;
    ent_sum = neg_ent;
    const float db = baseline[row] - vs[row];
    bl_sum = 0.5f * db * db;
    d_baseline[row] = db;

    for (int j = 0; j < A; ++j) {
      const float p = __expf(z[j] - m) * inv_s;
      const float lp = z[j] - lse;
      d_logits_pg[row * A + j] = adv * (p - (j == a ? 1.f : 0.f));
      d_logits_ent[row * A + j] = p * (lp - neg_ent);
    }
  }

  red[0][threadIdx.x] = pg_sum;
  red[1][threadIdx.x] = bl_sum;
  red[2][threadIdx.x] = ent_sum;
  __syncthreads();
  for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      red[0][threadIdx.x] += red[0][threadIdx.x + stride];
      red[1][threadIdx.x] += red[1][threadIdx.x + stride];
      red[2][threadIdx.x] += red[2][threadIdx.x + stride];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(&losses[0], red[0][0]);
    atomicAdd(&losses[1], red[1][0]);
    atomicAdd(&losses[2], red[2][0]);
  }
}

std::vector<torch::Tensor> fused_impala_loss_fwd(
    torch::Tensor logits, torch::Tensor baseline, torch::Tensor actions,
    torch::Tensor pg_advantages, torch::Tensor vs) {
  TORCH_CHECK(logits.is_cuda(), "fused_impala_loss: expected GPU tensors");
  const int A = logits.size(-1);
  const int64_t R = logits.numel() / A;
  auto opts = logits.options();
  auto losses = torch::zeros({3}, opts);
  auto d_logits_pg = torch::empty_like(logits);
  auto d_logits_ent = torch::empty_like(logits);
  auto d_baseline = torch::empty_like(baseline);
  auto actions_i64 = actions.to(torch::kInt64).contiguous();

  const int threads = 256;
  hipLaunchKernelGGL(impala_loss_kernel, dim3(ceil_div(R, threads)),
                     dim3(threads), 0, at::cuda::getCurrentCUDAStream(),
                     logits.data_ptr<float>(), baseline.data_ptr<float>(),
                     actions_i64.data_ptr<int64_t>(),
                     pg_advantages.data_ptr<float>(), vs.data_ptr<float>(), R,
                     A, losses.data_ptr<float>(),
                     d_logits_pg.data_ptr<float>(),
                     d_logits_ent.data_ptr<float>(),
                     d_baseline.data_ptr<float>());
  return {losses[0], losses[1], losses[2], d_logits_pg, d_logits_ent,
          d_baseline};
}

// ---------------------------------------------------------------------------
// Fused global-norm clip + RMSProp over a flat parameter buffer.
// ---------------------------------------------------------------------------

__global__ void grad_norm_sq_kernel(const float* __restrict__ grad, int64_t n,
                                    float* __restrict__ out) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float g = grad[i];
    acc += g * g;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int stride = blockDim.x / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) red[threadIdx.x] += red[threadIdx.x + stride];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out, red[0]);
}

// torch.optim.RMSprop semantics (no weight decay). MOMENTUM adds the velocity
// buffer, CENTERED the running gradient mean; <false,false> touches neither
// pointer and keeps the plain update's expression order.
template <bool MOMENTUM, bool CENTERED>
__global__ void rmsprop_update_kernel(
    float* __restrict__ param, const float* __restrict__ grad,
    float* __restrict__ square_avg,
    float* __restrict__ momentum_buf,  // MOMENTUM only
    float* __restrict__ grad_avg,      // CENTERED only
    int64_t n, float lr,
    const float* __restrict__ lr_ptr,  // overrides lr when non-null
    float alpha, float eps, float momentum, float clip_norm,
    const float* __restrict__ norm_sq, float* __restrict__ norm_out) {
  const float norm = sqrtf(*norm_sq);
  float coef = 1.f;
  if (clip_norm > 0.f) coef = fminf(1.f, clip_norm / (norm + 1e-6f));
  if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  // hipGraph capture freezes by-value arguments; when the learning rate
  // must keep decaying across graph replays it is read from device memory.
  if (lr_ptr != nullptr) lr = *lr_ptr;

  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float g = grad[i] * coef;
    float s = square_avg[i];
    s = alpha * s + (1.f - alpha) * g * g;
    square_avg[i] = s;
    if constexpr (!MOMENTUM && !CENTERED) {
      param[i] -= lr * g / (sqrtf(s) + eps);
    } else {
      float avg;
      if constexpr (CENTERED) {
        float m = grad_avg[i];
        m += (g - m) * (1.f - alpha);
        grad_avg[i] = m;
        // Rounding can push s - m*m below zero (torch yields NaN there).
        avg = sqrtf(fmaxf(s - m * m, 0.f)) + eps;
      } else {
        avg = sqrtf(s) + eps;
      }
      if constexpr (MOMENTUM) {
        // lr scales the velocity at the update, never inside the buffer.
        const float b = momentum * momentum_buf[i] + g / avg;
        momentum_buf[i] = b;
        param[i] -= lr * b;
      } else {
        param[i] -= lr * g / avg;
      }
    }
  }
}

// A short or mistyped buffer would be an out-of-bounds access on the device;
// reject it on the host instead.
static void check_rmsprop_buffer(const torch::Tensor& t,
                                 const torch::Tensor& param,
                                 const char* name) {
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, "rmsprop: ", name,
              " must be float32, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), "rmsprop: ", name, " must be contiguous");
  TORCH_CHECK(t.device() == param.device(), "rmsprop: ", name, " is on ",
              t.device(), ", param on ", param.device());
  TORCH_CHECK(t.numel() == param.numel(), "rmsprop: ", name, " has ",
              t.numel(), " elements, param has ", param.numel());
}

torch::Tensor rmsprop_step(torch::Tensor param, torch::Tensor grad,
                           torch::Tensor square_avg, double lr, double alpha,
                           double eps, double clip_norm,
                           std::optional<torch::Tensor> lr_tensor = {},
                           std::optional<torch::Tensor> momentum_buf = {},
                           std::optional<torch::Tensor> grad_avg = {},
                           double momentum = 0.0) {
  TORCH_CHECK(param.is_cuda() && param.dim() == 1 && param.numel() > 0,
              "rmsprop: flat GPU tensor");
  check_rmsprop_buffer(param, param, "param");
  check_rmsprop_buffer(grad, param, "grad");
  check_rmsprop_buffer(square_avg, param, "square_avg");
  TORCH_CHECK(momentum >= 0.0, "rmsprop: momentum must be >= 0, got ",
              momentum);
  const bool use_momentum = momentum > 0.0;
  const bool centered = grad_avg.has_value();
  TORCH_CHECK(!use_momentum || momentum_buf.has_value(),
              "rmsprop: momentum=", momentum, " needs a momentum_buf");
  if (momentum_buf) check_rmsprop_buffer(*momentum_buf, param, "momentum_buf");
  if (grad_avg) check_rmsprop_buffer(*grad_avg, param, "grad_avg");
  if (lr_tensor) {
    TORCH_CHECK(lr_tensor->scalar_type() == torch::kFloat32 &&
                    lr_tensor->numel() >= 1 &&
                    lr_tensor->device() == param.device(),
                "rmsprop: lr_tensor must be a float32 tensor on param's "
                "device");
  }
  const int64_t n = param.numel();
  auto norm_sq = torch::zeros({1}, param.options());
  auto norm_out = torch::empty({}, param.options());
  const float* lr_p =
      lr_tensor ? lr_tensor->data_ptr<float>() : nullptr;
  float* mom_p = use_momentum ? momentum_buf->data_ptr<float>() : nullptr;
  float* gavg_p = centered ? grad_avg->data_ptr<float>() : nullptr;

  const int threads = 256;
  const int blocks = std::min<int64_t>(2048, ceil_div(n, threads));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(grad_norm_sq_kernel, dim3(blocks), dim3(threads), 0,
                     stream, grad.data_ptr<float>(), n,
                     norm_sq.data_ptr<float>());
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream,
                       param.data_ptr<float>(), grad.data_ptr<float>(),
                       square_avg.data_ptr<float>(), mom_p, gavg_p, n,
                       (float)lr, lr_p, (float)alpha, (float)eps,
                       (float)momentum, (float)clip_norm,
                       norm_sq.data_ptr<float>(), norm_out.data_ptr<float>());
  };
  if (use_momentum) {
    if (centered) launch(rmsprop_update_kernel<true, true>);
    else launch(rmsprop_update_kernel<true, false>);
  } else {
    if (centered) launch(rmsprop_update_kernel<false, true>);
    else launch(rmsprop_update_kernel<false, false>);
  }
  return norm_out;
}

// ---------------------------------------------------------------------------
// Policy sampling: softmax + multinomial (philox) / argmax.
// ---------------------------------------------------------------------------

__global__ void policy_sample_kernel(const float* __restrict__ logits,
                                     int64_t N, int A, bool greedy,
                                     uint64_t seed,
                                     int64_t* __restrict__ actions) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (row >= N) return;
  const float* z = logits + row * A;

  if (greedy) {
    float best = z[0];
    int64_t best_j = 0;
    for (int j = 1; j < A; ++j) {
      if (z[j] > best) {
        best = z[j];
        best_j = j;
      }
    }
    actions[row] = best_j;
    return;
  }

  float m = z[0];
  for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
  float s = 0.f;
  for (int j = 0; j < A; ++j) s += __expf(z[j] - m);

  hiprandStatePhilox4_32_10_t state;
  hiprand_init(seed, row, 0, &state);
  const float u = hiprand_uniform(&state) * s;

  float cdf = 0.f;
  int64_t pick = A - 1;
  for (int j = 0; j < A; ++j) {
    cdf += __expf(z[j] - m);
    if (u <= cdf) {
      pick = j;
      break;
    }
  }
  actions[row] = pick;
}

torch::Tensor policy_sample(torch::Tensor logits, bool greedy, int64_t seed) {
  TORCH_CHECK(logits.is_cuda(), "policy_sample: expected GPU tensor");
  const int A = logits.size(-1);
  const int64_t N = logits.numel() / A;
  auto out_sizes = logits.sizes().vec();
  out_sizes.pop_back();
  auto actions =
      torch::empty(out_sizes, logits.options().dtype(torch::kInt64));
  const int threads = 256;
  hipLaunchKernelGGL(policy_sample_kernel, dim3(ceil_div(N, threads)),
                     dim3(threads), 0, at::cuda::getCurrentCUDAStream(),
                     logits.data_ptr<float>(), N, A, greedy, (uint64_t)seed,
                     actions.data_ptr<int64_t>());
  return actions;
}

// ---------------------------------------------------------------------------
// Done-masked LSTM unroll (persistent cooperative kernel per layer).
// ---------------------------------------------------------------------------
// Done-masked LSTM unroll: v4 persistent kernels live in lstm_v4.hip.
// ---------------------------------------------------------------------------

namespace tbamd {
// v4 persistent-kernel launchers (lstm_v4.hip): h-slice ownership, LDS
// bf16 weight slices, agent-scope barriers (no cg::grid_sync).
struct Lstm4Geometry { int hs; int nblocks; size_t fwd_lds; size_t bwd_lds; };
Lstm4Geometry lstm4_geometry(int B, int H);
void lstm4_fwd_launch(torch::Tensor precomp, torch::Tensor w_hh_bf,
                      torch::Tensor notdone, torch::Tensor h0,
                      torch::Tensor c0, torch::Tensor out, torch::Tensor gates,
                      torch::Tensor hm, torch::Tensor cm,
                      torch::Tensor c_stash, torch::Tensor hT,
                      torch::Tensor cT);
void lstm4_bwd_launch(torch::Tensor gates, torch::Tensor cm,
                      torch::Tensor c_stash, torch::Tensor w_hh_t_bf,
                      torch::Tensor notdone, torch::Tensor d_out,
                      torch::Tensor d_hT, torch::Tensor d_cT,
                      torch::Tensor dgates, torch::Tensor dh_out,
                      torch::Tensor dc_out);

}  // namespace tbamd

// Multi-layer forward. flat_weights: [w_ih, w_hh, b_ih, b_hh] per layer.
std::vector<torch::Tensor> lstm_unroll_fwd(
    torch::Tensor x, torch::Tensor notdone, torch::Tensor h0,
    torch::Tensor c0, std::vector<torch::Tensor> flat_weights) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "lstm: x must be [T,B,I] on GPU");
  const int T = x.size(0);
  const int B = x.size(1);
  const int L = flat_weights.size() / 4;
  const int H = h0.size(2);
  auto opts = x.options();
  auto stream = at::cuda::getCurrentCUDAStream();

  auto notdone_f = notdone.to(torch::kFloat32).contiguous();
  auto hT = torch::empty({L, B, H}, opts);
  auto cT = torch::empty({L, B, H}, opts);

  std::vector<torch::Tensor> stash;  // per layer: input, gates, hm, cm, c
  torch::Tensor layer_in = x.contiguous();
  torch::Tensor out;

  for (int l = 0; l < L; ++l) {
    auto w_ih = flat_weights[4 * l].contiguous();
    auto w_hh = flat_weights[4 * l + 1].contiguous();
    auto bias = (flat_weights[4 * l + 2] + flat_weights[4 * l + 3]);

    // The parallel 90%: one GEMM over all T*B rows.
    auto precomp =
        (torch::matmul(layer_in.reshape({(int64_t)T * B, -1}), w_ih.t()) +
         bias)
            .reshape({T, B, 4 * H})
            .contiguous();

    out = torch::empty({T, B, H}, opts);
    auto gates = torch::empty({T, B, 4 * H}, opts);
    auto hm = torch::empty({T, B, H}, opts);
    auto cm = torch::empty({T, B, H}, opts);
    auto c_out = torch::empty({T, B, H}, opts);
    auto h0_l = h0[l].contiguous();
    auto c0_l = c0[l].contiguous();

    auto w_hh_bf = w_hh.to(torch::kBFloat16).contiguous();
    tbamd::lstm4_fwd_launch(precomp, w_hh_bf, notdone_f, h0_l, c0_l, out,
                            gates, hm, cm, c_out, hT[l], cT[l]);

    stash.push_back(layer_in);
    stash.push_back(gates);
    stash.push_back(hm);
    stash.push_back(cm);
    stash.push_back(c_out);
    layer_in = out;
  }

  std::vector<torch::Tensor> result = {out, hT, cT};
  result.insert(result.end(), stash.begin(), stash.end());
  return result;
}

std::vector<torch::Tensor> lstm_unroll_bwd(
    torch::Tensor notdone, torch::Tensor h0, torch::Tensor c0,
    std::vector<torch::Tensor> flat_weights,
    std::vector<torch::Tensor> stash, torch::Tensor d_out_top,
    torch::Tensor d_hT, torch::Tensor d_cT) {
  const int L = flat_weights.size() / 4;
  const int T = d_out_top.size(0);
  const int B = d_out_top.size(1);
  const int H = h0.size(2);
  auto opts = d_out_top.options();
  auto stream = at::cuda::getCurrentCUDAStream();
  auto notdone_f = notdone.to(torch::kFloat32).contiguous();

  auto d_h0 = torch::empty({L, B, H}, opts);
  auto d_c0 = torch::empty({L, B, H}, opts);
  std::vector<torch::Tensor> d_weights(4 * L);

  torch::Tensor d_out = d_out_top.contiguous();
  for (int l = L - 1; l >= 0; --l) {
    auto layer_in = stash[5 * l];
    auto gates = stash[5 * l + 1];
    auto hm = stash[5 * l + 2];
    auto cm = stash[5 * l + 3];
    auto c_out = stash[5 * l + 4];
    auto w_ih = flat_weights[4 * l].contiguous();
    auto w_hh = flat_weights[4 * l + 1].contiguous();
    auto w_hh_t_bf =
        w_hh.t().contiguous().to(torch::kBFloat16).contiguous();  // [H,4H]

    auto dgates = torch::empty({T, B, 4 * H}, opts);
    auto dh = torch::empty({B, H}, opts);
    auto dc = torch::empty({B, H}, opts);
    auto d_hT_l = d_hT[l].contiguous();
    auto d_cT_l = d_cT[l].contiguous();
    tbamd::lstm4_bwd_launch(gates, cm, c_out, w_hh_t_bf, notdone_f, d_out,
                            d_hT_l, d_cT_l, dgates, dh, dc);

    // Weight/input grads: plain GEMMs (rocBLAS).
    auto dg2 = dgates.reshape({(int64_t)T * B, 4 * H});
    auto in2 = layer_in.reshape({(int64_t)T * B, -1});
    auto hm2 = hm.reshape({(int64_t)T * B, H});
    d_weights[4 * l] = torch::matmul(dg2.t(), in2);       // dW_ih
    d_weights[4 * l + 1] = torch::matmul(dg2.t(), hm2);   // dW_hh
    auto db = dg2.sum(0);
    d_weights[4 * l + 2] = db;                            // db_ih
    d_weights[4 * l + 3] = db.clone();                    // db_hh
    d_h0[l] = dh;
    d_c0[l] = dc;

    if (l > 0) {
      d_out = torch::matmul(dg2, w_ih).reshape({T, B, -1});
    } else {
      d_out = torch::matmul(dg2, w_ih).reshape({T, B, -1});
    }
  }

  std::vector<torch::Tensor> result = {d_out, d_h0, d_c0};
  result.insert(result.end(), d_weights.begin(), d_weights.end());
  return result;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("atari_trunk_fwd", &tbamd::atari_trunk_fwd);
  m.def("atari_trunk_supported", &tbamd::atari_trunk_supported);
  m.def("conv_trunk_fwd", &tbamd::conv_trunk_fwd);
  m.def("conv_trunk_mask_d3", &tbamd::conv_trunk_mask_d3);
  m.def("conv_trunk_dgrad3", &tbamd::conv_trunk_dgrad3);
  m.def("conv_trunk_dgrad2", &tbamd::conv_trunk_dgrad2);
  m.def("conv_trunk_wgrad1", &tbamd::conv_trunk_wgrad1);
  m.def("conv_trunk_wgrad2", &tbamd::conv_trunk_wgrad2);
  m.def("conv_trunk_wgrad3", &tbamd::conv_trunk_wgrad3);
  m.def("resnet_conv", &tbamd::resnet_conv);
  m.def("resnet_conv_supported", &tbamd::resnet_conv_supported);
  m.def("resnet_conv_wgrad", &tbamd::resnet_conv_wgrad);
  m.def("resnet_conv_any", &tbamd::resnet_conv_any);
  m.def("resnet_conv_any_supported", &tbamd::resnet_conv_any_supported);
  m.def("resnet_conv_any_wgrad", &tbamd::resnet_conv_any_wgrad);
  m.def("barrier_probe", &tbamd::barrier_probe);
  m.def("launch_probe", &tbamd::launch_probe);
  m.def("mfma_gemm", &tbamd::mfma_gemm);
  m.def("mfma_gemm_probe", &tbamd::mfma_gemm_probe);
  m.def("mfma_gemm_v2", &tbamd::mfma_gemm_v2);
  m.def("vtrace_from_logits", &vtrace_from_logits,
        py::arg("behavior_logits"), py::arg("target_logits"),
        py::arg("actions"), py::arg("discounts"), py::arg("rewards"),
        py::arg("values"), py::arg("bootstrap"), py::arg("clip_rho"),
        py::arg("clip_pg"), py::arg("lambda_") = 1.0);
  m.def("vtrace_from_importance_weights", &vtrace_from_importance_weights,
        py::arg("log_rhos"), py::arg("discounts"), py::arg("rewards"),
        py::arg("values"), py::arg("bootstrap"), py::arg("clip_rho"),
        py::arg("clip_pg"), py::arg("lambda_") = 1.0);
  m.def("fused_impala_loss_fwd", &fused_impala_loss_fwd);
  m.def("rmsprop_step", &rmsprop_step, py::arg("param"), py::arg("grad"),
        py::arg("square_avg"), py::arg("lr"), py::arg("alpha"),
        py::arg("eps"), py::arg("clip_norm"),
        py::arg("lr_tensor") = std::nullopt,
        py::arg("momentum_buf") = std::nullopt,
        py::arg("grad_avg") = std::nullopt, py::arg("momentum") = 0.0);
  m.def("policy_sample", &policy_sample);
  m.def("lstm_unroll_fwd", &lstm_unroll_fwd);
  m.def("lstm_unroll_bwd", &lstm_unroll_bwd);
}
