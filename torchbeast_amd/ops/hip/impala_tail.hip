// The IMPALA learner tail in one launch (gfx950). After the model's forward
// the learner computes, on [T+1, ...] tensors as the queue and the model
// produce them,
//
//   rewards   = clamp(rewards, -1, 1)           (optional)
//   discounts = !done * discounting
//   vs, pg_adv = V-trace(behavior, target, actions, ...)
//   pg  = sum ce(target, actions) * pg_adv
//   bl  = 0.5 sum (vs - baseline)^2
//   ent = sum p log p
//   total = pg + baseline_cost bl + entropy_cost ent
//
// and, in the backward, d total / d target_logits and d total / d baseline.
// impala_tail_kernel does all of it: it reads the six inputs unshifted and
// writes the four scalars and the two final gradients laid out for T + 1
// rows. "Row t", t in [0, T), pairs target_logits[t] and baseline[t] with
// behavior_logits[t+1], actions[t+1], rewards[t+1] and done[t+1]; the
// bootstrap value is baseline[T]. Indexing takes the place of the shift.
//
// Work split: one 256-thread workgroup per batch column b, because the
// V-trace recurrence is sequential in T per column and a column's whole
// state fits in LDS (10 floats per row).
//
//   Phase 1  A 16-lane group owns a row: a wave takes 4 rows, the workgroup
//            16 per pass. Lane l of the group holds logits l, l + 16, l + 32,
//            l + 48 (A <= 64), so neighbouring lanes read neighbouring
//            words. Max, sum, sum p log p and the selected logit of both
//            policies are butterfly-reduced inside the 16 lanes; every lane
//            ends with the same value. The action is compared with the column
//            index and never used as one: an action outside [0, A) selects
//            nothing and reads nothing. Lane 0 of the group leaves the row's
//            lse (as the pair max, log sum), sum p log p, target log-prob,
//            log_rho, reward, discount, v, c and delta in LDS.
//   Phase 2  Thread 0 runs the reverse recurrence from LDS alone and
//            overwrites delta[t] with vs[t] - v[t].
//   Phase 3  Same row ownership, one more pass over the target row with no
//            reduction left: p = exp(z - lse), taken as (z - max) - log sum
//            so that it is not rounded at the magnitude of lse. Writes
//            d_logits, d_baseline, vs and pg_adv; lane 0 of each group
//            accumulates its rows' three loss terms in row order. Row T of
//            both gradients is written as zeros here.
//   Losses   The 16 group sums meet in LDS and thread 0 adds them in a fixed
//            tree, writes the column's partials[b][3] and takes a ticket with
//            an agent-scope acq-rel integer fetch_add. The workgroup that
//            draws ticket B - 1 sums the partials in column order, in double,
//            and writes the four scalars. No float atomics, so results repeat
//            bit for bit; nothing spins, so nothing can hang.

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <climits>
#include <cmath>
#include <vector>

#include "impala_tail.h"
#include "vtrace_math.h"

namespace tbamd {

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                        // lanes that share a row
constexpr int kRowsPerPass = kThreads / kGroup;   // 16
constexpr int kPerLane = 4;                       // logits held by a lane
constexpr int kMaxActions = kGroup * kPerLane;    // 64
constexpr int kRowFloats = 10;                    // LDS floats per row
constexpr int kRedFloats = 3 * kRowsPerPass;      // loss partials per group

// Same caution as heads_mfma.hip: keep packed-fp32 forms out of the
// four-logits-per-lane arithmetic.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

// Butterflies over the 16 lanes of a group: every lane gets the result, and
// the order of the additions does not depend on anything but the lane ids.
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int m = kGroup / 2; m > 0; m >>= 1)
    v = fmaxf(v, __shfl_xor(v, m, kGroup));
  return v;
}

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = kGroup / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kGroup);
  return v;
}

// This lane's share of a row: columns l, l + 16, l + 32, l + 48. Columns at
// or past A, and every column of a row past T, are -inf and never read.
__device__ __forceinline__ void load_row(const float* __restrict__ row, int A,
                                         int l, bool valid,
                                         float z[kPerLane]) {
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int j = l + kGroup * k;
    z[k] = (valid && j < A) ? row[j] : -INFINITY;
  }
}

// Max m, log of sum exp(z - m), and the logit at column a (0 if a is no
// column), the same on all 16 lanes.
__device__ __forceinline__ void row_stats(const float z[kPerLane], int A, int l,
                                          int64_t a, float* m, float* log_s,
                                          float* z_a) {
  float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  mx = group_max(mx);
  float s = 0.f, sel = 0.f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int j = l + kGroup * k;
    if (j < A) {
      s += __expf(z[k] - mx);
      if ((int64_t)j == a) sel = z[k];
    }
  }
  *m = mx;
  *log_s = __logf(group_sum(s));
  *z_a = group_sum(sel);
}

template <typename ActT>
__global__ void __launch_bounds__(kThreads) impala_tail_kernel(
    const float* __restrict__ behavior_logits,  // [T+1,B,A]
    const float* __restrict__ target_logits,    // [T+1,B,A]
    const ActT* __restrict__ actions,           // [T+1,B]
    const float* __restrict__ rewards,          // [T+1,B]
    const bool* __restrict__ done,              // [T+1,B]
    const float* __restrict__ baseline,         // [T+1,B]
    float discounting, int clip_reward, float clip_rho, float clip_pg,
    float lambda, float baseline_cost, float entropy_cost, int T, int B, int A,
    float* __restrict__ losses,      // [4]: total, pg, baseline, entropy
    float* __restrict__ d_logits,    // [T+1,B,A]
    float* __restrict__ d_baseline,  // [T+1,B]
    float* __restrict__ vs,          // [T,B]
    float* __restrict__ pg_adv,      // [T,B]
    float* __restrict__ partials,    // [B,3]
    unsigned int* __restrict__ ticket) {
  extern __shared__ float smem[];
  float* s_m = smem;             // [T] each: max of the target row
  float* s_logs = smem + T;      // log sum exp(z - max)
  float* s_nent = smem + 2 * T;  // sum p log p
  float* s_tlp = smem + 3 * T;   // target log-prob of the action
  float* s_lrho = smem + 4 * T;
  float* s_r = smem + 5 * T;
  float* s_disc = smem + 6 * T;
  float* s_v = smem + 7 * T;
  float* s_c = smem + 8 * T;
  float* s_delta = smem + 9 * T;  // delta, then vs - v
  float* s_red = smem + (size_t)kRowFloats * T;  // [3][16]

  const int b = blockIdx.x;
  const int g = threadIdx.x / kGroup;  // row of the pass
  const int l = threadIdx.x % kGroup;  // lane of the group

  // Phase 1. The loop bounds are the same for every thread, so all 64 lanes
  // of a wave take part in every shuffle.
  for (int t0 = 0; t0 < T; t0 += kRowsPerPass) {
    const int t = t0 + g;
    const bool valid = t < T;
    const int64_t cur = (int64_t)t * B + b;  // target_logits, baseline
    const int64_t nxt = cur + B;             // the other four
    const int64_t a = valid ? (int64_t)actions[nxt] : -1;

    float zt[kPerLane], zb[kPerLane];
    load_row(target_logits + cur * A, A, l, valid, zt);
    load_row(behavior_logits + nxt * A, A, l, valid, zb);

    float m, log_s, z_a;
    row_stats(zt, A, l, a, &m, &log_s, &z_a);
    const float t_m = m, t_log_s = log_s;
    const float t_lp = z_a - m - log_s;
    float pl = 0.f;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      if (l + kGroup * k < A) {
        const float lp = (zt[k] - t_m) - t_log_s;
        pl += __expf(lp) * lp;
      }
    }
    const float nent = group_sum(pl);

    row_stats(zb, A, l, a, &m, &log_s, &z_a);
    const float lr = t_lp - (z_a - m - log_s);

    if (valid && l == 0) {
      float r = rewards[nxt];
      if (clip_reward) r = fminf(fmaxf(r, -1.f), 1.f);
      const float disc = done[nxt] ? 0.f : discounting;
      const float v = baseline[cur];
      // Row t + 1 of baseline always exists: at t = T - 1 it is the bootstrap.
      const float v_next = baseline[nxt];
      float crho, c;
      vtrace_clip(lr, clip_rho, lambda, &crho, &c);
      s_m[t] = t_m;
      s_logs[t] = t_log_s;
      s_nent[t] = nent;
      s_tlp[t] = t_lp;
      s_lrho[t] = lr;
      s_r[t] = r;
      s_disc[t] = disc;
      s_v[t] = v;
      s_c[t] = c;
      s_delta[t] = vtrace_delta(crho, r, disc, v_next, v);
    }
  }
  __syncthreads();

  // Phase 2: the inherently sequential reverse recurrence over T.
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      acc = vtrace_scan_step(s_delta[t], s_disc[t], s_c[t], acc);
      s_delta[t] = acc;
    }
  }
  __syncthreads();

  // Phase 3.
  const float bootstrap = baseline[(int64_t)T * B + b];
  float pg_sum = 0.f, bl_sum = 0.f, ent_sum = 0.f;
  for (int t0 = 0; t0 < T; t0 += kRowsPerPass) {
    const int t = t0 + g;
    if (t >= T) continue;  // no shuffles below
    const int64_t cur = (int64_t)t * B + b;
    const int64_t a = (int64_t)actions[cur + B];
    const float v = s_v[t];
    const float vs_t = s_delta[t] + v;
    const float vs_next = (t + 1 < T) ? (s_delta[t + 1] + s_v[t + 1]) : bootstrap;
    const float adv =
        vtrace_advantage(s_lrho[t], clip_pg, s_r[t], s_disc[t], vs_next, v);
    const float m = s_m[t];
    const float log_s = s_logs[t];
    const float nent = s_nent[t];

    const float* __restrict__ row = target_logits + cur * A;
    float* __restrict__ out = d_logits + cur * A;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const int j = l + kGroup * k;
      if (j < A) {
        const float lp = (row[j] - m) - log_s;
        const float p = __expf(lp);
        out[j] = adv * (p - ((int64_t)j == a ? 1.f : 0.f)) +
                 entropy_cost * (p * (lp - nent));
      }
    }
    if (l == 0) {
      const float db = v - vs_t;
      d_baseline[cur] = baseline_cost * db;
      vs[cur] = vs_t;
      pg_adv[cur] = adv;
      pg_sum += -s_tlp[t] * adv;
      bl_sum += 0.5f * db * db;
      ent_sum += nent;
    }
  }

  // Row T of both gradients: the bootstrap row gets no gradient.
  {
    const int64_t last = (int64_t)T * B + b;
    if ((int)threadIdx.x < A) d_logits[last * A + threadIdx.x] = 0.f;
    if (threadIdx.x == 0) d_baseline[last] = 0.f;
  }

  if (l == 0) {
    s_red[g] = pg_sum;
    s_red[kRowsPerPass + g] = bl_sum;
    s_red[2 * kRowsPerPass + g] = ent_sum;
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    float col[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float* r = s_red + q * kRowsPerPass;
      for (int stride = kRowsPerPass / 2; stride > 0; stride >>= 1)
        for (int i = 0; i < stride; ++i) r[i] += r[i + stride];
      col[q] = r[0];
      __hip_atomic_store(&partials[(int64_t)b * 3 + q], col[q],
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Release this column's partials, acquire everyone else's.
    const unsigned int drawn = __hip_atomic_fetch_add(
        ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn == (unsigned int)(B - 1)) {
      double pg = 0.0, bl = 0.0, ent = 0.0;
      for (int i = 0; i < B; ++i) {
        const float* p = partials + (int64_t)i * 3;
        pg += __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bl += __hip_atomic_load(p + 1, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
        ent += __hip_atomic_load(p + 2, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      }
      losses[0] = (float)(pg + (double)baseline_cost * bl +
                          (double)entropy_cost * ent);
      losses[1] = (float)pg;
      losses[2] = (float)bl;
      losses[3] = (float)ent;
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

enum class Kind { kFloat, kInt, kBool };

// A tensor of the wrong shape, dtype or device would be an out-of-bounds or
// misread access on the device; reject it on the host instead.
void check_tail_tensor(const torch::Tensor& t, const torch::Tensor& first,
                       at::IntArrayRef shape, const char* name, Kind kind) {
  TORCH_CHECK(t.device() == first.device(), "impala_tail: ", name, " is on ",
              t.device(), ", expected ", first.device());
  if (kind == Kind::kInt) {
    TORCH_CHECK(t.scalar_type() == torch::kInt32 ||
                    t.scalar_type() == torch::kInt64,
                "impala_tail: ", name, " must be int32 or int64, got ",
                t.scalar_type());
  } else if (kind == Kind::kBool) {
    TORCH_CHECK(t.scalar_type() == torch::kBool, "impala_tail: ", name,
                " must be bool, got ", t.scalar_type());
  } else {
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "impala_tail: ", name,
                " must be float32, got ", t.scalar_type());
  }
  TORCH_CHECK(t.is_contiguous(), "impala_tail: ", name, " must be contiguous");
  TORCH_CHECK(t.sizes() == shape, "impala_tail: ", name, " has shape ",
              t.sizes(), ", expected ", shape);
}

}  // namespace

std::vector<torch::Tensor> impala_tail_fwd(
    torch::Tensor behavior_logits, torch::Tensor target_logits,
    torch::Tensor actions, torch::Tensor rewards, torch::Tensor done,
    torch::Tensor baseline, double discounting, bool clip_reward,
    double clip_rho, double clip_pg, double lambda, double baseline_cost,
    double entropy_cost) {
  TORCH_CHECK(target_logits.is_cuda() && target_logits.dim() == 3,
              "impala_tail: target_logits must be a [T+1,B,A] GPU tensor");
  const int64_t T1 = target_logits.size(0);
  const int64_t B = target_logits.size(1);
  const int64_t A = target_logits.size(2);
  const int64_t T = T1 - 1;
  check_tail_tensor(target_logits, target_logits, {T1, B, A}, "target_logits",
                    Kind::kFloat);
  check_tail_tensor(behavior_logits, target_logits, {T1, B, A},
                    "behavior_logits", Kind::kFloat);
  check_tail_tensor(actions, target_logits, {T1, B}, "actions", Kind::kInt);
  check_tail_tensor(rewards, target_logits, {T1, B}, "rewards", Kind::kFloat);
  check_tail_tensor(done, target_logits, {T1, B}, "done", Kind::kBool);
  check_tail_tensor(baseline, target_logits, {T1, B}, "baseline",
                    Kind::kFloat);
  TORCH_CHECK(T >= 1, "impala_tail: T must be >= 1, got T+1=", T1,
              " rows (the last row is the bootstrap)");
  TORCH_CHECK(B >= 1 && B <= INT_MAX, "impala_tail: B must be in [1, ",
              INT_MAX, "], got B=", B);
  TORCH_CHECK(A >= 1 && A <= kMaxActions, "impala_tail: A must be in [1, ",
              kMaxActions, "], got A=", A);
  TORCH_CHECK(lambda >= 0.0 && lambda <= 1.0,
              "impala_tail: lambda must be in [0, 1], got ", lambda);
  const size_t limit =
      at::cuda::getDeviceProperties(target_logits.get_device())
          ->sharedMemPerBlock;
  const size_t fixed = kRedFloats * sizeof(float);
  const size_t per_row = kRowFloats * sizeof(float);
  const size_t max_t = limit > fixed ? (limit - fixed) / per_row : 0;
  TORCH_CHECK((uint64_t)T <= max_t, "impala_tail: unroll length T=", T,
              " needs ", per_row, "*T+", fixed,
              " bytes of LDS, the device allows ", limit,
              " per workgroup (T <= ", max_t, ")");
  const size_t lds = per_row * (size_t)T + fixed;

  const at::cuda::CUDAGuard device_guard(target_logits.device());
  auto opts = target_logits.options();
  auto losses = torch::empty({4}, opts);
  auto d_logits = torch::empty_like(target_logits);
  auto d_baseline = torch::empty_like(baseline);
  auto vs = torch::empty({T, B}, opts);
  auto pg_adv = torch::empty({T, B}, opts);
  auto partials = torch::empty({B, 3}, opts);
  auto ticket = torch::zeros({1}, opts.dtype(torch::kInt32));

  auto launch = [&](auto kernel, const auto* actions_ptr) {
    hipLaunchKernelGGL(
        kernel, dim3((unsigned int)B), dim3(kThreads), lds,
        at::cuda::getCurrentCUDAStream(),
        behavior_logits.data_ptr<float>(), target_logits.data_ptr<float>(),
        actions_ptr, rewards.data_ptr<float>(), done.data_ptr<bool>(),
        baseline.data_ptr<float>(), (float)discounting, (int)clip_reward,
        (float)clip_rho, (float)clip_pg, (float)lambda, (float)baseline_cost,
        (float)entropy_cost, (int)T, (int)B, (int)A, losses.data_ptr<float>(),
        d_logits.data_ptr<float>(), d_baseline.data_ptr<float>(),
        vs.data_ptr<float>(), pg_adv.data_ptr<float>(),
        partials.data_ptr<float>(),
        reinterpret_cast<unsigned int*>(ticket.data_ptr<int32_t>()));
  };
  // Actions are read in their own width: no int64 copy.
  if (actions.scalar_type() == torch::kInt32) {
    launch(impala_tail_kernel<int32_t>, actions.data_ptr<int32_t>());
  } else {
    launch(impala_tail_kernel<int64_t>, actions.data_ptr<int64_t>());
  }
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "impala_tail: launch failed: ",
              hipGetErrorString(err));
  return {losses, d_logits, d_baseline, vs, pg_adv};
}

}  // namespace tbamd
