// Declarations for runtime_kernels.hip (gather_obs, fused_heads_sample,
// unpack_rollouts).
#pragma once

#include <torch/extension.h>

#include <tuple>
#include <vector>

#include "rollout_gather.h"

namespace tbruntime {

std::vector<torch::Tensor> gather_obs(torch::Tensor slab_frames,
                                      torch::Tensor slab_rew,
                                      torch::Tensor slab_done,
                                      torch::Tensor ids_cpu, int64_t bp,
                                      std::vector<int64_t> frame_shape);

std::vector<torch::Tensor> fused_heads_sample(torch::Tensor x,
                                              torch::Tensor rew,
                                              torch::Tensor policy_w,
                                              torch::Tensor policy_b,
                                              torch::Tensor base_w,
                                              torch::Tensor base_b, int64_t b,
                                              bool greedy, int64_t seed);

// Same kernel, results written into caller-owned pinned host buffers
// (action [b], logits [b, A], baseline [b]); allocates nothing.
void fused_heads_sample_out(const torch::Tensor& x, const torch::Tensor& rew,
                            const torch::Tensor& policy_w,
                            const torch::Tensor& policy_b,
                            const torch::Tensor& base_w,
                            const torch::Tensor& base_b, int64_t b,
                            bool greedy, int64_t seed, int64_t* out_action,
                            float* out_logits, float* out_baseline);

// Rollout unpack (layout in rollout_gather.h): one launch on the current
// stream; staging and every column's dst are device memory, staging holds
// B rows of `stride` bytes and each column fits inside a row.
void launch_unpack_rollouts(const uint8_t* staging, int64_t stride, int64_t B,
                            const UnpackColumn* columns, int n_columns);

// Test surface: columns are (src_off, outer, inner_bytes); allocates the
// outputs (uint8 [outer, B, inner_bytes] views of one arena) and calls
// launch_unpack_rollouts.
std::vector<torch::Tensor> unpack_rollouts(
    torch::Tensor staging, int64_t stride, int64_t B,
    std::vector<std::tuple<int64_t, int64_t, int64_t>> columns);

}  // namespace tbruntime
