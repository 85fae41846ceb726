// Declarations for runtime_kernels.hip (gather_obs, fused_heads_sample,
// unpack_rollouts, gather_rows).
#pragma once

#include <torch/extension.h>

#include <tuple>
#include <vector>

#include "rollout_gather.h"
#include "row_gather.h"

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

// Bytes of a frame that one workgroup of gather_rows_kernel copies. Swept
// over 4/8/16/32 KB on the MI355X at 100,800-byte frames, b = 64/128/256
// (profiles/PROFILE_r5.md): 8, 16 and 32 KB tie within 1 % (42/46/50 GB/s of
// the 63 GB/s host link), 4 KB is 3 % behind at b = 128. 16 KB still gives a
// 64-frame batch 448 workgroups for 256 CUs.
constexpr int64_t kGatherRowsChunkBytes = 16384;
int64_t gather_rows_chunk_bytes();

// Inference-batch gather from rollout rows (kernel comment in the .hip): one
// launch on the current stream. frame_src / rew_src are tables of `b`
// pointers in pinned host memory, filled by build_row_table() (row_gather.h)
// -- the caller has thereby checked that every [ptr, ptr + fsz) and every
// reward lies inside the pinned slab; a pointer that does not is a GPU fault.
// Tables and rows must stay unchanged until the stream has run the kernel.
// out_frames is [cap, fsz] (16-byte aligned base), out_rew [cap], cap >= b;
// rows >= b are not written. chunk_bytes other than the default is for the
// chunk-size sweep only (4, 8, 16 or 32 KB).
void launch_gather_rows(const uint8_t* const* frame_src,
                        const float* const* rew_src, int64_t b, int64_t fsz,
                        uint8_t* out_frames, float* out_rew,
                        int64_t chunk_bytes = kGatherRowsChunkBytes);

// Test surface: `slab` is a pinned uint8 CPU tensor, the offsets are byte
// offsets of b frames (fsz bytes) and b float rewards inside it, each
// bounds-checked (IndexError) before anything is launched. Returns
// (frames [cap, fsz] uint8, rew [cap, 1] float32) on the GPU, pre-filled with
// 0xA5 / -7.0 so that untouched rows show. chunk_bytes 0 = the default.
std::tuple<torch::Tensor, torch::Tensor> gather_rows(
    torch::Tensor slab, std::vector<int64_t> frame_offsets,
    std::vector<int64_t> reward_offsets, int64_t fsz, int64_t cap,
    int64_t chunk_bytes = 0);

}  // namespace tbruntime
