// Declarations for runtime_kernels.hip (gather_obs, fused_heads_sample,
// unpack_rollouts, gather_rows, lstm_serve_layer).
#pragma once

#include <torch/extension.h>

#include <optional>
#include <tuple>
#include <vector>

#include "rollout_gather.h"
#include "row_gather.h"

namespace tbruntime {

// Inference batch from slot ids (kernel comment in the .hip). The three slabs
// are pinned host tensors over the same slots (frames uint8 [slots, ...] of
// frame_shape, rewards float32, dones uint8), ids_cpu b int32 or int64 slot
// ids on the CPU, 1 <= b <= bp. All of that, every id against the slot count
// and the frame size against the 16-byte accesses, is checked (RuntimeError)
// before anything is allocated or launched. Returns frames [bp, ...] uint8,
// rew [bp, 1] clamped and nd [bp] = 1 - done on the GPU; rows >= b are zero
// frames, reward 0, not-done 1. Bound as _tbruntime.gather_obs for the tests.
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

// The heads kernel over raw pointers. `core` is [>= b, D] f32 on the device;
// with `rew` ([>= b] f32) the heads see [core, rew] (length D + 1), with
// rew == nullptr the core alone (the recurrent tail: the last LSTM layer's
// h). Same sampling code either way. Weights and biases are checked here
// (contiguous f32 on the current GPU, [A, Dc] / A / [1, Dc] / 1 elements,
// 1 <= A <= 64, the core within the LDS limit) and so is the launch's
// result; the raw pointers are the caller's to vouch for, which
// fused_heads_sample_out and heads_sample do for tensors.
void launch_heads_sample(const float* core, const float* rew, int64_t D,
                         const torch::Tensor& policy_w,
                         const torch::Tensor& policy_b,
                         const torch::Tensor& base_w,
                         const torch::Tensor& base_b, int64_t b, bool greedy,
                         int64_t seed, int64_t* out_action, float* out_logits,
                         float* out_baseline);

// Test surface: launch_heads_sample in either core form, [x, rew] or, with
// rew = None, x alone, on caller-made tensors. action (int64), logits
// ([n, A]) and baseline are pinned CPU tensors of at least b rows; rows >= b
// are not written. The seed reaches the kernel unchanged (negative ones
// too, as InferenceRunner::next_seed() makes them). Every argument is checked
// (RuntimeError) before the launch; returns after the stream has run it.
void heads_sample(torch::Tensor x, std::optional<torch::Tensor> rew,
                  torch::Tensor policy_w, torch::Tensor policy_b,
                  torch::Tensor base_w, torch::Tensor base_b, int64_t b,
                  bool greedy, int64_t seed, torch::Tensor action,
                  torch::Tensor logits, torch::Tensor baseline);

// One LSTM layer's weights as lstm_serve_layer_kernel reads them (layout in
// the kernel comment): w [4, Hn, Kp] bf16, bias [4, Hn] f32 = b_ih + b_hh.
struct LstmLayerPack {
  torch::Tensor w, bias;
  int64_t I = 0, H = 0, Ip = 0, Kp = 0, Hn = 0;
};
// Packs with ATen ops on the current stream (a handful of launches and two
// allocations: once per weight version, not per batch).
LstmLayerPack pack_lstm_layer(const torch::Tensor& w_ih,
                              const torch::Tensor& w_hh,
                              const torch::Tensor& b_ih,
                              const torch::Tensor& b_hh);

// Does a layer with input length I and hidden size H fit the layer kernel's
// LDS tile (16 rows of Ip + Hk bf16 plus 16 KB of partial sums in 64 KB:
// I + H up to about 1,500)? The runner declines the recurrent row path for a
// model that does not.
bool lstm_serve_layer_fits(int64_t I, int64_t H);

// The LSTM serve step's kernels (comments in the .hip), each one launch on
// the current stream. The tables hold `b` pointers each in pinned host
// memory and are filled by build_state_table() (row_gather.h), which checked
// them; a wrong one is a GPU fault. Tables, state block and rows stay
// unchanged until the stream has run the kernels.
//
// Stage: request r's previous state (n_floats = 2 L H floats, zeros for a
// done row) from the pinned state rows into row r of `staged` (device,
// [>= b, n_floats]).
void launch_lstm_stage_state(const float* const* state_in,
                             const uint8_t* const* done_src, int64_t b,
                             int64_t n_floats, float* staged);
// One layer. `in` is [>= b, in_stride] f32 on the device; for layer 0, `rew`
// ([>= b]) is appended as the input's last element, for the other layers it
// is nullptr. h_out is [>= b, H] on the device.
void launch_lstm_serve_layer(float* const* state_out, const float* staged,
                             const float* in, int64_t in_stride,
                             const float* rew, const LstmLayerPack& pack,
                             int64_t b, int64_t layer, int64_t L,
                             float* h_out);

// Test surface: every layer kernel and the heads on caller-made tensors. x
// [n, D] and rew [n] f32 on the GPU (n >= b), lstm_weights four tensors per
// layer (w_ih, w_hh, b_ih, b_hh) on the GPU. The state lives in
// `state_block`, a pinned f32 CPU tensor: request r reads 2*L*H floats (h
// [L, H], then c) at byte offset in_offsets[r] and writes as many at
// out_offsets[r]; its done byte is at done_offsets[r] of the pinned uint8
// `done_slab`. All offsets go through build_state_table() (IndexError /
// ValueError) before anything is launched. Returns pinned (action [cap],
// logits [cap, A], baseline [cap]) and then one device [cap, H] h per
// layer, all pre-filled with -7 so that untouched rows show.
std::vector<torch::Tensor> lstm_serve_step(
    torch::Tensor x, torch::Tensor rew, std::vector<torch::Tensor> lstm_weights,
    torch::Tensor policy_w, torch::Tensor policy_b, torch::Tensor base_w,
    torch::Tensor base_b, torch::Tensor state_block,
    std::vector<int64_t> in_offsets, std::vector<int64_t> out_offsets,
    torch::Tensor done_slab, std::vector<int64_t> done_offsets, int64_t cap,
    bool greedy, int64_t seed);

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
