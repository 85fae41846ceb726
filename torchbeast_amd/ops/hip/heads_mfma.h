// fp32 MFMA policy and baseline heads for the learner (gfx950). See
// heads_mfma.hip for the kernels and heads_plan.h for the work split.
//
// The core input is virtual: [x | clamp(reward, -1, 1) | one_hot(last_action)]
// is composed while tiles are staged and never exists in memory. reward and
// last_action are optional: without them core = x (the LSTM output).
#pragma once

#include <torch/extension.h>

#include <vector>

namespace tbamd {

using OptTensor = c10::optional<torch::Tensor>;

// D >= 1, extra in {0, 1, 1 + A}, 1 <= A <= 63.
bool heads_supported(int64_t d, int64_t extra_columns, int64_t a);

// {logits [M, A], baseline [M]}. x [M, D] f32, reward [M] f32, last_action
// [M] int64 or int32, policy_w [A, Kc], policy_b [A], baseline_w [1, Kc],
// baseline_b [1], Kc = D (+ 1 (+ A)). The weights need no alignment beyond
// 4 bytes.
std::vector<torch::Tensor> heads_fwd(torch::Tensor x, OptTensor reward,
                                     OptTensor last_action,
                                     torch::Tensor policy_w,
                                     torch::Tensor policy_b,
                                     torch::Tensor baseline_w,
                                     torch::Tensor baseline_b);

// dx [M, D] = [dlogits | dbaseline] . W[:, :D]. A missing gradient is a zero
// operand; at least one is required.
torch::Tensor heads_dgrad(OptTensor dlogits, OptTensor dbaseline,
                          torch::Tensor policy_w, torch::Tensor baseline_w,
                          int64_t d);

// {d_policy_w [A, Kc], d_policy_b [A], d_baseline_w [1, Kc], d_baseline_b
// [1]}, views of one buffer. num_actions is read only when dlogits is
// missing.
std::vector<torch::Tensor> heads_wgrad(torch::Tensor x, OptTensor reward,
                                       OptTensor last_action,
                                       OptTensor dlogits, OptTensor dbaseline,
                                       int64_t num_actions);

}  // namespace tbamd
