// The IMPALA learner tail in one launch (gfx950): reward clip, discounts,
// V-trace, the three losses, their weighted total and the total's gradients
// with respect to the target logits and the baseline. See impala_tail.hip.
#pragma once

#include <torch/extension.h>

#include <vector>

namespace tbamd {

// behavior_logits, target_logits [T+1, B, A] f32; actions [T+1, B] int32 or
// int64; rewards, baseline [T+1, B] f32; done [T+1, B] bool. All as the queue
// and the model produce them: row t of target_logits and baseline meets row
// t + 1 of the other four, the bootstrap is baseline[T]. T, B >= 1,
// 1 <= A <= 64, lambda in [0, 1]; a clip threshold of +inf does not clip.
//
// {losses [4] = (total, pg, baseline, entropy), d_logits [T+1, B, A],
//  d_baseline [T+1, B], vs [T, B], pg_adv [T, B]}. The gradients are those of
// total; their rows T are zero.
std::vector<torch::Tensor> impala_tail_fwd(
    torch::Tensor behavior_logits, torch::Tensor target_logits,
    torch::Tensor actions, torch::Tensor rewards, torch::Tensor done,
    torch::Tensor baseline, double discounting, bool clip_reward,
    double clip_rho, double clip_pg, double lambda, double baseline_cost,
    double entropy_cost);

}  // namespace tbamd
