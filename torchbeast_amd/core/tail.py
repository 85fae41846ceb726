"""The learner tail: everything between the model's forward and backward().

monobeast.learn and polybeast_learner.learn.device_step share it. By default
it is the sequence both spelled out before: shift, reward clip, discounts,
`vtrace.from_logits`, `fused_impala_loss`, weighted total. With
TBAMD_FUSED_TAIL=1 (--fused_tail), fp32 GPU tensors and at most 64 actions it
is one launch of `ops.impala_tail` (ops/hip/impala_tail.hip), which reads the
[T+1, ...] tensors unshifted and hands autograd the two final gradients.
"""

import os

import torch

from torchbeast_amd.core import vtrace
from torchbeast_amd.ops import functional as tbops


def _fused(learner_logits, learner_baseline, actor_logits, env_rewards):
    """TBAMD_FUSED_TAIL=1 and inputs the kernel takes; unset, no impala_tail*
    symbol is looked up."""
    if os.environ.get("TBAMD_FUSED_TAIL") != "1":
        return False
    floats = (learner_logits, learner_baseline, actor_logits, env_rewards)
    return (learner_logits.is_cuda
            and all(t.dtype == torch.float32 for t in floats)
            and learner_logits.shape[-1] <= 64)


def learner_tail(flags, env_rewards, env_done, actor_logits, actor_actions,
                 learner_logits, learner_baseline):
    """(total, pg, baseline, entropy) losses of a [T+1, B] batch. env_* and
    actor_* are what the queue delivers, learner_* the model's outputs, all
    with T + 1 rows."""
    if _fused(learner_logits, learner_baseline, actor_logits, env_rewards):
        return tbops.impala_tail(
            actor_logits,
            learner_logits,
            actor_actions,
            env_rewards,
            env_done,
            learner_baseline,
            flags.discounting,
            clip_reward=flags.reward_clipping == "abs_one",
            lambda_=flags.vtrace_lambda,
            baseline_cost=flags.baseline_cost,
            entropy_cost=flags.entropy_cost,
        )

    bootstrap_value = learner_baseline[-1]

    # Shift: env_outputs[t+1] is the consequence of actions[t].
    env_rewards, env_done = env_rewards[1:], env_done[1:]
    actor_logits, actor_actions = actor_logits[1:], actor_actions[1:]
    learner_logits, learner_baseline = learner_logits[:-1], learner_baseline[:-1]

    if flags.reward_clipping == "abs_one":
        clipped_rewards = torch.clamp(env_rewards, -1, 1)
    else:
        clipped_rewards = env_rewards

    discounts = (~env_done).float() * flags.discounting

    vtrace_returns = vtrace.from_logits(
        behavior_policy_logits=actor_logits,
        target_policy_logits=learner_logits,
        actions=actor_actions,
        discounts=discounts,
        rewards=clipped_rewards,
        values=learner_baseline,
        bootstrap_value=bootstrap_value,
        lambda_=flags.vtrace_lambda,
    )

    pg_loss, baseline_loss, entropy_loss = tbops.fused_impala_loss(
        learner_logits,
        learner_baseline,
        actor_actions,
        vtrace_returns.pg_advantages,
        vtrace_returns.vs,
    )
    total_loss = (
        pg_loss
        + flags.baseline_cost * baseline_loss
        + flags.entropy_cost * entropy_loss
    )
    return total_loss, pg_loss, baseline_loss, entropy_loss
