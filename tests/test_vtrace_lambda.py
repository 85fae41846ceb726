"""V-trace with lambda and with unclipped (None) thresholds, on the CPU path,
against an independent float64 NumPy transcription of the paper formula
(arXiv:1802.01561 eq. (1) with Remark 2: c_t = lambda * min(1, rho_t))."""

import functools

import numpy as np
import pytest
import torch

from torchbeast_amd.core import vtrace

SHAPES = [(1, 1), (5, 2), (80, 8), (257, 3)]
# (clip_rho_threshold, clip_pg_rho_threshold, lambda_)
PARAMS = [
    (1.0, 1.0, 1.0),
    (None, None, 1.0),
    (1.0, 1.0, 0.9),
    (None, None, 0.5),
    (3.0, None, 0.0),
]


def ground_truth_vtrace(
    log_rhos,
    discounts,
    rewards,
    values,
    bootstrap_value,
    clip_rho_threshold=1.0,
    clip_pg_rho_threshold=1.0,
    lambda_=1.0,
):
    """O(T^2) literal transcription; None thresholds mean no clipping."""
    if clip_rho_threshold is None:
        clip_rho_threshold = np.inf
    if clip_pg_rho_threshold is None:
        clip_pg_rho_threshold = np.inf
    rhos = np.exp(log_rhos)
    clipped_rhos = np.minimum(rhos, clip_rho_threshold)
    cs = lambda_ * np.minimum(rhos, 1.0)
    T = rewards.shape[0]

    values_t_plus_1 = np.concatenate([values[1:], bootstrap_value[None]], axis=0)
    deltas = clipped_rhos * (rewards + discounts * values_t_plus_1 - values)

    vs = []
    for s in range(T):
        v_s = values[s].astype(np.float64).copy()
        for t in range(s, T):
            coeff = np.prod(discounts[s:t] * cs[s:t], axis=0) if t > s else 1.0
            v_s = v_s + coeff * deltas[t]
        vs.append(v_s)
    vs = np.stack(vs)

    vs_t_plus_1 = np.concatenate([vs[1:], bootstrap_value[None]], axis=0)
    pg_rhos = np.minimum(rhos, clip_pg_rho_threshold)
    pg_advantages = pg_rhos * (rewards + discounts * vs_t_plus_1 - values)
    return vs, pg_advantages


@functools.lru_cache(maxsize=None)
def _random_inputs(T, B, seed=0):
    rng = np.random.RandomState(seed)
    inp = dict(
        log_rhos=(rng.uniform(-1.5, 1.5, (T, B))).astype(np.float32),
        discounts=(rng.uniform(0.0, 1.0, (T, B)) > 0.1).astype(np.float32) * 0.99,
        rewards=rng.randn(T, B).astype(np.float32),
        values=rng.randn(T, B).astype(np.float32),
        bootstrap_value=rng.randn(B).astype(np.float32),
    )
    for v in inp.values():
        v.setflags(write=False)
    return inp


def _tensors(inp):
    return {k: torch.from_numpy(v.copy()) for k, v in inp.items()}


@pytest.mark.parametrize("clip_rho,clip_pg,lambda_", PARAMS)
@pytest.mark.parametrize("T,B", SHAPES)
def test_from_importance_weights_matches_numpy(T, B, clip_rho, clip_pg, lambda_):
    inp = _random_inputs(T, B)
    expected_vs, expected_pg = ground_truth_vtrace(
        **inp,
        clip_rho_threshold=clip_rho,
        clip_pg_rho_threshold=clip_pg,
        lambda_=lambda_,
    )
    out = vtrace.from_importance_weights(
        **_tensors(inp),
        clip_rho_threshold=clip_rho,
        clip_pg_rho_threshold=clip_pg,
        lambda_=lambda_,
    )
    np.testing.assert_allclose(out.vs.numpy(), expected_vs, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(
        out.pg_advantages.numpy(), expected_pg, rtol=1e-4, atol=1e-4
    )


@pytest.mark.parametrize("T,B", SHAPES)
def test_lambda_zero_is_one_step_target(T, B):
    """With lambda = 0 every trace is cut: acc_t = delta_t + disc*0*acc is
    delta_t exactly, so vs = values + delta bit for bit."""
    t = _tensors(_random_inputs(T, B))
    out = vtrace.from_importance_weights(
        **t, clip_rho_threshold=3.0, clip_pg_rho_threshold=None, lambda_=0.0
    )
    next_values = torch.cat([t["values"][1:], t["bootstrap_value"][None]], dim=0)
    delta = torch.exp(t["log_rhos"]).clamp(max=3.0) * (
        t["rewards"] + t["discounts"] * next_values - t["values"]
    )
    assert torch.equal(out.vs, delta + t["values"])


@pytest.mark.parametrize("bad", [1.5, -0.1])
def test_lambda_out_of_range_raises(bad):
    t = _tensors(_random_inputs(5, 2))
    with pytest.raises(ValueError):
        vtrace.from_importance_weights(**t, lambda_=bad)
    logits = torch.zeros(5, 2, 3)
    actions = torch.zeros(5, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        vtrace.from_logits(
            logits, logits, actions, t["discounts"], t["rewards"], t["values"],
            t["bootstrap_value"], lambda_=bad,
        )


def test_from_logits_lambda_consistent_with_importance_weights():
    T, B, A = 6, 4, 5
    rng = np.random.RandomState(2)
    behavior_logits = torch.from_numpy(rng.randn(T, B, A).astype(np.float32))
    target_logits = torch.from_numpy(rng.randn(T, B, A).astype(np.float32))
    actions = torch.from_numpy(rng.randint(0, A, (T, B)))
    t = _tensors(_random_inputs(T, B, seed=3))
    rest = (t["discounts"], t["rewards"], t["values"], t["bootstrap_value"])

    out = vtrace.from_logits(
        behavior_logits, target_logits, actions, *rest, lambda_=0.9
    )
    core = vtrace.from_importance_weights(out.log_rhos, *rest, lambda_=0.9)
    torch.testing.assert_close(out.vs, core.vs)
    torch.testing.assert_close(out.pg_advantages, core.pg_advantages)

    # lambda really reaches from_logits: the default gives other targets.
    default = vtrace.from_logits(behavior_logits, target_logits, actions, *rest)
    assert not torch.allclose(default.vs, out.vs)


def test_trainers_accept_vtrace_lambda_flag():
    from torchbeast_amd import monobeast, polybeast_learner

    for parser in (monobeast.parser, polybeast_learner.parser):
        assert parser.parse_args([]).vtrace_lambda == 1.0
        assert parser.parse_args(["--vtrace_lambda", "0.9"]).vtrace_lambda == 0.9
