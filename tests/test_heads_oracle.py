"""The heads oracle (tests/helpers/heads_oracle.py) checked on its own,
without a GPU: that the integer cases of tests/test_serve_heads_gpu.py are
exact in float32 and are not tests of zeros, that both comparison rules
reject what a subtly wrong heads kernel would return, and that the sampler
statistics pass a numpy model of the kernel's Gumbel draw and reject broken
variants of it.
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import heads_oracle as ho  # noqa: E402

TWO24 = 2.0 ** 24
FORMS = [pytest.param(True, id="x_rew"), pytest.param(False, id="x_only")]


def _is_int(t):
    return bool((t == t.round()).all())


def _covered(t, what):
    share = float((t != 0).double().mean())
    assert 0.2 <= share <= 0.8, f"{what}: {share:.3f} of elements nonzero"


# ---- the exact cases ----


@pytest.mark.parametrize("with_rew", FORMS)
@pytest.mark.parametrize("D", ho.D_VALUES)
def test_exact_cases_are_exact_covered_and_distinct(D, with_rew):
    for A in ho.A_VALUES:
        c = ho.exact_case(D, A, with_rew)
        tag = f"D={D} A={A}"
        assert c["x"].dtype == torch.float32 and c["x"].shape == (ho.ROWS, D)
        assert _is_int(c["x"]) and 0 <= c["x"].min() and c["x"].max() <= 4
        if with_rew:
            assert set(c["rew"].tolist()) == {-1.0, 0.0, 1.0}
            assert c["policy_w"].shape == (A, D + 1)
            # the reward's column is live in both heads
            live = torch.arange(A) % ho.DEAD_OUT != 1
            assert bool((c["policy_w"][live, D] != 0).all())
            assert c["base_w"][0, D] != 0
        else:
            assert c["rew"] is None and c["policy_w"].shape == (A, D)
        for k in ("policy_w", "base_w"):
            assert set(c[k].unique().tolist()) <= {-1.0, 0.0, 1.0}
        for k in ("policy_b", "base_b"):
            assert _is_int(c[k])
        assert c["base_b"] != 0 and c["policy_b"][0] != 0
        dead = torch.arange(A) % ho.DEAD_OUT == 1
        assert not bool(c["policy_w"][dead].any())
        (logits, baseline), (s_l, s_b) = ho.reference(c)
        # Every partial sum of magnitudes is an integer far below 2^24: any
        # summation order gives the same float32.
        assert _is_int(logits) and _is_int(baseline)
        assert float(s_l.max()) < 4096 and float(s_b.max()) < 4096 < TWO24
        _covered(logits, f"{tag} logits")
        _covered(baseline, f"{tag} baseline")
        # ... also over the first rows alone, for the smaller batches
        _covered(logits[:70], f"{tag} logits[:70]")
        _covered(baseline[:70], f"{tag} baseline[:70]")
        core = ho.core_of(c["x"], c["rew"])
        assert not bool((core[1:] == core[:-1]).all(1).any()), tag
        assert not bool((logits[1:] == logits[:-1]).all(1).any()), tag
        assert not bool((baseline[1:] == baseline[:-1]).any()), tag
        # The float32 eager path agrees exactly, as the kernel must.
        got = F.linear(core, c["policy_w"], c["policy_b"])
        assert torch.equal(got.double(), logits)


def test_zero_sum_rows_always_terminate():
    """The move that makes a row's sum zero has an entry to move while the
    sum is off: with w[0] = -1, entries in 0..4, |fixed| <= 1 and bias 1 or
    2, a stuck positive sum would need every -1 entry at 4 and every +1 entry
    at 0 (sum <= -4 + 1 + 2 < 0), a stuck negative one every -1 entry at 0
    and every +1 entry at 4 (sum >= -1 + 1 = 0). The smallest core shows
    both ends."""
    g = torch.Generator().manual_seed(0)
    w = torch.tensor([-1])
    for start in range(5):
        for fixed in (-1, 0, 1):
            for bias in (1, 2):
                x = ho._zero_a_sum(torch.tensor([start]), fixed, w, bias, g)
                assert int(x[0]) == fixed + bias


# ---- the comparison rules ----

# (D, A, with reward): a core below one stride, one past a stride with and
# without the reward, the LSTM width, one action.
MUTATION_CASES = [(1, 1, True), (63, 6, False), (64, 18, True),
                  (65, 6, False), (519, 18, True), (519, 64, False),
                  (256, 1, True)]


def _faults(D, with_rew):
    Dc = D + 1 if with_rew else D
    out = ["base_from_policy", "no_bias"]
    if with_rew:
        out.append("reward_at_0")
    if Dc % 64:
        out.append("tail_dropped")
    return out


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("D,A,with_rew", MUTATION_CASES)
def test_rules_reject_broken_heads(kind, D, A, with_rew):
    c = ho.case(kind, D, A, with_rew)
    refs, s = ho.reference(c)
    # What a faultless kernel stores, the float32 rounding of the answer
    # (half an ulp: at most 2^-24 of the result, which S bounds), passes ...
    bad, worst = ho.judge(kind, refs[0].float(), refs[1].float(), refs, s)
    assert bad == [] and worst <= 1.0
    # ... and so does float32 arithmetic in another order.
    core = ho.core_of(c["x"], c["rew"])
    flipped = (F.linear(core.flip(1), c["policy_w"].flip(1), c["policy_b"]),
               F.linear(core.flip(1), c["base_w"].flip(1),
                        c["base_b"]).reshape(-1))
    bad, _ = ho.judge(kind, *flipped, refs, s)
    assert bad == []
    faults = _faults(D, with_rew)
    assert len(faults) >= 2
    for fault in faults:
        got = ho.broken_heads(c, fault)
        bad, _ = ho.judge(kind, *got, refs, s)
        assert bad, f"{kind} D={D} A={A}: {fault} passes"
        if fault in ("base_from_policy",):
            assert any(m.startswith("baseline") for m in bad)


def test_every_fault_is_tried_somewhere():
    seen = set()
    for D, _, with_rew in MUTATION_CASES:
        seen |= set(_faults(D, with_rew))
    assert seen == {"reward_at_0", "base_from_policy", "tail_dropped",
                    "no_bias"}


def test_messages_name_output_and_row():
    ref = torch.zeros(4, 3, dtype=torch.float64)
    got = ref.clone()
    got[2, 1] = 1
    msg = ho.exact_mismatch(got, ref, "logits")
    assert msg.startswith("logits") and "row 2" in msg and "(2, 1)" in msg
    assert ho.exact_mismatch(ref.clone(), ref, "logits") is None
    s = torch.ones(4, dtype=torch.float64)
    got = torch.zeros(4, dtype=torch.float64)
    got[3] = 1e-5
    msg, ratio = ho.bound_excess(got, torch.zeros(4, dtype=torch.float64), s,
                                 ho.K, "baseline")
    assert msg.startswith("baseline") and "row 3" in msg and ratio > 100
    got[3] = float("nan")
    msg, ratio = ho.bound_excess(got, torch.zeros(4, dtype=torch.float64), s,
                                 ho.K, "baseline")
    assert msg is not None and ratio == float("inf")


def test_cpu_float32_ratio_recorded():
    """r, from which K = 4 r is derived: a plain float32 F.linear on the CPU
    against float64 over the bounded cases; it must itself sit within K."""
    r = ho.cpu_float32_ratio()
    print(f"float32 F.linear on the CPU vs float64: {r:.3f} of 2^-24*S,"
          f" recorded r = {ho.CPU_RATIO}, K = {ho.K:.2f}")
    assert ho.K == 4 * ho.CPU_RATIO
    assert r <= ho.K


# ---- the sampler statistics on a numpy model of the draw ----


def test_runner_seeds():
    assert ho.runner_seed(1) == ho.GOLDEN - (1 << 64) < 0
    assert ho.runner_seed(2) == (2 * ho.GOLDEN) % (1 << 64) > 0
    seeds = [ho.runner_seed(k) for k in range(1, ho.N_LAUNCHES + 1)]
    assert all(-(1 << 63) <= v < (1 << 63) for v in seeds)
    assert len(set(seeds)) == ho.N_LAUNCHES
    assert any(v < 0 for v in seeds) and any(v > 0 for v in seeds)


def test_model_uniform_is_capped_below_one():
    """hiprand_uniform's float rounding reaches 1.0 for the largest 32-bit
    values; the cap changes those draws and no other."""
    bits = np.array([[0, 1 << 31, (1 << 32) - 200, (1 << 32) - 1]], np.uint32)
    p32 = np.float32(2.0 ** -32)
    raw = p32 + bits.astype(np.float32) * p32
    assert raw.dtype == np.float32
    assert raw[0, 0] == p32 and raw[0, 1] == np.float32(0.5)
    assert raw[0, 3] == np.float32(1) and raw[0, 2] < np.float32(1)
    capped = np.minimum(raw, ho.ONE_BELOW)
    assert (capped[0, :3] == raw[0, :3]).all()
    assert capped[0, 3] == ho.ONE_BELOW == np.float32(1 - 2.0 ** -24)
    ceiling = -np.log(-np.log(np.float64(ho.ONE_BELOW)))
    assert 16.6 < ceiling < 16.7
    # A masked action below the ceiling's reach is never drawn, the largest
    # uniform included; without the cap it would be.
    z = np.array([[0.0, -1e9]], np.float32)
    top = np.array([[0, (1 << 32) - 1]], np.uint32)
    assert ho.model_draw(z, top)[0] == 0
    with np.errstate(divide="ignore"):
        uncapped = z - np.log(-np.log(p32 + top.astype(np.float32) * p32))
    assert np.argmax(uncapped[0]) == 1


@pytest.fixture(scope="module")
def correct_draws():
    return ho.model_one_launch(), ho.model_launches()


def test_statistics_pass_a_correct_sampler(correct_draws):
    verdicts = ho.sampler_verdicts(*correct_draws)
    assert all(verdicts.values()), verdicts
    a18, a2 = correct_draws[0]
    assert a18.shape == (ho.N_DRAWS,) and a2.shape == (ho.N_DRAWS,)
    assert correct_draws[1][0].shape == (ho.N_LAUNCHES, ho.LAUNCH_ROWS)
    assert ho.LAUNCH_ROWS % 4 == 0  # pooled rows keep their vector: r % 4


# Which statistic has to catch which fault (others may as well).
CATCHES = {
    "neg_log": ("chi2", "chi2_launches"),
    "last_never": ("chi2", "chi2_launches"),
    "rows_share": ("neighbours",),
    "seed_shared": ("chi2_launches", "launch_neighbours"),
}


@pytest.mark.parametrize("fault", ho.BROKEN_SAMPLERS)
def test_statistics_reject_a_broken_sampler(fault, correct_draws):
    one = (correct_draws[0] if fault == "seed_shared"
           else ho.model_one_launch(fault))
    verdicts = ho.sampler_verdicts(one, ho.model_launches(fault))
    print(fault, verdicts)
    for name in CATCHES[fault]:
        assert not verdicts[name], f"{fault} passes {name}"


def test_dead_cell_count_sees_a_drawn_dead_action():
    a18, _ = ho.model_one_launch()
    a18 = a18.copy()
    a18[0] = ho.DEAD[0][1]  # row 0 holds vector 0
    _, dead = ho.chi2_per_group(torch.from_numpy(a18),
                                ho.four_logit_vectors())
    assert dead == 1
