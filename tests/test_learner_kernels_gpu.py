"""impala_loss_kernel and policy_sample_kernel (ops/hip/tbops.hip) at the
shapes the learner runs, against float64 references.

Fused loss. One thread per row, a block reduction in LDS, then one atomicAdd
per block and loss. The cases reach a second block, tail blocks of 41 and of
1 row, ten blocks at the learner's R = T*B = 2560, A = 1, 2, 6 and 18,
saturated logits (where ce = lse - z[a] cancels), int32 actions and a
non-contiguous logits view. Gradients are compared per element through
backward() at the tolerance tests/test_ops_gpu.py uses. Loss values are held
to

    |gpu - ref| <= K * 2^-24 * S   (+ 1e-6 for pg and entropy)

with S the sum of per-row magnitudes from the float64 reference
(tests/helpers/loss_oracle.py). K is derived, not chosen: the float32 eager
CPU path measured against float64 over these same cases reaches at most 1.34
of 2^-24 * S (1.331, on the baseline loss of the transposed case; most of it
is the rounding of the result itself), and the kernel gets 8x that for
__expf and __logf, whose error is a few ulp where libm's is under one:
K = 8 * 1.34 = 10.72. At R = 2560 one dropped row moves a loss by about 4e-4
relative, some hundreds of times this bound.

Sampler. Inverse-CDF draw with one philox stream per row, seeded from the
CPU generator, so torch.manual_seed makes every run deterministic. The tests
check the distribution row by row distinct (chi-square against the float64
softmax, at a threshold the CPU's torch.multinomial is shown to pass too),
independence of neighbouring rows, determinism, and greedy mode against
first-index argmax with exact ties, with a grid tail and [T,B,A] input.
"""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.ops import functional as tbops
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import heads_oracle as ho  # noqa: E402
import loss_oracle as lso  # noqa: E402

CPU_RATIO = 1.34  # measured: float32 eager CPU vs float64, see above
K = 8 * CPU_RATIO


# ---- fused IMPALA loss ----


def _gpu_losses(name):
    inp = lso.case_inputs(name)
    layout = lso.CASES[name][4]
    baseline = inp["baseline"].cuda().requires_grad_()
    actions = inp["actions"].cuda()
    if layout == "transposed":
        leaf = inp["logits"].transpose(0, 1).contiguous().cuda()
        leaf.requires_grad_()
        logits = leaf.transpose(0, 1)  # [T,B,A] view of [B,T,A] storage
        assert not logits.is_contiguous()
        actions = actions.to(torch.int32)
    else:
        leaf = inp["logits"].cuda().requires_grad_()
        logits = leaf
    pg, bl, ent = tbops.fused_impala_loss(
        logits, baseline, actions, inp["pg_adv"].cuda(), inp["vs"].cuda())
    w = lso.WEIGHTS
    (w[0] * pg + w[1] * bl + w[2] * ent).backward()
    d_logits = leaf.grad.cpu()
    if layout == "transposed":
        d_logits = d_logits.transpose(0, 1)
    return dict(pg=pg.detach().cpu(), baseline=bl.detach().cpu(),
                entropy=ent.detach().cpu(), d_logits=d_logits,
                d_baseline=baseline.grad.cpu())


@pytest.mark.parametrize("name", list(lso.CASES))
def test_fused_loss_matches_float64(name):
    T, B, A, scale, layout = lso.CASES[name]
    ref, s = lso.reference(name)
    got = _gpu_losses(name)

    for key in ("pg", "baseline", "entropy"):
        print(f"{name} {key}: gpu {float(got[key])!r} ref {float(ref[key])!r}"
              f" ratio {lso.ratio(got[key], ref[key], s[key]):.3f} of"
              f" 2^-24*S, K = {K:.2f}")
    if A == 1:
        assert float(ref["pg"]) == 0.0 and float(ref["entropy"]) == 0.0

    for key in ("pg", "baseline", "entropy"):
        assert got[key].shape == () and got[key].dtype == torch.float32
        err = abs(float(got[key]) - float(ref[key]))
        assert err <= lso.bound(K, s[key], key), (
            f"{key}: |{float(got[key])!r} - {float(ref[key])!r}| = {err:.3e}"
            f" over {lso.bound(K, s[key], key):.3e}")

    torch.testing.assert_close(got["d_logits"], ref["d_logits"].float(),
                               rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got["d_baseline"], ref["d_baseline"].float(),
                               rtol=1e-4, atol=1e-5)


def test_fused_loss_cpu_float32_ratio_recorded():
    """Prints the figure K is derived from, so a run shows it beside the
    kernel's ratios; the eager float32 path must itself sit within K."""
    measured = lso.cpu_float32_ratio()
    print(f"float32 eager CPU vs float64: {measured:.3f} of 2^-24*S "
          f"(recorded {CPU_RATIO}, K = {K:.2f})")
    assert measured <= K


# ---- policy sampler ----

# The logit vectors and the chi-square statistic are shared with the serve
# plane's sampler tests (tests/test_serve_heads_gpu.py).
N_DRAWS = ho.N_DRAWS
A_FULL = ho.A_FULL
DEAD = ho.DEAD  # the two -40 entries per vector
_four_logit_vectors = ho.four_logit_vectors
_chi2_per_group = ho.chi2_per_group


def test_policy_sample_distribution_chi2():
    from scipy.stats import chi2

    limit = float(chi2.ppf(1 - 1e-6, 15))
    z = _four_logit_vectors()
    assert float(torch.softmax(z.double(), -1)[z > -1].min()) >= 0.01
    logits = z.repeat(N_DRAWS // 4, 1)  # row r holds vector r % 4
    assert logits.shape == (N_DRAWS, A_FULL) and N_DRAWS % 256 != 0

    # The CPU sampler (torch.multinomial) under the same seed and the same
    # logits passes the same test: the threshold is not too tight.
    torch.manual_seed(41)
    cpu_actions = tbops.policy_sample(logits)
    cpu_stats, cpu_dead = _chi2_per_group(cpu_actions, z)
    print("chi2 limit", limit, "cpu", cpu_stats)
    assert cpu_dead == 0
    assert max(cpu_stats) < limit

    torch.manual_seed(41)
    gpu_actions = tbops.policy_sample(logits.cuda()).cpu()
    assert gpu_actions.shape == (N_DRAWS,)
    assert gpu_actions.dtype == torch.int64
    assert int(gpu_actions.min()) >= 0 and int(gpu_actions.max()) < A_FULL
    gpu_stats, gpu_dead = _chi2_per_group(gpu_actions, z)
    print("gpu", gpu_stats)
    assert gpu_dead == 0, "an action at logit -40 was drawn"
    assert max(gpu_stats) < limit, gpu_stats


def test_policy_sample_rows_are_independent():
    logits = torch.zeros(N_DRAWS, 2)
    n = N_DRAWS - 1
    sigma = n ** 0.5 / 2

    torch.manual_seed(42)
    a = tbops.policy_sample(logits.cuda()).cpu()
    agree = int((a[1:] == a[:-1]).sum())
    ones = int(a.sum())
    print(f"adjacent rows agreeing: {agree}, expected {n / 2} +- {sigma:.1f};"
          f" ones: {ones}")
    assert abs(agree - n / 2) <= 5 * sigma
    assert abs(ones - N_DRAWS / 2) <= 5 * N_DRAWS ** 0.5 / 2


def test_policy_sample_is_deterministic_under_manual_seed():
    logits = _four_logit_vectors().repeat(1000, 1).cuda()
    torch.manual_seed(43)
    a = tbops.policy_sample(logits)
    torch.manual_seed(43)
    b = tbops.policy_sample(logits)
    torch.manual_seed(44)
    c = tbops.policy_sample(logits)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


def test_policy_sample_greedy_is_first_index_argmax():
    N = 1001  # 3 full blocks of 256 and a tail of 233
    g = torch.Generator().manual_seed(45)
    z = torch.randn(N, A_FULL, generator=g)
    # Exact ties in the last row of all and in every 7th of the first 1000:
    # the maximum copied to an earlier or a later index, all equal, or a
    # tie between the first and the last action.
    for r in list(range(0, 1000, 7)) + [N - 1]:
        kind = (r // 7) % 4
        top = z[r].max()
        if kind == 0:
            z[r, (int(z[r].argmax()) + 5) % A_FULL] = top
        elif kind == 1:
            z[r] = 0.25
        elif kind == 2:
            z[r, 0] = z[r, A_FULL - 1] = top + 1
        else:
            z[r, int(z[r].argmax()) - 1] = top  # index -1 wraps to the last
    expected = torch.from_numpy(np.argmax(z.numpy(), axis=-1))  # first max
    assert torch.equal(torch.argmax(z, -1), expected)
    ties = (z == z.max(-1, keepdim=True).values).sum(-1) > 1
    assert int(ties.sum()) >= 140

    got = tbops.policy_sample(z.cuda(), greedy=True).cpu()
    assert got.shape == (N,) and got.dtype == torch.int64
    assert torch.equal(got, expected)


def test_policy_sample_time_major_input():
    T, B = 7, 37
    g = torch.Generator().manual_seed(46)
    z = torch.randn(T, B, A_FULL, generator=g)
    got = tbops.policy_sample(z.cuda(), greedy=True).cpu()
    assert got.shape == (T, B)
    assert torch.equal(got, torch.argmax(z, -1))

    torch.manual_seed(47)
    drawn = tbops.policy_sample(z.cuda()).cpu()
    assert drawn.shape == (T, B)
    assert int(drawn.min()) >= 0 and int(drawn.max()) < A_FULL
    # the flattened rows draw what the same rows draw as [N, A]
    torch.manual_seed(47)
    flat = tbops.policy_sample(z.reshape(T * B, A_FULL).cuda()).cpu()
    assert torch.equal(drawn.reshape(-1), flat)


@pytest.mark.parametrize("greedy", [True, False])
def test_policy_sample_single_action(greedy):
    torch.manual_seed(48)
    z = torch.randn(300, 1)
    got = tbops.policy_sample(z.cuda(), greedy=greedy).cpu()
    assert got.shape == (300,)
    assert (got == 0).all()
