"""HIP kernel numerics vs plain PyTorch fp32 references (CPU oracles).

Every fused CDNA4 kernel is compared against the eager implementation that
the CPU path uses (which is itself oracle-tested against NumPy in
test_vtrace.py / test_losses.py / test_flat.py)."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.core import vtrace
    from torchbeast_amd.ops import functional as tbops
    from torchbeast_amd.parallel import flat as tbflat
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

from lstm_oracle import lstm_mimic as _lstm_mimic  # noqa: E402


def test_hip_extension_loaded():
    import torchbeast_amd.ops as ops

    assert ops.hip_available(), "_tbops must be built and importable on GPU"


@pytest.mark.parametrize("T,B,A", [(80, 8, 6), (7, 3, 18), (1, 1, 2)])
def test_vtrace_kernel_matches_eager(T, B, A):
    torch.manual_seed(0)
    behavior = torch.randn(T, B, A)
    target = torch.randn(T, B, A)
    actions = torch.randint(0, A, (T, B))
    discounts = (torch.rand(T, B) > 0.1).float() * 0.99
    rewards = torch.randn(T, B)
    values = torch.randn(T, B)
    bootstrap = torch.randn(B)

    cpu = vtrace.from_logits(behavior, target, actions, discounts, rewards,
                             values, bootstrap)
    gpu = vtrace.from_logits(
        behavior.cuda(), target.cuda(), actions.cuda(), discounts.cuda(),
        rewards.cuda(), values.cuda(), bootstrap.cuda()
    )
    for name in cpu._fields:
        torch.testing.assert_close(
            getattr(gpu, name).cpu(), getattr(cpu, name),
            rtol=2e-4, atol=2e-4, msg=lambda m, n=name: f"{n}: {m}",
        )


def test_fused_loss_matches_eager_values_and_grads():
    T, B, A = 20, 8, 6
    torch.manual_seed(1)
    logits_cpu = torch.randn(T, B, A, requires_grad=True)
    baseline_cpu = torch.randn(T, B, requires_grad=True)
    actions = torch.randint(0, A, (T, B))
    pg_adv = torch.randn(T, B)
    vs = torch.randn(T, B)

    pg_c, bl_c, ent_c = tbops.fused_impala_loss(
        logits_cpu, baseline_cpu, actions, pg_adv, vs
    )
    total_c = pg_c + 0.5 * bl_c + 0.01 * ent_c
    total_c.backward()

    logits_gpu = logits_cpu.detach().cuda().requires_grad_()
    baseline_gpu = baseline_cpu.detach().cuda().requires_grad_()
    pg_g, bl_g, ent_g = tbops.fused_impala_loss(
        logits_gpu, baseline_gpu, actions.cuda(), pg_adv.cuda(), vs.cuda()
    )
    total_g = pg_g + 0.5 * bl_g + 0.01 * ent_g
    total_g.backward()

    torch.testing.assert_close(pg_g.cpu(), pg_c, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(bl_g.cpu(), bl_c, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(ent_g.cpu(), ent_c, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(logits_gpu.grad.cpu(), logits_cpu.grad,
                               rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(baseline_gpu.grad.cpu(), baseline_cpu.grad,
                               rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("clip", [None, 1.0])
def test_rmsprop_kernel_matches_eager(clip):
    torch.manual_seed(2)
    n = 10_000
    param_c = torch.randn(n)
    grad = torch.randn(n)
    sq_c = torch.rand(n)

    param_g = param_c.cuda().clone()
    sq_g = sq_c.cuda().clone()

    norm_c = tbops.rmsprop_step(param_c, grad.clone(), sq_c, 0.01, 0.99, 0.01,
                                clip)
    norm_g = tbops.rmsprop_step(param_g, grad.cuda(), sq_g, 0.01, 0.99, 0.01,
                                clip)

    torch.testing.assert_close(norm_g.cpu(), norm_c, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(param_g.cpu(), param_c, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(sq_g.cpu(), sq_c, rtol=1e-4, atol=1e-5)


def test_policy_sample_distribution_and_greedy():
    torch.manual_seed(3)
    logits = torch.tensor([[2.0, 0.0, -2.0]]).repeat(20000, 1).cuda()
    actions = tbops.policy_sample(logits, greedy=False)
    assert actions.shape == (20000,)
    probs = torch.softmax(logits[0], -1)
    freq = torch.bincount(actions.cpu(), minlength=3).float() / 20000
    assert torch.allclose(freq, probs.cpu(), atol=0.02)

    greedy = tbops.policy_sample(logits[:5], greedy=True)
    assert (greedy.cpu() == 0).all()


@pytest.mark.parametrize("L,H,use_done", [(1, 32, True), (2, 519, True),
                                          (2, 64, False)])
def test_lstm_unroll_matches_eager(L, H, use_done):
    T, B, I = 12, 4, 24
    torch.manual_seed(4)
    core_cpu = torch.nn.LSTM(I, H, num_layers=L)
    core_gpu = torch.nn.LSTM(I, H, num_layers=L).cuda()
    core_gpu.load_state_dict(core_cpu.state_dict())

    x = torch.randn(T, B, I)
    notdone = (
        (torch.rand(T, B) > 0.2).float() if use_done else torch.ones(T, B)
    )
    h0 = torch.randn(L, B, H)
    c0 = torch.randn(L, B, H)

    # Precision-faithful oracle (bf16 recurrent matmul, like the kernel).
    out_c, (hT_c, cT_c) = _lstm_mimic(core_cpu, x, notdone, (h0, c0))
    loss_c = out_c.square().sum() + hT_c.sum() + cT_c.sum()
    loss_c.backward()

    xg = x.cuda().requires_grad_()
    h0g = h0.cuda().requires_grad_()
    c0g = c0.cuda().requires_grad_()
    out_g, (hT_g, cT_g) = tbops.lstm_unroll(core_gpu, xg, notdone.cuda(),
                                            (h0g, c0g))
    loss_g = out_g.square().sum() + hT_g.sum() + cT_g.sum()
    loss_g.backward()

    torch.testing.assert_close(out_g.cpu(), out_c, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(hT_g.cpu(), hT_c, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(cT_g.cpu(), cT_c, rtol=2e-3, atol=2e-3)

    # Weight grads vs CPU autograd through the bf16-faithful mimic. The
    # kernel's backward places its bf16 rounding slightly differently
    # (dgates@W in bf16), so tolerances are rounding-scaled.
    for (name_c, p_c), (name_g, p_g) in zip(
        core_cpu.named_parameters(), core_gpu.named_parameters()
    ):
        assert name_c == name_g
        scale = p_c.grad.abs().max().clamp_min(1e-4)
        err = (p_g.grad.cpu() - p_c.grad).abs().max() / scale
        assert err < 2e-2, f"grad {name_c}: rel-max err {err:.4f}"

    # And the fp32 eager loop must still agree directionally.
    core_fp = torch.nn.LSTM(core_cpu.input_size, H, num_layers=L)
    core_fp.load_state_dict(
        {k: v.detach().clone() for k, v in core_cpu.state_dict().items()})
    out_f, _ = tbops.lstm_unroll(core_fp, x, notdone, (h0, c0))
    cos = torch.nn.functional.cosine_similarity(
        out_g.detach().cpu().flatten(), out_f.detach().flatten(), dim=0)
    assert cos > 0.999, f"cosine vs fp32 eager: {cos}"


def test_lstm_input_grads_match():
    T, B, I, H, L = 6, 3, 10, 16, 2
    torch.manual_seed(5)
    core_cpu = torch.nn.LSTM(I, H, num_layers=L)
    core_gpu = torch.nn.LSTM(I, H, num_layers=L).cuda()
    core_gpu.load_state_dict(core_cpu.state_dict())

    x_c = torch.randn(T, B, I, requires_grad=True)
    notdone = (torch.rand(T, B) > 0.3).float()
    h0 = torch.zeros(L, B, H)
    c0 = torch.zeros(L, B, H)
    out_c, _ = tbops.lstm_unroll(core_cpu, x_c, notdone, (h0, c0))
    out_c.sum().backward()

    x_g = x_c.detach().cuda().requires_grad_()
    out_g, _ = tbops.lstm_unroll(core_gpu, x_g, notdone.cuda(),
                                 (h0.cuda(), c0.cuda()))
    out_g.sum().backward()
    # bf16 recurrent rounding: compare against autograd through the mimic.
    x_m = x_c.detach().clone().requires_grad_()
    out_m, _ = _lstm_mimic(core_cpu, x_m, notdone, (h0, c0))
    out_m.sum().backward()
    torch.testing.assert_close(x_g.grad.cpu(), x_m.grad, rtol=2e-2, atol=2e-3)


@pytest.mark.parametrize("N,shape", [(7, (4, 84, 84)), (3, (4, 36, 36)),
                                     (64, (4, 84, 84))])
def test_atari_trunk_matches_eager(N, shape):
    import torch.nn.functional as Fn

    torch.manual_seed(6)
    conv1 = torch.nn.Conv2d(shape[0], 32, 8, stride=4).cuda()
    conv2 = torch.nn.Conv2d(32, 64, 4, stride=2).cuda()
    conv3 = torch.nn.Conv2d(64, 64, 3, stride=1).cuda()
    frames = torch.randint(0, 256, (N, *shape), dtype=torch.uint8).cuda()

    # no_grad -> the per-sample fp32 VALU trunk serves small batches; its
    # numerics are exact vs eager fp32. (The bf16 MFMA training path has its
    # own precision-scaled oracle in tests/test_conv_mfma.py.)
    with torch.no_grad():
        out = tbops.atari_trunk(frames, conv1, conv2, conv3)
        assert out is not None
        x = frames.float() / 255.0
        ref = Fn.relu(conv3(Fn.relu(conv2(Fn.relu(conv1(x)))))).view(N, -1)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)

    # Training path (bf16 MFMA, 84x84 only): gradients must agree with the
    # eager chain directionally; exact-precision oracles live in
    # tests/test_conv_mfma.py.
    out2 = tbops.atari_trunk(frames, conv1, conv2, conv3)
    if out2 is None:
        return  # unsupported-geometry grad path falls back to eager convs
    out2.square().sum().backward()
    fused_grads = [p.grad.clone() for c in (conv1, conv2, conv3)
                   for p in (c.weight, c.bias)]
    for c in (conv1, conv2, conv3):
        c.weight.grad = None
        c.bias.grad = None
    x = x.detach()
    ref2 = Fn.relu(conv3(Fn.relu(conv2(Fn.relu(conv1(x)))))).view(N, -1)
    ref2.square().sum().backward()
    eager_grads = [p.grad for c in (conv1, conv2, conv3)
                   for p in (c.weight, c.bias)]
    for fg, eg in zip(fused_grads, eager_grads):
        cos = torch.nn.functional.cosine_similarity(
            fg.flatten(), eg.flatten(), dim=0)
        assert cos > 0.995, f"grad cosine {cos}"


def test_atari_trunk_rejects_oversized_frames():
    import torchbeast_amd.ops as ops

    ext = ops.require_ext()
    assert ext.atari_trunk_supported(4, 84, 84)
    assert not ext.atari_trunk_supported(3, 210, 160)


def test_model_forward_gpu_runs_with_fused_ops():
    from torchbeast_amd.models import AtariNet

    T, B, A = 5, 3, 6
    net = AtariNet((4, 84, 84), A, use_lstm=True).cuda()
    inputs = dict(
        frame=torch.randint(0, 255, (T, B, 4, 84, 84), dtype=torch.uint8).cuda(),
        reward=torch.randn(T, B).cuda(),
        done=(torch.rand(T, B) < 0.1).cuda(),
        last_action=torch.randint(0, A, (T, B)).cuda(),
    )
    state = tuple(t.cuda() for t in net.initial_state(B))
    out, new_state = net(inputs, state)
    assert out["policy_logits"].shape == (T, B, A)
    out["baseline"].sum().backward()
