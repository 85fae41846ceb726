"""AtariNet (with and without last_action) and ResNet with their heads on the
fp32 MFMA heads kernels behind TBAMD_HEADS_MFMA=1, at T * B = 34.

Heads: from the fc output the GPU model itself produced, logits, baseline and
the four head gradients lie within K * 2^-24 * S of float64 on the CPU, the
margin of tests/test_heads_mfma_gpu.py. Everything upstream goes through the
bf16 trunk and is held to the existing trunk tolerances against a float64 copy
of the whole model on the CPU: rtol 5e-2, atol 5e-3 for the outputs (the bf16
stages in front of the heads, tests/test_inference_runner_gpu.py) and cosine
> 0.98 for every parameter gradient (tests/test_resnet_mfma.py). Unset,
heads_fwd is never looked up and the outputs are the eager lines' bit for bit.
"""

import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.models.atari_net import AtariNet
    from torchbeast_amd.models.resnet import ResNet
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_heads_mfma_gpu import K_BOUND, U  # noqa: E402

A, T, B = 6, 2, 17
KINDS = ["atari", "atari_no_action", "resnet"]


def _net(kind):
    torch.manual_seed(1)
    if kind == "resnet":
        return ResNet((4, 84, 84), A)
    return AtariNet((4, 84, 84), A, use_last_action=kind == "atari")


def _inputs():
    g = torch.Generator().manual_seed(2)
    return dict(
        frame=torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8,
                            generator=g),
        reward=2 * torch.randn(T, B, generator=g),
        done=torch.zeros(T, B, dtype=torch.bool),
        last_action=torch.randint(0, A, (T, B), generator=g),
    ), torch.randn(T, B, A, generator=g), torch.randn(T, B, generator=g)


def _run(net, inputs):
    out, _ = net(inputs, ())
    if isinstance(out, dict):
        return out["policy_logits"], out["baseline"]
    return out[1], out[2]


def _core(kind, h, inputs):
    """The eager lines' core input from the fc output h."""
    cols = [h, inputs["reward"].clamp(-1, 1).view(-1, 1).to(h)]
    if kind == "atari":
        cols.append(F.one_hot(inputs["last_action"].flatten(), A).to(h))
    return torch.cat(cols, -1)


def _count_heads_fwd(monkeypatch):
    ext, seen = ops_mod.require_ext(), [0]

    class Counting:
        def __getattr__(self, name):
            if name == "heads_fwd":
                seen[0] += 1
            return getattr(ext, name)

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


def _within(got, ref, s, what):
    ratio = float(((got.cpu().double() - ref).abs()
                   / (U * s).clamp_min(1e-300)).max())
    print(f"RATIO heads model {what}: {ratio:.3f} of 2^-24*S")
    assert ratio <= K_BOUND, (what, ratio)


@pytest.mark.parametrize("kind", KINDS)
def test_model_on_the_kernels_against_float64(kind, monkeypatch):
    monkeypatch.setenv("TBAMD_HEADS_MFMA", "1")
    monkeypatch.delenv("TBAMD_FC_MFMA", raising=False)
    seen = _count_heads_fwd(monkeypatch)
    inputs, gl, gb = _inputs()
    net = _net(kind)
    net64 = copy.deepcopy(net).double()
    first = next(m for m in net64.modules() if isinstance(m, torch.nn.Conv2d))
    first.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    net = net.cuda()
    got = {}
    net.fc.register_forward_hook(lambda mod, args, out: got.update(h=out))

    logits, base = _run(net, {k: v.cuda() for k, v in inputs.items()})
    assert seen[0] >= 1
    ((logits * gl.cuda()).sum() + (base * gb.cuda()).sum()).backward()
    logits64, base64 = _run(net64, inputs)
    ((logits64 * gl).sum() + (base64 * gb).sum()).backward()

    # The heads alone, from the GPU's own fc output.
    core = _core(kind, F.relu(got["h"]).detach().cpu().double(), inputs)
    w = torch.cat([net.policy.weight, net.baseline.weight]).detach().cpu().double()
    b = torch.cat([net.policy.bias, net.baseline.bias]).detach().cpu().double()
    dy = torch.cat([gl.view(-1, A), gb.view(-1, 1)], 1).double()
    y = torch.cat([logits.view(-1, A), base.view(-1, 1)], 1).detach()
    _within(y, core @ w.t() + b, core.abs() @ w.abs().t() + b.abs(), "y")
    _within(torch.cat([net.policy.weight.grad, net.baseline.weight.grad]),
            dy.t() @ core, dy.abs().t() @ core.abs(), "dW")
    _within(torch.cat([net.policy.bias.grad, net.baseline.bias.grad]),
            dy.sum(0), dy.abs().sum(0), "db")

    # The whole model against its float64 copy, at the trunk's tolerance.
    for a, r in ((logits, logits64), (base, base64)):
        torch.testing.assert_close(a.detach().cpu().double(), r.detach(),
                                   rtol=5e-2, atol=5e-3)
    ref = dict(net64.named_parameters())
    for name, p in net.named_parameters():
        cos = F.cosine_similarity(p.grad.cpu().double().flatten(),
                                  ref[name].grad.flatten(), dim=0)
        assert cos > 0.98, f"{name}: grad cosine {cos:.4f}"


@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_is_the_eager_lines(kind, monkeypatch):
    monkeypatch.delenv("TBAMD_HEADS_MFMA", raising=False)
    monkeypatch.delenv("TBAMD_FC_MFMA", raising=False)
    seen = _count_heads_fwd(monkeypatch)
    inputs = {k: v.cuda() for k, v in _inputs()[0].items()}
    net = _net(kind).cuda()
    got = {}
    net.fc.register_forward_hook(lambda mod, args, out: got.update(h=out))
    with torch.no_grad():
        logits, base = _run(net, inputs)
        core = _core(kind, F.relu(got["h"]), inputs)
        assert torch.equal(logits.flatten(0, 1), net.policy(core))
        assert torch.equal(base.flatten(), net.baseline(core).flatten())
    assert seen[0] == 0
