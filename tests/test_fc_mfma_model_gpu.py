"""The fc of AtariNet and ResNet on the MFMA linear kernels behind
TBAMD_FC_MFMA=1: the models take the new path (launches counted as
tests/test_resnet_any_gpu.py counts them) and agree with the eager fc within
that file's cosine bounds; unset, nothing runs and the output is bit-identical
to the eager line. The C++ runner serves through the kernels within the
tolerances of tests/test_inference_runner_gpu.py, and repacks the fc weight
after mark_weights_dirty().
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.models.atari_net import AtariNet
    from torchbeast_amd.models.resnet import ResNet
    from torchbeast_amd.ops import functional as tbf
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_inference_runner_gpu import (  # noqa: E402
    _check, _compute, _make_inputs, _reference, _start_runner)

NAMES = ("linear_pack", "linear_fwd", "linear_dgrad", "linear_wgrad")
MODELS = ["atari", "resnet"]


def _calls(monkeypatch):
    """Count the launches of the linear entry points through ops.functional."""
    ext = ops_mod.require_ext()
    seen = dict.fromkeys(NAMES, 0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(ext, name)
            if name not in seen:
                return fn

            def counted(*a):
                seen[name] += 1
                return fn(*a)
            return counted

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


def _net(kind):
    torch.manual_seed(1)
    if kind == "atari":
        return AtariNet((4, 84, 84), 6, use_last_action=False).cuda()
    return ResNet((4, 84, 84), 6).cuda()


def _run(net, inputs):
    out, _ = net(inputs, ())
    if isinstance(out, dict):
        return out["policy_logits"], out["baseline"]
    return out[1], out[2]


def _inputs(T=2, B=3):
    torch.manual_seed(2)
    return dict(
        frame=torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8,
                            device="cuda"),
        reward=torch.randn(T, B, device="cuda"),
        done=torch.zeros(T, B, dtype=torch.bool, device="cuda"),
    )


@pytest.mark.parametrize("kind", MODELS)
def test_model_takes_the_kernels_and_matches_eager(kind, monkeypatch):
    seen = _calls(monkeypatch)
    net, inputs = _net(kind), _inputs()
    feats = {}
    net.fc.register_forward_hook(
        lambda mod, args, out: feats.update(x=args[0].detach()))

    monkeypatch.delenv("TBAMD_FC_MFMA", raising=False)
    logits0, base0 = _run(net, inputs)
    assert seen == dict.fromkeys(NAMES, 0)
    (logits0.square().mean() + base0.square().mean()).backward()
    eager = {n: p.grad.clone() for n, p in net.named_parameters()}
    x = feats["x"]
    with torch.no_grad():
        fc_eager = F.relu(net.fc(x))
        assert tbf.fc_relu(net.fc, x) is None
        monkeypatch.setenv("TBAMD_FC_MFMA", "1")
        fc_mfma = tbf.fc_relu(net.fc, x)
    assert seen == dict(linear_pack=1, linear_fwd=1, linear_dgrad=0,
                        linear_wgrad=0)
    cos = F.cosine_similarity(fc_mfma.flatten(), fc_eager.flatten(), dim=0)
    assert cos > 0.999, f"fc cosine {cos:.5f}"

    net.zero_grad()
    logits1, base1 = _run(net, inputs)
    (logits1.square().mean() + base1.square().mean()).backward()
    # The features need a gradient in both models: dgrad runs.
    assert seen == dict(linear_pack=2, linear_fwd=2, linear_dgrad=1,
                        linear_wgrad=1)
    for name, p in net.named_parameters():
        assert torch.isfinite(p.grad).all(), name
        cos = F.cosine_similarity(p.grad.flatten(), eager[name].flatten(),
                                  dim=0)
        assert cos > 0.98, f"{name}: grad cosine {cos:.4f}"


@pytest.mark.parametrize("kind", MODELS)
def test_switch_off_is_bit_identical_to_the_eager_line(kind, monkeypatch):
    monkeypatch.delenv("TBAMD_FC_MFMA", raising=False)
    seen = _calls(monkeypatch)
    net, inputs = _net(kind), _inputs()
    got = {}
    net.fc.register_forward_hook(
        lambda mod, args, out: got.update(x=args[0], out=out))
    with torch.no_grad():
        logits, base = _run(net, inputs)
        h = F.relu(net.fc(got["x"]))
        core = torch.cat([h, inputs["reward"].clamp(-1, 1).view(-1, 1)], -1)
        assert torch.equal(logits.flatten(0, 1), net.policy(core))
        assert torch.equal(base.flatten(), net.baseline(core).flatten())
    assert seen == dict.fromkeys(NAMES, 0)


def test_runner_serves_through_the_kernels_and_repacks(monkeypatch):
    monkeypatch.setenv("TBAMD_FC_MFMA", "1")
    obs = (4, 84, 84)
    model = _net("atari")
    inp = _make_inputs(model, 5, obs, "tensor", False)
    batcher, runner = _start_runner(model, greedy=True)
    try:
        first = _compute(batcher, inp, "tensor")
        ref_first = _reference(model, inp)
        with torch.no_grad():
            model.fc.weight.mul_(0.5)
        third = _compute(batcher, inp, "tensor")  # not marked: old pack
        runner.mark_weights_dirty()
        second = _compute(batcher, inp, "tensor")
        ref_second = _reference(model, inp)
    finally:
        runner.stop()
    _check(first, *ref_first, 5, greedy=True)
    _check(second, *ref_second, 5, greedy=True)
    assert torch.equal(third[1], first[1])  # the library fc would have moved
    assert not torch.equal(second[1], first[1])
