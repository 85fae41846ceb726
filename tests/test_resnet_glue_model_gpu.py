"""The deep ResNet trunk with TBAMD_RESNET_GLUE=1: max-pool, ReLU, skip add
and flatten on ops/hip/resnet_glue.hip between the unchanged MFMA convs.

The new path rounds exactly where the ATen path does, so _features is held
with torch.equal against the switch unset, and the flattened exit against
relu + reshape of it. Gradients of every trunk parameter are compared with a
float64 CPU copy of the model run through plain feat_extract:
err = max|g - g64| / max|g64|, and err_on <= 2 err_off (the new path adds the
two gradients of a tensor in fp32 before one rounding; the factor allows for
the moved rounding points that feed the convs' wgrad). Unset, no
resnet_glue_* symbol is looked up.
"""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.models.resnet import ResNet
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

N = 3  # T * B


def _count_glue(monkeypatch):
    ext, seen = ops_mod.require_ext(), []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("resnet_glue_"):
                seen.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


def _trunk_grads(net, feats, weight):
    net.zero_grad()
    (feats * weight).sum().backward()
    return {k: p.grad.detach().double().cpu()
            for k, p in net.feat_extract.named_parameters()}


@pytest.mark.parametrize("obs,any_geometry", [((4, 84, 84), False),
                                              ((3, 64, 64), True)])
def test_glue_trunk_matches_aten_trunk(obs, any_geometry, monkeypatch):
    monkeypatch.delenv("TBAMD_RESNET", raising=False)
    monkeypatch.delenv("TBAMD_RESNET_GLUE", raising=False)
    if any_geometry:
        monkeypatch.setenv("TBAMD_RESNET_ANY", "1")
    torch.manual_seed(17 + obs[1])
    cpu = ResNet(obs)
    x = torch.randint(0, 256, (N, *obs)).float() / 255.0
    weight = torch.randn(N, cpu.fc.in_features)

    net64 = copy.deepcopy(cpu).double()
    feats64 = F.relu(net64.feat_extract(x.double())).reshape(N, -1)
    ref = _trunk_grads(net64, feats64, weight.double())

    net, xg, wg = copy.deepcopy(cpu).cuda(), x.cuda(), weight.cuda()
    seen = _count_glue(monkeypatch)
    off = net._features(xg)
    off_flat = F.relu(off).reshape(N, -1)
    g_off = _trunk_grads(net, off_flat, wg)
    assert off.dtype == torch.float32 and seen == []

    monkeypatch.setenv("TBAMD_RESNET_GLUE", "1")
    assert torch.equal(net._features(xg), off)
    on_flat = net._features(xg, flat=True)
    assert torch.equal(on_flat, off_flat)
    g_on = _trunk_grads(net, on_flat, wg)
    assert {"resnet_glue_pool_fwd", "resnet_glue_pool_bwd",
            "resnet_glue_ew_fwd", "resnet_glue_ew_bwd",
            "resnet_glue_flat_fwd", "resnet_glue_flat_bwd"} <= set(seen)

    assert len(ref) == 30
    for key, g64 in ref.items():
        scale = g64.abs().max()
        err_off = ((g_off[key] - g64).abs().max() / scale).item()
        err_on = ((g_on[key] - g64).abs().max() / scale).item()
        print(f"{obs} {key}: err_off {err_off:.3e} err_on {err_on:.3e}")
        assert scale > 0 and err_on <= 2 * err_off, key


def test_model_forward_takes_the_flatten_kernel(monkeypatch):
    monkeypatch.delenv("TBAMD_RESNET", raising=False)
    torch.manual_seed(5)
    net = ResNet((4, 84, 84)).cuda().eval()
    inputs = dict(
        frame=torch.randint(0, 256, (N, 1, 4, 84, 84), dtype=torch.uint8,
                            device="cuda"),
        reward=torch.randn(N, 1, device="cuda"),
        done=torch.zeros(N, 1, dtype=torch.bool, device="cuda"))
    monkeypatch.delenv("TBAMD_RESNET_GLUE", raising=False)
    seen = _count_glue(monkeypatch)
    with torch.no_grad():
        (_, logits_off, baseline_off), _ = net(inputs, ())
        assert seen == []
        monkeypatch.setenv("TBAMD_RESNET_GLUE", "1")
        (_, logits_on, baseline_on), _ = net(inputs, ())
    assert "resnet_glue_flat_fwd" in seen
    assert torch.equal(logits_on, logits_off)
    assert torch.equal(baseline_on, baseline_off)
