"""The run-time-geometry ResNet convs (ops/hip/conv_mfma.hip conv_any_kernel,
wgrad_any_kernel; entry points resnet_conv_any, resnet_conv_any_wgrad,
resnet_conv_any_supported) against the float64 references of
tests/helpers/conv_oracle.py, and their wiring into ops.functional,
models/resnet.py and the C++ InferenceRunner behind TBAMD_RESNET_ANY=1.

Integer cases are held to exact equality, random-valued ones to
conv_oracle's bound K * 2^-24 * S (plus the bf16 half ulp of a bf16 output);
tests/test_conv_any_oracle.py checks the cases themselves on the CPU. The
model and runner tests use the tolerances of tests/test_resnet_mfma.py and
tests/test_inference_runner_gpu.py. With the switch unset nothing may move:
the last tests of each group pin that.
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.models.resnet import ResNet
    from torchbeast_amd.ops import functional as tbf
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import conv_oracle as co  # noqa: E402
import conv_any_oracle as ca  # noqa: E402
from test_inference_runner_gpu import ATEN, _check, _serve_once  # noqa: E402

ANY = {"TBAMD_RESNET_ANY": "1"}


def _bf(t):
    return t.to(torch.bfloat16).cuda().contiguous()


def _cl(t):
    """NHWC values as the channels_last NCHW tensor the ResNet ops take."""
    return _bf(t).permute(0, 3, 1, 2)


def _empty():
    return torch.empty(0, dtype=torch.float32, device="cuda")


def _run(kind, ops):
    ext = ops_mod.require_ext()
    if kind == "fwd":
        return dict(y=ext.resnet_conv_any(_cl(ops["x"]), ops["wp"].cuda(),
                                          ops["b"].cuda(), True))
    if kind == "dgrad":
        return dict(dx=ext.resnet_conv_any(_cl(ops["dy"]), ops["wr"].cuda(),
                                           _empty(), False))
    dw, db = ext.resnet_conv_any_wgrad(_cl(ops["x"]), _cl(ops["dy"]))
    return dict(dW=dw, db=db)


def _assert_exact(got, refs):
    assert set(got) == set(refs)
    for k, ref in refs.items():
        bad = co.exact_mismatch(got[k], ref)
        assert bad is None, f"{k}: {bad}"


def _assert_bound(label, got, refs, s):
    assert set(got) == set(refs)
    for k, ref in refs.items():
        bad, ratio = co.bound_excess(got[k], ref, s[k], co.K,
                                     k in co.BF16_OUT)
        print(f"RATIO {label} {k}: {ratio:.3f} of 2^-24*S, K = {co.K:.2f}")
        assert bad is None, f"{label} {k}: {bad}"


# ---- the kernels on the integer and random-valued cases ----


@pytest.mark.parametrize("n", ca.NS)
@pytest.mark.parametrize("geom", ca.GEOMS, ids=str)
def test_fwd_exact(geom, n):
    _assert_exact(_run("fwd", ca.int_ops(geom, n)), ca.refs(geom, "fwd", n))


@pytest.mark.parametrize("n", ca.NS)
@pytest.mark.parametrize("geom", [g for g in ca.GEOMS if ca.has_dgrad(g)],
                         ids=str)
def test_dgrad_exact(geom, n):
    _assert_exact(_run("dgrad", ca.int_ops(geom, n)),
                  ca.refs(geom, "dgrad", n))


@pytest.mark.parametrize("geom,n", [(g, n) for g in ca.GEOMS for n in ca.NS]
                         + list(ca.WGRAD_CHUNK_CASES), ids=str)
def test_wgrad_exact(geom, n):
    got = _run("wgrad", ca.int_ops(geom, n))
    _assert_exact(got, ca.refs(geom, "wgrad", n))
    assert not bool(got["dW"][..., 3 * geom[0]:].any())


@pytest.mark.parametrize("geom,n", [(g, ca.NMAX) for g in ca.GEOMS]
                         + list(ca.WGRAD_CHUNK_CASES), ids=str)
def test_random_within_bound(geom, n):
    ops = ca.rand_ops(geom, n)
    for kind in ("fwd", "dgrad", "wgrad"):
        if kind == "dgrad" and not ca.has_dgrad(geom):
            continue
        _assert_bound(f"{kind} {geom} N={n}", _run(kind, ops),
                      ca.refs(geom, kind, n, False),
                      ca.refs(geom, kind, n, False, True))


@pytest.mark.parametrize("geom", co.RESNET_GEOMS, ids=str)
def test_square_geometries_equal_the_template_kernels(geom):
    """On conv_oracle's own operands the new entry points equal the float64
    references exactly; tests/test_conv_mfma_exact_gpu.py holds the template
    kernels to the same equality, so the two implementations agree. The
    template kernels run here too, on the same tensors."""
    ext = ops_mod.require_ext()
    ci, hw, c_out = geom
    n = co.RESNET_NMAX[hw]
    ops = co.int_ops("rn_fwd", geom, n)
    x, dy = _cl(ops["x"]), _cl(ops["dy"])
    wp, wr, b = ops["wp"].cuda(), ops["wr"].cuda(), ops["b"].cuda()
    y = ext.resnet_conv_any(x, wp, b, True)
    _assert_exact(dict(y=y), co.entry_refs("rn_fwd", ops))
    assert torch.equal(y, ext.resnet_conv(x, wp, b, ci, hw, c_out, True))
    dw, db = ext.resnet_conv_any_wgrad(x, dy)
    _assert_exact(dict(dW=dw, db=db), co.entry_refs("rn_wgrad", ops))
    dw0, db0 = ext.resnet_conv_wgrad(x, dy, ci, hw, c_out)
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    if ci != 8:
        dx = ext.resnet_conv_any(dy, wr, _empty(), False)
        _assert_exact(dict(dx=dx), co.entry_refs("rn_dgrad", ops))
        assert torch.equal(dx, ext.resnet_conv(dy, wr, _empty(), c_out, hw,
                                               ci, False))


# ---- the host side ----


def test_supported_agrees_with_the_planner():
    ext = ops_mod.require_ext()
    for geom in ca.GEOMS + ca.SQUARE + tuple(g for g, _ in
                                             ca.WGRAD_CHUNK_CASES):
        assert ext.resnet_conv_any_supported(*geom), geom
        assert tbf.resnet_conv_any_supported(*geom), geom
    for geom in ca.REFUSED:
        assert not ext.resnet_conv_any_supported(*geom), geom
    for ci, c_out in ((8, 16), (16, 16), (16, 32), (32, 16), (32, 32)):
        for h, w in ((1, 1), (1, 256), (256, 1), (256, 256)):
            assert ext.resnet_conv_any_supported(ci, h, w, c_out)


def test_host_checks_raise_before_any_launch():
    ext = ops_mod.require_ext()
    geom = (16, 5, 7, 16)
    ops = ca.int_ops(geom, 1)
    x, dy = _cl(ops["x"]), _cl(ops["dy"])
    wp, wr, b = ops["wp"].cuda(), ops["wr"].cuda(), ops["b"].cuda()
    torch.cuda.synchronize()
    bad = [
        ("CPU tensor", lambda: ext.resnet_conv_any(x.cpu(), wp, b, True)),
        ("fp32 tensor", lambda: ext.resnet_conv_any(x.float(), wp, b, True)),
        ("NCHW-contiguous",
         lambda: ext.resnet_conv_any(x.contiguous(), wp, b, True)),
        ("wrong K", lambda: ext.resnet_conv_any(x, wp[:, :128].contiguous(),
                                                b, True)),
        ("bias for dgrad", lambda: ext.resnet_conv_any(dy, wr, b, False)),
        ("no bias for fwd",
         lambda: ext.resnet_conv_any(x, wp, _empty(), True)),
        ("W = 257", lambda: ext.resnet_conv_any(
            torch.zeros(1, 1, 257, 16, dtype=torch.bfloat16,
                        device="cuda").permute(0, 3, 1, 2), wp, b, True)),
        ("wgrad CPU", lambda: ext.resnet_conv_any_wgrad(x.cpu(), dy)),
        ("wgrad fp32", lambda: ext.resnet_conv_any_wgrad(x, dy.float())),
        ("wgrad NCHW",
         lambda: ext.resnet_conv_any_wgrad(x.contiguous(), dy)),
        ("wgrad shapes", lambda: ext.resnet_conv_any_wgrad(x, dy[:, :, :4])),
        ("wgrad H = 257", lambda: ext.resnet_conv_any_wgrad(
            torch.zeros(1, 257, 1, 16, dtype=torch.bfloat16,
                        device="cuda").permute(0, 3, 1, 2),
            torch.zeros(1, 257, 1, 16, dtype=torch.bfloat16,
                        device="cuda").permute(0, 3, 1, 2))),
    ]
    for name, call in bad:
        try:
            call()
        except RuntimeError:
            continue
        pytest.fail(f"{name}: no error raised")
    torch.cuda.synchronize()  # nothing faulted: nothing was launched
    # and the operands still give the right answer afterwards
    _assert_exact(dict(y=ext.resnet_conv_any(x, wp, b, True)),
                  ca.refs(geom, "fwd", 1))


# ---- end to end through the autograd Functions ----


def test_conv3x3_end_to_end_exact():
    geom, n = (16, 36, 48, 32), 3
    c = ca.int_case(geom)
    x = _cl(c["x"][:n]).detach().requires_grad_()
    w = c["w"].cuda().requires_grad_()
    b = c["b"].cuda().requires_grad_()
    out = tbf._ResNetConv3x3.apply(x, w, b)
    _assert_exact(dict(y=out.permute(0, 2, 3, 1)), ca.refs(geom, "fwd", n))
    out.backward(_cl(c["dy"][:n]))
    dx, dw, db = ca.int_autograd(geom, n)
    _assert_exact(dict(dx=x.grad, dw=w.grad, db=b.grad),
                  dict(dx=dx, dw=dw, db=db))


def test_first_conv_end_to_end_exact():
    geom, n, ci = (8, 72, 96, 16), 3, 3
    c = ca.int_case(geom)
    x8 = c["x"][:n].clone()
    x8[..., ci:] = 0.0  # as resnet_first_conv pads the observation channels
    w = c["w"][:, :ci].contiguous().cuda().requires_grad_()
    b = c["b"].cuda().requires_grad_()
    conv = torch.nn.Conv2d(ci, 16, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    out = tbf.resnet_first_conv(conv, co.nchw(x8[..., :ci]).float().cuda())
    _assert_exact(dict(y=out.permute(0, 2, 3, 1)),
                  dict(y=co.resnet_conv(x8, c["wp"], c["b"], True)))
    out.backward(_cl(c["dy"][:n]))
    _, dw, db = ca.int_autograd(geom, n, first_ci=ci)
    _assert_exact(dict(dw=conv.weight.grad, db=conv.bias.grad),
                  dict(dw=dw, db=db))


# ---- the model ----

FRAMES = [(3, 64, 64), (3, 72, 96)]


def _calls(monkeypatch):
    """Count the launches of the new entry points through ops.functional."""
    ext = ops_mod.require_ext()
    seen = dict(conv=0, wgrad=0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(ext, name)
            if name == "resnet_conv_any":
                def counted(*a):
                    seen["conv"] += 1
                    return fn(*a)
                return counted
            if name == "resnet_conv_any_wgrad":
                def counted_w(*a):
                    seen["wgrad"] += 1
                    return fn(*a)
                return counted_w
            return fn

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


@pytest.mark.parametrize("shape", FRAMES, ids=str)
def test_model_features_match_eager(shape, monkeypatch):
    monkeypatch.setenv("TBAMD_RESNET_ANY", "1")
    seen = _calls(monkeypatch)
    torch.manual_seed(0)
    net = ResNet(shape, 6).cuda()
    x = torch.randn(3, *shape, device="cuda")
    with torch.no_grad():
        fused = net._features(x)
        ref = net.feat_extract(x)
    assert seen["conv"] == 15  # every conv of the trunk, none on ATen
    assert fused.shape == ref.shape
    cos = F.cosine_similarity(fused.flatten(), ref.flatten(), dim=0)
    assert cos > 0.999, f"trunk cosine {cos:.5f}"
    denom = ref.abs().mean().clamp_min(1e-3)
    assert (fused - ref).abs().mean() / denom < 5e-2


@pytest.mark.parametrize("shape", FRAMES, ids=str)
def test_model_end_to_end_grads(shape, monkeypatch):
    monkeypatch.setenv("TBAMD_RESNET_ANY", "1")
    seen = _calls(monkeypatch)
    torch.manual_seed(1)
    net = ResNet(shape, 6, use_lstm=False).cuda()
    T, B = 2, 3
    inputs = dict(
        frame=torch.randint(0, 256, (T, B, *shape), dtype=torch.uint8,
                            device="cuda"),
        reward=torch.randn(T, B, device="cuda"),
        done=torch.zeros(T, B, dtype=torch.bool, device="cuda"),
    )
    (_, logits, baseline), _ = net(inputs, ())
    (logits.float().square().mean() + baseline.float().square().mean()
     ).backward()
    # 15 forwards and 14 dgrads (the first conv has none); 15 wgrads.
    assert seen == dict(conv=29, wgrad=15)
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name

    net2 = ResNet(shape, 6).cuda()
    net2.load_state_dict(net.state_dict())
    monkeypatch.setenv("TBAMD_RESNET", "aten")  # still wins over the switch
    (_, l2, b2), _ = net2(inputs, ())
    (l2.float().square().mean() + b2.float().square().mean()).backward()
    assert seen == dict(conv=29, wgrad=15)
    for (n1, p1), (_, p2) in zip(net.named_parameters(),
                                 net2.named_parameters()):
        if "conv" not in n1 and "feat" not in n1:
            continue
        cos = F.cosine_similarity(p1.grad.flatten(), p2.grad.flatten(), dim=0)
        assert cos > 0.98, f"{n1}: grad cosine {cos:.4f}"


@pytest.mark.parametrize("shape", FRAMES, ids=str)
def test_model_switch_off_is_bit_identical_to_eager(shape, monkeypatch):
    monkeypatch.delenv("TBAMD_RESNET_ANY", raising=False)
    seen = _calls(monkeypatch)
    torch.manual_seed(0)
    net = ResNet(shape, 6).cuda()
    x = torch.randn(3, *shape, device="cuda")
    with torch.no_grad():
        assert torch.equal(net._features(x), net.feat_extract(x))
    assert seen == dict(conv=0, wgrad=0)


# ---- the C++ runner ----


@pytest.mark.parametrize("shape,use_lstm", [((3, 64, 64), False),
                                            ((3, 72, 96), False),
                                            ((3, 64, 64), True)], ids=str)
def test_runner_switch_on_matches_model(shape, use_lstm, monkeypatch):
    torch.manual_seed(1)
    model = ResNet(shape, 6, use_lstm=use_lstm).cuda()
    (out,), ref_out, ref_state = _serve_once(
        model, 5, use_lstm, shape, "tensor", True, ANY, monkeypatch)
    _check(out, ref_out, ref_state, 5, greedy=True)


def test_runner_switch_off_serves_through_aten(monkeypatch):
    """Unset, a 3x64x64 deep model is served as before: here through the
    ATen trunk and heads under the first-serve lock, within the runner's
    tolerances of the ATen model."""
    monkeypatch.delenv("TBAMD_RESNET_ANY", raising=False)
    monkeypatch.setenv("TBAMD_RESNET", "aten")
    torch.manual_seed(1)
    model = ResNet((3, 64, 64), 6).cuda()
    # The first serve includes MIOpen's solution search for new conv shapes.
    (out,), ref_out, ref_state = _serve_once(
        model, 5, False, (3, 64, 64), "tensor", True, ATEN, monkeypatch,
        timeout=240)
    _check(out, ref_out, ref_state, 5, greedy=True)
