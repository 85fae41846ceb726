"""Every entry point of ops/hip/conv_mfma.hip against the float64 references
of tests/helpers/conv_oracle.py, called directly so that each kernel is judged
on its own operands, at the sizes where its grid arithmetic changes.

Integer cases. Operands are small integers (frames in {0, 255}, which stage
as exactly 0.0 and 1.0), so every product and partial sum of the bf16 x bf16
-> fp32 arithmetic is an integer below 2^24 and every bf16 output is exact:
the result does not depend on summation order and is compared with
torch.equal. A failure names the element. tests/test_conv_oracle.py asserts,
without a GPU, that these cases stay in range, that 20-80 % of every compared
tensor is nonzero, that neighbouring samples differ, and that the comparison
rejects a zeroed tap, a dropped wgrad row, a neighbour's tile and a zeroed
edge column. What the sizes reach:

  trunk forward   N = 1023 | 1024: the switch from per-sample kernels to the
                  multi-sample ones (SB = 3 and 6); 1024, 1025, 1026 give
                  sample tails 1/4, 2/5 and none. Batches repeat 7 distinct
                  samples, coprime to 3 and 6, so block contents rotate.
                  210x160: last bands of 12 of 13 (conv1) and 4 of 6 rows.
  mask_d3         N = 168 (and 24 at 210x160): the grid-stride loop wraps.
  dgrad3          N = 6, 7, 8: SB = 4 tails 2, 3, none; 210x160: two bands.
  dgrad2          210x160: seven bands, the last of 3 rows, IWL = 42.
  wgrad           M below one 64-row round (49), multiples of 64 (1600) and
                  of the chunk (128 * 400 = 25 * 2048), chunk boundaries
                  inside a sample, second chunks of 5, 58 and 352 rows; the
                  K-padding columns of dW must be exactly zero.
  ResNet          all five geometries, CI = 8 and 16 being the per-lane-group
                  ky path with K padded 72 -> 96 and 144 -> 160; wgrad with
                  second chunks of 2960 and of 65 = 64 + 1 rows.
  end to end      the autograd Functions against float64 autograd of the same
                  integer network: pins the weight rotation and the unpack
                  permutes on the Python side.

Random-valued cases. One per entry point at the smallest N with a second
block or chunk (the forward also at N = 1025), operands rounded to bf16 on the
host, against float64 on those same operands:

    fp32 outputs (out3, dW, db)   |got - ref| <= K * 2^-24 * S
    bf16 outputs                  |got - ref| <= 2^-8 * |ref| + K * 2^-24 * S

S = sum|terms| + |bias| per element, 2^-8 * |ref| half a bf16 ulp. Each
forward layer is given the kernel's own previous activation, so it is judged
on its own arithmetic. K is derived: float32 F.conv2d / conv2d_input /
conv2d_weight on the CPU reach r = 2.57 of 2^-24 * S over these cases (2.00
forward, 2.57 dgrad, 2.51 wgrad, 0.09 db), and K = 4 r = 10.28 allows for the
kernels' different but no deeper summation order. The kernels measure at most
2.22 (dW of wgrad3 at N = 21; 1.77 for out3, 1.75 and 0.89 for the dW of
wgrad2 and wgrad1, under 0.1 for every db); the bf16 outputs exceed their
half ulp by at most 0.08 of 2^-24 * S. Every test prints its ratio.
"""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.ops import functional as tbf
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import conv_oracle as co  # noqa: E402


def _bf(t):
    return t.to(torch.bfloat16).cuda().contiguous()


def _cl(t):
    """NHWC values as the channels_last NCHW tensor the ResNet ops take."""
    return _bf(t).permute(0, 3, 1, 2)


def _run(entry, ops):
    """The extension's outputs for the operands of one entry point."""
    ext = ops_mod.require_ext()
    if entry == "fwd":
        out3, a1, a2 = ext.conv_trunk_fwd(
            ops["frames"].cuda(), ops["w1p"].cuda(), ops["b1"].cuda(),
            ops["w2p"].cuda(), ops["b2"].cuda(), ops["w3p"].cuda(),
            ops["b3"].cuda(), True)
        return dict(a1=a1, a2=a2, out3=out3)
    if entry == "mask":
        return dict(d3m=ext.conv_trunk_mask_d3(ops["d_out"].cuda(),
                                               ops["out3"].cuda()))
    if entry in ("dgrad3", "dgrad2"):
        fn = getattr(ext, "conv_trunk_" + entry)
        name = "d2" if entry == "dgrad3" else "d1"
        return {name: fn(_bf(ops["dy"]), ops["wr"].cuda(), _bf(ops["act"]))}
    if entry in ("wgrad1", "wgrad2", "wgrad3"):
        x = ops["x"].cuda() if entry == "wgrad1" else _bf(ops["x"])
        dw, db = getattr(ext, "conv_trunk_" + entry)(x, _bf(ops["dy"]))
        return dict(dW=dw, db=db)
    n, hw, _, ci = ops["x"].shape
    co_ = ops["dy"].shape[-1]
    if entry == "rn_fwd":
        return dict(y=ext.resnet_conv(_cl(ops["x"][:n]), ops["wp"].cuda(),
                                      ops["b"].cuda(), ci, hw, co_, True))
    if entry == "rn_dgrad":
        empty = torch.empty(0, dtype=torch.float32, device="cuda")
        return dict(dx=ext.resnet_conv(_cl(ops["dy"]), ops["wr"].cuda(),
                                       empty, co_, hw, ci, False))
    dw, db = ext.resnet_conv_wgrad(_cl(ops["x"]), _cl(ops["dy"]), ci, hw, co_)
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


def _exact_case(entry, geom, n):
    ops = co.int_ops(entry, geom, n)
    _assert_exact(_run(entry, ops), co.entry_refs(entry, ops))


def _random_case(entry, geom, n):
    ops = co.rand_ops(entry, geom, n)
    _assert_bound(f"{entry} {geom} N={n}", _run(entry, ops),
                  co.entry_refs(entry, ops),
                  co.entry_refs(entry, ops, absolute=True))


# ---- trunk forward ----


@pytest.mark.parametrize("geom,n", co.FWD_CASES)
def test_trunk_fwd_exact(geom, n):
    frames, refs = co.int_fwd_refs(geom, n)
    ops = dict(co.int_ops("fwd", geom, 1), frames=frames)
    assert frames.shape[0] == n
    _assert_exact(_run("fwd", ops), refs)


def test_trunk_fwd_without_stash_exact():
    frames, refs = co.int_fwd_refs("84", 1025)
    c = co.int_chain("84")
    (out3,) = ops_mod.require_ext().conv_trunk_fwd(
        frames.cuda(), c["w1p"].cuda(), c["b1"].cuda(), c["w2p"].cuda(),
        c["b2"].cuda(), c["w3p"].cuda(), c["b3"].cuda(), False)
    _assert_exact(dict(out3=out3), dict(out3=refs["out3"]))


@pytest.mark.parametrize("geom,n", co.RANDOM_FWD_CASES)
def test_trunk_fwd_random(geom, n):
    c = co.rand_trunk_case(geom, n)
    m = c["frames"].shape[0]
    frames = c["frames"] if m == n else co.rotated(c["frames"], n)
    got = {k: v.cpu() for k, v in _run("fwd", dict(c, frames=frames)).items()}
    if m != n:
        # Repeated samples give repeated results whichever block and tail
        # they fall into; the first ROTATE then stand for all.
        for k, v in got.items():
            assert torch.equal(v, co.rotated(v[:m], n)), k
    x = c["frames"]
    for layer, name in ((1, "a1"), (2, "a2"), (3, "out3")):
        wp, b = c["w%dp" % layer], c["b%d" % layer]
        _assert_bound(
            f"fwd {geom} N={n}", {name: got[name][:m]},
            {name: co.trunk_layer(layer, x, wp, b)},
            {name: co.trunk_layer(layer, x, wp, b, absolute=True)})
        x = got[name][:m]  # the kernel's own stash feeds the next reference


# ---- mask_d3, dgrad ----


@pytest.mark.parametrize("geom,n", co.MASK_CASES)
def test_mask_d3_exact(geom, n):
    _exact_case("mask", geom, n)


@pytest.mark.parametrize("geom,n", co.RANDOM_MASK_CASES)
def test_mask_d3_random_is_bitwise(geom, n):
    ops = co.rand_ops("mask", geom, n)
    got = _run("mask", ops)["d3m"].cpu()
    want = co.conv_trunk_mask_d3(ops["d_out"], ops["out3"], geom).to(
        torch.bfloat16)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (
        co.exact_mismatch(got, want.double()))


@pytest.mark.parametrize("geom,n", co.DGRAD3_CASES)
def test_dgrad3_exact(geom, n):
    _exact_case("dgrad3", geom, n)


@pytest.mark.parametrize("geom,n", co.DGRAD2_CASES)
def test_dgrad2_exact(geom, n):
    _exact_case("dgrad2", geom, n)


@pytest.mark.parametrize("entry,geom,n", [
    (e, g, n) for e, cases in (("dgrad3", co.RANDOM_DGRAD3_CASES),
                               ("dgrad2", co.RANDOM_DGRAD2_CASES))
    for g, n in cases])
def test_dgrad_random(entry, geom, n):
    _random_case(entry, geom, n)


# ---- wgrad ----


@pytest.mark.parametrize("layer,geom,n", [
    (layer, g, n) for layer, cases in co.WGRAD_CASES.items()
    for g, n in cases])
def test_wgrad_exact(layer, geom, n):
    entry = "wgrad%d" % layer
    ops = co.int_ops(entry, geom, n)
    got = _run(entry, ops)
    dwp, db = co.int_wgrad(geom, layer, n)
    _assert_exact(got, dict(dW=dwp, db=db))
    ci = co.GEOM[geom]["frame"][0] if layer == 1 else co.CO[layer - 1]
    assert not bool(got["dW"][..., co.KS[layer] * ci:].any())


@pytest.mark.parametrize("layer,geom,n", [
    (layer, g, n) for layer, cases in co.RANDOM_WGRAD_CASES.items()
    for g, n in cases])
def test_wgrad_random(layer, geom, n):
    _random_case("wgrad%d" % layer, geom, n)


# ---- ResNet 3x3 ----


@pytest.mark.parametrize("geom,n", co.RESNET_FWD_CASES)
def test_resnet_fwd_exact(geom, n):
    _exact_case("rn_fwd", geom, n)


@pytest.mark.parametrize("geom,n", co.RESNET_DGRAD_CASES)
def test_resnet_dgrad_exact(geom, n):
    _exact_case("rn_dgrad", geom, n)


@pytest.mark.parametrize("geom,n", co.RESNET_WGRAD_CASES)
def test_resnet_wgrad_exact(geom, n):
    ops = co.int_ops("rn_wgrad", geom, n)
    got = _run("rn_wgrad", ops)
    _assert_exact(got, co.entry_refs("rn_wgrad", ops))
    assert not bool(got["dW"][..., 3 * geom[0]:].any())


@pytest.mark.parametrize("geom,n", co.RANDOM_RESNET_CASES)
def test_resnet_random(geom, n):
    for entry in ("rn_fwd", "rn_dgrad", "rn_wgrad"):
        if entry == "rn_dgrad" and geom[0] == 8:
            continue  # the first conv has no dgrad: frames carry no grad
        _random_case(entry, geom, n)


# ---- end to end through the autograd Functions ----


@pytest.mark.parametrize("geom,n", [("84", 6), ("fr", 2)])
def test_trunk_end_to_end_exact(geom, n):
    ch = co.int_chain(geom)
    params = [ch[k].cuda().requires_grad_()
              for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    out = tbf._AtariTrunkMfma.apply(ch["frames"][:n].cuda(), *params)
    _assert_exact(dict(out3=out), dict(out3=ch["out3"][:n]))
    out.backward(ch["d_out"][:n].cuda())
    names = ("dw1", "db1", "dw2", "db2", "dw3", "db3")
    _assert_exact({k: p.grad for k, p in zip(names, params)},
                  dict(zip(names, co.int_autograd(geom, n))))


def test_resnet_conv3x3_end_to_end_exact():
    geom, n = (16, 42, 32), 3
    c = co.resnet_int_case(geom)
    x = _cl(c["x"][:n]).detach().requires_grad_()
    w = c["w"].cuda().requires_grad_()
    b = c["b"].cuda().requires_grad_()
    out = tbf._ResNetConv3x3.apply(x, w, b)
    _assert_exact(dict(y=out.permute(0, 2, 3, 1)),
                  dict(y=co.resnet_int_ref(geom, "fwd", n)))
    out.backward(_cl(c["dy"][:n]))
    dx, dw, db = co.resnet_int_autograd(geom, n)
    _assert_exact(dict(dx=x.grad, dw=w.grad, db=b.grad),
                  dict(dx=dx, dw=dw, db=db))


def test_resnet_first_conv_end_to_end_exact():
    geom, n, ci = (8, 84, 16), 3, 4
    c = co.resnet_int_case(geom)
    x8 = c["x"][:n].clone()
    x8[..., ci:] = 0.0  # as resnet_first_conv pads the observation channels
    w = c["w"][:, :ci].contiguous().cuda().requires_grad_()
    b = c["b"].cuda().requires_grad_()
    out = tbf._ResNetFirstConv.apply(_cl(x8), w, b)
    _assert_exact(dict(y=out.permute(0, 2, 3, 1)),
                  dict(y=co.resnet_conv(x8, c["wp"], c["b"], True)))
    out.backward(_cl(c["dy"][:n]))
    _, dw, db = co.resnet_int_autograd(geom, n, first_ci=ci)
    _assert_exact(dict(dw=w.grad, db=b.grad), dict(dw=dw, db=db))
