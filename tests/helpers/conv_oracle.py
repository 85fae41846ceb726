"""Float64 references for the MFMA conv kernels (ops/hip/conv_mfma.hip).

One reference per extension entry point, on the operands that entry point
takes and in the layout it returns: NHWC activations, packed weights, the
packed [KH][CO][KWCP] weight gradient. They are F.conv2d, conv2d_input and
conv2d_weight in float64 on the CPU. Every reference has a companion, reached
through sum_abs(), that runs the same sum on absolute values and returns
S = sum|terms| + |bias| per output element: what a float32 accumulation's
rounding error scales with.

Two kinds of cases are generated, all seeded:

* Integer cases. Frames in {0, 255} (255 * (1.0f / 255.0f) is 1.0f exactly),
  weights in {-1, 0, 1}, small integer biases and output gradients. Every
  product and partial sum is then an integer below 2^24, exact in float32 in
  any summation order, and every bf16 output is exact while |v| <= 256, so a
  kernel is held to the reference with torch.equal. One output channel in
  four is dead (zero weights, bias -1), as ReLU networks have them: it keeps
  the share of nonzero elements of every compared tensor below 80 %.
  tests/test_conv_oracle.py asserts the range and coverage conditions on the
  references alone.
* Random-valued cases, operands rounded to bf16 on the host, held to
      fp32 outputs  |got - ref| <= K * 2^-24 * S
      bf16 outputs  |got - ref| <= 2^-8 * |ref| + K * 2^-24 * S
  which see what exact cases cannot: a truncating bf16 conversion or a
  reduced-precision accumulate.
"""

import functools

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

EPS32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8

# frame shape and the spatial sizes after conv1, conv2, conv3.
GEOM = {
    "84": dict(frame=(4, 84, 84), hw=((20, 20), (9, 9), (7, 7))),
    "fr": dict(frame=(3, 210, 160), hw=((51, 39), (24, 18), (22, 16))),
}
KS = {1: 8, 2: 4, 3: 3}       # kernel size per trunk layer
STRIDE = {1: 4, 2: 2, 3: 1}
CO = {1: 32, 2: 64, 3: 64}
NMAX = {"84": 128, "fr": 5}   # samples in the shared integer chain

RESNET_GEOMS = ((8, 84, 16), (16, 42, 16), (16, 42, 32), (32, 21, 32),
                (32, 11, 32))
RESNET_NMAX = {84: 3, 42: 3, 21: 5, 11: 9}

# ---- the cases of tests/test_conv_mfma_exact_gpu.py ----
FWD_CASES = (("84", 1), ("84", 2), ("84", 1023), ("84", 1024), ("84", 1025),
             ("84", 1026), ("fr", 1), ("fr", 3))
ROTATE = 7  # batches of N >= 1023 repeat 7 samples; coprime to SB = 3 and 6
MASK_CASES = (("84", 1), ("84", 168), ("fr", 1), ("fr", 24))
DGRAD3_CASES = (("84", 1), ("84", 6), ("84", 7), ("84", 8), ("fr", 1),
                ("fr", 2))
DGRAD2_CASES = (("84", 1), ("84", 3), ("fr", 1), ("fr", 2))
WGRAD_CASES = {
    1: (("84", 1), ("84", 4), ("84", 6), ("84", 128), ("fr", 1), ("fr", 2)),
    2: (("84", 1), ("84", 26), ("fr", 1), ("fr", 5)),
    3: (("84", 1), ("84", 21), ("84", 22), ("fr", 1), ("fr", 3)),
}
RESNET_FWD_CASES = tuple((g, n) for g in RESNET_GEOMS for n in (1, 3))
RESNET_DGRAD_CASES = tuple((g, n) for g in RESNET_GEOMS[1:] for n in (1, 3))
RESNET_WGRAD_CASES = (((8, 84, 16), 1), ((16, 42, 16), 1), ((16, 42, 16), 2),
                      ((16, 42, 32), 1), ((16, 42, 32), 2), ((32, 21, 32), 1),
                      ((32, 21, 32), 5), ((32, 11, 32), 1), ((32, 11, 32), 9))
# One random-valued case per entry point: the smallest N with a second block
# or chunk. The forward also runs on the multi-sample path with both tails.
RANDOM_FWD_CASES = (("84", 3), ("84", 1025), ("fr", 3))
RANDOM_MASK_CASES = (("84", 168), ("fr", 24))
RANDOM_DGRAD3_CASES = (("84", 6), ("fr", 2))
RANDOM_DGRAD2_CASES = (("84", 3), ("fr", 2))
RANDOM_WGRAD_CASES = {1: (("84", 6), ("fr", 2)), 2: (("84", 26), ("fr", 5)),
                      3: (("84", 21), ("fr", 3))}
RANDOM_RESNET_CASES = (((8, 84, 16), 1), ((16, 42, 16), 2), ((16, 42, 32), 2),
                       ((32, 21, 32), 5), ((32, 11, 32), 9))


# ---------------------------------------------------------------------------
# Layouts.
# ---------------------------------------------------------------------------


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def kwcp(kw, ci):
    return (kw * ci + 15) // 16 * 16


def pack_w1(w):
    """[CO,CI,8,8] -> [CO, CI*64], the native (c,ky,kx) flatten."""
    return w.reshape(w.shape[0], -1).contiguous()


def pack_w(w, pad32=False):
    """[CO,CI,KH,KW] -> [CO, KH*KW*CI], (ky,kx,c)-major; pad32 zero-pads K
    to a multiple of 32 as the ResNet entry points want it."""
    flat = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return _pad_cols(flat, 32) if pad32 else flat.contiguous()


def pack_rot(w, pad32=False):
    """The dgrad operand [CI, KH*KW*CO] with spatially flipped taps."""
    flat = w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1)
    return _pad_cols(flat, 32) if pad32 else flat.contiguous()


def _pad_cols(flat, mult):
    k = flat.shape[1]
    kp = (k + mult - 1) // mult * mult
    if kp != k:
        flat = torch.cat([flat, flat.new_zeros(flat.shape[0], kp - k)], 1)
    return flat.contiguous()


def unpack_w1(w1p):
    return w1p.double().reshape(w1p.shape[0], -1, 8, 8)


def unpack_w(wp, ks, ci):
    co = wp.shape[0]
    return (wp[:, :ks * ks * ci].double().reshape(co, ks, ks, ci)
            .permute(0, 3, 1, 2))


def unpack_rot(wr, ks, co):
    ci = wr.shape[0]
    return (wr[:, :ks * ks * co].double().reshape(ci, ks, ks, co)
            .permute(3, 0, 1, 2).flip(2, 3))


def pack_dw(dw, c_major):
    """[CO,CI,KH,KW] -> [KH][CO][KWCP]: (c,kx)-minor for conv1, (kx,c)-minor
    otherwise, columns [KW*CI, KWCP) zero."""
    co, ci, kh, kw = dw.shape
    if c_major:
        p = dw.permute(2, 0, 1, 3).reshape(kh, co, ci * kw)
    else:
        p = dw.permute(2, 0, 3, 1).reshape(kh, co, kw * ci)
    return _pad_cols(p.reshape(kh * co, -1), 16).reshape(kh, co, -1)


def unpack_dw(dwp, ci, c_major):
    kh, co, _ = dwp.shape
    kw = kh
    p = dwp[..., :kw * ci]
    if c_major:
        return p.reshape(kh, co, ci, kw).permute(1, 2, 0, 3).contiguous()
    return p.reshape(kh, co, kw, ci).permute(1, 3, 0, 2).contiguous()


def frames_operand(frames):
    """What the kernels stage from a u8 frame: bf16(u8 * (1.0f / 255.0f))."""
    inv = torch.tensor(1.0, dtype=torch.float32) / 255.0
    return (frames.float() * inv).to(torch.bfloat16).double()


# ---------------------------------------------------------------------------
# References, one per entry point. absolute=True gives S instead.
# ---------------------------------------------------------------------------


def _mag(t, absolute):
    return t.abs() if absolute else t


def trunk_layer(layer, x, wp, b, absolute=False):
    """One forward layer in its kernel's layouts. layer 1: u8 NCHW frames ->
    NHWC a1; 2: NHWC a1 -> NHWC a2; 3: NHWC a2 -> NCHW-flat out3."""
    if layer == 1:
        xin, w = frames_operand(x), unpack_w1(wp)
    else:
        xin, w = nchw(x.double()), unpack_w(wp, KS[layer], x.shape[-1])
    y = F.conv2d(_mag(xin, absolute), _mag(w, absolute),
                 _mag(b.double(), absolute), stride=STRIDE[layer])
    if not absolute:
        y = y.clamp_min(0.0)
    return y.reshape(y.shape[0], -1) if layer == 3 else nhwc(y)


def conv_trunk_fwd(frames, w1p, b1, w2p, b2, w3p, b3, absolute=False):
    """(a1, a2, out3). Activations pass on in float64: the integer cases keep
    them exact in bf16, which tests/test_conv_oracle.py asserts."""
    a1 = trunk_layer(1, frames, w1p, b1, absolute)
    a2 = trunk_layer(2, a1, w2p, b2, absolute)
    return a1, a2, trunk_layer(3, a2, w3p, b3, absolute)


def conv_trunk_mask_d3(d_out3, out3, geom):
    """float32 NHWC where(out3 > 0, d, 0); the kernel rounds it to bf16."""
    oh, ow = GEOM[geom]["hw"][2]
    m = torch.where(out3 > 0, d_out3, torch.zeros_like(d_out3))
    return nhwc(m.reshape(-1, CO[3], oh, ow))


def _dgrad(layer, dy, wr, act, pad, absolute):
    w = unpack_rot(wr, KS[layer], dy.shape[-1])
    shape = (act.shape[0], act.shape[3], act.shape[1], act.shape[2])
    dx = conv2d_input(shape, _mag(w, absolute),
                      _mag(nchw(dy.double()), absolute).contiguous(),
                      stride=STRIDE[layer], padding=pad)
    dx = nhwc(dx)
    return dx if absolute else dx * (act > 0)


def conv_trunk_dgrad3(d3m, w3r, a2, absolute=False):
    return _dgrad(3, d3m, w3r, a2, 0, absolute)


def conv_trunk_dgrad2(d2, w2r, a1, absolute=False):
    return _dgrad(2, d2, w2r, a1, 0, absolute)


def _wgrad(x, dy, ks, stride, pad, c_major, absolute):
    dyn = _mag(nchw(dy.double()), absolute).contiguous()
    shape = (dy.shape[-1], x.shape[1], ks, ks)
    dw = conv2d_weight(_mag(x, absolute).contiguous(), shape, dyn,
                       stride=stride, padding=pad)
    return pack_dw(dw, c_major), dyn.sum((0, 2, 3))


def conv_trunk_wgrad1(frames, d1, absolute=False):
    return _wgrad(frames_operand(frames), d1, 8, 4, 0, True, absolute)


def conv_trunk_wgrad2(a1, d2, absolute=False):
    return _wgrad(nchw(a1.double()), d2, 4, 2, 0, False, absolute)


def conv_trunk_wgrad3(a2, d3m, absolute=False):
    return _wgrad(nchw(a2.double()), d3m, 3, 1, 0, False, absolute)


WGRAD = {1: conv_trunk_wgrad1, 2: conv_trunk_wgrad2, 3: conv_trunk_wgrad3}


def resnet_conv(x, w, bias, fwd, absolute=False):
    """x NHWC. fwd: w = pack_w(weight, pad32) and a bias, no ReLU; dgrad:
    x is dy, w = pack_rot(weight, pad32), bias is None."""
    if fwd:
        y = F.conv2d(_mag(nchw(x.double()), absolute),
                     _mag(unpack_w(w, 3, x.shape[-1]), absolute),
                     _mag(bias.double(), absolute), padding=1)
        return nhwc(y)
    wt = unpack_rot(w, 3, x.shape[-1])
    shape = (x.shape[0], w.shape[0], x.shape[1], x.shape[2])
    return nhwc(conv2d_input(shape, _mag(wt, absolute),
                             _mag(nchw(x.double()), absolute).contiguous(),
                             padding=1))


def resnet_conv_wgrad(x, dy, absolute=False):
    return _wgrad(nchw(x.double()), dy, 3, 1, 1, False, absolute)


def sum_abs(fn, *args):
    """S = sum|terms| + |bias| per output element of reference `fn`."""
    return fn(*args, absolute=True)


# ---------------------------------------------------------------------------
# The two comparison rules.
# ---------------------------------------------------------------------------


def exact_mismatch(got, ref):
    """None if `got` equals `ref` exactly, else a message naming the first
    differing element."""
    got = got.detach().cpu().double()
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if torch.equal(got, ref.double()):
        return None
    bad = (got != ref).nonzero()
    i = tuple(int(v) for v in bad[0])
    return (f"{bad.shape[0]} of {ref.numel()} elements differ, first at {i}:"
            f" got {float(got[i])!r}, want {float(ref[i])!r}")


def bound_excess(got, ref, s, k, bf16_out):
    """(message or None, ratio). ratio is the largest |got - ref|, less the
    bf16 half ulp of a bf16 output, in units of 2^-24 * S."""
    got = got.detach().cpu().double()
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref.shape)}", float("inf")
    err = (got - ref).abs()
    if bf16_out:
        err = (err - HALF_ULP_BF16 * ref.abs()).clamp_min(0.0)
    unit = EPS32 * s
    ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    worst = float(ratio.max())
    if worst <= k:
        return None, worst
    i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    return (f"{int((ratio > k).sum())} elements over the bound, worst at {i}:"
            f" got {float(got[i])!r}, want {float(ref[i])!r}, S"
            f" {float(s[i]):.4g}, ratio {worst:.3g} > K = {k:.3g}"), worst


# ---------------------------------------------------------------------------
# Integer cases: one chain per geometry, sliced per case.
# ---------------------------------------------------------------------------

DEAD = 4  # output channel c is dead when c % DEAD == 0


def _gen(*key):
    return torch.Generator().manual_seed(
        sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(map(str, key)))))


def _ternary(g, shape, p):
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (sign * (torch.rand(shape, generator=g) < p)).float()


def _int_weights(g, co, ci, ks, p, bias_lo, bias_hi):
    w = _ternary(g, (co, ci, ks, ks), p)
    b = torch.randint(bias_lo, bias_hi + 1, (co,), generator=g).float()
    w[::DEAD] = 0.0
    b[::DEAD] = -1.0
    return w, b


@functools.lru_cache(maxsize=None)
def int_chain(geom):
    """Operands and float64 references of every trunk kernel for NMAX[geom]
    samples, each kernel's operands being the references of the kernels
    before it. Shared between tests; never modified."""
    c, h, w = GEOM[geom]["frame"]
    n = NMAX[geom]
    g = _gen("trunk", geom)
    ch = dict(geom=geom)
    ch["frames"] = (torch.randint(0, 2, (n, c, h, w), generator=g) * 255).to(
        torch.uint8)
    ch["w1"], ch["b1"] = _int_weights(g, 32, c, 8, 0.5, -1, 3)
    ch["w2"], ch["b2"] = _int_weights(g, 64, 32, 4, 0.125, -1, 3)
    ch["w3"], ch["b3"] = _int_weights(g, 64, 64, 3, 0.125, -1, 3)
    bf = torch.bfloat16
    ch["w1p"] = pack_w1(ch["w1"]).to(bf)
    ch["w2p"], ch["w3p"] = pack_w(ch["w2"]).to(bf), pack_w(ch["w3"]).to(bf)
    ch["w2r"], ch["w3r"] = pack_rot(ch["w2"]).to(bf), pack_rot(ch["w3"]).to(bf)
    ch["a1"], ch["a2"], ch["out3"] = conv_trunk_fwd(
        ch["frames"], ch["w1p"], ch["b1"], ch["w2p"], ch["b2"], ch["w3p"],
        ch["b3"])
    ch["d_out"] = _ternary(g, tuple(ch["out3"].shape), 0.75)
    ch["d3m"] = conv_trunk_mask_d3(ch["d_out"], ch["out3"].float(),
                                   geom).double()
    ch["d2"] = conv_trunk_dgrad3(ch["d3m"], ch["w3r"], ch["a2"])
    ch["d1"] = conv_trunk_dgrad2(ch["d2"], ch["w2r"], ch["a1"])
    return ch


WGRAD_OPERANDS = {1: ("frames", "d1"), 2: ("a1", "d2"), 3: ("a2", "d3m")}


@functools.lru_cache(maxsize=None)
def int_wgrad(geom, layer, n, absolute=False):
    """(dWp, db) of the first n samples of the chain."""
    ch = int_chain(geom)
    x, dy = WGRAD_OPERANDS[layer]
    return WGRAD[layer](ch[x][:n], ch[dy][:n], absolute=absolute)


def rotated(t, n):
    """Sample i of the batch is sample i % ROTATE of `t`."""
    return t[torch.arange(n) % ROTATE]


@functools.lru_cache(maxsize=None)
def int_mask_case(geom, n):
    """Direct operands for conv_trunk_mask_d3: integer out3 with exact
    zeros, integer d_out3."""
    oh, ow = GEOM[geom]["hw"][2]
    g = _gen("mask", geom, n)
    shape = (n, CO[3] * oh * ow)
    out3 = torch.randint(-3, 4, shape, generator=g).clamp_min(0).float()
    d = torch.randint(-2, 3, shape, generator=g).float()
    return out3, d


@functools.lru_cache(maxsize=None)
def int_autograd(geom, n):
    """dw1, db1, dw2, db2, dw3, db3 of the integer network by plain float64
    autograd, in nn.Conv2d's own [co,ci,kh,kw] layout."""
    ch = int_chain(geom)
    ps = [ch[k].double().requires_grad_() for k in
          ("w1", "b1", "w2", "b2", "w3", "b3")]
    x = ch["frames"][:n].double() / 255.0
    for layer in (1, 2, 3):
        x = F.relu(F.conv2d(x, ps[2 * layer - 2], ps[2 * layer - 1],
                            stride=STRIDE[layer]))
    x.reshape(n, -1).backward(ch["d_out"][:n].double())
    return [p.grad for p in ps]


@functools.lru_cache(maxsize=None)
def resnet_int_case(geom):
    """Integer operands of one ResNet geometry for RESNET_NMAX samples: x
    NHWC with nonzero corners, weights with dead output and input channels,
    dy with dead channels; and the references of all three kernels' inputs."""
    ci, hw, co = geom
    n = RESNET_NMAX[hw]
    g = _gen("resnet", *geom)

    def ints(shape):
        return (torch.randint(1, 3, shape, generator=g).float()
                * _ternary(g, shape, 0.5))

    x = ints((n, hw, hw, ci))
    for yy in (0, hw - 1):
        for xx in (0, hw - 1):
            x[:, yy, xx, :] = 1.0 + ((yy + xx) > 0)
    w = _ternary(g, (co, ci, 3, 3), 0.25)
    w[::DEAD] = 0.0
    w[:, ::DEAD] = 0.0
    b = torch.randint(-2, 3, (co,), generator=g).float()
    b[::DEAD] = 0.0
    dy = ints((n, hw, hw, co))
    dy[..., ::DEAD] = 0.0
    bf = torch.bfloat16
    return dict(x=x, w=w, b=b, dy=dy, wp=pack_w(w, True).to(bf),
                wr=pack_rot(w, True).to(bf))


@functools.lru_cache(maxsize=None)
def resnet_int_ref(geom, kind, n, absolute=False):
    c = resnet_int_case(geom)
    if kind == "fwd":
        return resnet_conv(c["x"][:n], c["wp"], c["b"], True, absolute)
    if kind == "dgrad":
        return resnet_conv(c["dy"][:n], c["wr"], None, False, absolute)
    return resnet_conv_wgrad(c["x"][:n], c["dy"][:n], absolute)


@functools.lru_cache(maxsize=None)
def resnet_int_autograd(geom, n, first_ci=None):
    """(dx, dw, db) by float64 autograd; first_ci keeps only the first
    channels of x and w, as the first conv pads them back to 8 with zeros."""
    c = resnet_int_case(geom)
    x = nchw(c["x"][:n]).double()
    w = c["w"].double()
    if first_ci is not None:
        x, w = x[:, :first_ci], w[:, :first_ci]
    x = x.contiguous().requires_grad_()
    w = w.contiguous().requires_grad_()
    b = c["b"].double().requires_grad_()
    F.conv2d(x, w, b, padding=1).backward(nchw(c["dy"][:n]).double())
    return x.grad, w.grad, b.grad


# ---------------------------------------------------------------------------
# Random-valued cases: operands rounded to bf16 on the host.
# ---------------------------------------------------------------------------


def _bf(t):
    return t.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def rand_trunk_case(geom, n):
    """Direct random operands for every trunk entry point at n samples (the
    forward of n >= 1023 rotates the first ROTATE of them)."""
    c, h, w = GEOM[geom]["frame"]
    (h1, w1), (h2, w2), (h3, w3) = GEOM[geom]["hw"]
    g = _gen("rand", geom, n)
    m = n if n < 1023 else ROTATE

    def rn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    ws = [rn(32, c, 8, 8, scale=(c * 64) ** -0.5),
          rn(64, 32, 4, 4, scale=512 ** -0.5),
          rn(64, 64, 3, 3, scale=576 ** -0.5)]
    ws = [_bf(t).float() for t in ws]
    case = dict(
        geom=geom,
        frames=torch.randint(0, 256, (m, c, h, w), generator=g,
                             dtype=torch.uint8),
        b1=rn(32, scale=0.1), b2=rn(64, scale=0.1), b3=rn(64, scale=0.1),
        w1p=_bf(pack_w1(ws[0])), w2p=_bf(pack_w(ws[1])),
        w3p=_bf(pack_w(ws[2])), w2r=_bf(pack_rot(ws[1])),
        w3r=_bf(pack_rot(ws[2])),
        a1=_bf(rn(m, h1, w1, 32).clamp_min(0.0)),
        a2=_bf(rn(m, h2, w2, 64).clamp_min(0.0)),
        d1=_bf(rn(m, h1, w1, 32)), d2=_bf(rn(m, h2, w2, 64)),
        d3m=_bf(rn(m, h3, w3, 64)),
    )
    return case


@functools.lru_cache(maxsize=None)
def rand_mask_case(geom, n):
    oh, ow = GEOM[geom]["hw"][2]
    g = _gen("randmask", geom, n)
    shape = (n, CO[3] * oh * ow)
    return (torch.randn(shape, generator=g).clamp_min(0.0),
            torch.randn(shape, generator=g))


@functools.lru_cache(maxsize=None)
def rand_resnet_case(geom, n):
    ci, hw, co = geom
    g = _gen("randresnet", *geom, n)
    w = _bf(torch.randn(co, ci, 3, 3, generator=g) * (9 * ci) ** -0.5).float()
    return dict(x=_bf(torch.randn(n, hw, hw, ci, generator=g) * 0.5),
                dy=_bf(torch.randn(n, hw, hw, co, generator=g)),
                b=torch.randn(co, generator=g) * 0.1,
                wp=_bf(pack_w(w, True)), wr=_bf(pack_rot(w, True)))


def _ratio32(fn32, ref, s):
    return float(((fn32.double() - ref).abs()
                  / (EPS32 * s).clamp_min(1e-300)).max())


def cpu_float32_ratio():
    """r: the largest |f32 - f64| / (2^-24 * S) of float32 F.conv2d,
    conv2d_input and conv2d_weight on the CPU over the random-valued cases
    (the forward on the float64 chain's own bf16-rounded activations)."""
    worst = {}

    def note(kind, got32, ref, s):
        worst[kind] = max(worst.get(kind, 0.0), _ratio32(got32, ref, s))

    for geom, n in RANDOM_FWD_CASES:
        c = rand_trunk_case(geom, n)
        x = c["frames"]
        for layer, wp, b in ((1, "w1p", "b1"), (2, "w2p", "b2"),
                             (3, "w3p", "b3")):
            ref = trunk_layer(layer, x, c[wp], c[b])
            s = trunk_layer(layer, x, c[wp], c[b], absolute=True)
            if layer == 1:
                xin, w = frames_operand(x).float(), unpack_w1(c[wp]).float()
            else:
                xin = nchw(x.float())
                w = unpack_w(c[wp], KS[layer], x.shape[-1]).float()
            y = F.conv2d(xin, w, c[b], stride=STRIDE[layer]).clamp_min(0.0)
            y = y.reshape(y.shape[0], -1) if layer == 3 else nhwc(y)
            note("fwd", y, ref, s)
            x = _bf(ref) if layer < 3 else None
    for cases, layer, dy, wr, act in ((RANDOM_DGRAD3_CASES, 3, "d3m", "w3r",
                                       "a2"),
                                      (RANDOM_DGRAD2_CASES, 2, "d2", "w2r",
                                       "a1")):
        for geom, n in cases:
            c = rand_trunk_case(geom, n)
            ref = _dgrad(layer, c[dy], c[wr], c[act], 0, False)
            s = _dgrad(layer, c[dy], c[wr], c[act], 0, True)
            w = unpack_rot(c[wr], KS[layer], c[dy].shape[-1]).float()
            a = c[act]
            dx = conv2d_input((a.shape[0], a.shape[3], a.shape[1], a.shape[2]),
                              w, nchw(c[dy].float()).contiguous(),
                              stride=STRIDE[layer])
            note("dgrad", nhwc(dx) * (a > 0), ref, s)
    for layer, cases in RANDOM_WGRAD_CASES.items():
        for geom, n in cases:
            c = rand_trunk_case(geom, n)
            xk, dk = WGRAD_OPERANDS[layer]
            ref, rdb = WGRAD[layer](c[xk], c[dk])
            s, sdb = WGRAD[layer](c[xk], c[dk], absolute=True)
            x = (frames_operand(c[xk]) if layer == 1
                 else nchw(c[xk].double())).float().contiguous()
            dyn = nchw(c[dk].float()).contiguous()
            ks = KS[layer]
            dw = conv2d_weight(x, (dyn.shape[1], x.shape[1], ks, ks), dyn,
                               stride=STRIDE[layer])
            note("wgrad", pack_dw(dw, layer == 1), ref, s)
            note("db", dyn.sum((0, 2, 3)), rdb, sdb)
    for geom, n in RANDOM_RESNET_CASES:
        c = rand_resnet_case(geom, n)
        ci, hw, co = geom
        x, dyn = nchw(c["x"].float()).contiguous(), nchw(
            c["dy"].float()).contiguous()
        w = unpack_w(c["wp"], 3, ci).float()
        note("fwd", nhwc(F.conv2d(x, w, c["b"], padding=1)),
             resnet_conv(c["x"], c["wp"], c["b"], True),
             resnet_conv(c["x"], c["wp"], c["b"], True, absolute=True))
        if ci != 8:
            note("dgrad", nhwc(conv2d_input(x.shape, w, dyn, padding=1)),
                 resnet_conv(c["dy"], c["wr"], None, False),
                 resnet_conv(c["dy"], c["wr"], None, False, absolute=True))
        ref, rdb = resnet_conv_wgrad(c["x"], c["dy"])
        s, sdb = resnet_conv_wgrad(c["x"], c["dy"], absolute=True)
        note("wgrad", pack_dw(conv2d_weight(x, w.shape, dyn, padding=1),
                              False), ref, s)
        note("db", dyn.sum((0, 2, 3)), rdb, sdb)
    return worst


CPU_RATIO = 2.57  # r, measured by cpu_float32_ratio(): the dgrads are largest
K = 4 * CPU_RATIO

# ---------------------------------------------------------------------------
# Entry points by name: operands in, {output name: reference} out. The GPU
# module runs the same operands through the extension; the mutation checks of
# tests/test_conv_oracle.py run damaged operands through the references.
# ---------------------------------------------------------------------------

BF16_OUT = frozenset(("a1", "a2", "y1", "y2", "d3m", "d2", "d1", "y", "dx"))


def entry_refs(entry, ops, absolute=False):
    a = dict(absolute=absolute)
    if entry == "fwd":
        a1, a2, out3 = conv_trunk_fwd(
            ops["frames"], ops["w1p"], ops["b1"], ops["w2p"], ops["b2"],
            ops["w3p"], ops["b3"], **a)
        return dict(a1=a1, a2=a2, out3=out3)
    if entry in ("conv1", "conv2", "conv3"):
        layer = int(entry[-1])
        name = "out3" if layer == 3 else "y%d" % layer
        return {name: trunk_layer(layer, ops["x"], ops["wp"], ops["b"], **a)}
    if entry == "mask":
        m = conv_trunk_mask_d3(ops["d_out"], ops["out3"], ops["geom"])
        if absolute:  # a selection and one rounding: nothing accumulates
            return dict(d3m=torch.zeros_like(m, dtype=torch.float64))
        return dict(d3m=m.to(torch.bfloat16).double())
    if entry == "dgrad3":
        return dict(d2=conv_trunk_dgrad3(ops["dy"], ops["wr"], ops["act"],
                                         **a))
    if entry == "dgrad2":
        return dict(d1=conv_trunk_dgrad2(ops["dy"], ops["wr"], ops["act"],
                                         **a))
    if entry in ("wgrad1", "wgrad2", "wgrad3"):
        dw, db = WGRAD[int(entry[-1])](ops["x"], ops["dy"], **a)
        return dict(dW=dw, db=db)
    if entry == "rn_fwd":
        return dict(y=resnet_conv(ops["x"], ops["wp"], ops["b"], True, **a))
    if entry == "rn_dgrad":
        return dict(dx=resnet_conv(ops["dy"], ops["wr"], None, False, **a))
    if entry == "rn_wgrad":
        dw, db = resnet_conv_wgrad(ops["x"], ops["dy"], **a)
        return dict(dW=dw, db=db)
    raise KeyError(entry)


def _trunk_ops(entry, c, n):
    """Operands of one trunk entry point from a chain or random case `c`."""
    if entry == "fwd":
        ops = {k: c[k] for k in ("w1p", "b1", "w2p", "b2", "w3p", "b3")}
        ops["frames"] = c["frames"][:n]
        return ops
    if entry in ("conv1", "conv2", "conv3"):
        layer = int(entry[-1])
        x = ("frames", "a1", "a2")[layer - 1]
        return dict(x=c[x][:n], wp=c["w%dp" % layer], b=c["b%d" % layer])
    if entry == "dgrad3":
        return dict(dy=c["d3m"][:n], wr=c["w3r"], act=c["a2"][:n])
    if entry == "dgrad2":
        return dict(dy=c["d2"][:n], wr=c["w2r"], act=c["a1"][:n])
    x, dy = WGRAD_OPERANDS[int(entry[-1])]
    return dict(x=c[x][:n], dy=c[dy][:n])


def int_ops(entry, geom, n):
    if entry == "mask":
        out3, d = int_mask_case(geom, n)
        return dict(out3=out3, d_out=d, geom=geom)
    if entry.startswith("rn_"):
        c = resnet_int_case(geom)
        return dict(x=c["x"][:n], dy=c["dy"][:n], wp=c["wp"], wr=c["wr"],
                    b=c["b"])
    return _trunk_ops(entry, int_chain(geom), n)


def rand_ops(entry, geom, n):
    if entry == "mask":
        out3, d = rand_mask_case(geom, n)
        return dict(out3=out3, d_out=d, geom=geom)
    if entry.startswith("rn_"):
        return dict(rand_resnet_case(geom, n))
    return _trunk_ops(entry, rand_trunk_case(geom, n), n)


def int_fwd_refs(geom, n):
    """(frames, {a1, a2, out3}) of one integer forward case; batches of
    n >= 1023 rotate the chain's first ROTATE samples."""
    m = n if n < 1023 else ROTATE
    ops = int_ops("fwd", geom, m)
    refs = entry_refs("fwd", ops)
    if m == n:
        return ops["frames"], refs
    return rotated(ops["frames"], n), {k: rotated(v, n)
                                       for k, v in refs.items()}


# ---- damaged operands: what a subtly wrong kernel would compute ----

WEIGHT_KEY = dict(fwd="w2p", conv1="wp", conv2="wp", conv3="wp", dgrad3="wr",
                  dgrad2="wr", rn_fwd="wp", rn_dgrad="wr")
INPUT_KEY = dict(fwd="frames", conv1="x", conv2="x", conv3="x", dgrad3="dy",
                 dgrad2="dy", wgrad1="x", wgrad2="x", wgrad3="x", rn_fwd="x",
                 rn_dgrad="dy", rn_wgrad="x")


def mutate_tap(entry, ops):
    """One tap of one output channel reads as zero."""
    ops = dict(ops)
    w = ops[WEIGHT_KEY[entry]].clone()
    row, col = (int(v) for v in (w != 0).nonzero()[-1])
    w[row, col] = 0
    ops[WEIGHT_KEY[entry]] = w
    return ops


def mutate_m_row(entry, ops):
    """One output position never enters the wgrad sum."""
    ops = dict(ops)
    dy = ops["dy"].clone()
    n, oy, ox, _ = (int(v) for v in (dy != 0).nonzero()[-1])
    dy[n, oy, ox, :] = 0
    ops["dy"] = dy
    return ops


def mutate_neighbour_in(entry, ops):
    """The last sample's input tile is read from the sample before it."""
    ops = dict(ops)
    x = ops[INPUT_KEY[entry]].clone()
    x[-1] = x[-2]
    ops[INPUT_KEY[entry]] = x
    return ops


def mutate_neighbour_out(refs):
    """The last sample's output tile is the tile of the sample before it."""
    out = {}
    for k, v in refs.items():
        v = v.clone()
        v[-1] = v[-2]
        out[k] = v
    return out


def mutate_edge(entry, ops):
    """The last column the kernel stages of the first sample reads as zero."""
    ops = dict(ops)
    key = INPUT_KEY[entry]
    x = ops[key].clone()
    if x.dtype == torch.uint8:        # NCHW frames, all 8x8 s4 windows
        x[0, :, :, (x.shape[3] - 8) // 4 * 4 + 7] = 0
    elif entry in ("conv2", "wgrad2"):  # NHWC a1 under 4x4 s2
        x[0, :, (x.shape[2] - 4) // 2 * 2 + 3, :] = 0
    else:
        x[0, :, -1, :] = 0
    ops[key] = x
    return ops
