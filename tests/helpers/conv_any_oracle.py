"""Cases for the run-time-geometry ResNet convs (resnet_conv_any,
resnet_conv_any_wgrad), keyed on (ci, h, w, co).

The references are the shape-agnostic ones of conv_oracle.py (resnet_conv,
resnet_conv_wgrad); this module only generates operands, following
conv_oracle.resnet_int_case and rand_resnet_case, and mirrors the planner's
wgrad chunk rule (ops/hip/conv_any_plan.h) so the chunk-spanning cases can be
chosen and checked without the extension.
"""

import functools

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import conv_oracle as co

FIRST = ((8, 64, 64, 16), (8, 72, 96, 16))       # forward and wgrad only
TRUNK = ((16, 32, 32, 16), (16, 36, 48, 32), (32, 36, 48, 16),
         (32, 16, 16, 32), (32, 18, 24, 32), (32, 8, 8, 32), (32, 9, 12, 32))
PRIME = ((16, 13, 37, 32),)     # short last band, M tail under one fragment
TINY = ((16, 5, 7, 16), (32, 2, 3, 32), (32, 1, 1, 32))
WIDE = ((8, 3, 250, 16),)       # near the width bound
GEOMS = FIRST + TRUNK + PRIME + TINY + WIDE
NS = (1, 3)
NMAX = 3

# The five square geometries the template kernels are instantiated for.
SQUARE = tuple((ci, hw, hw, c) for ci, hw, c in co.RESNET_GEOMS)

# One wgrad case per channel pair whose N*H*W spans at least two chunks and
# is no multiple of 64 (so the last staging round of the last chunk is cut).
WGRAD_CHUNK_CASES = (((8, 3, 250, 16), 1), ((16, 13, 37, 16), 1),
                     ((16, 13, 37, 32), 1), ((32, 18, 24, 16), 1),
                     ((32, 9, 12, 32), 3))

REFUSED = ((16, 0, 8, 16), (16, 8, 0, 16), (16, 257, 8, 16), (16, 8, 257, 16),
           (4, 8, 8, 16), (16, 8, 8, 24), (8, 8, 8, 32), (8, 8, 8, 8))


def has_dgrad(geom):
    """The first conv has none: frames carry no grad (and 16 -> 8 is no
    channel pair of the network)."""
    return geom[0] != 8


def wgrad_chunk(m):
    """(chunk length, chunk count) the planner gives m = N*H*W positions."""
    mc = -(-m // 256)
    mc = max(-(-mc // 64) * 64, 256)
    return mc, -(-m // mc)


@functools.lru_cache(maxsize=None)
def int_case(geom):
    """Integer operands for NMAX samples: x NHWC with nonzero corners,
    weights with dead output and input channels, dy with dead channels."""
    ci, h, w, c_out = geom
    g = co._gen("resnet", *geom)

    def ints(shape):
        return (torch.randint(1, 3, shape, generator=g).float()
                * co._ternary(g, shape, 0.5))

    x = ints((NMAX, h, w, ci))
    for yy in (0, h - 1):
        for xx in (0, w - 1):
            x[:, yy, xx, :] = 1.0 + ((yy + xx) > 0)
    wt = co._ternary(g, (c_out, ci, 3, 3), 0.25)
    wt[::co.DEAD] = 0.0
    wt[:, ::co.DEAD] = 0.0
    b = torch.randint(-2, 3, (c_out,), generator=g).float()
    b[::co.DEAD] = 0.0
    dy = ints((NMAX, h, w, c_out))
    dy[..., ::co.DEAD] = 0.0
    bf = torch.bfloat16
    return dict(x=x, w=wt, b=b, dy=dy, wp=co.pack_w(wt, True).to(bf),
                wr=co.pack_rot(wt, True).to(bf))


def int_ops(geom, n):
    c = int_case(geom)
    return dict(x=c["x"][:n], dy=c["dy"][:n], wp=c["wp"], wr=c["wr"],
                b=c["b"])


@functools.lru_cache(maxsize=None)
def rand_ops(geom, n):
    ci, h, w, c_out = geom
    g = co._gen("randany", *geom, n)
    wt = co._bf(torch.randn(c_out, ci, 3, 3, generator=g)
                * (9 * ci) ** -0.5).float()
    return dict(x=co._bf(torch.randn(n, h, w, ci, generator=g) * 0.5),
                dy=co._bf(torch.randn(n, h, w, c_out, generator=g)),
                b=torch.randn(c_out, generator=g) * 0.1,
                wp=co._bf(co.pack_w(wt, True)),
                wr=co._bf(co.pack_rot(wt, True)))


ENTRY = dict(fwd="rn_fwd", dgrad="rn_dgrad", wgrad="rn_wgrad")


@functools.lru_cache(maxsize=None)
def refs(geom, kind, n, exact=True, absolute=False):
    """{output name: float64 reference} of one kernel on one case."""
    ops = int_ops(geom, n) if exact else rand_ops(geom, n)
    return co.entry_refs(ENTRY[kind], ops, absolute=absolute)


@functools.lru_cache(maxsize=None)
def int_autograd(geom, n, first_ci=None):
    """(dx, dw, db) by float64 autograd; first_ci keeps only the first
    channels of x and w, as the first conv pads them back to 8 with zeros."""
    c = int_case(geom)
    x = co.nchw(c["x"][:n]).double()
    w = c["w"].double()
    if first_ci is not None:
        x, w = x[:, :first_ci], w[:, :first_ci]
    x = x.contiguous().requires_grad_()
    w = w.contiguous().requires_grad_()
    b = c["b"].double().requires_grad_()
    F.conv2d(x, w, b, padding=1).backward(co.nchw(c["dy"][:n]).double())
    return x.grad, w.grad, b.grad


def cpu_float32_ratio(n=NMAX):
    """The largest |f32 - f64| / (2^-24 * S) of float32 F.conv2d,
    conv2d_input and conv2d_weight on the CPU over the random-valued cases of
    GEOMS, as conv_oracle.cpu_float32_ratio() measures it."""
    worst = {}

    def note(kind, got32, ref, s):
        worst[kind] = max(worst.get(kind, 0.0), co._ratio32(got32, ref, s))

    for geom in GEOMS:
        c = rand_ops(geom, n)
        ci = geom[0]
        x = co.nchw(c["x"].float()).contiguous()
        dyn = co.nchw(c["dy"].float()).contiguous()
        w = co.unpack_w(c["wp"], 3, ci).float()
        note("fwd", co.nhwc(F.conv2d(x, w, c["b"], padding=1)),
             refs(geom, "fwd", n, False)["y"],
             refs(geom, "fwd", n, False, True)["y"])
        if has_dgrad(geom):
            note("dgrad", co.nhwc(conv2d_input(x.shape, w, dyn, padding=1)),
                 refs(geom, "dgrad", n, False)["dx"],
                 refs(geom, "dgrad", n, False, True)["dx"])
        r, s = refs(geom, "wgrad", n, False), refs(geom, "wgrad", n, False,
                                                   True)
        note("wgrad", co.pack_dw(conv2d_weight(x, w.shape, dyn, padding=1),
                                 False), r["dW"], s["dW"])
        note("db", dyn.sum((0, 2, 3)), r["db"], s["db"])
    return worst
