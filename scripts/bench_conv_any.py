"""Micro-benchmark: run-time-geometry ResNet convs (resnet_conv_any*) against
the template instantiations and against bf16 channels_last library convs.

Run on a GPU box:  python scripts/bench_conv_any.py [templates|library] [N...]
Method of scripts/bench_conv_mfma.py: a host clock around 30 calls that end
in a device synchronise, after 5 warm-up calls. Each pair is measured three
times, alternating, so the run-to-run spread stands next to the difference.
"""

import os
import sys
import timeit

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import torchbeast_amd.ops as ops_mod
from torchbeast_amd.ops import functional as tbf

SQUARE = ((8, 84, 84, 16), (16, 42, 42, 16), (16, 42, 42, 32),
          (32, 21, 21, 32), (32, 11, 11, 32))
# Every conv of the Procgen (64x64) and DMLab (72x96) trunks.
PROCGEN = ((8, 64, 64, 16), (16, 32, 32, 16), (16, 32, 32, 32),
           (32, 16, 16, 32), (32, 8, 8, 32))
DMLAB = ((8, 72, 96, 16), (16, 36, 48, 16), (16, 36, 48, 32),
         (32, 18, 24, 32), (32, 9, 12, 32))


def timed(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = timeit.default_timer()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (timeit.default_timer() - t0) / iters * 1e3


def operands(geom, n):
    ci, h, w, co = geom
    g = torch.Generator(device="cuda").manual_seed(ci * h + w + co + n)
    cl = torch.channels_last
    x = (torch.randn(n, ci, h, w, device="cuda", generator=g) * 0.5).to(
        torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(n, co, h, w, device="cuda", generator=g).to(
        torch.bfloat16).contiguous(memory_format=cl)
    wt = torch.randn(co, ci, 3, 3, device="cuda", generator=g) * (9 * ci) ** -0.5
    b = torch.randn(co, device="cuda", generator=g) * 0.1
    return x, dy, wt, b


def three(a, b):
    """Three alternating measurements of two callables, in ms."""
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(a))
        tb.append(timed(b))
    return ta, tb


def fmt(ts):
    return "/".join(f"{t:.3f}" for t in ts)


def line(label, kind, n, ta, tb, names):
    ratio = sorted(tb)[1] / sorted(ta)[1]
    print(f"{label:18s} {kind:5s} N={n:<5d} {names[0]} {fmt(ta)} ms  "
          f"{names[1]} {fmt(tb)} ms  median ratio {ratio:.2f}", flush=True)


def against_templates(ns):
    ext = ops_mod.require_ext()
    empty = torch.empty(0, device="cuda")
    for geom in SQUARE:
        ci, hw, _, co = geom
        for n in ns:
            x, dy, wt, b = operands(geom, n)
            wp = tbf._pack_resnet_weight(wt)
            wr = tbf._pack_resnet_weight(wt, rotate=True)
            pairs = [("fwd", lambda: ext.resnet_conv(x, wp, b, ci, hw, co, True),
                      lambda: ext.resnet_conv_any(x, wp, b, True)),
                     ("wgrad", lambda: ext.resnet_conv_wgrad(x, dy, ci, hw, co),
                      lambda: ext.resnet_conv_any_wgrad(x, dy))]
            if ci != 8:  # the dgrad of 16 -> 32 is the 32 -> 16 template
                pairs.insert(1, (
                    "dgrad",
                    lambda: ext.resnet_conv(dy, wr, empty, co, hw, ci, False),
                    lambda: ext.resnet_conv_any(dy, wr, empty, False)))
            for kind, tmpl, anyk in pairs:
                ta, tb = three(tmpl, anyk)
                line(str(geom), kind, n, ta, tb, ("template", "any"))


def against_library(ns):
    ext = ops_mod.require_ext()
    empty = torch.empty(0, device="cuda")
    for name, geoms in (("procgen", PROCGEN), ("dmlab", DMLAB)):
        for geom in geoms:
            ci = geom[0]
            for n in ns:
                x, dy, wt, b = operands(geom, n)
                wp = tbf._pack_resnet_weight(wt)
                wr = tbf._pack_resnet_weight(wt, rotate=True)
                wb = wt.to(torch.bfloat16).contiguous(
                    memory_format=torch.channels_last)
                bb = b.to(torch.bfloat16)

                def lib_bwd():
                    if ci != 8:
                        conv2d_input(x.shape, wb, dy, padding=1)
                    conv2d_weight(x, wb.shape, dy, padding=1)
                    dy.sum((0, 2, 3))

                def any_bwd():
                    if ci != 8:
                        ext.resnet_conv_any(dy, wr, empty, False)
                    ext.resnet_conv_any_wgrad(x, dy)

                ta, tb = three(lambda: F.conv2d(x, wb, bb, padding=1),
                               lambda: ext.resnet_conv_any(x, wp, b, True))
                line(f"{name} {geom}", "fwd", n, ta, tb, ("library", "any"))
                ta, tb = three(lib_bwd, any_bwd)
                line(f"{name} {geom}", "bwd", n, ta, tb, ("library", "any"))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "templates"
    ns = [int(a) for a in sys.argv[2:]] or [64, 2592]
    with torch.no_grad():
        (against_templates if which == "templates" else against_library)(ns)


if __name__ == "__main__":
    main()
