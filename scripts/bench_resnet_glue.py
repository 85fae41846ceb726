"""Times of the deep ResNet's glue kernels (ops/hip/resnet_glue.hip) against
the ATen ops they replace, and of the whole trunk with TBAMD_RESNET_GLUE unset
and set.

Trunk: _features forward + backward at 84x84, N = 2560 and N = 64, the two
settings alternating repetition by repetition in one process. Kernels, at the
first section's shape [N, 16, 84, 84] -> [N, 16, 42, 42]: pool_fwd against
max_pool2d + relu, pool_bwd against their two backwards and the add of the
two gradients, add + relu forward and backward, and at [N, 32, 11, 11] the
flatten against float + relu + reshape. Device events around every
repetition after a warm-up; prints the median and the 10th..90th percentile
in microseconds, one JSON line per measurement.

    python scripts/bench_resnet_glue.py [--reps 30] [--warmup 5]
"""

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torchbeast_amd.ops as ops_mod  # noqa: E402
from torchbeast_amd.models.resnet import ResNet  # noqa: E402

CL = torch.channels_last


def timed_pair(fns, reps, warmup):
    """Median and percentiles of each fn, the fns alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    events = [[(torch.cuda.Event(enable_timing=True),
                torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
              for _ in fns]
    for i in range(reps):
        for fn, ev in zip(fns, events):
            ev[i][0].record()
            fn()
            ev[i][1].record()
    torch.cuda.synchronize()
    out = []
    for ev in events:
        us = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
        out.append(dict(median_us=round(us[len(us) // 2], 2),
                        p10_us=round(us[len(us) // 10], 2),
                        p90_us=round(us[len(us) * 9 // 10], 2)))
    return out


def report(n, name, sides, fns, args):
    for side, t in zip(sides, timed_pair(fns, args.reps, args.warmup)):
        print(json.dumps(dict(n=n, op=f"{side} {name}", **t)), flush=True)


def act(n, c, h, w):
    return torch.randn(n, c, h, w, device="cuda").to(
        torch.bfloat16).contiguous(memory_format=CL)


def trunk(net, x, glue):
    def step():
        if glue:
            os.environ["TBAMD_RESNET_GLUE"] = "1"
        else:
            os.environ.pop("TBAMD_RESNET_GLUE", None)
        net.zero_grad(set_to_none=True)
        feats = net._features(x, flat=True)
        if feats.dim() == 4:
            feats = F.relu(feats).reshape(x.shape[0], -1)
        feats.backward(torch.ones_like(feats))
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2560, 64])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resnet_glue needs a GPU"
    ext = ops_mod.require_ext()
    torch.manual_seed(0)
    net = ResNet((4, 84, 84)).cuda()

    for n in args.batches:
        frames = torch.rand(n, 4, 84, 84, device="cuda")
        report(n, "trunk fwd+bwd", ("aten", "glue"),
               (trunk(net, frames, False), trunk(net, frames, True)), args)
        del frames

        x = act(n, 16, 84, 84)
        y, r, idx = ext.resnet_glue_pool_fwd(x)
        g_y, g_r = act(n, 16, 42, 42), act(n, 16, 42, 42)

        def aten_pool_bwd():
            xr = x.detach().requires_grad_()
            yy = F.max_pool2d(xr, 3, 2, 1)
            return xr, yy, F.relu(yy)

        xr, yy, rr = aten_pool_bwd()  # the graph is built outside the timing
        report(n, "pool fwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_pool_fwd(x),
                lambda: F.relu(F.max_pool2d(x, 3, 2, 1))), args)
        report(n, "pool bwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_pool_bwd(g_y, g_r, r, idx, 84, 84),
                lambda: torch.autograd.grad((yy, rr), xr, (g_y, g_r),
                                            retain_graph=True)), args)
        del x, xr, yy, rr, idx

        a, s = act(n, 16, 42, 42), y
        z = a + s
        report(n, "add+relu fwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_ew_fwd(a, s, True),
                lambda: F.relu(a + s)), args)
        report(n, "add+relu bwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_ew_bwd(g_y, g_r, r),
                lambda: g_y + torch.ops.aten.threshold_backward(g_r, z, 0)),
               args)
        del a, s, z, y, r, g_y, g_r

        t = act(n, 32, 11, 11)
        g = torch.randn(n, 32 * 121, device="cuda")
        tf = t.float()  # saved by autograd in the ATen path
        report(n, "flatten fwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_flat_fwd(t),
                lambda: F.relu(t.float()).reshape(n, -1)), args)
        report(n, "flatten bwd", ("glue", "aten"),
               (lambda: ext.resnet_glue_flat_bwd(g, t),
                lambda: torch.ops.aten.threshold_backward(
                    g.view(n, 32, 11, 11), tf, 0).to(
                        torch.bfloat16).contiguous(memory_format=CL)), args)
        del t, tf, g


if __name__ == "__main__":
    main()
