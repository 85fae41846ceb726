"""Isolated fused-RMSProp step at the headline model's parameter count.

python scripts/bench_rmsprop.py [--variants default,momentum,centered,both]
                                [--iters 400] [--repeats 5] [--n N]

Runs `rmsprop_step` back to back for each variant and prints one JSON line
per variant with the event-timed cost of a whole step (memset + norm kernel +
update kernel, possibly launch-bound). For the kernel time of
`rmsprop_update_kernel` alone, run this under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_rmsprop.py` in a
process of its own and read the per-instantiation rows.

`default` uses the positional call that predates momentum/centered, so the
script also runs against an older build of the package (PYTHONPATH).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch  # noqa: E402

from torchbeast_amd.models import AtariNet  # noqa: E402
from torchbeast_amd.ops import functional as tbops  # noqa: E402

VARIANTS = {  # name -> (momentum, centered)
    "default": (0.0, False),
    "momentum": (0.9, False),
    "centered": (0.0, True),
    "both": (0.9, True),
}


def headline_param_count():
    net = AtariNet((4, 84, 84), 6)
    return sum(p.numel() for p in net.parameters() if p.requires_grad)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--variants", default="default,momentum,centered,both")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--n", type=int, default=0,
                   help="Elements; 0 = the headline AtariNet's parameters.")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rmsprop.py needs a GPU")

    n = args.n or headline_param_count()
    dev = "cuda"
    torch.manual_seed(0)
    grad = torch.randn(n, device=dev) * 0.1
    lr_dev = torch.full((1,), 1e-4, device=dev)

    for name in args.variants.split(","):
        momentum, centered = VARIANTS[name]
        param = torch.randn(n, device=dev)
        square_avg = torch.zeros(n, device=dev)
        call = [param, grad, square_avg, 1e-4, 0.99, 0.01, 40.0, lr_dev]
        streams = 5
        if name != "default":
            call += [
                torch.zeros(n, device=dev) if momentum > 0 else None,
                torch.zeros(n, device=dev) if centered else None,
                momentum,
            ]
            streams += 2 * (momentum > 0) + 2 * centered

        for _ in range(50):
            tbops.rmsprop_step(*call)
        torch.cuda.synchronize()
        per_step_us = []
        for _ in range(args.repeats):
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                tbops.rmsprop_step(*call)
            end.record()
            end.synchronize()
            per_step_us.append(start.elapsed_time(end) * 1e3 / args.iters)
        print(json.dumps({
            "variant": name, "n": n, "iters": args.iters,
            "update_kernel_streams": streams,
            "update_kernel_bytes": streams * 4 * n,
            "step_us_median": round(statistics.median(per_step_us), 3),
            "step_us_min": round(min(per_step_us), 3),
            "step_us_max": round(max(per_step_us), 3),
        }), flush=True)


if __name__ == "__main__":
    main()
