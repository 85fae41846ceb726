"""Time of the learner tail (core/tail.py: learner_tail forward plus the
backward down to target_logits.grad and baseline.grad) with TBAMD_FUSED_TAIL
unset (vtrace_kernel + impala_loss_kernel + ATen glue) and set (one launch of
ops/hip/impala_tail.hip plus two scalings).

Device events around every repetition after a warm-up, the two sides
alternating repetition by repetition in one process; prints the median and the
10th..90th percentile in microseconds and the number of device kernels one
repetition launches, one JSON line per (shape, side). The kernels are counted
with the profiler after all timing is done, since its tracer stays loaded.
The repetitions are launched eagerly, so at these sizes the time is mostly
the host's launches.

    python scripts/bench_tail.py [--reps 300] [--warmup 30] [--names]
"""

import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

from torchbeast_amd.core import tail  # noqa: E402

SHAPES = [(81, 32, 6), (81, 32, 18), (81, 128, 18)]  # [T+1, B, A]
FLAGS = types.SimpleNamespace(discounting=0.99, reward_clipping="abs_one",
                              vtrace_lambda=1.0, baseline_cost=0.5,
                              entropy_cost=0.0006)


def launches(fn):
    """Names of the device kernels of one call, from the profiler; None if it
    has no device tracer."""
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CPU,
                                 ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
    except RuntimeError:  # no device tracer in this build
        return None
    return [e.name for e in p.events()
            if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower()] or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--names", action="store_true",
                    help="also print the kernel names of each side")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tail needs a GPU"
    torch.manual_seed(0)

    rows = []
    for t1, b, a in SHAPES:
        rewards = 2 * torch.randn(t1, b, device="cuda")
        done = torch.rand(t1, b, device="cuda") < 0.05
        actor_logits = torch.randn(t1, b, a, device="cuda")
        actions = torch.randint(0, a, (t1, b), device="cuda")
        logits = torch.randn(t1, b, a, device="cuda", requires_grad=True)
        baseline = torch.randn(t1, b, device="cuda", requires_grad=True)

        def step(switch):
            if switch:
                os.environ["TBAMD_FUSED_TAIL"] = "1"
            else:
                os.environ.pop("TBAMD_FUSED_TAIL", None)
            logits.grad = baseline.grad = None
            out = tail.learner_tail(FLAGS, rewards, done, actor_logits,
                                    actions, logits, baseline)
            out[0].backward()

        sides = (("off", False), ("on", True))
        for _ in range(args.warmup):
            for _, switch in sides:
                step(switch)
        torch.cuda.synchronize()
        events = {name: [] for name, _ in sides}
        for _ in range(args.reps):
            for name, switch in sides:
                start = torch.cuda.Event(enable_timing=True)
                end = torch.cuda.Event(enable_timing=True)
                start.record()
                step(switch)
                end.record()
                events[name].append((start, end))
        torch.cuda.synchronize()
        for name, switch in sides:
            us = sorted(s.elapsed_time(e) * 1e3 for s, e in events[name])
            rows.append((dict(shape=[t1, b, a], fused_tail=name,
                              median_us=round(us[len(us) // 2], 2),
                              p10_us=round(us[len(us) // 10], 2),
                              p90_us=round(us[len(us) * 9 // 10], 2)),
                         step, switch))
    for row, step, switch in rows:
        names = launches(lambda: step(switch))
        print(json.dumps(dict(row, kernels=names and len(names))), flush=True)
        if args.names and names:
            print("\n".join("    " + n[:110] for n in names), flush=True)


if __name__ == "__main__":
    main()
