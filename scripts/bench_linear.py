"""Kernel times of the MFMA linear family (ops/hip/linear_mfma.hip) against
the fp32 library fc it replaces, and, for information, the library's bf16 GEMM.

Device events around every repetition after a warm-up; prints the median and
the 10th..90th percentile in microseconds, one JSON line per (shape, op).

    python scripts/bench_linear.py [--reps 300] [--warmup 30]
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

SERVE = [(m, n, k) for (n, k) in ((512, 3136), (256, 3872))
         for m in (64, 128, 256)]
LEARNER = [(2592, 512, 3136), (2560, 256, 3872)]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True),
              torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for start, end in pairs:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    us = sorted(s.elapsed_time(e) * 1e3 for s, e in pairs)
    return dict(median_us=round(us[len(us) // 2], 2),
                p10_us=round(us[len(us) // 10], 2),
                p90_us=round(us[len(us) * 9 // 10], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_linear needs a GPU"
    ext = ops_mod.require_ext()
    torch.manual_seed(0)

    for m, n, k in SERVE + LEARNER:
        x = torch.randn(m, k, device="cuda")
        w = torch.randn(n, k, device="cuda") / k ** 0.5
        b = torch.randn(n, device="cuda")
        dy = torch.randn(m, n, device="cuda")
        wb, wt = ext.linear_pack(w)
        y = ext.linear_fwd(x, wb, b, True)
        xh, wh = x.bfloat16(), w.bfloat16()
        ops = {
            "mfma fwd": lambda: ext.linear_fwd(x, wb, b, True),
            "lib fp32 fwd": lambda: F.linear(x, w, b).relu_(),
            "lib bf16 gemm fwd (info)": lambda: F.linear(xh, wh),
        }
        if (m, n, k) in LEARNER:
            dym = dy * (y > 0)
            dyh = dym.bfloat16()
            ops.update({
                "mfma pack": lambda: ext.linear_pack(w),
                "mfma dgrad": lambda: ext.linear_dgrad(dy, y, wt, True),
                "mfma wgrad": lambda: ext.linear_wgrad(dy, y, x, True),
                "lib fp32 relu mask": lambda: dy * (y > 0),
                "lib fp32 dgrad": lambda: dym @ w,
                "lib fp32 wgrad": lambda: (dym.t() @ x, dym.sum(0)),
                "lib bf16 gemm dgrad (info)": lambda: dyh @ wh,
                "lib bf16 gemm wgrad (info)": lambda: dyh.t() @ xh,
            })
        for name, fn in ops.items():
            print(json.dumps(dict(m=m, n=n, k=k, op=name,
                                  **timed(fn, args.reps, args.warmup))),
                  flush=True)


if __name__ == "__main__":
    main()
