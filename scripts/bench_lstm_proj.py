"""Times of the LSTM projection kernels (ops/hip/lstm_proj_mfma.hip) against
the fp32 library sequence that lstm_unroll_fwd / lstm_unroll_bwd run per layer
without the switch, and, as the mark to beat, the library's bf16 GEMM on
pre-cast operands.

Per (shape, op) the candidates alternate repetition by repetition in one
process, device events around every call after a warm-up; prints the median
and the 10th..90th percentile in microseconds, one JSON line per candidate.

    python scripts/bench_lstm_proj.py [--reps 200] [--warmup 20]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torchbeast_amd.ops as ops_mod  # noqa: E402

# (M, I, H): the learner's AtariNet and ResNet cores, monobeast's AtariNet.
SHAPES = [(2560, 519, 519), (2560, 257, 256), (640, 519, 519)]


def timed_alternating(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            events[name].append((start, end))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in events.items():
        us = sorted(s.elapsed_time(e) * 1e3 for s, e in pairs)
        out[name] = dict(median_us=round(us[len(us) // 2], 2),
                         p10_us=round(us[len(us) // 10], 2),
                         p90_us=round(us[len(us) * 9 // 10], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lstm_proj needs a GPU"
    ext = ops_mod.require_ext()
    torch.manual_seed(0)

    for m, i, h in SHAPES:
        x = torch.randn(m, i, device="cuda")
        hm = torch.randn(m, h, device="cuda")
        w = torch.randn(4 * h, i, device="cuda") / i ** 0.5
        b_ih = torch.randn(4 * h, device="cuda")
        b_hh = torch.randn(4 * h, device="cuda")
        dg = torch.randn(m, 4 * h, device="cuda")
        wb, wt = ext.lstm_proj_pack(w)
        xh, hh, wh, dh = (t.bfloat16() for t in (x, hm, w, dg))

        def lib_fwd():  # the lines of lstm_unroll_fwd
            return (torch.matmul(x, w.t()) + (b_ih + b_hh)).reshape(
                1, m, 4 * h).contiguous()

        def lib_wgrad():  # the lines of lstm_unroll_bwd
            db = dg.sum(0)
            return torch.matmul(dg.t(), x), torch.matmul(dg.t(), hm), db, \
                db.clone()

        ops = {
            "fwd": {
                "mfma": lambda: ext.lstm_proj_fwd(x, wb, b_ih, b_hh),
                "mfma pack + fwd": lambda: ext.lstm_proj_fwd(
                    x, ext.lstm_proj_pack(w)[0], b_ih, b_hh),
                "lib fp32 sequence": lib_fwd,
                "lib bf16 gemm (mark)": lambda: torch.matmul(xh, wh.t()),
            },
            "dgrad": {
                "mfma": lambda: ext.lstm_proj_dgrad(dg, wt, i),
                "lib fp32 sequence": lambda: torch.matmul(dg, w),
                "lib bf16 gemm (mark)": lambda: torch.matmul(dh, wh),
            },
            "wgrad+db": {
                "mfma": lambda: ext.lstm_proj_wgrad(dg, x, hm),
                "lib fp32 sequence": lib_wgrad,
                "lib bf16 gemms (mark)": lambda: (torch.matmul(dh.t(), xh),
                                                  torch.matmul(dh.t(), hh)),
            },
        }
        for op, fns in ops.items():
            for name, t in timed_alternating(fns, args.reps,
                                             args.warmup).items():
                print(json.dumps(dict(m=m, i=i, h=h, op=op, impl=name, **t)),
                      flush=True)


if __name__ == "__main__":
    main()
