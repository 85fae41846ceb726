"""Kernel times of the fp32 MFMA heads (ops/hip/heads_mfma.hip) against the
eager sequence the models run without them: clamp, one_hot, float and cat to
build the core input, two library GEMMs forward, and in the backward two dX
GEMMs, an add and the cat's slice copy, two dW GEMMs and two bias sums.

Device events around every repetition after a warm-up, the two sides of each
op alternating repetition by repetition in one process; prints the median and
the 10th..90th percentile in microseconds, one JSON line per (shape, op).

    python scripts/bench_heads.py [--reps 300] [--warmup 30]
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

# (M, Kc, A, form): form 2 is [x | r | one_hot], 1 is [x | r], 0 is plain.
SHAPES = [(2592, 519, 6, 2), (2592, 513, 6, 1), (2560, 257, 15, 1),
          (2560, 256, 15, 0)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heads needs a GPU"
    ext = ops_mod.require_ext()
    torch.manual_seed(0)

    for m, kc, a, form in SHAPES:
        d = kc - (form >= 1) - (a if form == 2 else 0)
        x = torch.randn(m, d, device="cuda")
        r = torch.randn(m, device="cuda") if form >= 1 else None
        act = torch.randint(0, a, (m,), device="cuda") if form == 2 else None
        pw = torch.randn(a, kc, device="cuda") / kc ** 0.5
        bw = torch.randn(1, kc, device="cuda") / kc ** 0.5
        pb, bb = torch.randn(a, device="cuda"), torch.randn(1, device="cuda")
        dl, db = torch.randn(m, a, device="cuda"), torch.randn(m, device="cuda")

        def core():
            if form == 0:
                return x
            cols = [x, torch.clamp(r, -1, 1).view(m, 1)]
            if form == 2:
                cols.append(F.one_hot(act, a).float())
            return torch.cat(cols, dim=-1)

        def eager_fwd():
            c = core()
            return F.linear(c, pw, pb), F.linear(c, bw, bb)

        def eager_dx():
            dc = dl @ pw + db.view(m, 1) @ bw
            return dc if form == 0 else dc[:, :d].contiguous()

        c = core()

        def eager_dw():  # the core input is saved by autograd: not rebuilt
            return (dl.t() @ c, db.view(1, m) @ c, dl.sum(0),
                    db.view(m, 1).sum(0))

        ops = {
            "fwd": (lambda: ext.heads_fwd(x, r, act, pw, pb, bw, bb),
                    eager_fwd),
            "dx": (lambda: ext.heads_dgrad(dl, db, pw, bw, d), eager_dx),
            "dw": (lambda: ext.heads_wgrad(x, r, act, dl, db), eager_dw),
        }
        for name, fns in ops.items():
            for side, t in zip(("mfma", "eager"),
                               timed_pair(fns, args.reps, args.warmup)):
                print(json.dumps(dict(m=m, kc=kc, a=a, form=form,
                                      op=f"{side} {name}", **t)), flush=True)


if __name__ == "__main__":
    main()
