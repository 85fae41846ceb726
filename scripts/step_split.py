"""Host-time split of bench.py's hipGraph learner step, from outside bench.py.

    python scripts/step_split.py LABEL --gpus 1 --steps 50 --warmup 10
    TBAMD_BENCH_TIMINGS=1 python scripts/step_split.py LABEL --gpus 1 ...

Wraps `_tbruntime.flatten`, `FusedRMSProp.push_lr`, `CUDAGraph.replay` and
`torch.cuda.synchronize` with perf_counter stamps, runs bench.py as
`__main__` with the remaining arguments and prints one `step_split:` JSON
line (milliseconds per timed step: mean, median, min, max) to stderr:

  next    flatten entry minus the previous replay's exit (and minus that
          step's sync): next(learner_queue), i.e. waiting for rollouts plus
          batch assembly, plus scheduler.step and mark_weights_dirty
  flatten `_tbruntime.flatten` of the dequeued nest
  copies  flatten exit to push_lr entry: the `.to(device)` no-ops and the
          eight `copy_` calls into the static batch (host issue time)
  push_lr the learning-rate upload
  replay  `CUDAGraph.replay()` on the host (the launch, not the GPU work)
  sync    `torch.cuda.synchronize()` right after a replay; bench.py calls
          it per step only under TBAMD_BENCH_TIMINGS, where it is the time
          the GPU still needs for the static copies and the graph after
          they were issued; 0 in a free-running run

The wrappers cost about a microsecond per call; bench.py's own JSON line of
the same run shows what the step rate was with them in place.
"""
import atexit
import json
import os
import runpy
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.chdir(ROOT)

import torch  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402
from torchbeast_amd.parallel import flat as tbflat  # noqa: E402

KEYS = ("next", "flatten", "copies", "push_lr", "replay", "sync")
events = []  # (tag, t_enter, t_exit), in call order of the learner thread


def _wrap(fn, tag):
    def wrapped(*args, **kwargs):
        t0 = time.perf_counter()
        result = fn(*args, **kwargs)
        events.append((tag, t0, time.perf_counter()))
        return result
    return wrapped


def _report(label, steps):
    # A graph step is the sequence flatten, push_lr, replay[, sync].
    rows = []
    prev_exit, prev_sync = None, 0.0
    i = 0
    while i + 2 < len(events):
        tags = (events[i][0], events[i + 1][0], events[i + 2][0])
        if tags != ("flatten", "push_lr", "replay"):
            i += 1
            continue
        f, p, r = events[i], events[i + 1], events[i + 2]
        sync = 0.0
        if i + 3 < len(events) and events[i + 3][0] == "sync":
            sync = events[i + 3][2] - events[i + 3][1]
        if prev_exit is not None:
            rows.append(dict(next=f[1] - prev_exit - prev_sync,
                             flatten=f[2] - f[1], copies=p[1] - f[2],
                             push_lr=p[2] - p[1], replay=r[2] - r[1],
                             sync=sync))
        prev_exit, prev_sync = r[2], sync
        i += 3
    rows = rows[-(steps - 1):]
    if not rows:
        print("step_split: no graph steps seen (eager run?)", file=sys.stderr)
        return
    out = {"label": label, "n": len(rows)}
    for k in KEYS:
        v = [row[k] * 1e3 for row in rows]
        out[k] = dict(mean=round(statistics.mean(v), 4),
                      median=round(statistics.median(v), 4),
                      min=round(min(v), 4), max=round(max(v), 4))
    out["sum_mean_ms"] = round(sum(out[k]["mean"] for k in KEYS), 4)
    print("step_split: " + json.dumps(out), file=sys.stderr, flush=True)


def main():
    label = sys.argv[1]
    steps = int(sys.argv[sys.argv.index("--steps") + 1])
    runtime._tbruntime.flatten = _wrap(runtime._tbruntime.flatten, "flatten")
    tbflat.FusedRMSProp.push_lr = _wrap(tbflat.FusedRMSProp.push_lr, "push_lr")
    torch.cuda.CUDAGraph.replay = _wrap(torch.cuda.CUDAGraph.replay, "replay")
    torch.cuda.synchronize = _wrap(torch.cuda.synchronize, "sync")
    atexit.register(_report, label, steps)
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
