"""Isolated LSTM unroll timings: fused kernel vs per-phase breakdown.

python scripts/bench_lstm.py [--gate_wide] [T B H L]

--gate_wide: the switch that alternates is TBAMD_LSTM_GATE_WIDE (the
wide-batch kernels, B > 64) instead of TBAMD_LSTM_GATE_MFMA; where lstm4
refuses the batch, its rows are left out.
"""
import os, sys, timeit
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from torchbeast_amd.ops import functional as tbf

WIDE = "--gate_wide" in sys.argv
argv = [a for a in sys.argv if a != "--gate_wide"]
SWITCH = "TBAMD_LSTM_GATE_WIDE" if WIDE else "TBAMD_LSTM_GATE_MFMA"
T = int(argv[1]) if len(argv) > 1 else 80
B = int(argv[2]) if len(argv) > 2 else (128 if WIDE else 32)
H = int(argv[3]) if len(argv) > 3 else 519
L = int(argv[4]) if len(argv) > 4 else 2
if WIDE:
    os.environ[SWITCH] = "1"

torch.manual_seed(0)
dev = "cuda"
core = torch.nn.LSTM(H, H, num_layers=L).to(dev)
x = torch.randn(T, B, H, device=dev)
notdone = (torch.rand(T, B, device=dev) > 0.05).float()
h0 = torch.zeros(L, B, H, device=dev)
c0 = torch.zeros(L, B, H, device=dev)
dout = torch.randn(T, B, H, device=dev)

def timed(fn, iters=20, warmup=5):
    for _ in range(warmup): fn()
    torch.cuda.synchronize()
    t0 = timeit.default_timer()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (timeit.default_timer() - t0) / iters * 1e3

def fwd():
    with torch.no_grad():
        tbf.lstm_unroll(core, x, notdone, (h0, c0))

def fwd_bwd():
    for p in core.parameters():
        p.grad = None
    out, _ = tbf.lstm_unroll(core, x, notdone, (h0, c0))
    out.backward(dout)

print(f"T={T} B={B} H={H} L={L}")
print(f"lstm fwd      : {timed(fwd):8.3f} ms")
print(f"lstm fwd+bwd  : {timed(fwd_bwd):8.3f} ms")

# lstm4 next to the persistent MFMA kernels (SWITCH=1), in this process,
# alternating; lstm_unroll reads the switch at every forward.
def switched(fn, on):
    def run():
        if on:
            os.environ[SWITCH] = "1"
        else:
            os.environ.pop(SWITCH, None)
        fn()
    return run

sides = [False, True]
try:
    switched(fwd, False)()
except RuntimeError as e:  # lstm4's LDS limit
    print("lstm4 refuses this shape:", str(e).splitlines()[0])
    sides = [True]
rows = {(n, on): [] for n in ("fwd", "fwd+bwd") for on in sides}
for _ in range(5):
    for (n, on), acc in rows.items():
        acc.append(timed(switched(fwd if n == "fwd" else fwd_bwd, on),
                         iters=10, warmup=2))
os.environ.pop(SWITCH, None)
for (n, on), acc in rows.items():
    acc.sort()
    print(f"{('gate-wide' if WIDE else 'gate-mfma') if on else 'lstm4    '} "
          f"{n:8s}: median "
          f"{acc[len(acc) // 2]:8.3f} ms  [{acc[0]:.3f} .. {acc[-1]:.3f}]")

# Eager torch baseline (cuDNN-style per-step loop, masked).
def eager():
    state = (h0, c0)
    outs = []
    with torch.no_grad():
        for xt, nd in zip(x.unbind(), notdone.unbind()):
            nd = nd.view(1, -1, 1)
            state = tuple(nd * s for s in state)
            o, state = core(xt.unsqueeze(0), state)
            outs.append(o)

print(f"eager step-loop fwd: {timed(eager, iters=5, warmup=2):8.3f} ms")

# --gate_wide: the recurrence alone, per layer. ext.lstm_unroll_fwd / _bwd on
# one layer with a 1-wide input, so the projection and wgrad GEMMs are the
# same small constant on both sides; device events around 5 calls, 15
# alternating rounds.
if WIDE:
    import torchbeast_amd.ops as ops_mod
    ext = ops_mod.require_ext()
    core1 = torch.nn.LSTM(1, H).to(dev)
    flat = [p.detach() for p in (core1.weight_ih_l0, core1.weight_hh_l0,
                                 core1.bias_ih_l0, core1.bias_hh_l0)]
    x1 = torch.randn(T, B, 1, device=dev)
    h1, c1 = torch.randn(2, 1, B, H, device=dev).unbind()
    g1 = torch.randn(1, B, H, device=dev)

    def layer_fwd(wide):
        return ext.lstm_unroll_fwd(x1, notdone, h1, c1, flat, False, False,
                                   wide)

    stash = {wide: layer_fwd(wide)[3:] for wide in sides}

    def layer_bwd(wide):
        return ext.lstm_unroll_bwd(notdone, h1, c1, flat, stash[wide], dout,
                                   g1, g1, False, False, wide)

    def events(fn, wide, n=5):
        fn(wide)
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(n):
            fn(wide)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    per = {(n, w): [] for n in ("fwd", "bwd") for w in sides}
    for _ in range(15):
        for (n, w), acc in per.items():
            acc.append(events(layer_fwd if n == "fwd" else layer_bwd, w))
    for (n, w), acc in per.items():
        acc.sort()
        print(f"per layer {'gate-wide' if w else 'lstm4    '} {n}: median "
              f"{acc[len(acc) // 2]:8.3f} ms  [{acc[0]:.3f} .. {acc[-1]:.3f}]")
