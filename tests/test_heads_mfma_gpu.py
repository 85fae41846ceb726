"""The fp32 MFMA heads kernels (ops/hip/heads_mfma.hip: heads_fwd, heads_dgrad,
heads_wgrad, heads_supported) against float64 on the CPU, in the three forms of
the core input: plain, [x | r] and [x | r | one_hot(a)].

Exact rule: x in 0..4 (two fifths of it zero), reward in {-2..2} so that the
clamp binds, weights in {-1, 0, 1}, integer biases and dy in -3..3, one action
in four never taken and one out of range. Head n is dead (zero weights, bias
and dy column) when n % 3 == 1, and so is row m of dy when m % 3 == 1, which
keeps every result between 20 % and 80 % nonzero. Every partial sum is an
integer far below 2^24 in any order, so outputs are compared with torch.equal.

Bounded rule: random operands at the learner's shapes, within K * 2^-24 * S per
element, S = sum |terms| + |bias|, K = 4 r. r = 4.33 is what plain float32
F.linear and its float32 autograd reach on the CPU against float64 on these
same cases (largest of y, dx, dW and db: dx at 2560 x 257, A = 15).

Shapes come from ops/hip/heads_plan.h: 16 forward rows and 64 dX rows per
workgroup, tiles of 64 columns, k-steps of 4 dealt to 4 waves, fragments of 16
head rows, dW rounds of 64 rows dealt to chunks.
"""

import re

import pytest
import torch

pytestmark = pytest.mark.gpu

CPU_RATIO = 4.33  # measured: float32 F.linear and autograd on the CPU
K_BOUND = 4 * CPU_RATIO
U = 2.0 ** -24
ROUND = 64  # kHeadsRound

# (M, D, A, form): form 0 plain, 1 [x | r], 2 [x | r | one_hot]. M around the
# 16-row tile and past one dX tile; ROUND + 17 rows are two dW chunks, the last
# one cut; D below one k-step, k-step and wave-split tails, unaligned rows;
# A + 1 at a fragment boundary, one past it, and the maximum.
EXACT = [(1, 65, 1, 0), (15, 1, 6, 1), (16, 3, 15, 2), (17, 4, 16, 0),
         (65, 5, 18, 1), (65, 63, 63, 2), (17, 64, 6, 0), (ROUND + 17, 257, 6, 1),
         (16, 519, 6, 0), (17, 512, 6, 2)]
RANDOM = [(2592, 519, 6, 0), (2592, 512, 6, 2), (2560, 256, 15, 1)]


def _case(m, d, a, form, exact, unaligned=False):
    g = torch.Generator().manual_seed(m * 7919 + d * 31 + a + form)
    kc = d + (form >= 1) + (a if form == 2 else 0)
    live_n = (torch.arange(a + 1) % 3 != 1).float()
    live_m = (torch.arange(m) % 3 != 1).float()
    if exact:
        x = (torch.randint(0, 5, (m, d), generator=g)
             * (torch.rand(m, d, generator=g) < 0.75)).float()
        r = torch.randint(-2, 3, (m,), generator=g).float()
        w = torch.randint(-1, 2, (a + 1, kc), generator=g).float()
        b = torch.randint(-3, 4, (a + 1,), generator=g).float()
        dy = torch.randint(-3, 4, (m, a + 1), generator=g).float()
        w, b = w * live_n[:, None], b * live_n
        dy = dy * live_n * live_m[:, None]
    else:
        x = torch.randn(m, d, generator=g)
        r = 1.5 * torch.randn(m, generator=g)
        w = torch.randn(a + 1, kc, generator=g) / kc ** 0.5
        b = torch.randn(a + 1, generator=g)
        dy = torch.randn(m, a + 1, generator=g)
    act = torch.randint(0, a, (m,), generator=g)
    act = act - (act % 4 == 3).long()  # actions 3, 7, ... are never taken
    act[0] = a  # out of range: an all-zero one-hot row
    flat = torch.zeros(1 + (a + 1) * (kc + 1))
    off = 1 if unaligned else 0  # weights as views of a flat buffer
    flat[off:off + w.numel()] = w.flatten()
    flat[off + w.numel():off + w.numel() + a + 1] = b
    c = dict(x=x, r=r if form >= 1 else None, a=act if form == 2 else None,
             dl=dy[:, :a].contiguous(), db=dy[:, a].contiguous(), flat=flat,
             off=off, A=a, kc=kc)
    if exact:
        for name, ref in _refs(c)[0].items():
            dense = float((ref != 0).double().mean())
            assert ref.min() != ref.max() and 0.2 <= dense <= 0.8, (name, dense)
    return c


def _weights(c, flat):
    a, kc, o = c["A"], c["kc"], c["off"]
    pw, bw = flat[o:o + a * kc].view(a, kc), flat[o + a * kc:][:kc].view(1, kc)
    pb = flat[o + (a + 1) * kc:][:a]
    return pw, pb, bw, flat[o + (a + 1) * kc + a:][:1]


def _refs(c, dl=True, db=True):
    """float64 results and the per-element sums of magnitudes S."""
    a, d = c["A"], c["x"].shape[1]
    cols = [c["x"].double()]
    if c["r"] is not None:
        cols.append(c["r"].double().clamp(-1, 1)[:, None])
    if c["a"] is not None:
        cols.append((c["a"][:, None] == torch.arange(a)).double())
    core = torch.cat(cols, 1)
    pw, pb, bw, bb = (t.double() for t in _weights(c, c["flat"]))
    w, b = torch.cat([pw, bw]), torch.cat([pb, bb])
    dy = torch.cat([c["dl"] * dl, c["db"][:, None] * db], 1).double()
    ref = dict(y=core @ w.t() + b, dx=(dy @ w)[:, :d], dw=dy.t() @ core,
               db=dy.sum(0))
    s = dict(y=core.abs() @ w.abs().t() + b.abs(),
             dx=(dy.abs() @ w.abs())[:, :d], dw=dy.abs().t() @ core.abs(),
             db=dy.abs().sum(0))
    return ref, s


# ---- GPU ----

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.ops import functional as tbf
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)


def _gpu(c):
    g = {k: v.cuda() if torch.is_tensor(v) else v for k, v in c.items()}
    g["w"] = _weights(c, g["flat"])
    return g


def _run(g):
    """All three entry points, results joined as _refs joins them."""
    ext = ops_mod.require_ext()
    pw, pb, bw, bb = g["w"]
    logits, base = ext.heads_fwd(g["x"], g["r"], g["a"], pw, pb, bw, bb)
    dx = ext.heads_dgrad(g["dl"], g["db"], pw, bw, g["x"].shape[1])
    dpw, dpb, dbw, dbb = ext.heads_wgrad(g["x"], g["r"], g["a"], g["dl"],
                                         g["db"])
    assert dpw.shape == pw.shape and dbw.shape == bw.shape
    return dict(y=torch.cat([logits, base[:, None]], 1), dx=dx,
                dw=torch.cat([dpw, dbw]), db=torch.cat([dpb, dbb]))


def _assert_exact(got, ref, what):
    assert got.dtype == torch.float32 and got.shape == ref.shape, what
    assert torch.equal(got.cpu().double(), ref), what


@pytest.mark.parametrize("m,d,a,form,unaligned",
                         [c + (False,) for c in EXACT] + [(17, 64, 6, 0, True)])
def test_entry_points_exact(m, d, a, form, unaligned):
    c = _case(m, d, a, form, True, unaligned)
    ref, _ = _refs(c)
    got = _run(_gpu(c))
    for name in ref:
        _assert_exact(got[name], ref[name], f"{name} {m, d, a, form}")


@pytest.mark.parametrize("missing", ["dbaseline", "dlogits"])
def test_autograd_function_with_a_missing_gradient(missing):
    """Only one output reaches the loss: the other gradient arrives as None
    and is a zero operand."""
    c = _case(65, 5, 18, 1, True)
    dl, db = missing != "dlogits", missing != "dbaseline"
    ref, _ = _refs(c, dl=dl, db=db)
    g = _gpu(c)
    x = g["x"].requires_grad_()
    ws = [t.detach().clone().requires_grad_() for t in g["w"]]
    logits, base = tbf._HeadsMfma.apply(x, g["r"], g["a"], *ws)
    _assert_exact(torch.cat([logits, base[:, None]], 1).detach(), ref["y"], "y")
    if dl:
        logits.backward(g["dl"])
    else:
        base.backward(g["db"])
    _assert_exact(x.grad, ref["dx"], "dx")
    _assert_exact(torch.cat([ws[0].grad, ws[2].grad]), ref["dw"], "dw")
    _assert_exact(torch.cat([ws[1].grad, ws[3].grad]), ref["db"], "db")


@pytest.mark.parametrize("m,d,a,form", RANDOM)
def test_random_within_bound(m, d, a, form):
    c = _case(m, d, a, form, False)
    ref, s = _refs(c)
    got = _run(_gpu(c))
    ratios = {}
    for name in ref:
        err = (got[name].cpu().double() - ref[name]).abs()
        ratios[name] = float((err / (U * s[name]).clamp_min(1e-300)).max())
    print(f"RATIO heads {m, d, a, form}: "
          + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items())
          + f" of 2^-24*S, K = {K_BOUND:.2f}")
    assert max(ratios.values()) <= K_BOUND, ratios


def _fwd(e, g, **kw):
    pw, pb, bw, bb = g["w"]
    a = dict(x=g["x"], r=g["r"], a=g["a"], pw=pw, pb=pb, bw=bw, bb=bb)
    a.update(kw)
    return e.heads_fwd(a["x"], a["r"], a["a"], a["pw"], a["pb"], a["bw"],
                       a["bb"])


BAD = {
    "x on the CPU": ("x", lambda e, g: _fwd(e, g, x=g["x"].cpu())),
    "x float64": ("x", lambda e, g: _fwd(e, g, x=g["x"].double())),
    "last_action float": ("last_action",
                          lambda e, g: _fwd(e, g, a=g["a"].float())),
    "x strided": ("x", lambda e, g: _fwd(e, g, x=g["x"].repeat(1, 2)[:, ::2])),
    "dgrad rows disagree": ("dbaseline", lambda e, g: e.heads_dgrad(
        g["dl"], g["db"][:4], g["w"][0], g["w"][2], 3)),
    "wgrad rows disagree": ("dlogits", lambda e, g: e.heads_wgrad(
        g["x"], g["r"], g["a"], g["dl"][:4], g["db"])),
    "A = 64": ("A=64", lambda e, g: e.heads_fwd(
        g["x"], None, None, torch.zeros(64, 3, device="cuda"),
        torch.zeros(64, device="cuda"), g["w"][2][:, :3].contiguous(),
        g["w"][3])),
    "reward length": ("reward", lambda e, g: _fwd(e, g, r=g["r"][:4])),
}


@pytest.mark.parametrize("name", list(BAD))
def test_host_checks_raise_before_any_launch(name):
    c = _case(16, 3, 15, 2, True)
    g = _gpu(c)
    arg, call = BAD[name]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    try:
        call(ops_mod.require_ext(), g)
    except RuntimeError as e:
        assert re.search(r"heads_\w+: .*" + arg, str(e)), str(e)
    else:
        pytest.fail(f"{name}: no error raised")
    assert torch.cuda.memory_allocated() == before  # nothing was allocated
    torch.cuda.synchronize()
    _assert_exact(_run(g)["y"], _refs(c)[0]["y"], "y after the refused call")
