"""The bf16 MFMA linear kernels (ops/hip/linear_mfma.hip: linear_pack,
linear_fwd, linear_dgrad, linear_wgrad, linear_supported) against float64 on
the CPU, operands rounded by torch's own .bfloat16().

Exact rule: x holds integers in 0..300 (257, 258, 259 and 262 among them,
which bf16 cannot hold: round-to-nearest-even in staging is pinned), weights
in {-1, 0, 1}, integer bias and dy, the bias shifted so that about a quarter
of y is <= 0. Every partial sum is an integer below 2^24 in any order, so
outputs are compared with torch.equal.

Bounded rule: random operands pre-rounded to bf16 at the real fc shapes,
within K * 2^-24 * S per element, S = sum |terms| + |bias|, K = 4 r. r = 2.74
is what plain float32 F.linear and its float32 autograd reach on the CPU
against float64 on these same cases (measured on the CPU, largest of forward,
dx, dW and db).

Shapes come from the constants of ops/hip/linear_plan.h: 64 x 64 tiles,
k-steps of 32, K-slices of at least 2 steps up to 256 workgroups, wgrad
staging rounds of 128 rows dealt to at most 32 chunks.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CPU_RATIO = 2.74  # measured: float32 F.linear and autograd on the CPU
K_BOUND = 4 * CPU_RATIO
U = 2.0 ** -24


def _bf(t):
    return t.bfloat16().double()


def _case(m, n, k, exact, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + m * 7919 + n * 31 + k)
    if exact:
        x = torch.randint(0, 301, (m, k), generator=g).float()
        x.view(-1)[:4] = torch.tensor([257.0, 258.0, 259.0, 262.0])
        w = torch.randint(-1, 2, (n, k), generator=g).float()
        # y has standard deviation ~141 sqrt(k); its lower quartile at zero.
        b = (torch.randint(-40, 41, (n,), generator=g)
             + round(0.674 * 141 * k ** 0.5)).float()
        dy = torch.randint(-3, 4, (m, n), generator=g).float()
    else:
        x = torch.randn(m, k, generator=g).bfloat16().float()
        w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16().float()
        b = (torch.randn(n, generator=g) + 0.674).bfloat16().float()
        dy = torch.randn(m, n, generator=g).bfloat16().float()
    return dict(x=x, w=w, b=b, dy=dy)


def _refs(c, relu=True, mask=True):
    """float64 results and the per-element sums of magnitudes S."""
    x, w, b, dy = _bf(c["x"]), _bf(c["w"]), c["b"].double(), c["dy"].double()
    pre = x @ w.t() + b
    y = pre.clamp_min(0) if relu else pre
    dym = dy * (pre > 0) if mask else dy
    ref = dict(y=y, dx=_bf(dym) @ w, dW=_bf(dym).t() @ x, db=dym.sum(0))
    s = dict(y=x.abs() @ w.abs().t() + b.abs(), dx=dym.abs() @ w.abs(),
             dW=dym.abs().t() @ x.abs(), db=dym.abs().sum(0))
    return ref, s, pre.clamp_min(0).float()


def _assert_exact(got, ref, what):
    assert ref.min() != ref.max(), f"{what}: constant reference"
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got.cpu().double(), ref), what


def _ratio(got, ref, s):
    assert ref.min() != ref.max()
    # S = 0 (a column the mask empties) admits no error at all.
    err = (got.cpu().double() - ref).abs()
    return float((err / (U * s).clamp_min(1e-300)).max())


# ---- GPU ----

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.ops import functional as tbf
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)


def _ext():
    return ops_mod.require_ext()


def _gpu(c):
    d = {k: v.cuda() for k, v in c.items()}
    d["wb"], d["wt"] = _ext().linear_pack(d["w"])
    return d


@pytest.mark.parametrize("n,k", [(64, 32), (512, 3136)])
def test_pack_bit_for_bit(n, k):
    w = torch.randn(n, k, generator=torch.Generator().manual_seed(n))
    w[0, :4] = torch.tensor([257.0, 258.0, 259.0, 262.0])
    wb, wt = _ext().linear_pack(w.cuda())
    want = w.bfloat16()
    assert wb.dtype == wt.dtype == torch.bfloat16
    assert torch.equal(wb.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(wt.cpu().view(torch.int16),
                       want.t().contiguous().view(torch.int16))


# M below a tile, at its edge, one past, 1; K of one step; (65, 64, 224): 7
# k-steps in 3 slices of 2, 2, 3; (2049, 512, 96): 264 tiles, one slice of 3
# steps; then the two fcs, sliced 32 and 32 ways.
FWD = [(63, 64, 32), (64, 64, 32), (65, 64, 32), (1, 64, 32), (65, 64, 224),
       (2049, 512, 96), (64, 512, 3136), (65, 256, 3872)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("m,n,k", FWD)
def test_fwd_exact(m, n, k, relu):
    c = _case(m, n, k, True)
    ref, _, _ = _refs(c, relu=relu)
    assert relu is False or 0.1 < float((ref["y"] == 0).double().mean()) < 0.4
    g = _gpu(c)
    y = _ext().linear_fwd(g["x"], g["wb"], g["b"], relu)
    _assert_exact(y, ref["y"], f"y {m, n, k}")
    assert torch.equal(y, _ext().linear_fwd(g["x"], g["wb"], g["b"], relu))


# The same M tails; N = 64 is two k-steps, K = 96 leaves a half-masked tile.
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("n", [64, 512])
@pytest.mark.parametrize("m", [63, 64, 65, 1])
def test_dgrad_exact(m, n, mask):
    c = _case(m, n, 96, True)
    ref, _, y = _refs(c, mask=mask)
    g = _gpu(c)
    dx = _ext().linear_dgrad(g["dy"], y.cuda(), g["wt"], mask)
    _assert_exact(dx, ref["dx"], f"dx {m, n} mask={mask}")


# M = 1; below, at and past one staging round (129 and 200: two chunks, the
# last one cut); 4200: 33 rounds dealt unevenly to 32 chunks; the learner's
# fc in one chunk.
WGRAD = [(1, 64, 96), (127, 64, 96), (128, 64, 96), (129, 64, 96),
         (200, 64, 96), (4200, 64, 96), (300, 512, 3136)]


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("m,n,k", WGRAD)
def test_wgrad_exact(m, n, k, mask):
    c = _case(m, n, k, True)
    ref, _, y = _refs(c, mask=mask)
    g = _gpu(c)
    dw, db = _ext().linear_wgrad(g["dy"], y.cuda(), g["x"], mask)
    _assert_exact(dw, ref["dW"], f"dW {m, n, k} mask={mask}")
    _assert_exact(db, ref["db"], f"db {m, n, k} mask={mask}")
    assert dw.is_contiguous()


@pytest.mark.parametrize("m,n,k", [(320, 512, 3136), (65, 256, 3872)])
def test_random_within_bound(m, n, k):
    c = _case(m, n, k, False)
    ref, s, y = _refs(c)
    g = _gpu(c)
    ext = _ext()
    dw, db = ext.linear_wgrad(g["dy"], y.cuda(), g["x"], True)
    got = dict(y=ext.linear_fwd(g["x"], g["wb"], g["b"], True),
               dx=ext.linear_dgrad(g["dy"], y.cuda(), g["wt"], True),
               dW=dw, db=db)
    ratios = {name: _ratio(got[name], ref[name], s[name]) for name in ref}
    print(f"RATIO linear {m, n, k}: "
          + ", ".join(f"{a} {r:.3f}" for a, r in ratios.items())
          + f" of 2^-24*S, K = {K_BOUND:.2f}")
    assert max(ratios.values()) <= K_BOUND, ratios


def test_rows_past_2_31_elements():
    """M * K > 2^31: the last row of x, dy and dx lies past a 32-bit
    element offset. Only the first and last rows are non-zero."""
    m, n, k = 65537, 64, 32768
    assert m * k > 2 ** 31
    ext = _ext()
    ends = _case(2, n, k, True)
    ref, _, _ = _refs(ends)
    g = _gpu(ends)
    x = torch.zeros(m, k, device="cuda")
    dy = torch.zeros(m, n, device="cuda")
    x[0], x[-1], dy[0], dy[-1] = g["x"][0], g["x"][1], g["dy"][0], g["dy"][1]
    y = ext.linear_fwd(x, g["wb"], g["b"], True)
    _assert_exact(y[[0, -1]], ref["y"], "y ends")
    assert torch.equal(y[1:-1], g["b"].clamp_min(0).expand(m - 2, n))
    dw, db = ext.linear_wgrad(dy, y, x, True)
    _assert_exact(dw, ref["dW"], "dW")
    _assert_exact(db, ref["db"], "db")
    del x
    dx = ext.linear_dgrad(dy, y, g["wt"], True)
    _assert_exact(dx[[0, -1]], ref["dx"], "dx ends")
    assert not bool(dx[1:-1].any())


BAD = {
    "fwd x on the CPU": lambda e, g: e.linear_fwd(g["x"].cpu(), g["wb"], g["b"], True),
    "fwd x float64": lambda e, g: e.linear_fwd(g["x"].double(), g["wb"], g["b"], True),
    "fwd x strided": lambda e, g: e.linear_fwd(g["x"].repeat(1, 2)[:, ::2], g["wb"], g["b"], True),
    "fwd x misaligned": lambda e, g: e.linear_fwd(
        torch.zeros(5 * 96 + 1, device="cuda")[1:].view(5, 96), g["wb"], g["b"], True),
    "fwd x 1-D": lambda e, g: e.linear_fwd(g["x"][0], g["wb"], g["b"], True),
    "fwd empty batch": lambda e, g: e.linear_fwd(g["x"][:0], g["wb"], g["b"], True),
    "fwd fp32 weight": lambda e, g: e.linear_fwd(g["x"], g["w"], g["b"], True),
    "fwd K disagrees": lambda e, g: e.linear_fwd(g["x"], g["wb"][:, :64].contiguous(), g["b"], True),
    "fwd bias length": lambda e, g: e.linear_fwd(g["x"], g["wb"], g["b"][:63], True),
    "fwd bias on the CPU": lambda e, g: e.linear_fwd(g["x"], g["wb"], g["b"].cpu(), True),
    "fwd N = 32": lambda e, g: e.linear_fwd(g["x"], g["wb"][:32].contiguous(), g["b"][:32], True),
    "fwd K = 48": lambda e, g: e.linear_fwd(
        g["x"][:, :48].contiguous(), g["wb"][:, :48].contiguous(), g["b"], True),
    "pack on the CPU": lambda e, g: e.linear_pack(g["w"].cpu()),
    "pack bf16": lambda e, g: e.linear_pack(g["wb"]),
    "pack N = 32": lambda e, g: e.linear_pack(g["w"][:32].contiguous()),
    "pack strided": lambda e, g: e.linear_pack(g["w"].t().contiguous().t()),
    "dgrad y shape": lambda e, g: e.linear_dgrad(g["dy"], g["y"][:4], g["wt"], True),
    "dgrad [N, K] pack": lambda e, g: e.linear_dgrad(g["dy"], g["y"], g["wb"], True),
    "dgrad dy float64": lambda e, g: e.linear_dgrad(g["dy"].double(), g["y"], g["wt"], True),
    "wgrad rows disagree": lambda e, g: e.linear_wgrad(g["dy"], g["y"], g["x"][:4], True),
    "wgrad y on the CPU": lambda e, g: e.linear_wgrad(g["dy"], g["y"].cpu(), g["x"], True),
    "wgrad K = 48": lambda e, g: e.linear_wgrad(g["dy"], g["y"], g["x"][:, :48].contiguous(), True),
}


@pytest.mark.parametrize("name", list(BAD))
def test_host_checks_raise_before_any_launch(name):
    c = _case(5, 64, 96, True)
    ref, _, y = _refs(c)
    g = dict(_gpu(c), y=y.cuda())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    try:
        BAD[name](_ext(), g)
    except RuntimeError as e:
        assert "linear_" in str(e)
    else:
        pytest.fail(f"{name}: no error raised")
    assert torch.cuda.memory_allocated() == before  # nothing was allocated
    torch.cuda.synchronize()
    _assert_exact(_ext().linear_fwd(g["x"], g["wb"], g["b"], True), ref["y"],
                  "y after the refused call")


def test_supported():
    ext = _ext()
    for shape in ((1, 64, 32), (2592, 512, 3136), (2560, 256, 3872)):
        assert ext.linear_supported(*shape), shape
    for shape in ((0, 64, 32), (5, 32, 32), (5, 96, 32), (5, 64, 48),
                  (5, 64, 0), (2 ** 31, 64, 32)):
        assert not ext.linear_supported(*shape), shape


@pytest.mark.parametrize("x_grad", [True, False])
def test_autograd_function_exact(x_grad):
    """End to end against float64 autograd: which operand goes where."""
    m, n, k = 130, 128, 96
    c = _case(m, n, k, True)
    xd = _bf(c["x"]).requires_grad_()
    wd = _bf(c["w"]).requires_grad_()
    bd = c["b"].double().requires_grad_()
    F.relu(F.linear(xd, wd, bd)).backward(c["dy"].double())
    x = c["x"].cuda().requires_grad_(x_grad)
    w = c["w"].cuda().requires_grad_()
    b = c["b"].cuda().requires_grad_()
    y = tbf._LinearMfma.apply(x, w, b, True)
    y.backward(c["dy"].cuda())
    _assert_exact(y.detach(), F.relu(F.linear(xd, wd, bd)).detach(), "y")
    _assert_exact(w.grad, wd.grad, "dW")
    _assert_exact(b.grad, bd.grad, "db")
    if x_grad:
        _assert_exact(x.grad, xd.grad, "dx")
    else:
        assert x.grad is None
