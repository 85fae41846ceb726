"""The bf16 MFMA LSTM projection kernels (ops/hip/lstm_proj_mfma.hip:
lstm_proj_pack, lstm_proj_fwd, lstm_proj_dgrad, lstm_proj_wgrad,
lstm_proj_supported) against float64 on the CPU, operands rounded by torch's
own .bfloat16().

Exact rule: `in` and `hm` hold integers in 0..300 (257, 258, 259 and 262 among
them, which bf16 cannot hold: round-to-nearest-even in staging is pinned),
weights in {-1, 0, 1}, integer biases, dg integers in -3..3. The largest sum is
the wgrad at M = 2560, 2560 * 3 * 300 < 2^24, so every partial sum is an
integer in any order and outputs are compared with torch.equal; _assert_exact
also holds every float64 reference to be non-constant and below 2^24.

Bounded rule: random operands pre-rounded to bf16 at the learner shapes,
within K * 2^-24 * S per element, S = sum |terms| (+ |b_ih| + |b_hh|),
K = 4 r. r = 2.53 is what plain float32 torch.matmul and its autograd reach
on the CPU against float64 on these same cases (largest of precomp, dx, dW_ih,
dW_hh and db: precomp at (2560, 257, 256); 1.68 at (2560, 519, 519)). The
kernels' own largest ratios on the MI355X: 1.97 (precomp), 2.30 (dx), 2.04
(dW_ih), 2.11 (dW_hh), 0.10 (db).

Shapes (M, I, H) come from the constants of ops/hip/lstm_proj_plan.h: 64 x 64
tiles, k-steps of 32, wgrad staging rounds of 128 rows dealt to at most 32
chunks below 256 tiles.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CPU_RATIO = 2.53  # measured: float32 torch.matmul and autograd on the CPU
K_BOUND = 4 * CPU_RATIO
U = 2.0 ** -24
PLANTED = torch.tensor([257.0, 258.0, 259.0, 262.0])


def _bf(t):
    return t.bfloat16().double()


def _plant(t):
    n = min(4, t.numel())
    t.view(-1)[:n] = PLANTED[:n]
    return t


@functools.lru_cache(maxsize=None)
def _case(m, i, h, exact):
    """Operands (float32, CPU), float64 references and the per-element sums
    of magnitudes S; built once per shape and never modified."""
    g = torch.Generator().manual_seed(m * 7919 + i * 31 + h)
    if exact:
        x = _plant(torch.randint(0, 301, (m, i), generator=g).float())
        hm = _plant(torch.randint(0, 301, (m, h), generator=g).float())
        w = torch.randint(-1, 2, (4 * h, i), generator=g).float()
        b_ih = torch.randint(-40, 41, (4 * h,), generator=g).float()
        b_hh = torch.randint(-40, 41, (4 * h,), generator=g).float()
        dg = torch.randint(-3, 4, (m, 4 * h), generator=g).float()
    else:
        x = torch.randn(m, i, generator=g).bfloat16().float()
        hm = torch.randn(m, h, generator=g).bfloat16().float()
        w = (torch.randn(4 * h, i, generator=g) / i ** 0.5).bfloat16().float()
        b_ih = torch.randn(4 * h, generator=g)
        b_hh = torch.randn(4 * h, generator=g)
        dg = torch.randn(m, 4 * h, generator=g).bfloat16().float()
    c = dict(x=x, hm=hm, w=w, b_ih=b_ih, b_hh=b_hh, dg=dg)
    xd, hd, wd, dd = _bf(x), _bf(hm), _bf(w), _bf(dg)
    ref = dict(y=xd @ wd.t() + b_ih.double() + b_hh.double(), dx=dd @ wd,
               dW_ih=dd.t() @ xd, dW_hh=dd.t() @ hd, db=dg.double().sum(0))
    s = dict(y=xd.abs() @ wd.abs().t() + b_ih.abs() + b_hh.abs(),
             dx=dd.abs() @ wd.abs(), dW_ih=dd.abs().t() @ xd.abs(),
             dW_hh=dd.abs().t() @ hd.abs(), db=dg.double().abs().sum(0))
    return c, ref, s


def _assert_exact(got, ref, what):
    assert ref.numel() == 1 or ref.min() != ref.max(), f"{what}: constant"
    assert ref.abs().max() < 2 ** 24, f"{what}: reference past 2^24"
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got.cpu().double(), ref), what


def _ratio(got, ref, s):
    assert ref.min() != ref.max()
    err = (got.cpu().double() - ref).abs()
    return float((err / (U * s).clamp_min(1e-300)).max())


# ---- GPU ----

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)


def _ext():
    return ops_mod.require_ext()


def _gpu(c):
    d = {k: v.cuda() for k, v in c.items()}
    d["wb"], d["wt"] = _ext().lstm_proj_pack(d["w"])
    return d


# M around the tile edge; I around the k-step (K tail of the forward, N tail
# of the dgrad; 32 on the 16-byte path, the others on the 4-byte one); 4H = 4
# below a fragment, 64 a full tile, 68 a tail of 4; I != H with the in/hm
# boundary inside the slab, (130, 257, 256) in two uneven wgrad chunks (128
# and 2 rows); the learner shape: 7 live columns in the last forward k-step,
# 28 in the last of the dgrad's 65.
SHAPES = [(1, 32, 16), (63, 32, 16), (64, 32, 16), (65, 32, 16),
          (65, 1, 16), (65, 31, 16), (65, 33, 16), (65, 33, 1), (65, 33, 17),
          (130, 5, 3), (130, 257, 256), (2560, 519, 519)]


@pytest.mark.parametrize("m,i,h", SHAPES)
def test_fwd_exact(m, i, h):
    c, ref, _ = _case(m, i, h, True)
    g = _gpu(c)
    y = _ext().lstm_proj_fwd(g["x"], g["wb"], g["b_ih"], g["b_hh"])
    _assert_exact(y, ref["y"], f"precomp {m, i, h}")
    assert torch.equal(
        y, _ext().lstm_proj_fwd(g["x"], g["wb"], g["b_ih"], g["b_hh"]))


@pytest.mark.parametrize("m,i,h", SHAPES)
def test_dgrad_exact(m, i, h):
    c, ref, _ = _case(m, i, h, True)
    g = _gpu(c)
    _assert_exact(_ext().lstm_proj_dgrad(g["dg"], g["wt"], i), ref["dx"],
                  f"dx {m, i, h}")


@pytest.mark.parametrize("m,i,h", SHAPES)
def test_wgrad_exact(m, i, h):
    c, ref, _ = _case(m, i, h, True)
    g = _gpu(c)
    dw_ih, dw_hh, db = _ext().lstm_proj_wgrad(g["dg"], g["x"], g["hm"])
    _assert_exact(dw_ih, ref["dW_ih"], f"dW_ih {m, i, h}")
    _assert_exact(dw_hh, ref["dW_hh"], f"dW_hh {m, i, h}")
    _assert_exact(db, ref["db"], f"db {m, i, h}")
    assert dw_ih.is_contiguous() and dw_hh.is_contiguous()
    assert dw_hh.data_ptr() == dw_ih.data_ptr() + 4 * dw_ih.numel()  # one slab


def test_base_off_alignment_takes_the_scalar_path():
    """Rows of 32 floats would allow 16-byte loads, the base 4 bytes past a
    16-byte boundary does not."""
    m, i, h = 65, 32, 16
    c, ref, _ = _case(m, i, h, True)
    g = _gpu(c)
    x = torch.zeros(m * i + 1, device="cuda")[1:].view(m, i).copy_(g["x"])
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    y = _ext().lstm_proj_fwd(x, g["wb"], g["b_ih"], g["b_hh"])
    _assert_exact(y, ref["y"], "precomp")
    dw_ih, dw_hh, _ = _ext().lstm_proj_wgrad(g["dg"], x, g["hm"])
    _assert_exact(dw_ih, ref["dW_ih"], "dW_ih")
    _assert_exact(dw_hh, ref["dW_hh"], "dW_hh")


@pytest.mark.parametrize("i,h", [(1, 1), (32, 16), (33, 17), (519, 519)])
def test_pack_bit_for_bit(i, h):
    w = torch.randn(4 * h, i, generator=torch.Generator().manual_seed(i))
    _plant(w)
    wb, wt = _ext().lstm_proj_pack(w.cuda())
    ip, np_ = -(-i // 32) * 32, -(-4 * h // 32) * 32
    want_b = torch.zeros(4 * h, ip, dtype=torch.bfloat16)
    want_b[:, :i] = w.bfloat16()
    want_t = torch.zeros(i, np_, dtype=torch.bfloat16)
    want_t[:, :4 * h] = w.bfloat16().t()
    assert wb.dtype == wt.dtype == torch.bfloat16
    assert wb.shape == want_b.shape and wt.shape == want_t.shape
    assert torch.equal(wb.cpu().view(torch.int16), want_b.view(torch.int16))
    assert torch.equal(wt.cpu().view(torch.int16), want_t.view(torch.int16))


@pytest.mark.parametrize("m,i,h", [(2560, 519, 519), (2560, 257, 256)])
def test_random_within_bound(m, i, h):
    c, ref, s = _case(m, i, h, False)
    g = _gpu(c)
    ext = _ext()
    dw_ih, dw_hh, db = ext.lstm_proj_wgrad(g["dg"], g["x"], g["hm"])
    got = dict(y=ext.lstm_proj_fwd(g["x"], g["wb"], g["b_ih"], g["b_hh"]),
               dx=ext.lstm_proj_dgrad(g["dg"], g["wt"], i),
               dW_ih=dw_ih, dW_hh=dw_hh, db=db)
    ratios = {name: _ratio(got[name], ref[name], s[name]) for name in ref}
    print(f"RATIO lstm_proj {m, i, h}: "
          + ", ".join(f"{a} {r:.3f}" for a, r in ratios.items())
          + f" of 2^-24*S, K = {K_BOUND:.2f}")
    assert max(ratios.values()) <= K_BOUND, ratios


def test_rows_past_2_31_elements():
    """M * 4H and M * I past 2^31: the last rows of dg, precomp and `in` lie
    beyond a 32-bit element offset. Only the first and last rows are
    non-zero, so two-row cases give the references."""
    ext = _ext()
    m, i, h = 262145, 8, 2048
    assert m * 4 * h > 2 ** 31
    c, ref, _ = _case(2, i, h, True)
    g = _gpu(c)
    x = torch.zeros(m, i, device="cuda")
    x[0], x[-1] = g["x"][0], g["x"][1]
    y = ext.lstm_proj_fwd(x, g["wb"], g["b_ih"], g["b_hh"])
    _assert_exact(y[[0, -1]], ref["y"], "precomp ends")
    assert torch.equal(y[1:-1], (g["b_ih"] + g["b_hh"]).expand(m - 2, 4 * h))
    y.zero_()  # reuse it as dg
    y[0], y[-1] = g["dg"][0], g["dg"][1]
    dx = ext.lstm_proj_dgrad(y, g["wt"], i)
    _assert_exact(dx[[0, -1]], ref["dx"], "dx ends")
    assert not bool(dx[1:-1].any())
    del x, y, dx

    m, i, h = 65537, 32768, 1
    assert m * i > 2 ** 31
    c, ref, _ = _case(2, i, h, True)
    g = _gpu(c)
    x = torch.zeros(m, i, device="cuda")
    hm = torch.zeros(m, h, device="cuda")
    dg = torch.zeros(m, 4 * h, device="cuda")
    for big, small in ((x, g["x"]), (hm, g["hm"]), (dg, g["dg"])):
        big[0], big[-1] = small[0], small[1]
    dw_ih, dw_hh, db = ext.lstm_proj_wgrad(dg, x, hm)
    _assert_exact(dw_ih, ref["dW_ih"], "dW_ih")
    _assert_exact(dw_hh, ref["dW_hh"], "dW_hh")
    _assert_exact(db, ref["db"], "db")


def _fwd(e, g, **kw):
    a = dict(g, **kw)
    return e.lstm_proj_fwd(a["x"], a["wb"], a["b_ih"], a["b_hh"])


BAD = {
    "fwd in on the CPU": lambda e, g: _fwd(e, g, x=g["x"].cpu()),
    "fwd in float64": lambda e, g: _fwd(e, g, x=g["x"].double()),
    "fwd in strided": lambda e, g: _fwd(e, g, x=g["x"].repeat(1, 2)[:, ::2]),
    "fwd in 1-D": lambda e, g: _fwd(e, g, x=g["x"][0]),
    "fwd empty batch": lambda e, g: _fwd(e, g, x=g["x"][:0]),
    "fwd fp32 weight": lambda e, g: _fwd(e, g, wb=g["w"]),
    "fwd pack not padded": lambda e, g: _fwd(e, g, wb=g["wb"][:, :33].contiguous()),
    "fwd pack rows": lambda e, g: _fwd(e, g, wb=g["wb"][:64].contiguous()),
    "fwd pack on the CPU": lambda e, g: _fwd(e, g, wb=g["wb"].cpu()),
    "fwd b_hh length": lambda e, g: _fwd(e, g, b_hh=g["b_hh"][:64]),
    "fwd b_ih not 4H": lambda e, g: _fwd(e, g, b_ih=g["b_ih"][:67], b_hh=g["b_hh"][:67]),
    "fwd b_ih on the CPU": lambda e, g: _fwd(e, g, b_ih=g["b_ih"].cpu()),
    "pack on the CPU": lambda e, g: e.lstm_proj_pack(g["w"].cpu()),
    "pack bf16": lambda e, g: e.lstm_proj_pack(g["wb"]),
    "pack rows not 4H": lambda e, g: e.lstm_proj_pack(g["w"][:67].contiguous()),
    "pack strided": lambda e, g: e.lstm_proj_pack(g["w"].t().contiguous().t()),
    "dgrad [4H, Ip] pack": lambda e, g: e.lstm_proj_dgrad(g["dg"], g["wb"], 33),
    "dgrad I disagrees": lambda e, g: e.lstm_proj_dgrad(g["dg"], g["wt"], 32),
    "dgrad I = 0": lambda e, g: e.lstm_proj_dgrad(g["dg"], g["wt"], 0),
    "dgrad dg float64": lambda e, g: e.lstm_proj_dgrad(g["dg"].double(), g["wt"], 33),
    "dgrad dg not 4H": lambda e, g: e.lstm_proj_dgrad(g["dg"][:, :66].contiguous(), g["wt"], 33),
    "wgrad in rows": lambda e, g: e.lstm_proj_wgrad(g["dg"], g["x"][:4], g["hm"]),
    "wgrad hm rows": lambda e, g: e.lstm_proj_wgrad(g["dg"], g["x"], g["hm"][:4]),
    "wgrad hm columns": lambda e, g: e.lstm_proj_wgrad(g["dg"], g["x"], g["hm"][:, :16].contiguous()),
    "wgrad hm on the CPU": lambda e, g: e.lstm_proj_wgrad(g["dg"], g["x"], g["hm"].cpu()),
    "wgrad in float64": lambda e, g: e.lstm_proj_wgrad(g["dg"], g["x"].double(), g["hm"]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_host_checks_raise_before_any_launch(name):
    c, ref, _ = _case(5, 33, 17, True)
    g = _gpu(c)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    try:
        BAD[name](_ext(), g)
    except RuntimeError as e:
        assert "lstm_proj_" in str(e)
    else:
        pytest.fail(f"{name}: no error raised")
    assert torch.cuda.memory_allocated() == before  # nothing was allocated
    torch.cuda.synchronize()
    _assert_exact(_fwd(_ext(), g), ref["y"], "precomp after the refused call")


def test_supported():
    ext = _ext()
    for shape in ((1, 1, 1), (2560, 519, 519), (2560, 257, 256),
                  (2 ** 31 - 256, 5, 5)):
        assert ext.lstm_proj_supported(*shape), shape
    for shape in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (2 ** 31, 5, 5),
                  (5, 2 ** 19 + 1, 5), (5, 5, 2 ** 19 + 1)):
        assert not ext.lstm_proj_supported(*shape), shape
