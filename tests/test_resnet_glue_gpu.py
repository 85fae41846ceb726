"""The resnet_glue_* bindings (ops/hip/resnet_glue.hip) against float64 CPU
references computed from the same bf16-representable inputs.

Forwards are exact, so they are held with torch.equal: the pool's y, relu(y)
and tap index (F.max_pool2d on the CPU, index turned into ky * 3 + kx), a + s
rounded once, the ReLU + NCHW flatten. Backwards: with integer gradients
(|g| <= 64) every fp32 sum is exact and the result equals float64 autograd
rounded to bf16; with random bf16 gradients each element is held to
2^-8 |ref| + 2^-24 sum|terms| (half a bf16 ulp and one fp32 rounding of the
sum). Shapes: all-border windows, odd and even sizes, a width near the conv
kernels' bound, and (128, 13, 5), where the plan gives bands of two rows with
a short last one. 20-80 % of every compared value tensor is nonzero (the tap
index is an index, not a value).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

CL = torch.channels_last
BF = torch.bfloat16
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 5, 7), (3, 13, 37), (2, 42, 42),
          (1, 3, 250), (128, 13, 5)]
CASES = [(c, s) for c in (16, 32) for s in SHAPES]


def _ext():
    return ops_mod.require_ext()


def _dev(t):
    return None if t is None else t.cuda().contiguous(memory_format=CL)


def _sane(t, lo=0.2, hi=0.8):
    frac = (t != 0).double().mean().item()
    assert lo <= frac <= hi, f"{frac:.2f} of the compared tensor is nonzero"


def _grad(shape, gen, ints, density=1.0):
    if ints:
        g = torch.randint(1, 65, shape, generator=gen).double()
        g = g * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    else:
        g = torch.randn(shape, generator=gen, dtype=torch.float64)
    g = g * (torch.rand(shape, generator=gen) < density)
    return g.to(BF).contiguous(memory_format=CL)


@functools.lru_cache(maxsize=None)
def _pool_case(c, shape):
    """Input and CPU forward of the pool: window centres are positive (40 %),
    zero (40 %) or negative, everything else negative with 10 % zeros, so
    relu(y) is mixed and equal maxima (zeros) meet the tie rule."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(1000 * c + 100 * n + 10 * h + w)
    x = -(torch.rand(n, c, h, w, generator=gen) * 4 + 0.25)
    x[torch.rand(x.shape, generator=gen) < 0.1] = 0
    centre = x[:, :, ::2, ::2]
    u = torch.rand(centre.shape, generator=gen)
    centre[u < 0.8] = 0
    centre[u < 0.4] = torch.rand(centre.shape, generator=gen)[u < 0.4] + 0.5
    x = x.to(BF).contiguous(memory_format=CL)
    y, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    return x, y, F.relu(y), _taps(flat, w)


def _taps(flat, w):
    """max_pool2d's flat input index -> ky * 3 + kx of its window."""
    oh, ow = flat.shape[2:]
    oy = torch.arange(oh).view(1, 1, oh, 1)
    ox = torch.arange(ow).view(1, 1, 1, ow)
    ky = torch.div(flat, w, rounding_mode="floor") - (2 * oy - 1)
    kx = flat % w - (2 * ox - 1)
    return (ky * 3 + kx).to(torch.uint8)


def _pool_ref_bwd(x, g_y, g_r):
    """float64 autograd of g_y . y + g_r . relu(y); a missing gradient is 0."""
    x64 = x.double().requires_grad_()
    y = F.max_pool2d(x64, 3, 2, 1)
    loss = 0.0
    if g_y is not None:
        loss = loss + (y * g_y.double()).sum()
    if g_r is not None:
        loss = loss + (F.relu(y) * g_r.double()).sum()
    return torch.autograd.grad(loss, x64)[0]


def _held(got, ref, terms):
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -24 * terms
    excess = ((got.double() - ref).abs() - tol).max().item()
    assert excess <= 0, f"{excess:.3e} over the tolerance"


@pytest.mark.parametrize("c,shape", CASES)
def test_pool_forward_is_exact(c, shape):
    x, y, r, taps = _pool_case(c, shape)
    got_y, got_r, got_idx = _ext().resnet_glue_pool_fwd(_dev(x))
    assert got_y.is_contiguous(memory_format=CL)
    assert torch.equal(got_y.cpu(), y) and torch.equal(got_r.cpu(), r)
    assert torch.equal(got_idx.cpu(), taps)
    _sane(y), _sane(r)
    assert 0 < (y > 0).sum() < y.numel()


def test_pool_plan_gives_short_last_band():
    rows, bands, lds = _ext().resnet_glue_pool_plan(128, 13, 5, 16)
    assert rows >= 2 and bands >= 2 and 7 % rows != 0
    assert lds == min(2 * rows + 1, 13) * 5 * 16 * 2


@pytest.mark.parametrize("kind", ["constant", "nan"])
def test_pool_tie_and_nan_rule(kind):
    x = torch.ones(2, 16, 5, 7)
    if kind == "nan":
        x = torch.randn(2, 16, 5, 7, generator=torch.Generator().manual_seed(3))
        x[0, :, 2, 3] = float("nan")   # in four windows
        x[1, 3, 1:3, 1] = float("nan")  # two NaNs in one window
    x = x.to(BF).contiguous(memory_format=CL)
    y, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    got_y, got_r, got_idx = _ext().resnet_glue_pool_fwd(_dev(x))
    assert torch.equal(got_idx.cpu(), _taps(flat, 7))
    assert torch.equal(got_y.cpu().isnan(), y.isnan())
    assert y.isnan().any() == (kind == "nan")
    assert torch.equal(got_y.cpu().nan_to_num(7.0), y.nan_to_num(7.0))
    assert torch.equal(got_r.cpu().nan_to_num(7.0), F.relu(y).nan_to_num(7.0))


@pytest.mark.parametrize("ints", [True, False], ids=["ints", "random"])
@pytest.mark.parametrize("c,shape", CASES)
def test_pool_backward(c, shape, ints):
    x, y, r, taps = _pool_case(c, shape)
    gen = torch.Generator().manual_seed(7 + c + sum(shape))
    # dx has one nonzero per window at most: dense gradients, except where
    # the window is the whole 1 x 1 input.
    density = 0.5 if shape[1:] == (1, 1) else 1.0
    g_y, g_r = (_grad(y.shape, gen, ints, density) for _ in range(2))
    ref = _pool_ref_bwd(x, g_y, g_r)
    # relu(y) serves as the mask: only the sign is read.
    got = _ext().resnet_glue_pool_bwd(_dev(g_y), _dev(g_r), _dev(r),
                                      _dev(taps), shape[1], shape[2])
    assert got.shape == x.shape and got.is_contiguous(memory_format=CL)
    if ints:
        assert torch.equal(got.cpu(), ref.to(BF))
    else:
        _held(got.cpu(), ref, _pool_ref_bwd(x, g_y.abs(), g_r.abs()))
    _sane(ref.to(BF))


@pytest.mark.parametrize("missing", ["g_y", "g_r", "bad_idx"])
def test_pool_backward_missing_gradient_and_bad_index(missing):
    c, shape = 32, (2, 5, 7)
    x, y, r, taps = _pool_case(c, shape)
    gen = torch.Generator().manual_seed(11)
    g_y, g_r = _grad(y.shape, gen, True), _grad(y.shape, gen, True)
    if missing == "g_y":
        g_y = None
    elif missing == "g_r":
        g_r = None
    ref_y, ref_r = g_y, g_r
    if missing == "bad_idx":
        # Byte 200 names no tap: that element gives nothing, all else stays.
        taps = taps.clone()
        taps[1, 5, 2, 3] = 200
        ref_y, ref_r = g_y.clone(), g_r.clone()
        ref_y[1, 5, 2, 3] = 0
        ref_r[1, 5, 2, 3] = 0
    got = _ext().resnet_glue_pool_bwd(
        _dev(g_y), _dev(g_r), _dev(y if g_r is not None else None),
        _dev(taps), 5, 7)
    assert torch.equal(got.cpu(), _pool_ref_bwd(x, ref_y, ref_r).to(BF))


@functools.lru_cache(maxsize=None)
def _ew_case(c, shape):
    n, h, w = shape
    gen = torch.Generator().manual_seed(2000 * c + 100 * n + 10 * h + w)
    a = _grad((n, c, h, w), gen, False, 0.4)
    s = _grad((n, c, h, w), gen, False, 0.4)
    z = (a.double() + s.double()).to(BF)
    return a, s, z


@pytest.mark.parametrize("c,shape", CASES)
def test_ew_forward_is_exact(c, shape):
    a, s, z = _ew_case(c, shape)
    ext = _ext()
    got_z, got_r = ext.resnet_glue_ew_fwd(_dev(a), _dev(s), True)
    assert torch.equal(got_z.cpu(), z) and torch.equal(got_r.cpu(), F.relu(z))
    only_z, none_r = ext.resnet_glue_ew_fwd(_dev(a), _dev(s), False)
    assert none_r is None and torch.equal(only_z.cpu(), z)
    none_z, only_r = ext.resnet_glue_ew_fwd(_dev(z), None, True)
    assert none_z is None and torch.equal(only_r.cpu(), F.relu(z))
    _sane(z), _sane(F.relu(z))
    assert 0 < (z > 0).sum() < z.numel()


@pytest.mark.parametrize("mode", ["ints", "random", "no_g_z", "no_g_r"])
@pytest.mark.parametrize("c,shape", CASES)
def test_ew_backward(c, shape, mode):
    a, s, z = _ew_case(c, shape)
    gen = torch.Generator().manual_seed(13 + c + sum(shape))
    g_z = _grad(z.shape, gen, mode != "random", 0.4)
    g_r = _grad(z.shape, gen, mode != "random")
    g_z = None if mode == "no_g_z" else g_z
    g_r = None if mode == "no_g_r" else g_r
    t_z = 0 if g_z is None else g_z.double()
    t_r = 0 if g_r is None else g_r.double() * (z > 0)
    ref = t_z + t_r
    got = _ext().resnet_glue_ew_bwd(
        _dev(g_z), _dev(g_r), _dev(z if g_r is not None else None)).cpu()
    if mode == "random":
        _held(got, ref, abs(t_z) + abs(t_r))
    else:
        assert torch.equal(got, ref.to(BF))
    _sane(ref.to(BF))


@pytest.mark.parametrize("c,shape", CASES)
def test_flatten_forward_and_backward(c, shape):
    n, h, w = shape
    gen = torch.Generator().manual_seed(3000 * c + 100 * n + 10 * h + w)
    x = _grad((n, c, h, w), gen, False)
    ref = F.relu(x.float()).reshape(n, -1)
    got = _ext().resnet_glue_flat_fwd(_dev(x))
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), ref)
    # One term per element: the fp32 gradient rounded to bf16, or zero.
    g = torch.randn(n, c * h * w, generator=gen)
    ref_dx = (g.view(n, c, h, w) * (x > 0)).to(BF)
    got_dx = _ext().resnet_glue_flat_bwd(g.cuda(), _dev(x))
    assert got_dx.is_contiguous(memory_format=CL)
    assert torch.equal(got_dx.cpu(), ref_dx)
    _sane(ref), _sane(ref_dx)
    assert 0 < (x > 0).sum() < x.numel()


def _act(c=16, h=4, w=6, dtype=BF, device="cuda"):
    return torch.zeros(2, c, h, w, dtype=dtype,
                       device=device).contiguous(memory_format=CL)


def _misaligned():
    buf = torch.zeros(2 * 16 * 4 * 6 + 4, dtype=BF, device="cuda")
    return buf[4:].view(2, 4, 6, 16).permute(0, 3, 1, 2)


HOST_CHECKS = {
    "device": ("resnet_glue_pool_fwd", lambda: (_act(device="cpu"),),
               "x must be a GPU tensor"),
    "dtype": ("resnet_glue_flat_fwd", lambda: (_act(dtype=torch.float16),),
              "x must be BFloat16"),
    "layout": ("resnet_glue_pool_fwd",
               lambda: (torch.zeros(2, 16, 4, 6, dtype=BF, device="cuda"),),
               "x must be contiguous in channels_last"),
    "alignment": ("resnet_glue_ew_fwd", lambda: (_misaligned(), None, True),
                  "a must be 16-byte aligned"),
    "channels": ("resnet_glue_ew_fwd", lambda: (_act(c=24), None, True),
                 "a must have 16 or 32 channels"),
    "dims": ("resnet_glue_flat_fwd",
             lambda: (torch.zeros(2, 16, 4, dtype=BF, device="cuda"),),
             "x must be .N, C, H, W."),
    "shape": ("resnet_glue_ew_fwd", lambda: (_act(), _act(h=5), True),
              "s has shape"),
    "nothing": ("resnet_glue_ew_fwd", lambda: (_act(), None, False),
                "nothing to do"),
    "mask": ("resnet_glue_ew_bwd", lambda: (None, _act(), None),
             "z is needed with g_r"),
    "no_grads": ("resnet_glue_pool_bwd",
                 lambda: (None, None, None, _act(dtype=torch.uint8), 8, 12),
                 "g_y and g_r are both missing"),
    "pool_size": ("resnet_glue_pool_bwd",
                  lambda: (_act(), None, None, _act(dtype=torch.uint8), 9, 12),
                  "pools to"),
    "idx_dtype": ("resnet_glue_pool_bwd",
                  lambda: (_act(), None, None, _act(), 8, 12),
                  "idx must be Byte"),
    # One input row of 512 KiB: more LDS than a CDNA workgroup can have.
    "lds": ("resnet_glue_pool_fwd", lambda: (_act(h=1, w=16384),),
            "bytes of LDS"),
    "flat_grad": ("resnet_glue_flat_bwd",
                  lambda: (torch.zeros(2, 16 * 4 * 6 + 1, device="cuda"),
                           _act()),
                  "g has shape"),
}


@pytest.mark.parametrize("check", sorted(HOST_CHECKS))
def test_host_checks_raise_and_name_the_argument(check):
    name, args, message = HOST_CHECKS[check]
    with pytest.raises(RuntimeError, match=message):
        getattr(_ext(), name)(*args())
