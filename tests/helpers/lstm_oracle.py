"""Eager oracle of the done-masked LSTM unroll, shared by the LSTM tests.

`lstm_mimic` is the recurrence `ops/hip/lstm_v4.hip` implements, written as a
plain PyTorch loop so that autograd supplies every gradient. It has two
switches: the arithmetic type, and whether the recurrent-matmul operands are
rounded to bf16 where the kernel rounds them. float32 with rounding is the
precision-faithful oracle the GPU tests compare against; float64 without
rounding is the exact recurrence, which tests/test_lstm_oracle.py holds
against nn.LSTM itself.

The module also holds the shapes and inputs of the GPU cases, so that the
CPU tests that prove the oracle sensitive run on exactly those inputs.
"""

import functools

import torch

# (L, H, B, T, I) of the GPU cases; what each one reaches in the kernels is
# listed in tests/test_lstm_unroll_gpu.py.
CASES = {
    "A": (2, 519, 32, 6, 24),
    "B": (1, 175, 9, 5, 24),
    "C": (2, 521, 11, 4, 24),
    "D": (1, 32, 1, 1, 24),
    "E": (1, 8, 17, 3, 5),
    "F": (1, 519, 64, 2, 8),
}

# Tolerances of the comparison with the kernel (the ones test_ops_gpu.py has
# always used): forward per element, gradients max-scaled.
FWD_TOL = dict(rtol=2e-3, atol=2e-3)
GRAD_TOL = 2e-2
GRAD_FLOOR = 1e-4


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def lstm_mimic(core, x, notdone, state, dtype=torch.float32,
               round_bf16=True):
    """Eager unroll that rounds the recurrent-matmul operands to bf16 where
    the v4 kernel does (gates = precomp + bf16(masked h) @ bf16(W_hh)^T, the
    cell path unrounded) — the precision-faithful oracle. All arithmetic
    runs in `dtype`; `round_bf16=False` gives the exact recurrence."""
    rnd = _bf if round_bf16 else (lambda t: t)
    L = core.num_layers
    x = x.to(dtype)
    notdone = notdone.to(dtype)
    h, c = (s.to(dtype).clone() for s in state)
    layer_in = x
    for l in range(L):
        w_ih = getattr(core, f"weight_ih_l{l}").to(dtype)
        w_hh = getattr(core, f"weight_hh_l{l}").to(dtype)
        bias = (getattr(core, f"bias_ih_l{l}").to(dtype)
                + getattr(core, f"bias_hh_l{l}").to(dtype))
        pre = layer_in @ w_ih.t() + bias
        outs = []
        hl, cl = h[l], c[l]
        for t in range(x.shape[0]):
            nd = notdone[t].view(-1, 1)
            hm = nd * hl
            cmt = nd * cl
            gates = pre[t] + rnd(hm) @ rnd(w_hh).t()
            gi, gf, gg, go = gates.chunk(4, dim=-1)
            gi, gf, go = gi.sigmoid(), gf.sigmoid(), go.sigmoid()
            gg = gg.tanh()
            cl = gf * cmt + gi * gg
            hl = go * cl.tanh()
            outs.append(hl)
        layer_in = torch.stack(outs)
        h = torch.cat([h[:l], hl.unsqueeze(0), h[l + 1:]])
        c = torch.cat([c[:l], cl.unsqueeze(0), c[l + 1:]])
    return layer_in, (h, c)


def make_notdone(T, B):
    """rand > 0.2, then the edges forced: the first and the last element
    done, and for B > 2 a whole column done (a row that never carries
    state). Draws from the global generator."""
    notdone = (torch.rand(T, B) > 0.2).float()
    notdone[0, 0] = 0
    notdone[T - 1, B - 1] = 0
    if B > 2:
        notdone[:, 1] = 0
    return notdone


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(core, x, notdone, h0, c0) of one case, float32 on the CPU; built
    once and shared, so nothing in it may be modified."""
    L, H, B, T, I = CASES[name]
    state = torch.get_rng_state()
    torch.manual_seed(100 + ord(name))
    core = torch.nn.LSTM(I, H, num_layers=L)
    x = torch.randn(T, B, I)
    h0 = torch.randn(L, B, H)
    c0 = torch.randn(L, B, H)
    notdone = make_notdone(T, B)
    torch.set_rng_state(state)
    for p in core.parameters():
        p.requires_grad_(False)
    return core, x, notdone, h0, c0


def clone_core(core, dtype=torch.float32):
    """A trainable copy of `core`, so the shared one never gains grads."""
    new = torch.nn.LSTM(core.input_size, core.hidden_size,
                        num_layers=core.num_layers)
    new.load_state_dict(core.state_dict())
    return new.to(dtype)


def loss_of(out, hT, cT):
    return out.square().sum() + hT.sum() + cT.sum()


def run(fn, core, x, notdone, h0, c0):
    """Call `fn(core, x, notdone, (h0, c0))` on fresh leaves, backpropagate
    the test loss and return every compared quantity by name: out, hT, cT,
    d_x, d_h0, d_c0 and d_<parameter>."""
    x = x.detach().clone().requires_grad_()
    h0 = h0.detach().clone().requires_grad_()
    c0 = c0.detach().clone().requires_grad_()
    out, (hT, cT) = fn(core, x, notdone, (h0, c0))
    loss_of(out, hT, cT).backward()
    res = dict(out=out.detach(), hT=hT.detach(), cT=cT.detach(),
               d_x=x.grad, d_h0=h0.grad, d_c0=c0.grad)
    for name, p in core.named_parameters():
        res["d_" + name] = p.grad
    return res


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32, round_bf16=True):
    """The oracle's answer for one case; computed once and shared."""
    core, x, notdone, h0, c0 = case_inputs(name)
    fn = functools.partial(lstm_mimic, dtype=dtype, round_bf16=round_bf16)
    return run(fn, clone_core(core), x, notdone, h0, c0)


def forward_excess(got, ref):
    """max over elements of |got-ref| / (atol + rtol*|ref|): above 1 where
    assert_close with FWD_TOL would fail."""
    got, ref = got.double(), ref.double()
    bound = FWD_TOL["atol"] + FWD_TOL["rtol"] * ref.abs()
    return float(((got - ref).abs() / bound).max())


def grad_error(got, ref):
    """The max-scaled measure of the gradient comparison."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().clamp_min(GRAD_FLOOR)
    return float((got - ref).abs().max() / scale)
