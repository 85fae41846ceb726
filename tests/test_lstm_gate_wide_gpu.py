"""The wide-batch persistent MFMA LSTM kernels of ops/hip/lstm_gate_wide.hip
through their direct bindings (one layer), against a float64 recurrence with
the matmul operands rounded to bf16 where the kernels round them.

Forward: out, hT, cT and the stash [gates, hm, cm, c] within lo.FWD_TOL;
hm[t] == nd[t] * out[t-1] and cm[t] == nd[t] * c[t-1] bit for bit. Backward
(fed the reference stash): dgates, dh0, dc0 with lo.grad_error < lo.GRAD_TOL
and rows done at t = 0 exactly zero.

(H, B, T) and what each reaches:
  (8, 65, 3)      below one k-step; one live row in the last batch fragment
  (40, 129, 3)    first batch with two fragments on a wave
  (175, 80, 5)    ragged last workgroup, scalar stores, both buffers reused
  (519, 128, 4)   a real model width at a batch lstm4 still accepts
  (521, 138, 3)   past lstm4's limit
  (519, 256, 2)   the largest batch
  (1024, 256, 2)  the largest LDS footprint; the 16-byte store path
  (32, 1, 1)      the smallest everything
"""

import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import lstm_oracle as lo  # noqa: E402

SHAPES = [(8, 65, 3), (40, 129, 3), (175, 80, 5), (519, 128, 4),
          (521, 138, 3), (519, 256, 2), (1024, 256, 2), (32, 1, 1)]
FWD_NAMES = ("out", "hT", "cT", "gates", "hm", "cm", "c")


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ref_fwd(pre, w, nd, h0, c0):
    """float64; returns out, hT, cT, gates, hm, cm, c like the binding."""
    h, c, wb, rows = h0, c0, _bf(w), []
    for t in range(pre.shape[0]):
        m = nd[t].view(-1, 1)
        hm, cm = m * h, m * c
        gi, gf, gg, go = (pre[t] + _bf(hm) @ wb.t()).chunk(4, dim=-1)
        gi, gf, gg, go = gi.sigmoid(), gf.sigmoid(), gg.tanh(), go.sigmoid()
        c = gf * cm + gi * gg
        h = go * c.tanh()
        rows.append((h, torch.cat([gi, gf, gg, go], -1), hm, cm, c))
    out, gates, hms, cms, cs = (torch.stack(x) for x in zip(*rows))
    return out, h, c, gates, hms, cms, cs


def ref_bwd(gates, cm, c, w, nd, d_out, d_hT, d_cT):
    """float64; returns dgates, dh0, dc0 like the binding."""
    dh, dc, wb, rows = d_hT, d_cT, _bf(w), []
    for t in reversed(range(gates.shape[0])):
        gi, gf, gg, go = gates[t].chunk(4, dim=-1)
        dh_t, tc = dh + d_out[t], c[t].tanh()
        dc_t = dc + dh_t * go * (1 - tc * tc)
        dg = torch.cat([dc_t * gg * gi * (1 - gi), dc_t * cm[t] * gf * (1 - gf),
                        dc_t * gi * (1 - gg * gg), dh_t * tc * go * (1 - go)],
                       -1)
        m = nd[t].view(-1, 1)
        dh, dc = m * (_bf(dg) @ wb), m * dc_t * gf
        rows.append(dg)
    return torch.stack(rows[::-1]), dh, dc


@functools.lru_cache(maxsize=None)
def make(H, B, T):
    """Inputs and the float64 forward of one shape; built once, never
    modified."""
    state = torch.get_rng_state()
    torch.manual_seed(2000 + 7 * H + B + T)
    pre = torch.randn(T, B, 4 * H)
    w = torch.randn(4 * H, H) / H ** 0.5
    h0, c0 = torch.randn(B, H), torch.randn(B, H)
    nd = lo.make_notdone(T, B)
    grads = (torch.randn(T, B, H), torch.randn(B, H), torch.randn(B, H))
    torch.set_rng_state(state)
    ref = ref_fwd(*(t.double() for t in (pre, w, nd, h0, c0)))
    return (pre, w, nd, h0, c0), grads, ref


def _gpu(fn, *tensors):
    res = fn(*(t.cuda() for t in tensors))
    torch.cuda.synchronize()
    return [r.cpu() for r in res]


@pytest.mark.parametrize("H,B,T", SHAPES)
def test_forward(H, B, T):
    (pre, w, nd, h0, c0), _, ref = make(H, B, T)
    got = _gpu(ops_mod.require_ext().lstm_gate_wide_fwd, pre, w, nd, h0, c0)
    for name, g, r in zip(FWD_NAMES, got, ref):
        print(f"{name}: {lo.forward_excess(g, r.float()):.4f} of tolerance")
        torch.testing.assert_close(g, r.float(), **lo.FWD_TOL,
                                   msg=lambda m, k=name: f"{k}: {m}")
    out, _, _, _, hm, cm, c = got
    m = nd.unsqueeze(-1)
    assert torch.equal(hm[0], m[0] * h0) and torch.equal(cm[0], m[0] * c0)
    assert torch.equal(hm[1:], m[1:] * out[:-1])
    assert torch.equal(cm[1:], m[1:] * c[:-1])
    assert torch.equal(got[1], out[-1]) and torch.equal(got[2], c[-1])


@pytest.mark.parametrize("H,B,T", SHAPES)
def test_backward(H, B, T):
    (pre, w, nd, h0, c0), (d_out, d_hT, d_cT), fwd = make(H, B, T)
    _, _, _, gates, _, cm, c = fwd
    args = (gates, cm, c, w, nd, d_out, d_hT, d_cT)
    ref = ref_bwd(*(t.double() for t in args))
    got = _gpu(ops_mod.require_ext().lstm_gate_wide_bwd,
               *(t.float() for t in args))
    for name, g, r in zip(("dgates", "dh0", "dc0"), got, ref):
        err = lo.grad_error(g, r)
        print(f"{name}: rel-max err {err:.5f}")
        assert g.shape == r.shape and err < lo.GRAD_TOL, name
    done0 = nd[0] == 0
    assert done0.any()
    assert (got[1][done0] == 0).all() and (got[2][done0] == 0).all()


@pytest.mark.parametrize("what", ["batch", "width", "device", "dtype"])
def test_host_checks_raise_before_launch(what):
    ext = ops_mod.require_ext()
    H, B = (1025 if what == "width" else 8), (257 if what == "batch" else 3)
    fwd = [torch.rand(2, B, 4 * H), torch.rand(4 * H, H), torch.ones(2, B),
           torch.rand(B, H), torch.rand(B, H)]
    fwd = [t.cuda() for t in fwd]
    st = torch.rand(2, B, H).cuda()
    bwd = [fwd[0], st, st, fwd[1], fwd[2], st, fwd[3], fwd[4]]
    if what == "device":
        fwd[2], bwd[4], match = fwd[2].cpu(), fwd[2].cpu(), "notdone"
    elif what == "dtype":
        fwd[4], bwd[1], match = fwd[4].double(), st.double(), "Float"
    else:
        match = f"unsupported shape B={B} H={H}"
        assert not ext.lstm_gate_wide_supported(B, H)
    with pytest.raises(RuntimeError, match=match):
        ext.lstm_gate_wide_fwd(*fwd)
    with pytest.raises(RuntimeError, match=match):
        ext.lstm_gate_wide_bwd(*bwd)
