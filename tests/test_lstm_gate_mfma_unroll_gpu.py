"""lstm_unroll with TBAMD_LSTM_GATE_MFMA=1: the recurrence of every layer on
ops/hip/lstm_gate_mfma.hip, against the float32 oracle of
tests/helpers/lstm_oracle.py (the arithmetic is lstm4's, so the oracle is the
same) for cases A, C, E and F, and once with TBAMD_LSTM_MFMA=1 as well
against that oracle with layer_in and W_ih rounded straight-through. All
outputs and all 6 + 4L gradients at the helper's tolerances. Unset, no
lstm_gate_* symbol is looked up.
"""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.ops import functional as tbops
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import lstm_oracle as lo  # noqa: E402


def _st(t):
    return t + (lo._bf(t) - t).detach()


def mimic_proj_bf16(core, x, notdone, state):
    """lo.lstm_mimic (float32, bf16 recurrent operands) with layer_in and
    W_ih rounded straight-through in the input projection."""
    notdone = notdone.float()
    h, c = (s.clone() for s in state)
    layer_in, hs, cs = x, [], []
    for l in range(core.num_layers):
        w_ih = getattr(core, f"weight_ih_l{l}")
        w_hh = getattr(core, f"weight_hh_l{l}")
        bias = getattr(core, f"bias_ih_l{l}") + getattr(core, f"bias_hh_l{l}")
        pre = _st(layer_in) @ _st(w_ih).t() + bias
        outs, hl, cl = [], h[l], c[l]
        for t in range(x.shape[0]):
            nd = notdone[t].view(-1, 1)
            gates = pre[t] + lo._bf(nd * hl) @ lo._bf(w_hh).t()
            gi, gf, gg, go = gates.chunk(4, dim=-1)
            cl = gf.sigmoid() * (nd * cl) + gi.sigmoid() * gg.tanh()
            hl = go.sigmoid() * cl.tanh()
            outs.append(hl)
        layer_in = torch.stack(outs)
        hs.append(hl)
        cs.append(cl)
    return layer_in, (torch.stack(hs), torch.stack(cs))


def _count_gate(monkeypatch):
    ext, seen = ops_mod.require_ext(), []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("lstm_gate_"):
                seen.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


def _gpu_result(core, x, notdone, h0, c0):
    res = lo.run(tbops.lstm_unroll, lo.clone_core(core).cuda(), x.cuda(),
                 notdone.cuda(), h0.cuda(), c0.cuda())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("name,both", [("A", False), ("C", False),
                                       ("E", False), ("F", False),
                                       ("A", True)])
def test_switch_on_matches_oracle(name, both, monkeypatch):
    monkeypatch.setenv("TBAMD_LSTM_GATE_MFMA", "1")
    if both:
        monkeypatch.setenv("TBAMD_LSTM_MFMA", "1")
    else:
        monkeypatch.delenv("TBAMD_LSTM_MFMA", raising=False)
    seen = _count_gate(monkeypatch)
    core, x, notdone, h0, c0 = lo.case_inputs(name)
    ref = (lo.run(mimic_proj_bf16, lo.clone_core(core), x, notdone, h0, c0)
           if both else lo.oracle(name))
    got = _gpu_result(core, x, notdone, h0, c0)
    assert "lstm_gate_supported" in seen
    assert set(got) == set(ref) and len(ref) == 6 + 4 * core.num_layers
    for key in sorted(ref):
        if key.startswith("d_"):
            err = lo.grad_error(got[key], ref[key])
            print(f"case {name} {key}: rel-max err {err:.5f}")
            assert got[key].shape == ref[key].shape, key
            assert err < lo.GRAD_TOL, f"grad {key}: rel-max err {err:.4f}"
        else:
            print(f"case {name} {key}: "
                  f"{lo.forward_excess(got[key], ref[key]):.4f} of tolerance")
            torch.testing.assert_close(got[key], ref[key], **lo.FWD_TOL,
                                       msg=lambda m, k=key: f"{k}: {m}")


def test_switch_off_never_looks_the_kernels_up(monkeypatch):
    monkeypatch.delenv("TBAMD_LSTM_GATE_MFMA", raising=False)
    seen = _count_gate(monkeypatch)
    core, x, notdone, h0, c0 = lo.case_inputs("A")
    first = _gpu_result(core, x, notdone, h0, c0)
    second = _gpu_result(core, x, notdone, h0, c0)
    assert seen == []
    for key in first:
        assert torch.equal(first[key], second[key]), key
