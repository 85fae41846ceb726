"""lstm_unroll with TBAMD_LSTM_GATE_WIDE=1 at learner batches above 64: the
recurrence of every layer on ops/hip/lstm_gate_wide.hip, against the float32
oracle of tests/helpers/lstm_oracle.py (the arithmetic is lstm4's, so the
oracle is the same). (L, H, B, T, I) = (2, 519, 138, 2, 24) is past lstm4's
LDS limit and raises without the switch; (1, 256, 256, 3, 257) is the largest
batch. All outputs and all 6 + 4L gradients at the helper's tolerances.
Unset, no lstm_gate_wide_* symbol is looked up.
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


def _inputs(L, H, B, T, I):
    state = torch.get_rng_state()
    torch.manual_seed(300 + H + B)
    core = torch.nn.LSTM(I, H, num_layers=L)
    x, h0, c0 = torch.randn(T, B, I), torch.randn(L, B, H), torch.randn(L, B, H)
    notdone = lo.make_notdone(T, B)
    torch.set_rng_state(state)
    return core, x, notdone, h0, c0


def _count_wide(monkeypatch):
    ext, seen = ops_mod.require_ext(), []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("lstm_gate_wide_"):
                seen.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    return seen


def _gpu_result(core, x, notdone, h0, c0):
    res = lo.run(tbops.lstm_unroll, lo.clone_core(core).cuda(), x.cuda(),
                 notdone.cuda(), h0.cuda(), c0.cuda())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("shape", [(2, 519, 138, 2, 24),
                                   (1, 256, 256, 3, 257)])
def test_switch_on_matches_oracle(shape, monkeypatch):
    monkeypatch.setenv("TBAMD_LSTM_GATE_WIDE", "1")
    monkeypatch.delenv("TBAMD_LSTM_MFMA", raising=False)
    seen = _count_wide(monkeypatch)
    core, x, notdone, h0, c0 = _inputs(*shape)
    ref = lo.run(lo.lstm_mimic, lo.clone_core(core), x, notdone, h0, c0)
    got = _gpu_result(core, x, notdone, h0, c0)
    assert "lstm_gate_wide_supported" in seen
    assert set(got) == set(ref) and len(ref) == 6 + 4 * core.num_layers
    for key in sorted(ref):
        if key.startswith("d_"):
            err = lo.grad_error(got[key], ref[key])
            print(f"{shape} {key}: rel-max err {err:.5f}")
            assert got[key].shape == ref[key].shape, key
            assert err < lo.GRAD_TOL, f"grad {key}: rel-max err {err:.4f}"
        else:
            print(f"{shape} {key}: "
                  f"{lo.forward_excess(got[key], ref[key]):.4f} of tolerance")
            torch.testing.assert_close(got[key], ref[key], **lo.FWD_TOL,
                                       msg=lambda m, k=key: f"{k}: {m}")


def test_switch_off_never_looks_the_kernels_up(monkeypatch):
    monkeypatch.delenv("TBAMD_LSTM_GATE_WIDE", raising=False)
    seen = _count_wide(monkeypatch)
    core, x, notdone, h0, c0 = _inputs(1, 40, 80, 2, 8)
    first = _gpu_result(core, x, notdone, h0, c0)
    second = _gpu_result(core, x, notdone, h0, c0)
    assert seen == []
    for key in first:
        assert torch.equal(first[key], second[key]), key
