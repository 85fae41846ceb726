"""The LSTM oracle held to account, on the CPU.

tests/helpers/lstm_oracle.py is what the GPU tests of the done-masked
unroll compare against, so it is itself checked here: the exact recurrence
(float64, no bf16 rounding) against nn.LSTM driven by the eager branch of
tbops.lstm_unroll, and, on the very inputs of the GPU cases, that two
plausible kernel mistakes move the oracle's answer by at least ten times
the tolerance the GPU comparison allows, so that comparison could not pass
over either of them."""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import lstm_oracle as lo  # noqa: E402
from torchbeast_amd.ops import functional as tbops  # noqa: E402


def test_exact_oracle_matches_nn_lstm_float64():
    L, H, B, T, I = 2, 11, 9, 4, 5
    torch.manual_seed(11)
    core = torch.nn.LSTM(I, H, num_layers=L).double()
    x = torch.randn(T, B, I, dtype=torch.float64)
    h0 = torch.randn(L, B, H, dtype=torch.float64)
    c0 = torch.randn(L, B, H, dtype=torch.float64)
    notdone = lo.make_notdone(T, B).double()

    ref = lo.run(tbops.lstm_unroll, lo.clone_core(core, torch.float64), x,
                 notdone, h0, c0)
    exact = functools.partial(lo.lstm_mimic, dtype=torch.float64,
                              round_bf16=False)
    got = lo.run(exact, lo.clone_core(core, torch.float64), x, notdone, h0,
                 c0)

    assert set(got) == set(ref)
    assert {"d_x", "d_h0", "d_c0", "d_weight_hh_l1", "d_bias_ih_l0"} <= set(got)
    for name in ref:
        assert got[name].dtype == torch.float64, name
        torch.testing.assert_close(got[name], ref[name], rtol=1e-10,
                                   atol=1e-10, msg=lambda m, n=name: f"{n}: {m}")


def test_float32_rounding_oracle_is_the_default():
    """The switches' defaults are the oracle test_ops_gpu.py always had:
    float32 arithmetic, operands of the recurrent matmul rounded to bf16."""
    core, x, notdone, h0, c0 = lo.case_inputs("E")
    out_d, (hT_d, cT_d) = lo.lstm_mimic(core, x, notdone, (h0, c0))
    out_e, (hT_e, cT_e) = lo.lstm_mimic(core, x, notdone, (h0, c0),
                                        dtype=torch.float32, round_bf16=True)
    assert out_d.dtype == torch.float32
    assert torch.equal(out_d, out_e) and torch.equal(hT_d, hT_e)
    assert torch.equal(cT_d, cT_e)
    # and the rounding is really applied: the exact recurrence differs.
    out_x, _ = lo.lstm_mimic(core, x, notdone, (h0, c0), round_bf16=False)
    assert not torch.equal(out_d, out_x)


def _separation(wrong, right):
    """The largest figure, over the quantities the GPU comparison looks at,
    of error / tolerance, and the quantity that shows it."""
    worst, where = 0.0, None
    for name, ref in right.items():
        if name in ("out", "hT", "cT"):
            ratio = lo.forward_excess(wrong[name], ref)
        else:
            ratio = lo.grad_error(wrong[name], ref) / lo.GRAD_TOL
        if ratio > worst:
            worst, where = ratio, name
    return worst, where


def _dropped_hidden_unit(core, x, notdone, state):
    """The recurrent dot product stops one short: column H-1 of every W_hh
    is read as zero."""
    H = core.hidden_size
    drop = torch.zeros(H, dtype=torch.float64)
    drop[H - 1] = 1

    class Dropped:
        """`core` with the column's values zeroed. Its gradient still
        passes: the kernel's dW_hh comes from a separate GEMM, which a
        short dot product in the recurrence would not shorten."""
        num_layers = core.num_layers

        def __getattr__(self, name):
            p = getattr(core, name)
            if name.startswith("weight_hh"):
                p = p.double()
                p = p - (p * drop).detach()
            return p

    return lo.lstm_mimic(Dropped(), x, notdone, state, dtype=torch.float64)


def _stale_batch_chunk(core, x, notdone, state):
    """Rows of the second and later chunks of 8 see the done mask of the
    chunk before."""
    stale = notdone.clone()
    stale[:, 8:] = notdone[:, :-8]
    return lo.lstm_mimic(core, x, stale, state, dtype=torch.float64)


@pytest.mark.parametrize("mistake", [_dropped_hidden_unit,
                                     _stale_batch_chunk])
@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_oracle_separates_kernel_mistakes(name, mistake):
    core, x, notdone, h0, c0 = lo.case_inputs(name)
    right = lo.oracle(name, torch.float64, True)
    wrong = lo.run(mistake, lo.clone_core(core), x, notdone, h0, c0)
    ratio, where = _separation(wrong, right)
    print(f"case {name} {mistake.__name__}: {ratio:.1f}x tolerance on {where}")
    assert ratio >= 10.0, (
        f"case {name}: {mistake.__name__} moves the oracle by only "
        f"{ratio:.2f}x the GPU tolerance (most on {where})")


@pytest.mark.parametrize("name", sorted(lo.CASES))
def test_float32_oracle_within_tolerance_of_float64(name):
    """Float32 summation in the oracle costs far less than the margin the
    GPU comparison leaves: a bf16 rounding that flips is what remains."""
    f32 = lo.oracle(name)
    f64 = lo.oracle(name, torch.float64, True)
    ratio, where = _separation(f32, f64)
    print(f"case {name}: float32 oracle at {ratio:.3f}x tolerance on {where}")
    assert ratio < 0.5, (name, ratio, where)
