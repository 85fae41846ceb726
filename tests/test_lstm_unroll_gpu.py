"""The persistent done-masked LSTM unroll (ops/hip/lstm_v4.hip) against the
float32 bf16-rounding oracle, at the shapes where its loops change shape.

case  L   H   B  T  I   reaches
A     2  519  32 6  24  bench shape: 5 staging rounds of h (B*H = 16608 over
                        4096 floats a round), 4 full backward chunks, hs=3
B     1  175   9 5  24  hs=2, 88 workgroups, the last with one row (rs=1);
                        backward chunks 8+1
C     2  521  11 4  24  hs=4, 131 workgroups, last rs=1; rows padded by 7 to
                        528; backward chunks 8+3
D     1   32   1 1  24  T=1, B=1
E     1    8  17 3   5  H a multiple of 8 (no row pad), chunks 8+8+1
F     1  519  64 2   8  82.9 KB of dynamic LDS, above 64 KB

Every case compares out, hT and cT per element and every gradient (x, h0, c0
and all parameters) with the max-scaled measure; the margin of the latter is
what one flipped bf16 rounding costs (tests/test_lstm_oracle.py measures the
float32 oracle against the float64 one at up to 0.14 of it). The oracle and
the inputs live in tests/helpers/lstm_oracle.py; the CPU tests there show
that a dropped hidden unit or a stale batch chunk would exceed these
tolerances tenfold at cases A, B, C and E.
"""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from torchbeast_amd.ops import functional as tbops
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import lstm_oracle as lo  # noqa: E402


def _gpu_result(name):
    core, x, notdone, h0, c0 = lo.case_inputs(name)
    res = lo.run(tbops.lstm_unroll, lo.clone_core(core).cuda(), x.cuda(),
                 notdone.cuda(), h0.cuda(), c0.cuda())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("name", sorted(lo.CASES))
def test_lstm_unroll_matches_oracle(name):
    L, H, B, T, I = lo.CASES[name]
    ref = lo.oracle(name)
    got = _gpu_result(name)
    assert set(got) == set(ref)
    assert len(ref) == 6 + 4 * L  # nothing left uncompared

    for key in ("out", "hT", "cT"):
        print(f"case {name} {key}: {lo.forward_excess(got[key], ref[key]):.4f}"
              " of tolerance")
    for key in sorted(ref):
        if key.startswith("d_"):
            print(f"case {name} {key}: rel-max err "
                  f"{lo.grad_error(got[key], ref[key]):.5f}")

    for key in ("out", "hT", "cT"):
        torch.testing.assert_close(got[key], ref[key], **lo.FWD_TOL,
                                   msg=lambda m, k=key: f"{k}: {m}")
    for key in sorted(ref):
        if key.startswith("d_"):
            assert got[key].shape == ref[key].shape, key
            err = lo.grad_error(got[key], ref[key])
            assert err < lo.GRAD_TOL, f"grad {key}: rel-max err {err:.4f}"

    # Rows done at t=0 hand nothing back to the initial state: the kernel
    # multiplies by notdone, the oracle gives 0.0, and both are exact.
    notdone = lo.case_inputs(name)[2]
    done0 = notdone[0] == 0
    assert done0[0] and (B <= 2 or done0[1])
    for key in ("d_h0", "d_c0"):
        assert (ref[key][:, done0] == 0).all(), key
        assert (got[key][:, done0] == 0).all(), key
        if (~done0).any():
            assert (got[key][:, ~done0] != 0).any(), key


def _forward(H, B, T, I=8):
    torch.manual_seed(7)
    core = torch.nn.LSTM(I, H).cuda()
    x = torch.randn(T, B, I).cuda()
    state = (torch.zeros(1, B, H).cuda(), torch.zeros(1, B, H).cuda())
    with torch.no_grad():
        out, _ = tbops.lstm_unroll(core, x, torch.ones(T, B).cuda(), state)
    torch.cuda.synchronize()
    return out


def test_lstm_lds_limit_is_an_error():
    """The forward kernel needs 12480 + 1100*B bytes of LDS at H=519 and
    the host allows 160 KB, so B=137 is the last batch that fits; one more
    must be refused on the host, before any launch."""
    with pytest.raises(RuntimeError, match="LDS over budget"):
        _forward(H=519, B=138, T=1)
