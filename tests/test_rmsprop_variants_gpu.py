"""rmsprop_update_kernel<MOMENTUM, CENTERED> on the GPU: numerics against the
eager branch on CPU, the untouched default, the host-side buffer checks and
replay of a captured momentum step."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.ops import functional as tbops
    from torchbeast_amd.parallel import flat as tbflat
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

VARIANTS = [(0.9, False), (0.5, True), (0.0, True)]
ALPHA, EPS = 0.9, 0.01
LRS = (0.01, 0.004, 0.02)
# One element; one ragged block; more than the launch's 2048 x 256 threads,
# so the grid-stride loop takes a second, ragged trip.
SIZES = [1, 257, 2048 * 256 + 257]


def _zero_state(n, momentum, centered, device):
    return dict(
        square_avg=torch.zeros(n, device=device),
        momentum_buf=(torch.zeros(n, device=device) if momentum > 0
                      else None),
        grad_avg=torch.zeros(n, device=device) if centered else None,
    )


def _three_steps(param, grads, state, momentum, clip):
    norms = []
    for lr, grad in zip(LRS, grads):
        norms.append(tbops.rmsprop_step(
            param, grad, state["square_avg"], lr, ALPHA, EPS, clip, None,
            state["momentum_buf"], state["grad_avg"], momentum))
    return norms


def _assert_state_close(param_g, state_g, param_c, state_c):
    torch.testing.assert_close(param_g.cpu(), param_c, rtol=1e-4, atol=1e-5)
    for name, buf_c in state_c.items():
        if buf_c is None:
            assert state_g[name] is None
            continue
        torch.testing.assert_close(
            state_g[name].cpu(), buf_c, rtol=1e-4, atol=1e-5,
            msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("momentum,centered", VARIANTS)
def test_variant_kernels_match_eager(momentum, centered, clip, n):
    torch.manual_seed(5)
    param_c = torch.randn(n)
    grads = [torch.randn(n) for _ in LRS]
    state_c = _zero_state(n, momentum, centered, "cpu")

    param_g = param_c.cuda()
    state_g = _zero_state(n, momentum, centered, "cuda")

    norms_c = _three_steps(param_c, grads, state_c, momentum, clip)
    norms_g = _three_steps(param_g, [g.cuda() for g in grads], state_g,
                           momentum, clip)

    for norm_g, norm_c in zip(norms_g, norms_c):
        torch.testing.assert_close(norm_g.cpu(), norm_c, rtol=1e-4, atol=1e-4)
    _assert_state_close(param_g, state_g, param_c, state_c)


@pytest.mark.parametrize("clip", [None, 1e6])
def test_default_through_new_signature_is_bit_identical(clip):
    """The norm is summed with one atomicAdd per block, so its last bit varies
    from launch to launch of the very same kernel. Bit equality is therefore
    asked of param and square_avg with no clip and with a clip that does not
    bind (coef is exactly 1 in both), and the norm is compared at 1e-4."""
    torch.manual_seed(6)
    n = 2048 * 256 + 257
    param = torch.randn(n, device="cuda")
    grad = torch.randn(n, device="cuda")
    square_avg = torch.rand(n, device="cuda")

    param_old, sq_old = param.clone(), square_avg.clone()
    norm_old = tbops.rmsprop_step(param_old, grad, sq_old, 0.01, 0.99, 0.01,
                                  clip)

    param_new, sq_new = param.clone(), square_avg.clone()
    norm_new = tbops.rmsprop_step(
        param_new, grad, sq_new, 0.01, 0.99, 0.01, clip, None,
        momentum_buf=None, grad_avg=None, momentum=0.0)
    # A buffer that momentum=0 does not use must change nothing either.
    param_buf, sq_buf = param.clone(), square_avg.clone()
    unused = torch.full((n,), 3.0, device="cuda")
    tbops.rmsprop_step(param_buf, grad, sq_buf, 0.01, 0.99, 0.01, clip, None,
                       momentum_buf=unused, momentum=0.0)

    assert not torch.equal(param_old, param)
    assert torch.equal(param_new, param_old)
    assert torch.equal(sq_new, sq_old)
    torch.testing.assert_close(norm_new, norm_old, rtol=1e-4, atol=1e-4)
    assert torch.equal(param_buf, param_old)
    assert torch.equal(sq_buf, sq_old)
    assert torch.equal(unused, torch.full_like(unused, 3.0))


def _bad_calls(n):
    return {
        "short momentum_buf": dict(
            momentum_buf=torch.zeros(n - 1, device="cuda"), momentum=0.9),
        "momentum without buffer": dict(momentum=0.9),
        "float64 momentum_buf": dict(
            momentum_buf=torch.zeros(n, device="cuda", dtype=torch.float64),
            momentum=0.9),
        "short grad_avg": dict(
            grad_avg=torch.zeros(n - 1, device="cuda")),
        "float64 grad_avg": dict(
            grad_avg=torch.zeros(n, device="cuda", dtype=torch.float64)),
        "cpu momentum_buf": dict(momentum_buf=torch.zeros(n), momentum=0.9),
        "strided momentum_buf": dict(
            momentum_buf=torch.zeros(2 * n, device="cuda")[::2],
            momentum=0.9),
        "short grad": dict(grad=torch.zeros(n - 1, device="cuda")),
        "short square_avg": dict(square_avg=torch.zeros(n - 1,
                                                        device="cuda")),
        "float64 square_avg": dict(
            square_avg=torch.zeros(n, device="cuda", dtype=torch.float64)),
    }


@pytest.mark.parametrize("case", [
    "short momentum_buf", "momentum without buffer", "float64 momentum_buf",
    "short grad_avg", "float64 grad_avg", "cpu momentum_buf",
    "strided momentum_buf", "short grad", "short square_avg",
    "float64 square_avg",
])
@pytest.mark.parametrize("through", ["functional", "extension"])
def test_host_checks_reject_bad_buffers(case, through):
    """Every bad buffer is a RuntimeError raised on the host, before any
    kernel is launched: the parameters stay untouched."""
    n = 1000
    torch.manual_seed(7)
    param = torch.randn(n, device="cuda")
    before = param.clone()
    kwargs = dict(grad=torch.randn(n, device="cuda"),
                  square_avg=torch.zeros(n, device="cuda"))
    kwargs.update(_bad_calls(n)[case])
    grad = kwargs.pop("grad")
    square_avg = kwargs.pop("square_avg")

    if through == "functional":
        def call():
            tbops.rmsprop_step(param, grad, square_avg, 0.01, ALPHA, EPS,
                               None, None, **kwargs)
    else:
        ext = ops_mod.require_ext()

        def call():
            ext.rmsprop_step(param, grad, square_avg, 0.01, ALPHA, EPS, -1.0,
                             None, **kwargs)

    with pytest.raises(RuntimeError):
        call()
    torch.cuda.synchronize()
    assert torch.equal(param, before)
    for buf in kwargs.values():
        if torch.is_tensor(buf):
            assert buf.abs().sum() == 0


def test_captured_momentum_step_replays_with_fresh_lr():
    """`momentum` by value and the buffers by address survive replay, and the
    decayed rate read from device memory reaches the buffer update."""
    n = 10_000
    torch.manual_seed(8)
    init = torch.randn(n)
    warm_grad = torch.randn(n)
    grads = [torch.randn(n) for _ in range(3)]
    factors = [1.0, 0.6, 0.25]

    def make(device):
        return tbflat.FusedRMSProp(
            init.to(device).clone(), torch.zeros(n, device=device), 0.01,
            ALPHA, EPS, 1.0, momentum=0.9)

    opt = make("cuda")
    opt.enable_device_lr()
    opt.grad.copy_(warm_grad)
    buf_addr = opt.momentum_buf.data_ptr()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()

    # Undo the warm-up so the twin starts equal.
    opt.param.copy_(init)
    opt.square_avg.zero_()
    opt.momentum_buf.zero_()

    twin = make("cpu")
    for grad, factor in zip(grads, factors):
        opt.grad.copy_(grad)
        opt.lr_factor = factor
        opt.push_lr()
        graph.replay()

        twin.grad.copy_(grad)
        twin.lr_factor = factor
        twin.step()
    torch.cuda.synchronize()

    assert opt.momentum_buf.data_ptr() == buf_addr
    assert opt.momentum_buf.abs().sum() > 0
    torch.testing.assert_close(opt.last_grad_norm.cpu(), twin.last_grad_norm,
                               rtol=1e-4, atol=1e-4)
    _assert_state_close(
        opt.param,
        dict(square_avg=opt.square_avg, momentum_buf=opt.momentum_buf),
        twin.param,
        dict(square_avg=twin.square_avg, momentum_buf=twin.momentum_buf))
