"""The V-trace API on the GPU: the from_importance_weights kernel, unclipped
(None) thresholds and lambda through both entry points, and the host-side
validation in front of both launches. The CPU path of core/vtrace.py is the
oracle (itself checked against NumPy in test_vtrace.py/test_vtrace_lambda.py).

Shapes: T=1 has no t+1 neighbour, T=257 puts one element into a second
stride of the 256-thread loops, B=1 and B=3 are grids that are no multiple
of anything; (80, 8) is the trainers' default.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops
    from torchbeast_amd.core import vtrace
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

SHAPES = [(1, 1), (5, 2), (80, 8), (257, 3)]
# (clip_rho_threshold, clip_pg_rho_threshold, lambda_)
PARAMS = [
    (1.0, 1.0, 1.0),
    (None, None, 1.0),
    (1.0, 1.0, 0.9),
    (None, None, 0.5),
    (3.0, None, 0.0),
]
# The tolerance test_ops_gpu.py uses for the sibling kernel against the same
# oracle: f32 on both sides, __expf on the device.
TOL = dict(rtol=2e-4, atol=2e-4)


@functools.lru_cache(maxsize=None)
def _iw_inputs(T, B):
    """(log_rhos, discounts, rewards, values, bootstrap) on the CPU; callers
    must not modify them."""
    g = torch.Generator().manual_seed(0)
    return (
        torch.rand(T, B, generator=g) * 3.0 - 1.5,
        (torch.rand(T, B, generator=g) > 0.1).float() * 0.99,
        torch.randn(T, B, generator=g),
        torch.randn(T, B, generator=g),
        torch.randn(B, generator=g),
    )


@functools.lru_cache(maxsize=None)
def _logit_inputs(T, B, A):
    """(behavior, target, actions) + the four trailing tensors above."""
    g = torch.Generator().manual_seed(1)
    head = (
        torch.randn(T, B, A, generator=g),
        torch.randn(T, B, A, generator=g),
        torch.randint(0, A, (T, B), generator=g),
    )
    return head + _iw_inputs(T, B)[1:]


@functools.lru_cache(maxsize=None)
def _cpu_iw(T, B, clip_rho, clip_pg, lambda_):
    return vtrace.from_importance_weights(
        *_iw_inputs(T, B), clip_rho, clip_pg, lambda_)


def _cuda(tensors):
    return tuple(t.cuda() for t in tensors)


def _lds_max_unroll():
    """Longest T whose three f32 rows fit one workgroup's LDS."""
    return torch.cuda.get_device_properties(0).shared_memory_per_block // 12


@pytest.mark.parametrize("clip_rho,clip_pg,lambda_", PARAMS)
@pytest.mark.parametrize("T,B", SHAPES)
def test_iw_kernel_matches_cpu(T, B, clip_rho, clip_pg, lambda_):
    cpu = _cpu_iw(T, B, clip_rho, clip_pg, lambda_)
    gpu = vtrace.from_importance_weights(
        *_cuda(_iw_inputs(T, B)), clip_rho, clip_pg, lambda_)
    torch.testing.assert_close(gpu.vs.cpu(), cpu.vs, **TOL)
    torch.testing.assert_close(gpu.pg_advantages.cpu(), cpu.pg_advantages, **TOL)


def test_iw_kernel_really_runs():
    assert hasattr(ops._load(), "vtrace_from_importance_weights")
    log_rhos, discounts, rewards, values, bootstrap = _cuda(_iw_inputs(5, 2))
    out = vtrace.from_importance_weights(
        log_rhos, discounts, rewards, values.requires_grad_(), bootstrap)
    assert isinstance(out, vtrace.VTraceReturns)
    for t in out:
        assert t.is_cuda and t.shape == (5, 2) and t.dtype == torch.float32
        assert not t.requires_grad


def test_iw_kernel_at_the_lds_limit():
    """The longest unroll the LDS check admits launches and is right: the
    last t of each of the three LDS rows is the byte just under the limit.
    Same tolerance: discount*c <= 0.99 makes the recurrence a contraction, so
    rounding errors do not grow with T."""
    T = _lds_max_unroll()
    cpu = _cpu_iw(T, 1, 1.0, 1.0, 1.0)
    gpu = vtrace.from_importance_weights(*_cuda(_iw_inputs(T, 1)))
    torch.testing.assert_close(gpu.vs.cpu(), cpu.vs, **TOL)
    torch.testing.assert_close(gpu.pg_advantages.cpu(), cpu.pg_advantages, **TOL)


@pytest.mark.parametrize("lambda_", [1.0, 0.9])
@pytest.mark.parametrize("T,B,A", [(5, 2, 3), (80, 8, 6)])
def test_from_logits_without_clipping(T, B, A, lambda_):
    inputs = _logit_inputs(T, B, A)
    kwargs = dict(clip_rho_threshold=None, clip_pg_rho_threshold=None,
                  lambda_=lambda_)
    cpu = vtrace.from_logits(*inputs, **kwargs)
    gpu = vtrace.from_logits(*_cuda(inputs), **kwargs)
    for name in cpu._fields:
        torch.testing.assert_close(
            getattr(gpu, name).cpu(), getattr(cpu, name),
            msg=lambda m, n=name: f"{n}: {m}", **TOL,
        )
    # Unclipped weights really are unclipped: some rho exceed 1 here.
    assert (gpu.log_rhos > 0).any()


@pytest.mark.parametrize("clip_rho,clip_pg,lambda_", PARAMS)
def test_entry_points_agree_on_gpu(clip_rho, clip_pg, lambda_):
    inputs = _cuda(_logit_inputs(80, 8, 6))
    full = vtrace.from_logits(*inputs, clip_rho, clip_pg, lambda_)
    core = vtrace.from_importance_weights(
        full.log_rhos, *inputs[3:], clip_rho, clip_pg, lambda_)
    torch.testing.assert_close(full.vs, core.vs)
    torch.testing.assert_close(full.pg_advantages, core.pg_advantages)


def _valid_ext_args(entry, T=5, B=2, A=3):
    """Positional tensors of a valid extension call, as a name -> tensor
    dict in argument order."""
    names = ["discounts", "rewards", "values", "bootstrap"]
    if entry == "vtrace_from_logits":
        names = ["behavior_logits", "target_logits", "actions"] + names
        tensors = _logit_inputs(T, B, A)
    else:
        names = ["log_rhos"] + names
        tensors = _iw_inputs(T, B)
    return dict(zip(names, _cuda(tensors)))


ENTRIES = ["vtrace_from_logits", "vtrace_from_importance_weights"]


@pytest.mark.parametrize("case", [
    "values_shape", "bootstrap_shape", "rewards_f64", "discounts_cpu",
    "lambda_range",
])
@pytest.mark.parametrize("entry", ENTRIES)
def test_extension_rejects_bad_arguments(entry, case):
    """The C++ entry points check on the host before they allocate or
    launch, so none of these reaches the device."""
    T, B = 5, 2
    args = _valid_ext_args(entry, T, B)
    lambda_ = 1.0
    if case == "values_shape":
        args["values"] = torch.zeros(T, B + 1, device="cuda")
    elif case == "bootstrap_shape":
        args["bootstrap"] = torch.zeros(B + 1, device="cuda")
    elif case == "rewards_f64":
        args["rewards"] = args["rewards"].double()
    elif case == "discounts_cpu":
        args["discounts"] = args["discounts"].cpu()
    elif case == "lambda_range":
        lambda_ = 1.5
    fn = getattr(ops._load(), entry)
    with pytest.raises(RuntimeError, match="vtrace"):
        fn(*args.values(), 1.0, 1.0, lambda_)
    # The unmodified call is accepted.
    fn(*_valid_ext_args(entry, T, B).values(), 1.0, 1.0, 1.0)


def test_from_logits_rejects_float_actions():
    args = _valid_ext_args("vtrace_from_logits")
    args["actions"] = args["actions"].float()
    with pytest.raises(RuntimeError, match="actions"):
        ops._load().vtrace_from_logits(*args.values(), 1.0, 1.0, 1.0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_unroll_longer_than_lds_is_an_error_naming_T(entry):
    T = _lds_max_unroll() + 1
    if entry == "vtrace_from_logits":
        logits = torch.zeros(T, 1, 2, device="cuda")
        head = (logits, logits, torch.zeros(T, 1, dtype=torch.int64,
                                            device="cuda"))
    else:
        head = (torch.zeros(T, 1, device="cuda"),)
    row = torch.zeros(T, 1, device="cuda")
    with pytest.raises(RuntimeError, match=f"T={T}"):
        getattr(ops._load(), entry)(
            *head, row, row, row, torch.zeros(1, device="cuda"), 1.0, 1.0, 1.0)


def test_python_wrappers_reject_bad_shapes_and_lambda():
    log_rhos, discounts, rewards, values, bootstrap = _cuda(_iw_inputs(5, 2))
    with pytest.raises(RuntimeError, match="values"):
        vtrace.from_importance_weights(
            log_rhos, discounts, rewards, torch.zeros(5, 3, device="cuda"),
            bootstrap)
    with pytest.raises(RuntimeError, match="discounts"):
        vtrace.from_importance_weights(
            log_rhos, discounts.cpu(), rewards, values, bootstrap)
    with pytest.raises(ValueError):
        vtrace.from_importance_weights(
            log_rhos, discounts, rewards, values, bootstrap, lambda_=1.5)
