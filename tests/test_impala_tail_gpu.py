"""The fused learner tail of ops/hip/impala_tail.hip (ops.impala_tail,
core.tail.learner_tail under TBAMD_FUSED_TAIL=1) against the eager composition
in float64 on the CPU: shift, clip, discounts, V-trace, the three losses,
their total and autograd through it.

Shapes (T, B, A) sit at the kernel's edges: one row, a cut last pass of 16
rows, lane tails at 4/5 and 16/17 logits, the full 64, more columns than CUs.
The error of a tensor is max|out - ref| / max(1, max|ref|). BOUNDS is four
times the largest error, over these same cases on an MI355X, of the two-kernel
path (vtrace.from_logits + fused_impala_loss + the eager combine) against the
same reference; docs/KERNELS.md lists those errors and the fused kernel's own.
"""

import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import torchbeast_amd.ops as ops_mod
    from torchbeast_amd.core import losses, tail
    from torchbeast_amd.core import vtrace as pyvtrace
else:  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

BOUNDS = {  # 4 x the two-kernel path's measured error
    "vs": 4 * 1.2175e-06,
    "pg_adv": 4 * 5.7135e-07,
    "total": 4 * 2.2325e-06,
    "pg": 4 * 2.8750e-06,
    "baseline": 4 * 6.3522e-07,
    "entropy": 4 * 1.4837e-06,
    "d_logits": 4 * 5.7135e-07,
    "d_baseline": 4 * 1.1836e-06,
}

SHAPES = [(1, 1, 1), (2, 1, 3), (15, 2, 4), (16, 2, 5), (17, 3, 16),
          (33, 2, 17), (5, 33, 6), (3, 300, 2), (80, 32, 18), (4, 2, 63),
          (4, 2, 64)]
VARIANTS = ["int32", "raw_reward", "lambda", "no_clip", "done_row1",
            "done_rowT", "done_all", "done_none", "scaled"]
CASES = [(s, "base") for s in SHAPES] + [
    (s, v) for v in VARIANTS for s in ((17, 3, 16), (5, 33, 6))]
INPUTS = ("behavior", "target", "actions", "rewards", "done", "baseline")


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """(float32 CPU inputs, scalar arguments, float64 reference)."""
    T, B, A = shape
    g = torch.Generator().manual_seed(1000 * T + 10 * B + A)
    scale = 30.0 if variant == "scaled" else 1.0
    x = {
        "behavior": scale * torch.randn(T + 1, B, A, generator=g),
        "target": scale * torch.randn(T + 1, B, A, generator=g),
        "actions": torch.randint(0, A, (T + 1, B), generator=g),
        "rewards": (3.0 if variant == "raw_reward" else 1.0)
        * torch.randn(T + 1, B, generator=g),
        "done": torch.rand(T + 1, B, generator=g) < 0.2,
        "baseline": torch.randn(T + 1, B, generator=g),
    }
    if variant == "int32":
        x["actions"] = x["actions"].int()
    if variant.startswith("done_"):
        x["done"][:] = variant == "done_all"
        if variant in ("done_row1", "done_rowT"):
            x["done"][1 if variant == "done_row1" else T] = True
    clip = None if variant == "no_clip" else 1.0
    kw = dict(discounting=0.99, clip_reward=variant != "raw_reward",
              clip_rho_threshold=clip, clip_pg_rho_threshold=clip,
              lambda_=0.5 if variant == "lambda" else 1.0, baseline_cost=0.5,
              entropy_cost=0.05)

    logits = x["target"].double().requires_grad_()
    baseline = x["baseline"].double().requires_grad_()
    actions = x["actions"][1:].long()
    rewards = x["rewards"][1:].double()
    if kw["clip_reward"]:
        rewards = torch.clamp(rewards, -1, 1)
    vt = pyvtrace.from_logits(
        x["behavior"][1:].double(), logits[:-1], actions,
        (~x["done"][1:]).double() * kw["discounting"], rewards, baseline[:-1],
        baseline[-1], clip, clip, kw["lambda_"])
    pg = losses.compute_policy_gradient_loss(logits[:-1], actions,
                                             vt.pg_advantages)
    bl = losses.compute_baseline_loss(vt.vs - baseline[:-1])
    ent = losses.compute_entropy_loss(logits[:-1])
    total = pg + kw["baseline_cost"] * bl + kw["entropy_cost"] * ent
    total.backward()
    ref = {"vs": vt.vs, "pg_adv": vt.pg_advantages, "total": total, "pg": pg,
           "baseline": bl, "entropy": ent, "d_logits": logits.grad,
           "d_baseline": baseline.grad}
    return x, kw, {k: v.detach() for k, v in ref.items()}


def _err(out, ref):
    ref = ref.double().cpu()
    diff = (out.detach().double().cpu() - ref).abs().max().item()
    return diff / max(1.0, ref.abs().max().item())


def _kernel(x, kw):
    inf = float("inf")
    res = ops_mod.require_ext().impala_tail_fwd(
        *(x[k].cuda() for k in INPUTS), kw["discounting"], kw["clip_reward"],
        kw["clip_rho_threshold"] or inf, kw["clip_pg_rho_threshold"] or inf,
        kw["lambda_"], kw["baseline_cost"], kw["entropy_cost"])
    torch.cuda.synchronize()
    out = dict(zip(("total", "pg", "baseline", "entropy"), res[0]))
    out.update(zip(("d_logits", "d_baseline", "vs", "pg_adv"), res[1:]))
    return out


@pytest.mark.parametrize("shape,variant", CASES)
def test_kernel_matches_float64(shape, variant):
    x, kw, ref = _case(shape, variant)
    out = _kernel(x, kw)
    assert torch.equal(out["d_logits"][-1], torch.zeros_like(out["d_logits"][-1]))
    assert torch.equal(out["d_baseline"][-1],
                       torch.zeros_like(out["d_baseline"][-1]))
    for key, bound in BOUNDS.items():
        assert out[key].shape == ref[key].shape, key
        err = _err(out[key], ref[key])
        print(f"{shape} {variant} {key}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{key}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("shape", [(80, 32, 18), (3, 300, 2)])
def test_two_calls_are_byte_identical(shape):
    x, kw, _ = _case(shape, "base")
    first, second = _kernel(x, kw), _kernel(x, kw)
    for key in first:
        assert torch.equal(first[key], second[key]), key


@pytest.mark.parametrize("shape,variant", [((33, 2, 17), "base"),
                                           ((5, 33, 6), "lambda")])
def test_autograd(shape, variant):
    x, kw, ref = _case(shape, variant)
    gpu = {k: x[k].cuda() for k in INPUTS}
    gpu["target"].requires_grad_()
    gpu["baseline"].requires_grad_()
    out = ops_mod.impala_tail(*(gpu[k] for k in INPUTS), **kw)
    assert [o.requires_grad for o in out] == [True, False, False, False]
    out[0].backward()
    for got, key in zip(out, ("total", "pg", "baseline", "entropy")):
        assert _err(got, ref[key]) <= BOUNDS[key], key
    assert _err(gpu["target"].grad, ref["d_logits"]) <= BOUNDS["d_logits"]
    assert _err(gpu["baseline"].grad, ref["d_baseline"]) <= BOUNDS["d_baseline"]


def _learner_tail(x, monkeypatch):
    ext, seen = ops_mod.require_ext(), []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("impala_tail"):
                seen.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops_mod, "require_ext", lambda: Counting())
    flags = types.SimpleNamespace(
        discounting=0.99, reward_clipping="abs_one", vtrace_lambda=1.0,
        baseline_cost=0.5, entropy_cost=0.05)
    gpu = {k: x[k].cuda() for k in INPUTS}
    gpu["target"].requires_grad_()
    gpu["baseline"].requires_grad_()
    out = tail.learner_tail(flags, gpu["rewards"], gpu["done"], gpu["behavior"],
                            gpu["actions"], gpu["target"], gpu["baseline"])
    out[0].backward()
    names = ("total", "pg", "baseline", "entropy", "d_logits", "d_baseline")
    return dict(zip(names, (*out, gpu["target"].grad, gpu["baseline"].grad))), seen


def test_switch(monkeypatch):
    x, _, _ = _case((80, 32, 18), "base")
    monkeypatch.delenv("TBAMD_FUSED_TAIL", raising=False)
    off, seen = _learner_tail(x, monkeypatch)
    assert seen == []
    monkeypatch.setenv("TBAMD_FUSED_TAIL", "1")
    on, seen = _learner_tail(x, monkeypatch)
    assert "impala_tail_fwd" in seen
    for key in on:
        assert _err(on[key], off[key]) <= BOUNDS[key], key


@pytest.mark.parametrize("change,match", [
    (lambda x, kw: x.update(rewards=x["rewards"].cpu()), "rewards is on"),
    (lambda x, kw: x.update(baseline=x["baseline"].double()),
     "baseline must be float32"),
    (lambda x, kw: x.update(done=x["done"][:-1]), "done has shape"),
    (lambda x, kw: x.update({k: x[k][:1] for k in INPUTS}), "T must be >= 1"),
    (lambda x, kw: x.update({k: torch.zeros(3, 1, 65, device="cuda")
                             for k in ("behavior", "target")}), "A must be"),
    (lambda x, kw: kw.update(lambda_=1.5), "lambda must be"),
    (lambda x, kw: x.update({k: x[k][:1].expand(20001, *x[k].shape[1:])
                             .contiguous() for k in INPUTS}), "T=20000"),
])
def test_host_checks_name_their_argument(change, match):
    cpu, kw, _ = _case((2, 1, 3), "base")
    x, kw = {k: cpu[k].cuda() for k in INPUTS}, dict(kw)
    change(x, kw)
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=match):
        ops_mod.require_ext().impala_tail_fwd(
            *(x[k] for k in INPUTS), kw["discounting"], kw["clip_reward"], 1.0,
            1.0, kw["lambda_"], kw["baseline_cost"], kw["entropy_cost"])
    assert torch.cuda.memory_allocated() == before  # checked before allocating
