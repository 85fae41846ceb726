"""C++ InferenceRunner numerics vs the Python model forward (GPU).

Every input form (tensor requests, slot-id requests), trunk (deep MFMA, deep
ATen, shallow MFMA, fused atari_trunk_fwd, shallow ATen) and tail (fused
heads, LSTM/ATen heads) of InferenceRunner::serve is served at least once
here; row requests are covered by test_actor_rows_gpu.py and
test_row_gather_gpu.py.
"""

import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

from torchbeast_amd import polybeast_learner as pbl  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402
from torchbeast_amd.models.atari_net import AtariNet  # noqa: E402
from torchbeast_amd.models.resnet import ResNet  # noqa: E402

TOL = dict(rtol=5e-2, atol=5e-3)
SLAB_ACTORS = 9


def _slot_ids(b):
    """Valid slot ids that are not the identity and repeat."""
    if b == 5:
        return torch.tensor([[8, 0, 3, 3, 1]], dtype=torch.int32)
    return ((torch.arange(b) * 4 + 8) % SLAB_ACTORS).to(torch.int32)[None]


def _make_inputs(model, b, obs_shape, form, use_lstm):
    """One batch of b samples: frame [1,b,C,H,W] u8, reward [1,b], done [1,b]
    bool, state; for the slot form also the pinned slab they were taken from
    and the ids that select them."""
    torch.manual_seed(0)
    inp = {}
    if form == "slot":
        n = SLAB_ACTORS
        slab = (
            torch.randint(0, 256, (n, *obs_shape), dtype=torch.uint8),
            torch.randn(n) * 2,  # some outside [-1, 1]: the gather clamps
            (torch.rand(n) < 0.3).to(torch.uint8),
        )
        assert slab[1].abs().max() > 1
        inp["slab"] = tuple(t.pin_memory() for t in slab)
        inp["ids"] = _slot_ids(b)
        sel = inp["ids"][0].long()
        inp["frame"] = slab[0][sel][None]
        inp["reward"] = slab[1][sel][None]
        inp["done"] = slab[2][sel][None].bool()
    else:
        inp["frame"] = torch.randint(0, 256, (1, b, *obs_shape),
                                     dtype=torch.uint8)
        inp["reward"] = torch.randn(1, b)
        inp["done"] = torch.rand(1, b) < 0.3
    if use_lstm:
        L, H = model.core.num_layers, model.core.hidden_size
        inp["state"] = (torch.randn(L, b, H), torch.randn(L, b, H))
    else:
        inp["state"] = ()
    return inp


def _start_runner(model, greedy=False):
    batcher = runtime.DynamicBatcher(batch_dim=1, minimum_batch_size=1)
    runner = pbl.make_inference_runner(model, batcher, greedy=greedy)
    runner.start(1)
    return batcher, runner


def _compute(batcher, inp, form, timeout=60):
    """One request through the batcher; (action, logits, baseline, state)."""
    b = inp["frame"].shape[1]
    if form == "slot":
        request = (inp["ids"], inp["state"])
    else:
        request = ((inp["frame"], inp["reward"], inp["done"],
                    torch.zeros(1, b, dtype=torch.int32), torch.zeros(1, b)),
                   inp["state"])
    result = {}

    def call():
        result["out"] = batcher.compute(request)

    t = threading.Thread(target=call)
    t.start()
    t.join(timeout)
    assert "out" in result, "runner did not serve the batch"
    (action, logits, baseline), new_state = result["out"]
    return action, logits, baseline, new_state


def _reference(model, inp):
    """The Python model on the same samples."""
    model.train()
    with torch.no_grad():
        ref_out, ref_state = model(
            dict(frame=inp["frame"].cuda(), reward=inp["reward"].cuda(),
                 done=inp["done"].cuda()),
            tuple(s.cuda() for s in inp["state"]),
        )
    return pbl._as_agent_output(ref_out), ref_state


def _serve_once(model, b, use_lstm, obs_shape=(4, 84, 84), form="tensor",
                greedy=False, env=None, monkeypatch=None, serves=1,
                timeout=60):
    """Serves one batch `serves` times through one fresh runner. `env` is set
    before the runner is constructed (its switches are read there). Returns
    the list of answers, the reference output and the reference state."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    inp = _make_inputs(model, b, obs_shape, form, use_lstm)
    batcher, runner = _start_runner(model, greedy)
    try:
        if form == "slot":
            runner.set_obs_slab(*inp["slab"])
        outs = [_compute(batcher, inp, form, timeout) for _ in range(serves)]
    finally:
        runner.stop()
    ref_out, ref_state = _reference(model, inp)
    return outs, ref_out, ref_state


def _check(out, ref_out, ref_state, b, greedy=False):
    action, logits, baseline, new_state = out
    torch.testing.assert_close(logits, ref_out[1].cpu(), **TOL)
    torch.testing.assert_close(baseline, ref_out[2].cpu(), **TOL)
    assert action.shape == (1, b) and action.dtype == torch.int64
    if greedy:
        assert torch.equal(action, logits.argmax(-1))
    assert len(new_state) == len(ref_state)
    for s, r in zip(new_state, ref_state):
        torch.testing.assert_close(s, r.cpu(), **TOL)


@pytest.mark.parametrize("use_lstm", [False, True])
def test_shallow_runner_matches_model(use_lstm):
    model = AtariNet((4, 84, 84), 6, use_lstm=use_lstm,
                     use_last_action=False).cuda()
    (out,), ref_out, ref_state = _serve_once(model, b=5, use_lstm=use_lstm)
    action, logits, baseline, new_state = out
    # The runner serves the trunk from the bf16 MFMA kernels while the
    # reference model forward here runs fp32; tolerances are set for that
    # operand rounding (behavior-policy logits, not learner math).
    torch.testing.assert_close(logits, ref_out[1].cpu(), rtol=5e-2, atol=5e-3)
    torch.testing.assert_close(baseline, ref_out[2].cpu(), rtol=5e-2,
                               atol=5e-3)
    assert action.shape == (1, 5) and action.dtype == torch.int64
    if use_lstm:
        for s, r in zip(new_state, ref_state):
            torch.testing.assert_close(s, r.cpu(), rtol=5e-2, atol=5e-3)


def test_deep_runner_matches_model():
    model = ResNet((4, 84, 84), 6).cuda()
    (out,), ref_out, _ = _serve_once(model, b=3, use_lstm=False)
    action, logits, baseline, new_state = out
    # Both sides run the bf16 MFMA trunk, but normalization rounding
    # differs (model: fp32/255 -> bf16; runner: u8 -> bf16, bf16 mul).
    torch.testing.assert_close(logits, ref_out[1].cpu(), rtol=5e-2, atol=5e-3)
    torch.testing.assert_close(baseline, ref_out[2].cpu(), rtol=5e-2,
                               atol=5e-3)


# (id, model, lstm, obs shape, form, b, env): one serve() pairing of input
# stage, trunk and tail each. b = 5 computes a batch of 64 with 59 pad rows,
# b = 70 one of 128. 4x36x36 is the smallest geometry atari_trunk_fwd admits.
ATEN = {"TBAMD_RUNNER_ATEN": "1"}
PAIRINGS = [
    # gather_obs -> MFMA trunk -> fused heads -> set_outputs
    ("slot-shallow", "shallow", False, (4, 84, 84), "slot", 5, None),
    # nd from the gather kernel (length bp) into the LSTM core
    ("slot-shallow-lstm", "shallow", True, (4, 84, 84), "slot", 5, None),
    # compute batch 128, zeroed pad rows 70..127
    ("tensor-shallow-b70", "shallow", False, (4, 84, 84), "tensor", 70, None),
    # pad_state with bp > b
    ("slot-shallow-lstm-b70", "shallow", True, (4, 84, 84), "slot", 70, None),
    # fused atari_trunk_fwd trunk (bp <= 384, non-84 geometry)
    ("tensor-shallow-36", "shallow", False, (4, 36, 36), "tensor", 5, None),
    # ATen trunk and ATen heads with a stateless model
    ("tensor-shallow-36-aten", "shallow", False, (4, 36, 36), "tensor", 5,
     ATEN),
    # deep ATen trunk, MFMA by weights but geometry not 84: no warm lock,
    # fused heads
    ("tensor-deep-36", "deep", False, (4, 36, 36), "tensor", 5, None),
    # deep MFMA trunk into the LSTM core
    ("tensor-deep-lstm", "deep", True, (4, 84, 84), "tensor", 5, None),
]


def _model(kind, obs_shape, use_lstm):
    torch.manual_seed(1)
    if kind == "deep":
        return ResNet(obs_shape, 6, use_lstm=use_lstm).cuda()
    return AtariNet(obs_shape, 6, use_lstm=use_lstm,
                    use_last_action=False).cuda()


@pytest.mark.parametrize("kind,use_lstm,obs_shape,form,b,env",
                         [p[1:] for p in PAIRINGS],
                         ids=[p[0] for p in PAIRINGS])
def test_serve_pairing_matches_model(kind, use_lstm, obs_shape, form, b, env,
                                     monkeypatch):
    model = _model(kind, obs_shape, use_lstm)
    (out,), ref_out, ref_state = _serve_once(
        model, b, use_lstm, obs_shape, form, True, env, monkeypatch)
    _check(out, ref_out, ref_state, b, greedy=True)


def test_deep_aten_warm_lock_then_warmed(monkeypatch):
    """TBAMD_RUNNER_ATEN on a deep model: the first batch of a size is served
    under the first-serve-per-shape lock, the second one without it."""
    model = _model("deep", (4, 36, 36), False)
    # The first serve includes MIOpen's solution search for eleven new conv
    # shapes: its own, longer limit.
    outs, ref_out, ref_state = _serve_once(
        model, 5, False, (4, 36, 36), "tensor", True, ATEN, monkeypatch,
        serves=2, timeout=240)
    for out in outs:
        _check(out, ref_out, ref_state, 5, greedy=True)


def _conv_weights(model):
    return [m.weight for m in model.modules()
            if isinstance(m, torch.nn.Conv2d)]


@pytest.mark.parametrize("kind", ["shallow", "deep"])
def test_weight_pack_follows_mark_weights_dirty(kind):
    """The bf16 weight pack is rebuilt after mark_weights_dirty() and only
    then: the runner holds views of the model's weights."""
    obs_shape = (4, 84, 84)
    model = _model(kind, obs_shape, False)
    inp = _make_inputs(model, 5, obs_shape, "tensor", False)
    batcher, runner = _start_runner(model, greedy=True)
    try:
        first = _compute(batcher, inp, "tensor")
        ref_first = _reference(model, inp)
        with torch.no_grad():
            for p in _conv_weights(model):
                p.mul_(0.5)
        runner.mark_weights_dirty()
        second = _compute(batcher, inp, "tensor")
        ref_second = _reference(model, inp)
        with torch.no_grad():
            for p in _conv_weights(model):
                p.mul_(0.5)
        third = _compute(batcher, inp, "tensor")  # not marked: old pack
    finally:
        runner.stop()
    _check(first, *ref_first, 5, greedy=True)
    _check(second, *ref_second, 5, greedy=True)
    assert not torch.equal(second[1], first[1])
    for s, t in zip(second[:3], third[:3]):
        assert torch.equal(s, t)


def test_slot_form_equals_tensor_form():
    """The same five samples as a tensor request and as a slot request: only
    how they reach the device differs, so the answers are bit-equal."""
    obs_shape = (4, 84, 84)
    model = _model("shallow", obs_shape, False)
    inp = _make_inputs(model, 5, obs_shape, "slot", False)
    batcher, runner = _start_runner(model, greedy=True)
    try:
        runner.set_obs_slab(*inp["slab"])
        as_tensor = _compute(batcher, inp, "tensor")
        as_slot = _compute(batcher, inp, "slot")
    finally:
        runner.stop()
    for t, s in zip(as_tensor[:3], as_slot[:3]):
        assert torch.equal(t, s)
