"""The recurrent row form on the GPU: lstm_serve_layer_kernel and the heads
against a bf16-faithful eager step, the C++ runner's recurrent tail on row
requests against the Python model, and a recurrent agent on state rows
served end to end."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import actor_rows_driver as drv  # noqa: E402
import row_gather_driver as rg  # noqa: E402
import state_rows_driver as sr  # noqa: E402
from torchbeast_amd import polybeast_learner as pbl  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402
from torchbeast_amd.models.atari_net import AtariNet  # noqa: E402
from torchbeast_amd.models.resnet import ResNet  # noqa: E402

tb = runtime._tbruntime

# ---- the kernels against the bf16-faithful step ----

# The kernel kept is the bf16 MFMA one: both matmuls take bf16 operands and
# accumulate in f32, everything else is f32. The oracle rounds the same
# operands and differs only in summation order; the tolerance is the one
# tests/test_ops_gpu.py::test_lstm_unroll_matches_eager uses for this
# rounding.
KTOL = dict(rtol=2e-3, atol=2e-3)
CAP = 128
A = 6
SENTINEL = -7.0
BLOCK_FILL = 1234.5


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _case(L, I, H, b):
    """Weights, inputs, state and the oracle's answer for one shape; built
    once and shared (nothing in it is modified)."""
    g = torch.Generator().manual_seed(1000 * L + 10 * H + b)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    k = 1.0 / H ** 0.5
    lstm = []
    for layer in range(L):
        i_l = I if layer == 0 else H
        lstm += [r(4 * H, i_l) * k, r(4 * H, H) * k, r(4 * H) * k,
                 r(4 * H) * k]
    heads = [r(A, H) * k, r(A) * k, r(1, H) * k, r(1) * k]
    x = r(CAP, I - 1).abs()  # the fc output is post-relu
    rew = torch.clamp(r(CAP), -1, 1)
    done = torch.rand(b, generator=g) < 0.3
    if b >= 5:
        done[0], done[1] = True, False
    h = r(L, b, H)
    c = r(L, b, H)

    layer_in = torch.cat([x[:b], rew[:b, None]], 1)
    keep = (~done).float()[:, None]
    hs, cs = [], []
    for layer in range(L):
        w_ih, w_hh, b_ih, b_hh = lstm[4 * layer:4 * layer + 4]
        gates = (_bf(layer_in) @ _bf(w_ih).t()
                 + _bf(keep * h[layer]) @ _bf(w_hh).t() + (b_ih + b_hh))
        gi, gf, gg, go = gates.chunk(4, dim=-1)
        c_new = gf.sigmoid() * (keep * c[layer]) + gi.sigmoid() * gg.tanh()
        h_new = go.sigmoid() * c_new.tanh()
        hs.append(h_new)
        cs.append(c_new)
        layer_in = h_new
    logits = layer_in @ heads[0].t() + heads[1]
    baseline = (layer_in @ heads[2].t() + heads[3]).reshape(b)
    return dict(lstm=lstm, heads=heads, x=x, rew=rew, done=done, h=h, c=c,
                want_h=torch.stack(hs), want_c=torch.stack(cs),
                want_logits=logits, want_baseline=baseline,
                gpu=dict(lstm=[w.cuda() for w in lstm],
                         heads=[w.cuda() for w in heads],
                         x=x.cuda(), rew=rew.cuda()))


def _layout(L, H, b):
    """Halves of the state block each request reads and writes: a shuffle of
    2 b + 2 halves (two stay unnamed), the block shifted by one float so that
    nothing is 16-byte aligned by luck; and where the done bytes sit."""
    n = 2 * L * H
    perm = torch.randperm(2 * b + 2,
                          generator=torch.Generator().manual_seed(b)).tolist()
    in_half, out_half = perm[:b], perm[b:2 * b]
    assert in_half != sorted(in_half) or b == 1
    to_off = lambda k: 4 * (1 + k * n)  # noqa: E731
    done_off = [(3 * r + 1) % 256 for r in range(b)]
    return n, in_half, out_half, to_off, done_off


def _run(case, L, H, b, h=None, c=None, greedy=True, seed=0):
    n, in_half, out_half, to_off, done_off = _layout(L, H, b)
    h = case["h"] if h is None else h
    c = case["c"] if c is None else c
    block = torch.full((1 + (2 * b + 2) * n,), BLOCK_FILL).pin_memory()
    for r in range(b):
        half = block[1 + in_half[r] * n:1 + (in_half[r] + 1) * n]
        half[:L * H] = h[:, r].reshape(-1)
        half[L * H:] = c[:, r].reshape(-1)
    before = block.clone()
    done_slab = torch.full((256,), 0, dtype=torch.uint8).pin_memory()
    for r in range(b):
        done_slab[done_off[r]] = int(case["done"][r])
    gpu = case["gpu"]
    out = tb.lstm_serve_step(
        gpu["x"], gpu["rew"], gpu["lstm"], *gpu["heads"], block,
        [to_off(k) for k in in_half], [to_off(k) for k in out_half],
        done_slab, done_off, CAP, greedy, seed)
    torch.cuda.synchronize()
    return dict(action=out[0], logits=out[1], baseline=out[2],
                hs=[t.cpu() for t in out[3:]], block=block, before=before)


SHAPES = [(1, 257, 256), (2, 513, 513), (1, 17, 16)]


@pytest.mark.parametrize("b", [1, 5, 70])
@pytest.mark.parametrize("L,I,H", SHAPES)
def test_step_matches_bf16_faithful_step(L, I, H, b):
    case = _case(L, I, H, b)
    got = _run(case, L, H, b)
    n, in_half, out_half, _, _ = _layout(L, H, b)
    block = got["block"]
    new_h = torch.stack([block[1 + k * n:1 + k * n + L * H].view(L, H)
                         for k in out_half], 1)
    new_c = torch.stack([block[1 + k * n + L * H:1 + (k + 1) * n].view(L, H)
                         for k in out_half], 1)
    for name, g, w in [("h", new_h, case["want_h"]),
                       ("c", new_c, case["want_c"]),
                       ("logits", got["logits"][:b], case["want_logits"]),
                       ("baseline", got["baseline"][:b],
                        case["want_baseline"])]:
        print(name, "max abs err", float((g - w).abs().max()))
    torch.testing.assert_close(new_h, case["want_h"], **KTOL)
    torch.testing.assert_close(new_c, case["want_c"], **KTOL)
    torch.testing.assert_close(got["logits"][:b], case["want_logits"], **KTOL)
    torch.testing.assert_close(got["baseline"][:b], case["want_baseline"],
                               **KTOL)
    assert got["action"].dtype == torch.int64
    assert torch.equal(got["action"][:b], got["logits"][:b].argmax(-1))
    # Every layer's h on the device is the h written to the block.
    for layer in range(L):
        assert torch.equal(got["hs"][layer][:b], new_h[layer])
    # Pad rows of every output keep the sentinel ...
    assert (got["action"][b:] == int(SENTINEL)).all()
    assert (got["logits"][b:] == SENTINEL).all()
    assert (got["baseline"][b:] == SENTINEL).all()
    for hs in got["hs"]:
        assert (hs[b:] == SENTINEL).all()
    # ... and so does whatever the table does not name as an out range: the
    # in halves, the two spare halves and the leading float.
    named = torch.zeros_like(block, dtype=torch.bool)
    for k in out_half:
        named[1 + k * n:1 + (k + 1) * n] = True
    assert torch.equal(block[~named], got["before"][~named])
    spare = set(range(2 * b + 2)) - set(in_half) - set(out_half)
    assert len(spare) == 2
    for k in spare:
        assert (block[1 + k * n:1 + (k + 1) * n] == BLOCK_FILL).all()
    assert not (block[named] == BLOCK_FILL).any()


@pytest.mark.parametrize("L,I,H", SHAPES)
def test_done_row_ignores_previous_state(L, I, H):
    b = 5
    case = _case(L, I, H, b)
    done = case["done"]
    assert done.any() and not done.all()
    runs = []
    for fill in (float("nan"), float("inf"), 3.0e38):
        h, c = case["h"].clone(), case["c"].clone()
        h[:, done] = fill
        c[:, done] = -fill
        runs.append(_run(case, L, H, b, h, c))
    n, _, out_half, _, _ = _layout(L, H, b)
    named = torch.zeros_like(runs[0]["block"], dtype=torch.bool)
    for k in out_half:
        named[1 + k * n:1 + (k + 1) * n] = True
    assert torch.isfinite(runs[0]["block"][named]).all()
    for other in runs[1:]:
        for key in ("action", "logits", "baseline"):
            assert torch.equal(runs[0][key], other[key]), key
        assert torch.equal(runs[0]["block"][named], other["block"][named])
    # And it is the answer to a zero state.
    torch.testing.assert_close(runs[0]["logits"][:b], case["want_logits"],
                               **KTOL)


def test_same_inputs_give_bit_equal_outputs():
    L, I, H, b = 2, 513, 513, 70
    case = _case(L, I, H, b)
    first, second = _run(case, L, H, b), _run(case, L, H, b)
    for key in ("action", "logits", "baseline", "block"):
        assert torch.equal(first[key], second[key]), key
    # Philox sampling: the same seed gives the same actions, the logits do
    # not depend on it, and the actions are actions.
    s1 = _run(case, L, H, b, greedy=False, seed=11)
    s2 = _run(case, L, H, b, greedy=False, seed=11)
    assert torch.equal(s1["action"], s2["action"])
    assert torch.equal(s1["logits"], first["logits"])
    assert ((s1["action"][:b] >= 0) & (s1["action"][:b] < A)).all()


def test_state_offsets_are_checked_before_launch():
    L, I, H, b = 1, 17, 16, 2
    case = _case(L, I, H, 5)
    n = 2 * L * H
    block = torch.full((6 * n,), BLOCK_FILL).pin_memory()
    done_slab = torch.zeros(64, dtype=torch.uint8).pin_memory()
    gpu = case["gpu"]
    nb = 4 * n  # bytes per half
    total = block.numel() * 4

    def step(ins, outs, dones, blk=block, slab=done_slab, cap=CAP):
        return tb.lstm_serve_step(gpu["x"], gpu["rew"], gpu["lstm"],
                                  *gpu["heads"], blk, ins, outs, slab, dones,
                                  cap, True, 0)

    for ins, outs, dones in [
            ([0, total - nb + 4], [nb, 2 * nb], [0, 1]),  # in past the end
            ([0, 2 * nb], [nb, total - nb + 4], [0, 1]),  # out past the end
            ([0, -4], [nb, 2 * nb], [0, 1]),              # in before
            ([0, 2 * nb], [nb, -nb], [0, 1]),             # out before
            ([0, 2 * nb], [nb, 3 * nb], [0, 64]),         # done past the end
            ([0, 2 * nb], [nb, 3 * nb], [-1, 0])]:        # done before
        with pytest.raises(IndexError):
            step(ins, outs, dones)
    for ins, outs in [
            ([0, 2 * nb + 2], [nb, 4 * nb]),   # misaligned
            ([0, 0], [nb, 2 * nb]),            # one stream twice
            ([0, nb], [nb, 2 * nb]),           # out of one is in of another
            ([0, 2 * nb], [nb - 4, 4 * nb])]:  # partial overlap
        with pytest.raises(ValueError):
            step(ins, outs, [0, 1])
    with pytest.raises(RuntimeError):  # block not pinned
        step([0, 2 * nb], [nb, 3 * nb], [0, 1], blk=block.clone())
    with pytest.raises(RuntimeError):  # done slab not pinned
        step([0, 2 * nb], [nb, 3 * nb], [0, 1], slab=done_slab.clone())
    with pytest.raises(RuntimeError):  # more requests than cap
        step([0, 2 * nb], [nb, 3 * nb], [0, 1], cap=1)
    torch.cuda.synchronize()
    # Nothing ran: the block is as it was.
    assert (block == BLOCK_FILL).all()
    # The last half of the block, exactly to its end, is fine (from a zero
    # state: a cell of 1234.5 behind an open forget gate stays 1234.5).
    block[:n] = 0
    step([0], [total - nb], [63])
    assert not (block[-n:] == BLOCK_FILL).any()


# ---- the runner's recurrent tail and the end-to-end path ----

TOL = dict(rtol=5e-2, atol=5e-3)  # tests/test_inference_runner_gpu.py


@functools.lru_cache(maxsize=None)
def _model(kind, obs_shape=(4, 84, 84)):
    torch.manual_seed(4321 if kind == "shallow" else 4322)
    if kind == "deep":
        return ResNet(obs_shape, 6, use_lstm=True).cuda()
    return AtariNet(obs_shape, 6, use_lstm=True, use_last_action=False).cuda()


def _initial_state(model):
    return tuple(t.cpu() for t in model.initial_state(batch_size=1))


def _serve_pool(model, env, n_envs, unroll, n_per_stream, *, use_obs_slab,
                recurrent_rows, chain, output_device=None):
    # Batches as large as the env count allows (70 envs: past one multiple
    # of 64, pad rows up to 128), as actor_rows_driver.run_gpu. For 70 envs
    # the learner queue is deep enough that no actor thread ever waits for
    # this test to take a rollout, and the batcher waits for all 70 requests
    # (the timeout only matters if something stalls): every batch has 70 rows.
    big = n_envs > 64
    batcher = runtime.DynamicBatcher(
        batch_dim=1, minimum_batch_size=n_envs, maximum_batch_size=128,
        timeout_ms=2000 if big else 20)
    return sr.run_pool([env] * n_envs, unroll, n_per_stream,
                       use_obs_slab=use_obs_slab,
                       recurrent_rows=recurrent_rows,
                       initial_agent_state=_initial_state(model),
                       serve=rg.gpu_runner_serve(model), batcher=batcher,
                       envs_per_thread=16, chain=chain,
                       output_device=output_device,
                       queue_size=512 if big else 8)


def _unroll_model(model, rollouts):
    """The model over recorded rollouts [(leaves, states)], each from its
    recorded initial state with its done masks. Returns what was recorded
    and what the model says: (logits, baseline), (logits, baseline), final
    state."""
    stack = lambda j: torch.from_numpy(  # noqa: E731
        np.stack([r[0][j] for r in rollouts], 1))
    frame, reward, done = stack(0), stack(1), stack(2)
    action, logits, baseline = stack(5), stack(6), stack(7)
    state = tuple(
        torch.from_numpy(np.concatenate([r[1][k] for r in rollouts], 1)).cuda()
        for k in range(2))
    model.train()
    # 32 rollouts at a time: the model's LSTM unroll kernel holds its batch
    # in LDS.
    ref_logits, ref_baseline, ref_h, ref_c = [], [], [], []
    with torch.no_grad():
        for lo in range(0, len(rollouts), 32):
            sl = slice(lo, lo + 32)
            ref, ref_state = model(
                dict(frame=frame[:, sl].cuda(), reward=reward[:, sl].cuda(),
                     done=done[:, sl].cuda()),
                tuple(s[:, sl].contiguous() for s in state))
            ref = pbl._as_agent_output(ref)
            ref_logits.append(ref[1].cpu())
            ref_baseline.append(ref[2].cpu())
            ref_h.append(ref_state[0].cpu())
            ref_c.append(ref_state[1].cpu())
    assert action.dtype == torch.int64
    assert torch.equal(action, logits.argmax(-1))
    return ((logits, baseline),
            (torch.cat(ref_logits, 1), torch.cat(ref_baseline, 1)),
            (torch.cat(ref_h, 1), torch.cat(ref_c, 1)))


@pytest.mark.parametrize("kind,n_envs", [("shallow", 5), ("shallow", 70),
                                         ("deep", 5)])
def test_runner_tail_matches_model_on_row_requests(kind, n_envs):
    """Unroll 1: rollout k + 1 starts at rollout k's row 1, and the state
    recorded with it is what the runner answered row 0 of rollout k with. So
    one served step (every stream's row 0 of its second rollout, a row
    request built by the pool) is checked on logits, baseline and new
    state."""
    model = _model(kind)
    run = _serve_pool(model, drv.GPU_ENV, n_envs, 1, 3, use_obs_slab=False,
                      recurrent_rows=True, chain=True)
    stats = run["stats"]
    assert stats["batcher_serve_state_row_batches"] > 0
    assert stats["batcher_serve_device_gather_batches"] == 0
    if n_envs > 64:
        assert stats["batcher_avg_batch_size"] > 64
    streams = run["streams"].ordered()
    assert len(streams) == n_envs
    second = [s[1] for s in streams]
    third = [s[2] for s in streams]
    # Row 0 alone, from the state recorded with the second rollout.
    step = [([leaf[:1] for leaf in leaves], states)
            for leaves, states in second]
    (logits, baseline), (ref_logits, ref_baseline), ref_state = \
        _unroll_model(model, step)
    new_state = tuple(
        torch.from_numpy(np.concatenate([r[1][k] for r in third], 1))
        for k in range(2))
    for name, g, w in [("logits", logits, ref_logits),
                       ("baseline", baseline, ref_baseline),
                       ("h", new_state[0], ref_state[0]),
                       ("c", new_state[1], ref_state[1])]:
        print(kind, n_envs, name, "max abs err", float((g - w).abs().max()))
    torch.testing.assert_close(logits, ref_logits, **TOL)
    torch.testing.assert_close(baseline, ref_baseline, **TOL)
    torch.testing.assert_close(new_state[0], ref_state[0], **TOL)
    torch.testing.assert_close(new_state[1], ref_state[1], **TOL)
    # Some request of the step was a done row (episodes of 7 steps, streams
    # out of phase only by their seeds: row 2 of a stream is never one, so
    # look at all rows for the mask having been exercised at all).
    assert any(leaves[2].any() for s in streams for leaves, _ in s)


def _assert_rollouts_match_model(model, rollouts, tag):
    (logits, baseline), (ref_logits, ref_baseline), _ = \
        _unroll_model(model, rollouts)
    print(tag, "logits max abs err",
          float((logits - ref_logits).abs().max()), "baseline max abs err",
          float((baseline - ref_baseline).abs().max()))
    torch.testing.assert_close(logits, ref_logits, **TOL)
    torch.testing.assert_close(baseline, ref_baseline, **TOL)


@pytest.mark.parametrize("n_envs", [5, 70])
def test_state_rows_end_to_end(n_envs):
    """Episodes of 7 steps, unroll 4, two chained rollouts per stream: every
    stream crosses a done and a rollout boundary."""
    model = _model("shallow")
    run = _serve_pool(model, drv.GPU_ENV, n_envs, drv.GPU_UNROLL, 2,
                      use_obs_slab=True, recurrent_rows=True, chain=True)
    assert run["slab"] == []
    stats = run["stats"]
    assert stats["batcher_serve_state_row_batches"] > 0
    # The start-up nests (and batches mixing them with rows) are no row
    # batches; every row batch took the recurrent tail.
    assert (stats["batcher_serve_state_row_batches"]
            == stats["batcher_serve_row_batches"])
    assert stats["batcher_serve_device_gather_batches"] > 0
    if n_envs > 64:
        assert stats["batcher_avg_batch_size"] > 64
    streams = run["streams"].ordered()
    assert len(streams) == n_envs
    rollouts = [r for s in streams for r in s[:2]]
    for s in streams:
        done = np.concatenate([s[0][0][2], s[1][0][2][1:]])
        assert done[1:].any(), "stream crossed no episode boundary"
    _assert_rollouts_match_model(model, rollouts, f"state rows n={n_envs}")


def test_parent_path_meets_the_same_bound():
    """The same assertion on the path without the switch (slot-id requests,
    tail_generic), same model, envs and seeds. Measured on the MI355X
    (profiles/PROFILE_r7.md section 7): the parent path's maximum absolute
    error over the 8 steps is 1.3e-5 on logits and 2.2e-5 on the baseline
    (state rows: 2.5e-5 and 1.2e-5), far inside TOL, so TOL is the bound for
    both and no doubled bound is needed."""
    model = _model("shallow")
    run = _serve_pool(model, drv.GPU_ENV, 5, drv.GPU_UNROLL, 2,
                      use_obs_slab=True, recurrent_rows=False, chain=True)
    assert len(run["slab"]) == 3
    assert run["stats"]["batcher_serve_state_row_batches"] == 0
    rollouts = [r for s in run["streams"].ordered() for r in s[:2]]
    _assert_rollouts_match_model(model, rollouts, "parent path n=5")


def test_obs_slab_on_equals_off_with_state_rows():
    model = _model("shallow")
    on = _serve_pool(model, drv.GPU_ENV, 5, drv.GPU_UNROLL, 2,
                     use_obs_slab=True, recurrent_rows=True, chain=True)
    assert on["stats"]["batcher_serve_device_gather_batches"] > 0
    off = _serve_pool(model, drv.GPU_ENV, 5, drv.GPU_UNROLL, 2,
                      use_obs_slab=False, recurrent_rows=True, chain=True)
    assert off["stats"]["batcher_serve_device_gather_batches"] == 0
    assert off["stats"]["batcher_serve_state_row_batches"] > 0
    got = drv.streams_as_dict(on["streams"], 2)
    want = drv.streams_as_dict(off["streams"], 2)
    assert sorted(got) == sorted(want)
    assert len(got) == 5 * 2 * 10
    # Same kernels on the same per-row inputs: equal, not merely close.
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key]), key


def test_full_resolution_frames_with_state_rows():
    big = _model("shallow", (3, 210, 160))
    run = _serve_pool(big, "synthetic:3x210x160:6:7", 3, 2, 2,
                      use_obs_slab=True, recurrent_rows=True, chain=False,
                      output_device="cuda:0")
    assert run["slab"] == []
    stats = run["stats"]
    assert stats["batcher_serve_device_gather_batches"] > 0
    assert stats["batcher_serve_state_row_batches"] > 0
    # The learner side still assembles its batches from whole slots.
    assert stats["gather_dequeues"] > 0
    assert len(run["streams"]) == 2 * 3
    _assert_rollouts_match_model(big, run["streams"], "3x210x160")
