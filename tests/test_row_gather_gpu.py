"""gather_rows (the inference batch gathered on the GPU from rollout rows):
the kernel against torch indexing, and the obs-slab row form served end to
end by the C++ InferenceRunner."""

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
from torchbeast_amd import polybeast_learner as pbl  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

tb = runtime._tbruntime
C = tb.gather_rows_chunk_bytes()
CAP = 128
SLAB_BYTES = 4 * C + 4096
REWARDS = [-3.0, -1.0, -0.5, 0.0, 1.0, 2.5]
REWARD_BASE = SLAB_BYTES - 64  # six floats, 16-byte aligned


@pytest.fixture(scope="module")
def slab():
    g = torch.Generator().manual_seed(7)
    s = torch.randint(0, 256, (SLAB_BYTES,), dtype=torch.uint8,
                      generator=g).pin_memory()
    s[REWARD_BASE:REWARD_BASE + 24] = torch.tensor(REWARDS).view(torch.uint8)
    return s


def _check(slab, frame_offsets, reward_index, fsz):
    b = len(frame_offsets)
    reward_offsets = [REWARD_BASE + 4 * i for i in reward_index]
    frames, rew = tb.gather_rows(slab, frame_offsets, reward_offsets, fsz, CAP)
    assert frames.is_cuda and frames.shape == (CAP, fsz)
    assert frames.dtype == torch.uint8
    assert rew.is_cuda and rew.shape == (CAP, 1) and rew.dtype == torch.float32
    frames, rew = frames.cpu(), rew.cpu()
    idx = (torch.tensor(frame_offsets).view(b, 1) + torch.arange(fsz))
    assert torch.equal(frames[:b], slab[idx])
    want = torch.clamp(torch.tensor(REWARDS)[reward_index], -1, 1).view(b, 1)
    assert torch.equal(rew[:b].view(torch.int32), want.view(torch.int32))
    # Rows [b, cap) are not touched.
    assert (frames[b:] == 0xA5).all()
    assert (rew[b:] == -7.0).all()


@pytest.mark.parametrize(
    "fsz", [16, 48, C - 16, C, C + 16, 2 * C + 48, 63, 100])
@pytest.mark.parametrize("b", [1, 5, 70])
def test_kernel_matches_indexing(slab, fsz, b):
    # Sources spread over the slab (they may overlap), 16-byte aligned.
    room = (SLAB_BYTES - fsz - 16) // 16
    offsets = [16 * ((r * 37 + 3) % room) for r in range(b)]
    reward_index = [r % len(REWARDS) for r in range(b)]
    _check(slab, offsets, reward_index, fsz)
    # The narrow-width paths: every source 4, then 1, past a 16-byte line.
    _check(slab, [o + 4 for o in offsets], reward_index, fsz)
    _check(slab, [o + 1 for o in offsets], reward_index, fsz)


def test_kernel_same_source_twice(slab):
    _check(slab, [256, 4096, 256, 256], [5, 0, 5, 1], 2 * C + 48)


def test_kernel_last_bytes_of_the_slab(slab):
    _check(slab, [SLAB_BYTES - (C + 16), 0], [0, 1], C + 16)


def test_offsets_are_checked_before_launch(slab):
    for frames, rewards, fsz in [
            ([0, SLAB_BYTES - 99], [REWARD_BASE] * 2, 100),
            ([0, -16], [REWARD_BASE] * 2, 100),
            ([0], [SLAB_BYTES - 3], 100),
            ([0], [-4], 100),
            ([SLAB_BYTES], [REWARD_BASE], 16)]:
        with pytest.raises(IndexError):
            tb.gather_rows(slab, frames, rewards, fsz, CAP)
    with pytest.raises(RuntimeError):  # not pinned
        tb.gather_rows(slab.clone(), [0], [REWARD_BASE], 16, CAP)
    with pytest.raises(RuntimeError):  # more rows than cap
        tb.gather_rows(slab, [0, 16, 32], [REWARD_BASE] * 3, 16, 2)
    torch.cuda.synchronize()


# ---- end to end: the obs-slab row form under the C++ runner ----


@pytest.fixture(scope="module")
def model():
    return drv.make_gpu_model()


def _run(model, env, n_envs, unroll, use_obs_slab, chain, output_device=None):
    # Batches as large as the env count allows (70 envs: past one multiple
    # of 64, pad rows up to 128), as actor_rows_driver.run_gpu.
    batcher = runtime.DynamicBatcher(
        batch_dim=1, minimum_batch_size=n_envs, maximum_batch_size=128,
        timeout_ms=20)
    return rg.run_pool([env] * n_envs, unroll, 2, use_obs_slab,
                       serve=rg.gpu_runner_serve(model), batcher=batcher,
                       envs_per_thread=16, chain=chain,
                       output_device=output_device)


def _assert_matches_model(model, rollouts, frame_shape, unroll):
    frame = torch.from_numpy(np.stack([r[0][0] for r in rollouts], 1))
    reward = torch.from_numpy(np.stack([r[0][1] for r in rollouts], 1))
    done = torch.from_numpy(np.stack([r[0][2] for r in rollouts], 1))
    action = torch.from_numpy(np.stack([r[0][5] for r in rollouts], 1))
    logits = torch.from_numpy(np.stack([r[0][6] for r in rollouts], 1))
    baseline = torch.from_numpy(np.stack([r[0][7] for r in rollouts], 1))
    assert frame.shape == (unroll + 1, len(rollouts)) + frame_shape
    model.train()
    with torch.no_grad():
        ref, _ = model(dict(frame=frame.cuda(), reward=reward.cuda(),
                            done=done.cuda()), ())
    ref = pbl._as_agent_output(ref)
    # Tolerances of tests/test_actor_rows_gpu.py (bf16 MFMA trunk in the
    # runner, fp32 reference).
    torch.testing.assert_close(logits, ref[1].cpu(), rtol=5e-2, atol=5e-3)
    torch.testing.assert_close(baseline, ref[2].cpu(), rtol=5e-2, atol=5e-3)
    assert action.dtype == torch.int64
    assert torch.equal(action, logits.argmax(-1))


@pytest.mark.parametrize("n_envs", [5, 70])
def test_obs_slab_rows_match_model(model, n_envs):
    run = _run(model, drv.GPU_ENV, n_envs, drv.GPU_UNROLL, True, chain=False)
    assert run["slab"] == []
    stats = run["stats"]
    assert stats["batcher_serve_device_gather_batches"] > 0
    assert (stats["batcher_serve_device_gather_batches"]
            == stats["batcher_serve_row_batches"])
    if n_envs > 64:
        assert stats["batcher_avg_batch_size"] > 64
    assert len(run["streams"]) == 2 * n_envs
    _assert_matches_model(model, run["streams"], (4, 84, 84), drv.GPU_UNROLL)


def test_device_gather_equals_host_gather(model):
    device = _run(model, drv.GPU_ENV, 5, drv.GPU_UNROLL, True, chain=True)
    assert device["stats"]["batcher_serve_device_gather_batches"] > 0
    host = _run(model, drv.GPU_ENV, 5, drv.GPU_UNROLL, False, chain=True)
    assert host["stats"]["batcher_serve_device_gather_batches"] == 0
    assert host["stats"]["batcher_serve_row_batches"] > 0
    got = drv.streams_as_dict(device["streams"], 2)
    want = drv.streams_as_dict(host["streams"], 2)
    assert sorted(got) == sorted(want)
    assert len(got) == 5 * 2 * 8
    # Same kernels on the same per-row inputs: equal, not merely close.
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key]), key


def test_full_resolution_frames():
    from torchbeast_amd.models.atari_net import AtariNet

    torch.manual_seed(4321)
    big = AtariNet((3, 210, 160), 6, use_lstm=False,
                   use_last_action=False).cuda()
    run = _run(big, "synthetic:3x210x160:6:7", 3, 2, True, chain=False,
               output_device="cuda:0")
    assert run["slab"] == []
    stats = run["stats"]
    assert stats["batcher_serve_device_gather_batches"] > 0
    # The learner side still assembles its batches from whole slots.
    assert stats["gather_dequeues"] > 0
    assert len(run["streams"]) == 2 * 3
    _assert_matches_model(big, run["streams"], (3, 210, 160), 2)
