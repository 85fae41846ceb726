"""Obs-slab mode on rollout rows (the row form for large frames), host side:
which pools take it, what their requests look like, that the rollouts equal
those of the plain row path, and the pointer-table builder behind the GPU
gather. CPU only."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import actor_rows_driver as drv  # noqa: E402
import row_gather_driver as rg  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

ADDRESSES = [drv.CPU_ENV] * drv.CPU_ENVS
N_PER_STREAM = 4


def test_row_form_in_obs_slab_mode():
    assert os.environ.get("TBAMD_ACTOR_FASTPATH", "1") != "0"
    slab_run = rg.run_pool(ADDRESSES, drv.CPU_UNROLL, N_PER_STREAM,
                           use_obs_slab=True, policy=rg.env_policy)
    # No second slab (asked for before anything served the pool, from a
    # thread joined after 5 s) ...
    assert slab_run["slab"] == []
    # ... and requests that carry frames, not int32 slot ids.
    assert slab_run["inputs"]
    for first_leaf in slab_run["inputs"]:
        assert first_leaf.dtype == torch.uint8
        assert first_leaf.shape[2:] == (1, 8, 16)
    streams = slab_run["streams"]
    assert len(streams.streams) == drv.CPU_ENVS
    # The rows travelled in place: the learner queue got slab slots back.
    assert slab_run["stats"]["slab_slots"] > 0

    plain_run = rg.run_pool(ADDRESSES, drv.CPU_UNROLL, N_PER_STREAM,
                            use_obs_slab=False, policy=rg.env_policy)
    assert plain_run["slab"] == []
    got = drv.streams_as_dict(streams, N_PER_STREAM)
    want = drv.streams_as_dict(plain_run["streams"], N_PER_STREAM)
    assert sorted(got) == sorted(want)
    assert len(got) == drv.CPU_ENVS * N_PER_STREAM * 8
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype, key
        assert got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), key


def test_recurrent_agent_keeps_slot_ids():
    run = rg.run_pool(ADDRESSES, drv.CPU_UNROLL, 2, use_obs_slab=True,
                      initial_agent_state=(torch.zeros(1, 1, 1),),
                      policy=rg.slot_policy, chain=False)
    slab = run["slab"]
    assert len(slab) == 3
    assert slab[0].shape == (drv.CPU_ENVS, 1, 8, 16)
    assert slab[0].dtype == torch.uint8
    assert slab[1].shape == (drv.CPU_ENVS,) and slab[2].shape == (drv.CPU_ENVS,)
    assert run["inputs"]
    seen = set()
    for ids in run["inputs"]:
        assert ids.dtype == torch.int32 and ids.dim() == 2
        seen.update(ids[0].tolist())
    assert seen == set(range(drv.CPU_ENVS))
    # Rollouts still carry whole frames and the counted agent state.
    assert len(run["streams"]) == 2 * drv.CPU_ENVS
    for leaves, states in run["streams"]:
        assert leaves[0].shape == (drv.CPU_UNROLL + 1, 1, 8, 16)
        assert len(states) == 1


BASE = 0x7F0000100000  # a 16-aligned address nobody dereferences
SLAB_BYTES = 1 << 20


def _table(frame_offsets, reward_offsets, fsz):
    return runtime._tbruntime.build_row_table(
        BASE, SLAB_BYTES, [BASE + o for o in frame_offsets],
        [BASE + o for o in reward_offsets], fsz)


@pytest.mark.parametrize("shift,fsz,width", [
    (0, 128, 16), (4, 128, 4), (8, 128, 8), (1, 128, 1),
    (0, 100, 4), (0, 63, 1), (0, 100800, 16)])
def test_table_pointers_and_width(shift, fsz, width):
    stride = (fsz + 255) // 256 * 256
    frames = [4096 + r * stride + shift for r in range(5)]
    rewards = [4 * r for r in range(5)]
    ft, rt, w = _table(frames, rewards, fsz)
    assert ft == [BASE + o for o in frames]
    assert rt == [BASE + o for o in rewards]
    assert w == width


def test_table_width_is_common_to_the_batch():
    _, _, w = _table([4096, 8192, 12288 + 4], [0, 4, 8], 128)
    assert w == 4


def test_table_rejects_rows_outside_the_slab():
    # Ends exactly at the end: fine. One byte past: refused.
    _table([SLAB_BYTES - 128], [0], 128)
    with pytest.raises(IndexError):
        _table([0, SLAB_BYTES - 127], [0, 4], 128)
    with pytest.raises(IndexError):
        _table([0], [SLAB_BYTES], 128)
    # Begins before the slab.
    with pytest.raises(IndexError):
        _table([0, -16], [0, 4], 128)
    with pytest.raises(IndexError):
        _table([0], [-4], 128)
    # A reward that is no aligned float; an empty batch.
    with pytest.raises(ValueError):
        _table([0], [4098], 128)
    with pytest.raises(ValueError):
        _table([], [], 128)
