"""State rows (ActorPool(recurrent_rows=...)), host side: the recurrent state
of every stream in the pool's block, which state a rollout records, the
obs-slab row form for a recurrent agent, equality with the pool without the
switch, and the checked pointer table behind the LSTM serve kernels. CPU
only; the pool is served by a Python thread."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import actor_rows_driver as drv  # noqa: E402
import state_rows_driver as sr  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

ADDRESSES = [drv.CPU_ENV] * drv.CPU_ENVS
T = drv.CPU_UNROLL


def _check_recorded_states(streams, n_min):
    checked = 0
    for stream in streams.ordered():
        for leaves, states in stream:
            h, c = states
            assert h.shape == (sr.STATE_L, 1, sr.STATE_H) and c.shape == h.shape
            # Steps counted since the last done == episode_step of the
            # rollout's first row (0 for the initial row, L at a done row).
            want = float(leaves[3][0])
            assert (h == want).all(), (h, want)
            assert (c == 2 * want).all(), (c, want)
            checked += 1
    assert checked >= n_min


def test_recorded_state_is_state_before_first_row():
    run = sr.run_pool(ADDRESSES, T, 6, recurrent_rows=True)
    assert len(run["streams"].streams) == drv.CPU_ENVS
    _check_recorded_states(run["streams"], drv.CPU_ENVS * 6)
    # A Python thread served the pool: no batch took the runner's path.
    assert run["stats"]["batcher_serve_state_row_batches"] == 0


def test_recorded_states_survive_later_steps():
    """Rollouts wait in the learner queue while every stream is served at
    least 2 T further steps: a recorded state that aliased the block would
    have moved on with it."""
    run = sr.run_pool(ADDRESSES, T, 4, recurrent_rows=True, queue_size=64,
                      wait_queued=4 * drv.CPU_ENVS)
    _check_recorded_states(run["streams"], drv.CPU_ENVS * 4)


def test_obs_slab_row_form_for_a_recurrent_agent():
    run = sr.run_pool(ADDRESSES, T, 2, use_obs_slab=True, recurrent_rows=True)
    # No second slab (asked for from a thread joined after 5 s) ...
    assert run["slab"] == []
    # ... and requests that carry u8 frames, not int32 slot ids.
    assert run["inputs"]
    for first_leaf in run["inputs"]:
        assert first_leaf.dtype == torch.uint8
        assert first_leaf.shape[2:] == (1, 8, 16)
    _check_recorded_states(run["streams"], drv.CPU_ENVS * 2)


@pytest.mark.parametrize("use_obs_slab", [False, True])
def test_switch_on_equals_switch_off(use_obs_slab):
    n = 4
    on = sr.run_pool(ADDRESSES, T, n, use_obs_slab=use_obs_slab,
                     recurrent_rows=True)
    # Off: plain rows (a pool in obs-slab mode would send slot ids).
    off = sr.run_pool(ADDRESSES, T, n, use_obs_slab=False,
                      recurrent_rows=False)
    got = drv.streams_as_dict(on["streams"], n)
    want = drv.streams_as_dict(off["streams"], n)
    assert sorted(got) == sorted(want)
    # 8 leaves and (h, c) per rollout
    assert len(got) == drv.CPU_ENVS * n * 10
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype, key
        assert got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), key


def _make_pool(state, **kwargs):
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=1,
        maximum_queue_size=8)
    batcher = runtime.DynamicBatcher(batch_dim=1, minimum_batch_size=1,
                                     maximum_batch_size=64, timeout_ms=2)
    return runtime.ActorPool(
        unroll_length=T, learner_queue=learner_queue,
        inference_batcher=batcher, env_server_addresses=ADDRESSES,
        initial_agent_state=state, rollout_budget_mb=1, **kwargs)


def test_switch_needs_an_h_c_state(monkeypatch):
    one_leaf = (torch.zeros(1, 1, 1),)
    with pytest.raises(ValueError):
        _make_pool(one_leaf, recurrent_rows=True)
    with pytest.raises(ValueError):
        _make_pool((), recurrent_rows=True)
    with pytest.raises(ValueError):  # not [L, 1, H]
        _make_pool((torch.zeros(1, 2, 4), torch.zeros(1, 2, 4)),
                   recurrent_rows=True)
    with pytest.raises(ValueError):  # not float32
        _make_pool((torch.zeros(1, 1, 4, dtype=torch.float64),) * 2,
                   recurrent_rows=True)
    _make_pool(sr.initial_state(), recurrent_rows=True)
    _make_pool(one_leaf, recurrent_rows=False)

    # The environment variable with such a state keeps today's behaviour:
    # slot-id requests in obs-slab mode, the counted state recorded.
    import row_gather_driver as rg

    monkeypatch.setenv("TBAMD_RECURRENT_ROWS", "1")
    run = rg.run_pool(ADDRESSES, T, 2, use_obs_slab=True,
                      initial_agent_state=one_leaf, policy=rg.slot_policy,
                      chain=False)
    assert len(run["slab"]) == 3
    assert run["inputs"]
    for ids in run["inputs"]:
        assert ids.dtype == torch.int32 and ids.dim() == 2


def test_environment_variable_turns_the_switch_on(monkeypatch):
    monkeypatch.setenv("TBAMD_RECURRENT_ROWS", "1")
    run = sr.run_pool(ADDRESSES, T, 2, use_obs_slab=True, recurrent_rows=None)
    assert run["slab"] == []
    for first_leaf in run["inputs"]:
        assert first_leaf.dtype == torch.uint8
    _check_recorded_states(run["streams"], drv.CPU_ENVS * 2)


# ---- build_state_table over plain integers ----

STATE_BASE = 0x7F0000100000  # 16-aligned addresses nobody dereferences
STATE_BYTES = 1 << 17
SLAB_BASE = 0x7E0000000000
SLAB_BYTES = 1 << 20
N_FLOATS = 2 * 2 * 513  # (h, c) x L x H of the shallow model
N_BYTES = 4 * N_FLOATS


def _table(in_offsets, out_offsets, done_offsets, n_floats=N_FLOATS):
    return runtime._tbruntime.build_state_table(
        STATE_BASE, STATE_BYTES, SLAB_BASE, SLAB_BYTES,
        [STATE_BASE + o for o in in_offsets],
        [STATE_BASE + o for o in out_offsets],
        [SLAB_BASE + o for o in done_offsets], n_floats)


def test_state_table_stores_checked_addresses():
    ins = [0, 6 * N_BYTES, 2 * N_BYTES + 4]
    outs = [N_BYTES, 7 * N_BYTES, 3 * N_BYTES + 4]
    dones = [7, 0, SLAB_BYTES - 1]
    i, o, d = _table(ins, outs, dones)
    assert i == [STATE_BASE + x for x in ins]
    assert o == [STATE_BASE + x for x in outs]
    assert d == [SLAB_BASE + x for x in dones]


def test_state_table_bounds():
    # A range ending exactly at the block's end: fine, in and out.
    _table([0], [STATE_BYTES - N_BYTES], [0])
    _table([STATE_BYTES - N_BYTES], [0], [0])
    # One byte (one float, to stay aligned; and one byte, misaligned) past.
    with pytest.raises(IndexError):
        _table([0], [STATE_BYTES - N_BYTES + 4], [0])
    with pytest.raises(IndexError):
        _table([STATE_BYTES - N_BYTES + 4], [0], [0])
    with pytest.raises(IndexError):
        _table([0], [STATE_BYTES - N_BYTES + 1], [0])
    # Before the block.
    with pytest.raises(IndexError):
        _table([-4], [N_BYTES], [0])
    with pytest.raises(IndexError):
        _table([0], [-N_BYTES], [0])
    # Far outside, in the slab's address range.
    with pytest.raises(IndexError):
        _table([SLAB_BASE - STATE_BASE], [0], [0])
    # The done byte: last byte of the slab is fine, the next one is not, nor
    # is one before the slab; nor a second request's.
    _table([0], [N_BYTES], [SLAB_BYTES - 1])
    with pytest.raises(IndexError):
        _table([0], [N_BYTES], [SLAB_BYTES])
    with pytest.raises(IndexError):
        _table([0], [N_BYTES], [-1])
    with pytest.raises(IndexError):
        _table([0, 2 * N_BYTES], [N_BYTES, 3 * N_BYTES], [0, SLAB_BYTES])


def test_state_table_alignment_and_empty_batch():
    with pytest.raises(ValueError):
        _table([2], [N_BYTES], [0])
    with pytest.raises(ValueError):
        _table([0], [N_BYTES + 1], [0])
    with pytest.raises(ValueError):
        _table([], [], [])
    with pytest.raises(ValueError):
        _table([0], [N_BYTES], [0], n_floats=0)
    with pytest.raises(ValueError):  # one done address short
        _table([0, 2 * N_BYTES], [N_BYTES, 3 * N_BYTES], [0])


def test_state_table_refuses_overlaps():
    # The same stream twice: same in and out ranges.
    with pytest.raises(ValueError):
        _table([0, 0], [N_BYTES, N_BYTES], [0, 1])
    # The same in range, different out ranges; and the reverse.
    with pytest.raises(ValueError):
        _table([0, 0], [N_BYTES, 2 * N_BYTES], [0, 1])
    with pytest.raises(ValueError):
        _table([0, 2 * N_BYTES], [N_BYTES, N_BYTES], [0, 1])
    # An in range equal to another request's out range, and its own.
    with pytest.raises(ValueError):
        _table([0, N_BYTES], [N_BYTES, 2 * N_BYTES], [0, 1])
    with pytest.raises(ValueError):
        _table([0], [0], [0])
    # Partial overlaps, by one float, either way round.
    with pytest.raises(ValueError):
        _table([0], [N_BYTES - 4], [0])
    with pytest.raises(ValueError):
        _table([N_BYTES - 4], [0], [0])
    with pytest.raises(ValueError):
        _table([0, 3 * N_BYTES - 4], [N_BYTES, 2 * N_BYTES], [0, 1])
    # Back to back is no overlap.
    _table([0, 2 * N_BYTES], [N_BYTES, 3 * N_BYTES], [0, 1])


def test_stateless_pool_leaves_the_counter_at_zero():
    _, stats = drv.run_cpu(3, n_per_stream=2)
    assert stats["batcher_serve_state_row_batches"] == 0
