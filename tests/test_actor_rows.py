"""Rollout rows written in place (the actor fast path) on native synthetic
envs with Python inference threads: equality with the nest/promise path,
episode bookkeeping, recurrent state, failure delivery, shutdown and slot
accounting. CPU only."""

import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import actor_rows_driver as drv  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = drv.CPU_UNROLL


def _joined(stream):
    """One stream's rollouts joined into per-leaf arrays without the
    duplicated overlap rows."""
    leaves = [[] for _ in range(8)]
    for r, (roll, _) in enumerate(stream):
        for j, leaf in enumerate(roll):
            leaves[j].append(leaf if r == 0 else leaf[1:])
    return [np.concatenate(x) for x in leaves]


@pytest.mark.parametrize("envs_per_thread", [1, 3])
def test_fast_path_equals_legacy_path(envs_per_thread, tmp_path):
    assert os.environ.get("TBAMD_ACTOR_FASTPATH", "1") != "0"
    streams, _ = drv.run_cpu(envs_per_thread)
    fast = drv.streams_as_dict(streams, 4)
    # ordered() asserted that the seeds give distinct initial frames.
    assert len(streams.streams) == drv.CPU_ENVS

    out = str(tmp_path / "legacy.npz")
    env = dict(os.environ, TBAMD_ACTOR_FASTPATH="0")
    subprocess.run(
        [sys.executable, os.path.join(ROOT, "tests", "helpers",
                                      "actor_rows_driver.py"),
         "cpu", out, str(envs_per_thread)],
        cwd=ROOT, env=env, timeout=120, check=True)
    legacy = dict(np.load(out))

    assert sorted(fast) == sorted(legacy)
    # 6 streams x 4 rollouts x (8 leaves; the state nest is empty)
    assert len(fast) == drv.CPU_ENVS * 4 * 8
    for key in sorted(fast):
        assert fast[key].dtype == legacy[key].dtype, key
        assert fast[key].shape == legacy[key].shape, key
        assert fast[key].tobytes() == legacy[key].tobytes(), key


def test_episode_bookkeeping_across_done():
    streams, _ = drv.run_cpu(3, n_per_stream=6)  # 24 steps: two dones each
    for stream in streams.ordered():
        _, reward, done, step, ret, action, logits, _ = _joined(stream)
        assert done[0] and step[0] == 0 and reward[0] == 0
        n_done = 0
        for t in range(1, len(done)):
            assert reward[t] in (-1.0, 0.0, 1.0)
            if done[t - 1]:
                assert step[t] == 1
                assert ret[t] == reward[t]
            else:
                assert step[t] == step[t - 1] + 1
                assert ret[t] == ret[t - 1] + reward[t]
            assert bool(done[t]) == (step[t] == drv.EPISODE_LEN)
            n_done += bool(done[t])
        assert n_done >= 2
        # The recorded agent outputs are the policy's, row by row.
        assert (logits[:, 2] * 255.0).round().astype(np.int64).tolist() == \
            step.tolist()
        assert ((action - step) % 3 == (logits[:, 0] * 255).round() % 3).all()


def test_recurrent_state_is_state_before_first_row():
    streams, _ = drv.run_streams(
        [drv.CPU_ENV] * drv.CPU_ENVS, T, 6, envs_per_thread=3,
        policy=drv.counting_policy,
        initial_agent_state=(torch.zeros(1, 1, 1),))
    checked = 0
    for stream in streams.ordered():
        for leaves, states in stream:
            (state,) = states
            assert state.shape == (1, 1, 1)
            # Steps counted since the last done == episode_step of the
            # rollout's first row (0 for the initial row, L at a done row).
            assert float(state.reshape(())) == float(leaves[3][0])
            checked += 1
    assert checked >= drv.CPU_ENVS * 6


def _pool(envs_per_thread=3, queue_size=8):
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=1,
        maximum_queue_size=queue_size)
    batcher = runtime.DynamicBatcher(batch_dim=1, minimum_batch_size=1,
                                     maximum_batch_size=64, timeout_ms=2)
    pool = runtime.ActorPool(
        unroll_length=T, learner_queue=learner_queue,
        inference_batcher=batcher,
        env_server_addresses=[drv.CPU_ENV] * drv.CPU_ENVS,
        initial_agent_state=(), rollout_budget_mb=1,
        envs_per_thread=envs_per_thread)
    result = {}

    def run():
        try:
            pool.run()
            result["ok"] = True
        except Exception as e:
            result["error"] = e

    thread = threading.Thread(target=run, daemon=True)
    thread.start()
    return learner_queue, batcher, thread, result


def test_dropped_batch_raises_async_error():
    learner_queue, batcher, thread, result = _pool()
    served = []
    drop = threading.Event()

    def inference():
        for batch in batcher:
            if drop.is_set() and "dropped" not in served:
                served.append("dropped")
                del batch  # destroyed without outputs
                continue
            batch.set_outputs(drv.det_policy(*batch.get_inputs()))
            served.append(1)

    threading.Thread(target=inference, daemon=True).start()
    # A whole rollout has arrived: every stream is past its nest-form first
    # step, so the dropped batch holds row requests and the error travels
    # through the actor mailboxes, not through a promise.
    next(iter(learner_queue))
    drop.set()
    t0 = time.monotonic()
    while "dropped" not in served:
        assert time.monotonic() - t0 < 5
        time.sleep(0.001)
    # Threads whose requests were not in the dropped batch unwind by the
    # closed queues; run() then rethrows the failure.
    batcher.close()
    learner_queue.close()
    thread.join(5)
    assert not thread.is_alive(), "run() hangs after a dropped batch"
    assert time.monotonic() - t0 < 5
    assert isinstance(result.get("error"), runtime.AsyncError), result


def test_close_unwinds_streams_holding_slots():
    learner_queue, batcher, thread, result = _pool()

    def inference():
        for batch in batcher:
            batch.set_outputs(drv.det_policy(*batch.get_inputs()))

    threading.Thread(target=inference, daemon=True).start()
    it = iter(learner_queue)
    for _ in range(3):
        next(it)
    assert learner_queue.stats()["slab_held"] >= drv.CPU_ENVS
    t0 = time.monotonic()
    batcher.close()
    learner_queue.close()
    thread.join(5)
    assert not thread.is_alive(), "run() did not unwind"
    assert time.monotonic() - t0 < 5
    assert result == {"ok": True}


def test_slot_accounting():
    learner_queue, batcher, thread, _ = _pool()

    def inference():
        for batch in batcher:
            batch.set_outputs(drv.det_policy(*batch.get_inputs()))

    threading.Thread(target=inference, daemon=True).start()
    it = iter(learner_queue)
    for _ in range(50):
        next(it)
    stats = learner_queue.stats()
    assert stats["slab_slots"] >= drv.CPU_ENVS + 8 + 2
    assert stats["slab_free"] + stats["slab_pending"] + stats["slab_held"] \
        == stats["slab_slots"]
    # Every stream holds the slot it fills (plus whatever is queued).
    assert stats["slab_held"] >= drv.CPU_ENVS
    assert stats["slab_held"] <= 2 * drv.CPU_ENVS + 8
    batcher.close()
    learner_queue.close()
    thread.join(5)
    assert not thread.is_alive()


def test_exit_right_after_close_is_clean():
    """A driver that closes the queues and leaves through an ordinary
    interpreter exit while its daemon inference threads are still unwinding
    (what bench.py does) must exit 0: rows unwind the actor pool within a
    millisecond of close(), so the consumers of the closed batcher stay out
    of the interpreter for a moment and park if it is finalizing."""
    for _ in range(3):
        out = subprocess.run(
            [sys.executable, os.path.join(ROOT, "tests", "helpers",
                                          "actor_rows_driver.py"),
             "exit", "-", "3"],
            cwd=ROOT, timeout=120, capture_output=True)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        assert b"exiting" in out.stdout
