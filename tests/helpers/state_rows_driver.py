"""Drive an ActorPool with state rows (recurrent_rows) on or off and rebuild
the per-env streams, for tests/test_state_rows.py and
tests/test_lstm_serve_gpu.py.

Like row_gather_driver.run_pool, whose pieces it reuses, but the pool's
recurrent_rows switch is the caller's, obs_slab() is always asked for from a
thread joined after 5 s, rollouts can be left waiting in the learner queue
while the pool goes on, and the batcher's counters are read once whatever
serves the pool has stopped.
"""

import os
import sys
import threading
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import actor_rows_driver as drv  # noqa: E402
import row_gather_driver as rg  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

STATE_L = 1
STATE_H = 4


def initial_state():
    return (torch.zeros(STATE_L, 1, STATE_H), torch.zeros(STATE_L, 1, STATE_H))


def counting_hc_policy(_slab, env_outputs, agent_state):
    """h counts the steps since the last done, c counts them twice."""
    (action, logits, baseline), _ = drv.det_policy(env_outputs, agent_state)
    done = env_outputs[2]
    b = done.shape[1]
    h, c = agent_state
    assert h.shape == (STATE_L, b, STATE_H) and c.shape == h.shape
    nd = (~done).float().view(1, b, 1)
    return ((action, logits, baseline), (h * nd + 1, c * nd + 2))


def run_pool(addresses, unroll, n_per_stream, *, use_obs_slab=False,
             recurrent_rows=None, initial_agent_state=None,
             policy=counting_hc_policy, serve=None, batcher=None,
             envs_per_thread=3, output_device=None, chain=True,
             queue_size=8, wait_queued=0, max_rollouts=2000):
    """Run a pool with a 1 MB rollout budget until every stream has
    n_per_stream rollouts (chain=False: until that many arrived in all).

    Inference: `serve(batcher, slab)` if given (returns a stop function), else
    one Python thread applying `policy(slab, *batch.get_inputs())`.
    wait_queued: take nothing from the learner queue before it holds that
    many rollouts (the pool goes on serving steps meanwhile).

    Returns a dict: streams (drv.Streams, or the flat list), slab (what
    obs_slab() answered), inputs (the first leaf of every get_inputs() the
    Python thread saw), stats (learner queue stats plus the batcher's under
    "batcher_", the latter read after the serving side has stopped).
    """
    if initial_agent_state is None:
        initial_agent_state = initial_state()
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=1,
        maximum_queue_size=queue_size, output_device=output_device)
    if batcher is None:
        batcher = runtime.DynamicBatcher(
            batch_dim=1, minimum_batch_size=1, maximum_batch_size=64,
            timeout_ms=2)
    pool = runtime.ActorPool(
        unroll_length=unroll, learner_queue=learner_queue,
        inference_batcher=batcher, env_server_addresses=addresses,
        initial_agent_state=initial_agent_state, use_obs_slab=use_obs_slab,
        rollout_budget_mb=1, envs_per_thread=envs_per_thread,
        recurrent_rows=recurrent_rows)
    errors = []

    def run():
        try:
            pool.run()
        except Exception as e:  # surfaced below
            errors.append(e)

    pool_thread = threading.Thread(target=run, daemon=True)
    pool_thread.start()

    slab_box = []
    slab_thread = threading.Thread(
        target=lambda: slab_box.append(pool.obs_slab()), daemon=True)
    slab_thread.start()
    slab_thread.join(5)
    assert not slab_thread.is_alive(), "obs_slab() blocked"
    slab = slab_box[0]

    inputs = []
    stop = None
    if serve is not None:
        stop = serve(batcher, slab)
    else:
        def inference():
            try:
                for batch in batcher:
                    batch_inputs = batch.get_inputs()
                    inputs.append(runtime._tbruntime.front(batch_inputs))
                    batch.set_outputs(policy(slab, *batch_inputs))
            except Exception as e:  # end the run instead of starving it
                errors.append(e)
                learner_queue.close()

        threading.Thread(target=inference, daemon=True).start()

    if wait_queued:
        t0 = time.monotonic()
        while learner_queue.size() < wait_queued:
            assert time.monotonic() - t0 < 30 and not errors, errors
            time.sleep(0.001)

    streams = drv.Streams()
    flat = []
    it = iter(learner_queue)
    got = 0
    while (streams.min_len(len(addresses)) < n_per_stream if chain
           else got < n_per_stream * len(addresses)):
        assert got < max_rollouts and not errors, errors
        item = next(it, None)
        assert item is not None, errors  # queue closed by a failure
        if chain:
            streams.add(*rg.flat_rollout(item))
        else:
            flat.append(rg.flat_rollout(item))
        got += 1
    stats = learner_queue.stats()
    batcher.close()
    learner_queue.close()
    pool_thread.join(5)
    assert not pool_thread.is_alive(), "actor pool did not unwind"
    if stop is not None:
        stop()
    assert not errors, errors
    stats.update({"batcher_" + k: v for k, v in batcher.stats().items()})
    return dict(streams=streams if chain else flat, slab=slab, inputs=inputs,
                stats=stats)
