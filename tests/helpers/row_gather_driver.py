"""Drive an ActorPool in obs-slab mode (or not) and rebuild the per-env
streams, for tests/test_row_gather.py and tests/test_row_gather_gpu.py.

Like actor_rows_driver.run_streams, whose pieces it reuses, but the pool's
obs-slab switch, the learner queue's output device and the env are the
caller's, and what the inference side saw is reported back.
"""

import os
import sys
import threading

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import actor_rows_driver as drv  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402


def flat_rollout(item):
    """drv.flat_rollout for a rollout that may live on the GPU."""
    return drv.flat_rollout(runtime._tbruntime.map(lambda t: t.cpu(), item))


def run_pool(addresses, unroll, n_per_stream, use_obs_slab, *,
             initial_agent_state=(), policy=drv.det_policy, serve=None,
             batcher=None, envs_per_thread=3, output_device=None, chain=True,
             max_rollouts=2000):
    """Run a pool with a 1 MB rollout budget until every stream has
    n_per_stream rollouts (chain=False: until that many arrived in all).

    Inference: `serve(batcher, slab)` if given (returns a stop function), else
    one Python thread applying `policy` to batch.get_inputs(). `slab` is what
    pool.obs_slab() returned, asked for from a thread joined after 5 s.

    Returns a dict: streams (drv.Streams, or the flat list), slab, inputs
    (the first leaf of every get_inputs() the Python thread saw), stats
    (learner queue stats plus the batcher's under "batcher_").
    """
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=1,
        maximum_queue_size=8, output_device=output_device)
    if batcher is None:
        batcher = runtime.DynamicBatcher(
            batch_dim=1, minimum_batch_size=1, maximum_batch_size=64,
            timeout_ms=2)
    pool = runtime.ActorPool(
        unroll_length=unroll, learner_queue=learner_queue,
        inference_batcher=batcher, env_server_addresses=addresses,
        initial_agent_state=initial_agent_state, use_obs_slab=use_obs_slab,
        rollout_budget_mb=1, envs_per_thread=envs_per_thread)
    errors = []

    def run():
        try:
            pool.run()
        except Exception as e:  # surfaced below
            errors.append(e)

    pool_thread = threading.Thread(target=run, daemon=True)
    pool_thread.start()

    inputs = []
    stop = None
    slab_box = []

    def start_serving(slab):
        nonlocal stop
        if serve is not None:
            stop = serve(batcher, slab)
            return

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

    def ask_slab():
        slab_box.append(pool.obs_slab())

    if use_obs_slab and not initial_agent_state:
        # The row form has no second slab: the answer comes at once, before
        # anything serves the pool.
        slab_thread = threading.Thread(target=ask_slab, daemon=True)
        slab_thread.start()
        slab_thread.join(5)
        assert not slab_thread.is_alive(), "obs_slab() blocked"
        start_serving(slab_box[0])
    else:
        # The slot-id form publishes its slab with the first observation,
        # which needs no inference either.
        ask_slab()
        start_serving(slab_box[0])

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
            streams.add(*flat_rollout(item))
        else:
            flat.append(flat_rollout(item))
        got += 1
    stats = learner_queue.stats()
    batcher_stats = batcher.stats()
    batcher.close()
    learner_queue.close()
    pool_thread.join(5)
    assert not pool_thread.is_alive(), "actor pool did not unwind"
    if stop is not None:
        stop()
    assert not errors, errors
    stats.update({"batcher_" + k: v for k, v in batcher_stats.items()})
    return dict(streams=streams if chain else flat, slab=slab_box[0],
                inputs=inputs, stats=stats)


def env_policy(_slab, env_outputs, agent_state):
    return drv.det_policy(env_outputs, agent_state)


def slot_policy(slab, ids, agent_state):
    """Slot-id requests: read the frames from the obs slab; the agent state
    counts steps (one leaf [1, b, 1])."""
    frames = slab[0]
    ids = ids.to(torch.int64)
    b = ids.shape[1]
    f0 = frames.reshape(frames.shape[0], -1)[ids[0], 0].to(torch.int64)
    action = (f0 % 3).reshape(1, b)
    logits = torch.zeros(1, b, 3)
    baseline = torch.zeros(1, b)
    (state,) = agent_state
    return ((action, logits, baseline), (state + 1,))


def gpu_runner_serve(model):
    """serve callback: the C++ runner, greedy, two threads."""
    from torchbeast_amd import polybeast_learner as pbl

    def serve(batcher, slab):
        runner = pbl.make_inference_runner(model, batcher, greedy=True)
        if slab:
            runner.set_obs_slab(*slab)
        runner.start(2)
        return runner.stop

    return serve
