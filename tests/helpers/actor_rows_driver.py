"""Drive a real ActorPool over native synthetic envs and rebuild the per-env
streams from what reaches the learner queue.

Imported by tests/test_actor_rows.py and tests/test_actor_rows_gpu.py, and
run as a script (fresh process) when a test needs the other setting of
TBAMD_ACTOR_FASTPATH, which the runtime reads when a pool is constructed:

    python actor_rows_driver.py cpu OUT.npz ENVS_PER_THREAD
    python actor_rows_driver.py gpu OUT.npz N_ENVS
    python actor_rows_driver.py exit - ENVS_PER_THREAD

`exit` runs the CPU configuration with a model forward in the inference
threads and then leaves through an ordinary interpreter exit right after
closing the queues, daemon threads still unwinding, as bench.py does.
"""

import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from torchbeast_amd import runtime  # noqa: E402

CPU_ENV = "synthetic:1x8x16:3:10"
CPU_UNROLL = 4
CPU_ENVS = 6
EPISODE_LEN = 10


def det_policy(env_outputs, agent_state):
    """Deterministic, per-sample function of the observation only."""
    frame, _reward, _done, episode_step, _ret = env_outputs
    b = frame.shape[1]
    f0 = frame.reshape(1, b, -1)[..., 0].to(torch.int64)
    f1 = frame.reshape(1, b, -1)[..., 1].to(torch.int64)
    es = episode_step.to(torch.int64)
    action = (f0 + es) % 3
    logits = torch.stack([f0, f1, es], dim=-1).float() / 255.0
    baseline = (f0 - f1).float() / 255.0
    return ((action, logits, baseline), agent_state)


def counting_policy(env_outputs, agent_state):
    """Agent state counts the steps since the last done."""
    (action, logits, baseline), _ = det_policy(env_outputs, agent_state)
    done = env_outputs[2]
    b = done.shape[1]
    (state,) = agent_state
    new_state = state * (~done).float().view(1, b, 1) + 1
    return ((action, logits, baseline), (new_state,))


def flat_rollout(item):
    """((env 5-tuple, agent 3-tuple), state) -> (list of 8 arrays [T+1, ...],
    list of state arrays), batch dim (size 1) dropped."""
    (env_outputs, agent_outputs), state = item
    leaves = [t[:, 0].contiguous().numpy().copy()
              for t in tuple(env_outputs) + tuple(agent_outputs)]
    states = [t.contiguous().numpy().copy() for t in runtime._tbruntime.flatten(state)]
    return leaves, states


class Streams:
    """Chains rollouts into per-env streams: row 0 of a rollout equals row T
    of its predecessor on every leaf; a stream starts at an initial row
    (done=True, episode_step=0)."""

    def __init__(self):
        self.streams = []  # list of lists of (leaves, states)

    @staticmethod
    def _row(leaves, t):
        return tuple(leaf[t].tobytes() for leaf in leaves)

    def add(self, leaves, states):
        first = self._row(leaves, 0)
        matches = [s for s in self.streams if self._row(s[-1][0], -1) == first]
        initial = bool(leaves[2][0]) and int(leaves[3][0]) == 0
        assert len(matches) <= 1, "ambiguous predecessor: pick other seeds"
        if matches:
            matches[0].append((leaves, states))
        else:
            assert initial, "rollout has no predecessor and is no initial one"
            self.streams.append([(leaves, states)])

    def min_len(self, n_streams):
        if len(self.streams) < n_streams:
            return 0
        return min(len(s) for s in self.streams)

    def ordered(self):
        """Streams in a process-independent order (by initial frame)."""
        out = sorted(self.streams, key=lambda s: s[0][0][0][0].tobytes())
        keys = [s[0][0][0][0].tobytes() for s in out]
        assert len(set(keys)) == len(keys), "initial frames are not distinct"
        return out


def run_streams(addresses, unroll, n_per_stream, envs_per_thread=1,
                serve=None, policy=det_policy, initial_agent_state=(),
                batcher=None, max_rollouts=2000, chain=True, n_threads=1):
    """Run a pool until every stream has n_per_stream rollouts (chain=False:
    until that many rollouts in all arrived, returned as a flat list of
    (leaves, states) with no stream reconstruction). `serve` (optional) is
    called with the batcher and must start whatever answers it, returning a
    stop function; default: one Python thread applying `policy`. Returns
    (streams or list, learner_queue stats)."""
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=1,
        maximum_queue_size=8)
    if batcher is None:
        batcher = runtime.DynamicBatcher(
            batch_dim=1, minimum_batch_size=1, maximum_batch_size=64,
            timeout_ms=2)
    pool = runtime.ActorPool(
        unroll_length=unroll, learner_queue=learner_queue,
        inference_batcher=batcher, env_server_addresses=addresses,
        initial_agent_state=initial_agent_state, rollout_budget_mb=1,
        envs_per_thread=envs_per_thread)
    errors = []

    def run_pool():
        try:
            pool.run()
        except Exception as e:  # surfaced by the caller
            errors.append(e)

    pool_thread = threading.Thread(target=run_pool, daemon=True)
    pool_thread.start()

    stop = None
    if serve is not None:
        stop = serve(batcher)
    else:
        def inference():
            for batch in batcher:
                batch.set_outputs(policy(*batch.get_inputs()))
        for _ in range(n_threads):
            threading.Thread(target=inference, daemon=True).start()

    streams = Streams()
    it = iter(learner_queue)
    got = 0
    flat = []
    while (streams.min_len(len(addresses)) < n_per_stream if chain
           else got < n_per_stream * len(addresses)):
        assert got < max_rollouts and not errors, errors
        if chain:
            streams.add(*flat_rollout(next(it)))
        else:
            flat.append(flat_rollout(next(it)))
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
    return (streams if chain else flat), stats


def save_streams(path, streams, n_per_stream, stats=None):
    out = streams_as_dict(streams, n_per_stream)
    for k, v in (stats or {}).items():
        out["stat_" + k] = np.asarray(v)
    np.savez(path, **out)


def streams_as_dict(streams, n_per_stream):
    out = {}
    for s, stream in enumerate(streams.ordered()):
        for r, (leaves, states) in enumerate(stream[:n_per_stream]):
            for j, leaf in enumerate(leaves):
                out[f"s{s}_r{r}_l{j}"] = leaf
            for j, st in enumerate(states):
                out[f"s{s}_r{r}_state{j}"] = st
    return out


def run_cpu(envs_per_thread, n_per_stream=4):
    return run_streams([CPU_ENV] * CPU_ENVS, CPU_UNROLL, n_per_stream,
                       envs_per_thread=envs_per_thread)


GPU_ENV = "synthetic:4x84x84:6:7"
GPU_UNROLL = 4


def make_gpu_model():
    from torchbeast_amd.models.atari_net import AtariNet

    torch.manual_seed(1234)
    return AtariNet((4, 84, 84), 6, use_lstm=False,
                    use_last_action=False).cuda()


def run_gpu(n_envs, model=None, n_per_stream=2, chain=True):
    """C++ runner, greedy, on `n_envs` synthetic 4x84x84 envs."""
    from torchbeast_amd import polybeast_learner as pbl

    if model is None:
        model = make_gpu_model()
    # Batches as large as the env count allows, so that 70 envs make
    # batches past one multiple of 64 (pad rows up to 128).
    batcher = runtime.DynamicBatcher(
        batch_dim=1, minimum_batch_size=n_envs, maximum_batch_size=128,
        timeout_ms=20)

    def serve(b):
        runner = pbl.make_inference_runner(model, b, greedy=True)
        runner.start(2)
        return runner.stop

    return run_streams([GPU_ENV] * n_envs, GPU_UNROLL, n_per_stream,
                       envs_per_thread=16, serve=serve, batcher=batcher,
                       chain=chain)


if __name__ == "__main__":
    mode, out_path, arg = sys.argv[1], sys.argv[2], int(sys.argv[3])
    if mode == "exit":
        lin = torch.nn.Linear(128, 3)

        def slow_policy(env_outputs, agent_state):
            # A real forward: tensor ops drop and retake the GIL.
            frame = env_outputs[0]
            for _ in range(20):
                lin(frame.reshape(frame.shape[1], -1).float())
            return det_policy(env_outputs, agent_state)

        run_streams([CPU_ENV] * CPU_ENVS, CPU_UNROLL, 2,
                    envs_per_thread=arg, policy=slow_policy, n_threads=4)
        print("exiting", flush=True)
        sys.exit(0)
    if mode == "cpu":
        result, _ = run_cpu(arg)
        save_streams(out_path, result, 4)
    else:
        result, stats = run_gpu(arg)
        save_streams(out_path, result, 2, {
            "serve_row_batches": stats["batcher_serve_row_batches"]})
    # Daemon threads may still sit in native waits; skip their teardown.
    sys.stdout.flush()
    os._exit(0)
