"""Learner-batch assembly by slot DMA + unpack kernel (GPU).

(a) The unpack kernel against the host reference unpack, bit for bit, over
    the row widths it has paths for.
(b) A GPU-output BatchingQueue behind a real ActorPool: the default (gather)
    path and TBAMD_QUEUE_GATHER=0 (per-leaf copies) deliver bit-identical
    streams, and the counters say which path ran.
"""

import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import actor_rows_driver as drv  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

_C = runtime._tbruntime


# ---------------------------------------------------------------------------
# (a) kernel vs host reference
# ---------------------------------------------------------------------------

def _packed(layouts):
    """(outer, inner) list -> [(src_off, outer, inner)] packed like a rollout
    slot (256-byte aligned columns) and the staging stride."""
    columns, used = [], 0
    for outer, inner in layouts:
        off = (used + 255) & ~255
        columns.append((off, outer, inner))
        used = off + outer * inner
    return columns, (used + 255) & ~255


def _check(columns, stride, B, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    staging = torch.randint(0, 256, (B * stride,), dtype=torch.uint8,
                            generator=gen)
    want = _C.unpack_rollouts_host(staging, stride, B, columns)
    got = _C.unpack_rollouts(staging.cuda(), stride, B, columns)
    torch.cuda.synchronize()
    assert len(got) == len(want) == len(columns)
    for (off, outer, inner), g, w in zip(columns, got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and g.is_contiguous()
        assert tuple(g.shape) == tuple(w.shape) == (outer, B, inner)
        assert torch.equal(g.cpu(), w), (off, outer, inner, B)
    return staging, want


LAYOUTS = [(5, 1), (5, 4), (5, 8), (5, 24), (5, 48), (5, 192), (1, 192)]


def test_host_reference_is_the_transpose():
    """The oracle itself, against plain indexing."""
    columns, stride = _packed(LAYOUTS)
    staging, want = _check(columns, stride, 3)
    rows = staging.view(3, stride)
    for (off, outer, inner), w in zip(columns, want):
        ref = rows[:, off:off + outer * inner].reshape(3, outer, inner)
        assert torch.equal(w, ref.transpose(0, 1).contiguous())


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_single_column(B, layout):
    columns, stride = _packed([layout])
    _check(columns, stride, B)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_kernel_all_layouts_one_launch(B):
    columns, stride = _packed(LAYOUTS)
    _check(columns, stride, B, seed=B)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_kernel_unaligned_column(B):
    # inner = 7 at an odd offset: the byte path; and next to aligned ones.
    _check([(13, 5, 7)], 256, B)
    _check([(0, 5, 16), (81, 5, 7), (128, 5, 8)], 256, B)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_kernel_sixteen_columns(B):
    layouts = (LAYOUTS + LAYOUTS + [(3, 2), (2, 12)])[:16]
    columns, stride = _packed(layouts)
    assert len(columns) == 16
    _check(columns, stride, B)
    # The staging tensor is large enough for 17 columns, so only the
    # column-count check can refuse this call.
    with pytest.raises(RuntimeError, match="columns"):
        _C.unpack_rollouts(torch.zeros(B * 4352, dtype=torch.uint8).cuda(),
                           4352, B, [(i * 256, 1, 16) for i in range(17)])


def test_kernel_workgroup_per_row_widths():
    # Rows of >= 256 bytes take the workgroup-per-row path; its 16-, 8-, 4-
    # and 1-byte widths, rows longer than one pass of the workgroup, and a
    # lane-per-row column spanning several workgroups.
    for B in (1, 3, 33):
        columns, stride = _packed([(3, 4112), (3, 264), (3, 260), (3, 257),
                                   (2, 4099), (20, 4)])
        _check(columns, stride, B)
    # Staging rows that are themselves only 4-byte aligned.
    _check([(4, 3, 272), (820, 3, 16)], 868, 3)


def test_kernel_headline_row_width():
    columns, stride = _packed([(2, 28224), (2, 4), (2, 1), (2, 24)])
    _check(columns, stride, 2)


def test_kernel_rejects_out_of_range_columns():
    staging = torch.zeros(3 * 256, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError):
        _C.unpack_rollouts(staging, 256, 3, [(200, 5, 16)])  # past the row
    with pytest.raises(RuntimeError):
        _C.unpack_rollouts(staging, 256, 4, [(0, 5, 16)])  # past staging


# ---------------------------------------------------------------------------
# (b) through a real ActorPool
# ---------------------------------------------------------------------------

N_ENVS = 6
BATCH = 3
N_PER_STREAM = 4


def _run_arm(policy, initial_agent_state):
    learner_queue = runtime.BatchingQueue(
        batch_dim=1, minimum_batch_size=BATCH, maximum_batch_size=BATCH,
        maximum_queue_size=8, output_device="cuda")
    batcher = runtime.DynamicBatcher(
        batch_dim=1, minimum_batch_size=1, maximum_batch_size=64,
        timeout_ms=2)
    pool = runtime.ActorPool(
        unroll_length=drv.CPU_UNROLL, learner_queue=learner_queue,
        inference_batcher=batcher,
        env_server_addresses=[drv.CPU_ENV] * N_ENVS,
        initial_agent_state=initial_agent_state, rollout_budget_mb=1,
        envs_per_thread=3)
    errors = []

    def run_pool():
        try:
            pool.run()
        except Exception as e:  # surfaced below
            errors.append(e)

    def inference():
        for batch in batcher:
            batch.set_outputs(policy(*batch.get_inputs()))

    pool_thread = threading.Thread(target=run_pool, daemon=True)
    pool_thread.start()
    threading.Thread(target=inference, daemon=True).start()

    streams = drv.Streams()
    it = iter(learner_queue)
    dequeues = 0
    while streams.min_len(N_ENVS) < N_PER_STREAM:
        assert dequeues < 200 and not errors, errors
        (env_outputs, agent_outputs), state = next(it)
        dequeues += 1
        leaves = tuple(env_outputs) + tuple(agent_outputs)
        assert len(leaves) == 8
        for t in leaves:
            assert t.is_cuda and t.is_contiguous()
            assert t.shape[:2] == (drv.CPU_UNROLL + 1, BATCH)
        host = [t.cpu().numpy() for t in leaves]
        host_state = [t.cpu().numpy() for t in _C.flatten(state)]
        for b in range(BATCH):
            streams.add([h[:, b].copy() for h in host],
                        [s[:, b:b + 1].copy() for s in host_state])
    stats = learner_queue.stats()
    batcher.close()
    learner_queue.close()
    pool_thread.join(5)
    assert not pool_thread.is_alive(), "actor pool did not unwind"
    assert not errors, errors
    assert stats["dequeues"] == dequeues
    return drv.streams_as_dict(streams, N_PER_STREAM), stats


@pytest.mark.parametrize("mixed", [False, True])
def test_gather_equals_per_leaf_copies(monkeypatch, mixed):
    if mixed:
        policy, state = drv.counting_policy, (torch.zeros(1, 1, 1),)
    else:
        policy, state = drv.det_policy, ()
    monkeypatch.delenv("TBAMD_QUEUE_GATHER", raising=False)
    fast, fast_stats = _run_arm(policy, state)
    assert fast_stats["gather_dequeues"] == fast_stats["dequeues"]
    assert fast_stats["gather_columns"] == 8 * fast_stats["dequeues"]

    # Read when the queue is constructed.
    monkeypatch.setenv("TBAMD_QUEUE_GATHER", "0")
    base, base_stats = _run_arm(policy, state)
    assert base_stats["gather_dequeues"] == 0
    assert base_stats["gather_columns"] == 0

    assert sorted(fast) == sorted(base)
    assert len(fast) == N_ENVS * N_PER_STREAM * (8 + (1 if mixed else 0))
    for key in sorted(fast):
        assert fast[key].dtype == base[key].dtype, key
        assert fast[key].shape == base[key].shape, key
        assert np.array_equal(fast[key], base[key]), key
    if mixed:
        # The agent state really varies (steps since the last done).
        states = {float(v.ravel()[0]) for k, v in fast.items()
                  if "state" in k}
        assert len(states) > 1
