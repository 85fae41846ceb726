"""Rollout rows served by the C++ InferenceRunner (GPU): what the runner
writes into the rows agrees with the Python model on the recorded inputs,
and the row serve path agrees with the tensor serve path."""

import os
import subprocess
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
from torchbeast_amd import polybeast_learner as pbl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return drv.make_gpu_model()


@pytest.mark.parametrize("n_envs", [5, 70])
def test_recorded_outputs_match_model(model, n_envs):
    rollouts, stats = drv.run_gpu(n_envs, model=model, chain=False)
    assert len(rollouts) == 2 * n_envs
    # The runner's row path (persistent staging, un-zeroed pad rows) served
    # them, not the get_inputs()/set_outputs() fall-back.
    assert stats["batcher_serve_row_batches"] > 0
    if n_envs > 64:
        # Batches past one multiple of 64: pad rows [b, 128) exist.
        assert stats["batcher_avg_batch_size"] > 64
    frame = torch.from_numpy(np.stack([r[0][0] for r in rollouts], 1))
    reward = torch.from_numpy(np.stack([r[0][1] for r in rollouts], 1))
    done = torch.from_numpy(np.stack([r[0][2] for r in rollouts], 1))
    action = torch.from_numpy(np.stack([r[0][5] for r in rollouts], 1))
    logits = torch.from_numpy(np.stack([r[0][6] for r in rollouts], 1))
    baseline = torch.from_numpy(np.stack([r[0][7] for r in rollouts], 1))
    assert frame.shape == (drv.GPU_UNROLL + 1, 2 * n_envs, 4, 84, 84)
    assert done.any() and not done.all()

    model.train()
    with torch.no_grad():
        ref, _ = model(dict(frame=frame.cuda(), reward=reward.cuda(),
                            done=done.cuda()), ())
    ref = pbl._as_agent_output(ref)
    # Tolerances of tests/test_inference_runner_gpu.py (bf16 MFMA trunk in
    # the runner, fp32 reference).
    torch.testing.assert_close(logits, ref[1].cpu(), rtol=5e-2, atol=5e-3)
    torch.testing.assert_close(baseline, ref[2].cpu(), rtol=5e-2, atol=5e-3)
    assert action.dtype == torch.int64
    assert torch.equal(action, logits.argmax(-1))


def test_row_serve_equals_tensor_serve(model, tmp_path):
    assert os.environ.get("TBAMD_ACTOR_FASTPATH", "1") != "0"
    streams, stats = drv.run_gpu(5, model=model)
    assert stats["batcher_serve_row_batches"] > 0
    fast = drv.streams_as_dict(streams, 2)

    out = str(tmp_path / "legacy.npz")
    env = dict(os.environ, TBAMD_ACTOR_FASTPATH="0")
    subprocess.run(
        [sys.executable, os.path.join(ROOT, "tests", "helpers",
                                      "actor_rows_driver.py"),
         "gpu", out, "5"],
        cwd=ROOT, env=env, timeout=120, check=True)
    legacy = dict(np.load(out))
    assert float(legacy.pop("stat_serve_row_batches")) == 0

    assert sorted(fast) == sorted(legacy)
    assert len(fast) == 5 * 2 * 8
    # Same kernels, same per-row inputs: equal, not merely close.
    for key in sorted(fast):
        assert fast[key].dtype == legacy[key].dtype, key
        assert np.array_equal(fast[key], legacy[key]), key
