"""bench.py --dump-outputs: the last timed step's outputs land in DIR as
float32 .npy files, and the seeded learner inputs make them reproducible."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import torch

EXPECTED = {
    "total_loss", "pg_loss", "baseline_loss", "entropy_loss", "policy_logits",
    "baseline", "vs", "pg_advantages", "grad_norm", "flat_param",
}
T, B, A = 16, 4, 6


def _run(outdir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--actors", "8", "--batch_size", str(B),
         "--unroll_length", str(T), "--num_actions", str(A),
         "--dump-outputs", str(outdir)],
        cwd=root, timeout=300, capture_output=True,
    )
    assert out.returncode == 0, out.stderr.decode()[-4000:]
    lines = [ln for ln in out.stdout.decode().splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1, lines
    result = json.loads(lines[0])
    assert result["steps"] == 2 and result["ms_per_step"] > 0
    return {
        os.path.basename(f)[:-4]: np.load(f)
        for f in glob.glob(os.path.join(str(outdir), "*.npy"))
    }


def test_dump_outputs_contract_and_repeatability(tmp_path):
    first = _run(tmp_path / "a")
    assert set(first) == EXPECTED
    assert sum(a.nbytes for a in first.values()) <= 64 * 2**20
    for name, a in first.items():
        assert a.dtype == np.float32, name
        assert np.isfinite(a).all(), name
    assert first["policy_logits"].shape == (T, B, A)
    assert first["baseline"].shape == first["vs"].shape == (T, B)

    second = _run(tmp_path / "b")
    for name, a in first.items():
        assert second[name].shape == a.shape, name
        if not torch.cuda.is_available():
            # CPU kernels are deterministic: same seed, same bits. (GPU
            # reductions may reorder float adds between runs.)
            np.testing.assert_array_equal(second[name], a, err_msg=name)
