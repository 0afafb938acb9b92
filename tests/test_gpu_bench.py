"""GPU: a plain ``bench.py`` run -- the contract line of exactly --steps timed steps and nothing else -- and ``--dump-outputs``,
whose keypoints are those of the last timed step and the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "4",
           "--rotate", "2", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "keypoints.npy"))


def test_plain_bench_prints_the_contract_line_and_dumps_reproducible_keypoints(synth, gpu, tmp_path):
    line, kp = _bench(tmp_path / "a")
    again, kp_again = _bench(tmp_path / "b")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line and key in again, key
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["config"]["global_batch"] == 4
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / 4 - 1) < 0.01               # images per second of the timed steps
    assert "extra" not in line and "roofline" not in line and "cpu_baseline" not in line  # the rest runs with --full only
    assert kp.dtype == np.float32 and kp.shape == (4, 9, 2) and np.isfinite(kp).all()
    np.testing.assert_array_equal(kp, kp_again)
    # the last timed step (2 + 7 - 1 = 8) voted on rotating batch 8 % 2 = 0: its keypoints are the ones the field was built from
    cfg = {k: v for k, v in synth.CONFIGS["cfg3"].items() if k not in ("B", "hn")}
    want = synth.make_batch(B=4, **cfg, first_index=0, device=gpu)["kpt_2d"].cpu().numpy()
    assert np.abs(kp - want).max() < 20
