"""bench.py's plain run and --dump-outputs: the line holds the headline keys for exactly --steps timed steps, and two runs with
the same arguments write the same outputs (float32 / float64 .npy files, rows past a frame's count zeroed)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64",
           "--clock-warmup-steps", "0", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_line_and_repeatable_dump(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["full"] is False and line["ms_per_step"] > 0
    assert abs(line["value"] - 64 * 3 / (3 * line["ms_per_step"] * 1e-3)) < 0.01 * line["value"]
    assert "roofline" not in line and "cpu_baseline" not in line and "value_end_to_end" not in line
    _bench(b)
    names = sorted(os.path.basename(p) for p in glob.glob(str(a / "*.npy")))
    assert names == sorted(os.path.basename(p) for p in glob.glob(str(b / "*.npy")))
    assert {"n_keypoints.npy", "keypoints.npy", "descriptors.npy", "match_index.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    frames = np.load(a / "sample_frames.npy").astype(int)
    counts = np.load(a / "n_keypoints.npy")[frames].astype(int)
    desc = np.load(a / "descriptors.npy")
    assert counts.min() > 0 and desc.shape[0] == len(frames) and desc.shape[2] == 32
    for f, c in enumerate(counts):
        assert not desc[f, c:].any() and desc[f, :c].any()
