"""bench.py's plain run and --dump-outputs: the line holds the headline keys for exactly --steps timed steps, two runs with
the same arguments write the same outputs (float32 / float64 .npy files, rows past a frame's count zeroed), and those outputs
are the C oracle's on the inputs bench.py builds."""
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


@pytest.fixture(scope="module")
def bench_run(tmp_path_factory):
    """one plain bench.py run with --dump-outputs, shared by the tests of this module: (dump directory, JSON line)"""
    a = tmp_path_factory.mktemp("bench") / "a"
    return a, _bench(a)


@pytest.mark.gpu
def test_plain_run_line_and_repeatable_dump(bench_run, tmp_path):
    a, line = bench_run
    b = tmp_path / "b"
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


def _bench_inputs(B, W, H, rank=0):
    """the resident batch bench.py main() builds ("synthetic resident batch": n_distinct frames of synth.make_frames, the rest
    noise-perturbed copies of them, the noise drawn from a CPU torch.Generator seeded 1234 + rank)"""
    import torch
    from monoorbslam3_amd import synth
    n_distinct = min(B, 32)
    base = synth.make_frames(n_distinct, W, H, seed=synth.DEFAULT_SEED + 101 * rank)
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    frames = torch.from_numpy(base)
    if B > n_distinct:
        reps = (B + n_distinct - 1) // n_distinct
        frames = frames.repeat(reps, 1, 1)[:B].contiguous()
        noise = torch.randint(-2, 3, frames.shape, generator=g, dtype=torch.int16)
        noise[:n_distinct] = 0
        frames = (frames.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8).contiguous()
    return frames.numpy()


@pytest.mark.gpu
def test_dumped_outputs_equal_the_oracle(bench_run, oracle_mod):
    """The dump of the plain run (--batch 64, 1242 x 375, 2000 features) against the C oracle on the same inputs: every frame's
    count, then the key points (all seven fields, bit-exact after the float32 round trip) and descriptors of 8 dumped frames, and
    their best-2 rows against the oracle's strict-'<' scan of the dumped descriptors of f and f + 1 (the last frame: frame 0)."""
    from concurrent.futures import ThreadPoolExecutor
    a, line = bench_run
    B, W, H = 64, 1242, 375
    assert (line["config"]["frames_per_gpu_per_step"], line["config"]["width"], line["config"]["height"]) == (B, W, H)
    frames = _bench_inputs(B, W, H)
    orc = oracle_mod.Oracle(2000, 1.2, 8, 20, 7)
    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
        ref = list(pool.map(lambda f: orc.extract(frames[f])[:2], range(B)))
    counts = np.load(a / "n_keypoints.npy").astype(np.int64)
    want = np.array([len(k) for k, _ in ref])
    assert np.array_equal(counts, want), "inputs no longer match bench.py's: counts %s, oracle %s" % (counts[:8], want[:8])
    sample = np.load(a / "sample_frames.npy").astype(np.int64).tolist()
    kps, desc = np.load(a / "keypoints.npy"), np.load(a / "descriptors.npy")
    idx, bd, sd = np.load(a / "match_index.npy"), np.load(a / "match_best_distance.npy"), np.load(a / "match_second_distance.npy")
    # 8 dumped frames whose match partner is dumped too: the first, the last and six seeded picks
    ok = [f for f in sample if (f + 1) % B in sample]
    pick = np.random.RandomState(5).choice(ok[1:-1], 6, replace=False).tolist()
    checked = sorted(set([ok[0], ok[-1]] + pick))
    assert len(checked) == 8, (sample, checked)
    fields = ("x", "y", "size", "angle", "response", "octave", "class_id")
    for f in checked:
        j, n = sample.index(f), counts[f]
        okp, odesc = ref[f]
        for c, fld in enumerate(fields):
            got = kps[j, :n, c]
            got = got.astype(np.int32) if fld in ("octave", "class_id") else got.astype(np.float32)
            assert got.tobytes() == okp[fld].tobytes(), "frame %d: key-point field %s" % (f, fld)
        d = desc[j, :n].astype(np.uint8)
        assert np.array_equal(desc[j, :n], d) and np.array_equal(d, odesc), "frame %d: descriptors" % f
        g = (f + 1) % B
        r_bi, r_bd, r_sd = oracle_mod.best2(d, desc[sample.index(g), :counts[g]].astype(np.uint8))
        assert np.array_equal(idx[j, :n].astype(np.int32), r_bi), "frame %d: match index (against frame %d)" % (f, g)
        assert np.array_equal(bd[j, :n].astype(np.uint16), r_bd), "frame %d: best distance (against frame %d)" % (f, g)
        assert np.array_equal(sd[j, :n].astype(np.uint16), r_sd), "frame %d: second distance (against frame %d)" % (f, g)
