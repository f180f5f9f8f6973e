"""Latency of the host-pointer BA entry points (include/orbba.h) through the Python wrappers, at the mapper's and the tracker's sizes:
  local_bundle_adjustment, optimize(5), linearize   20 poses (2 fixed), 3000 points, about 48000 edges (tests/test_ba.py `_perturbed`)
  pose_optimize_batch                                64 frames x 1000 correspondences
Host wall time of the whole call (checks, host index, copies, the LM loop's waits) and the device time the call reports; p50 / p90 of
`--reps` calls after `--warm` warm-up calls.  Writes profiles/ba_latency.txt (or the path given as the first argument)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path, warm, reps):
    import torch
    import test_ba
    from monoorbslam3_amd import _lib, ba
    assert torch.cuda.is_available(), "needs the GPU"
    pr, args = test_ba._perturbed(20, 3000, 5)
    cam, R0, t0, off, P, Z, W = test_ba._pose_frames([1000] * 64, 5)
    calls = [("local_bundle_adjustment", lambda: ba.local_bundle_adjustment(*args), "device_ms"),
             ("optimize(5)", lambda: ba.optimize(*args, iterations=5), "device_ms"),
             ("linearize", lambda: ba.linearize(*args), "kernel_ms"),
             ("pose_optimize_batch(64 x 1000)", lambda: ba.pose_optimize_batch(cam, R0, t0, off, P, Z, W), "kernel_ms")]
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = ["BA entry points on %d poses, %d points, %d edges; host wall time of the call and the device time it reports, p50 / p90 of %d after "
             "%d warm-up calls; kernels %s" % (len(args[1]), len(args[4]), len(args[5]), reps, warm, _lib.kernels_sha16())]
    for name, call, dev_key in calls:
        wall, dev = [], []
        for i in range(warm + reps):
            t = time.perf_counter()
            got = call()
            us = (time.perf_counter() - t) * 1e6
            if i >= warm:
                wall.append(us)
                dev.append(got[dev_key] * 1e3)
        note = ", %d its / %d solves, %d outliers" % (got["iterations"], got["trials"], got["outlier"].sum()) if "outlier" in got else ""
        lines.append("%s: wall %.1f / %.1f us, device %.1f / %.1f us%s" % (name, pct(wall, 50), pct(wall, 90), pct(dev, 50), pct(dev, 90), note))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "ba_latency.txt"))
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    main(a.out, a.warm, a.reps)
