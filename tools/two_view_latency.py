"""Latency of the H / F RANSAC of the two-view initialisation, both ways in one run, at 300 and at 2000 matches, iters = 200, on the
general scene of tests/two_view_model.py:
  device form   ONE orbm_two_view_ransac_device call (three launches) on a stream, device time between two HIP events; twice: the
                sets drawn on the device (d_sets = NULL), and the same sets given -- the difference is what the draw costs a call,
                above all the one lane of k_tv_prepare that makes the 8 * iters raw values one after the other
  host form     what a caller did before the call existed: wait for the stream, read matches12 back, run the float32 model of
                tests/two_view_model.py (numpy and LAPACK, 200 + 200 hypotheses each scored against every match).  Host wall time.  The
                loops are numpy's and Python's, not the reference's C++ threads: the figure bounds what the host hop costs here, it
                is not a measurement of TwoViewReconstruction::Reconstruct.
p50 (and p90) of 300 device calls after 20 warm-up calls; the host form 5 times.  Writes profiles/two_view_latency.txt (or the path
given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import two_view_model as tm
    from monoorbslam3_amd.extractor import KP_DTYPE
    from monoorbslam3_amd.matcher import MatcherHandle, ORBMatcher, two_view_sets
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps, iters = 20, 300, 200
    m = ORBMatcher(handle=MatcherHandle(device=0))
    lines = ["two-view RANSAC, iters = %d, %s" % (iters, torch.cuda.get_device_name(0)),
             "device: one orbm_two_view_ransac_device call between two events, p50 / p90 of %d calls (us)" % reps,
             "host: stream wait + read-back of matches12 + the float32 numpy model, p50 of 5 (ms)", ""]
    for n in (300, 2000):
        sc = tm.make_scene(n, 9 if n == 300 else 10)

        def rec(xy):
            k = np.zeros(len(xy), KP_DTYPE)
            k["x"], k["y"] = xy[:, 0], xy[:, 1]
            return torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).to(dev)

        n1, n2 = len(sc["xy1"]), len(sc["xy2"])
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        d = dict(kps1=rec(sc["xy1"]), kps2=rec(sc["xy2"]), matches12=torch.from_numpy(sc["matches12"]).to(dev), pairs=z((n1, 2), torch.int32),
                 H=z(9, torch.float32), F=z(9, torch.float32), inl_H=z(n1, torch.uint8), inl_F=z(n1, torch.uint8), score=z(2, torch.float32),
                 rh=z(1, torch.float32), result=z(8, torch.int32))
        stream = torch.cuda.Stream(device=dev)

        def timed():
            t = []
            with torch.cuda.stream(stream):
                for k in range(warm + reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    m.TwoViewRansacDevice(d, n1, n2, 1.0, iters)
                    b.record()
                    b.synchronize()
                    if k >= warm:
                        t.append(a.elapsed_time(b) * 1e3)
            return t

        times = timed()
        drawn = {k: d[k].cpu().numpy().copy() for k in ("H", "F", "score", "result")}
        d["sets"] = torch.from_numpy(two_view_sets(n, iters)).to(dev)
        given = timed()
        assert all(np.array_equal(drawn[k], d[k].cpu().numpy()) for k in drawn)
        del d["sets"]
        res = d["result"].cpu().numpy()
        assert res[0] == n and res[1] == 0, res
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            stream.synchronize()
            m12 = d["matches12"].cpu().numpy()
            out = tm.run_model(sc["xy1"], sc["xy2"], m12, 1.0, iters, dt=np.float32)
            host.append((time.perf_counter() - t0) * 1e3)
        assert out["win"][1] >= 0
        lines.append("%5d matches (n1 %d, n2 %d): device p50 %.1f us, p90 %.1f us (sets given: p50 %.1f us); host p50 %.1f ms; result %s, RH %.3f" % (
            n, n1, n2, np.percentile(times, 50), np.percentile(times, 90), np.percentile(given, 50), np.percentile(host, 50), res.tolist(), float(d["rh"][0])))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "two_view_latency.txt"))
