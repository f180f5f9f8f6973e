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
given as the first argument).

Behind it, the pose recovery (orbm_two_view_pose_device, three launches) on the same scenes with descriptors added, the same way:
  pose alone    ONE orbm_two_view_pose_device call on the outputs the RANSAC left on the device, family = -1
  the chain     orbm_search_for_initialization_device -> orbm_two_view_ransac_device -> orbm_two_view_pose_device on one stream, nothing
                between them, device time between two events around all three
  host form     wait, read back what the RANSAC left, run the float32 numpy model of tests/two_view_pose_model.py (LAPACK per match in
                numpy's batched SVD), push nothing back.  An ORDER OF MAGNITUDE only: numpy, not the reference's C++."""
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
    lines += pose_lines(m, dev, warm, reps, iters)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "w") as f:
        f.write(text)


def pose_lines(m, dev, warm, reps, iters):
    import torch
    import two_view_model as tm
    import two_view_pose_model as pm
    from monoorbslam3_amd.extractor import KP_DTYPE
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import ORBMatcher
    ms = ORBMatcher(0.9, True, handle=m._hd)
    lines = ["", "two-view pose recovery behind it (orbm_two_view_pose_device), the scenes with descriptors, matches12 from the search",
             "device: p50 / p90 of %d calls between two events (us); host: wait + read-back + the float32 numpy model, p50 of 5 (ms), an order of magnitude only" % reps, ""]
    for n in (300, 2000):
        sc = tm.make_scene(n, 9 if n == 300 else 10)
        r = np.random.RandomState(n)
        n1, n2 = len(sc["xy1"]), len(sc["xy2"])
        d1, d2 = r.randint(0, 256, (n1, 32)).astype(np.uint8), r.randint(0, 256, (n2, 32)).astype(np.uint8)
        for i in np.flatnonzero(sc["matches12"] >= 0):
            d2[sc["matches12"][i]] = d1[i]
            d2[sc["matches12"][i], r.randint(32)] ^= np.uint8(1 << r.randint(8))

        def rec(xy):
            k = np.zeros(len(xy), KP_DTYPE)
            k["x"], k["y"], k["size"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, -1
            return k

        k1, k2 = rec(sc["xy1"]), rec(sc["xy2"])
        post = FramePost(tm.W, tm.H, tm.FX, tm.FY, tm.CX, tm.CY)
        _, k2u, start, items = post(k2)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        kp = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        sd = dict(kps1=kp(k1), desc1=up(d1), kps2=kp(k2u), desc2=up(d2), cell_start=up(start.astype(np.int32)),
                  cell_items=up(np.concatenate([items, np.zeros(1, items.dtype)]).astype(np.int32)),
                  pre=up(np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)), matches12=z(n1, torch.int32), result=z(8, torch.int32))
        rv = dict(kps1=sd["kps1"], kps2=sd["kps2"], matches12=sd["matches12"], pairs=z((n1, 2), torch.int32), H=z(9, torch.float32),
                  F=z(9, torch.float32), inl_H=z(n1, torch.uint8), inl_F=z(n1, torch.uint8), score=z(2, torch.float32), rh=z(1, torch.float32),
                  result=z(8, torch.int32))
        pv = dict(kps1=sd["kps1"], kps2=sd["kps2"], matches12=sd["matches12"], ransac_result=rv["result"], R21=z(9, torch.float32),
                  t21=z(3, torch.float32), points3D=z((n1, 3), torch.float32), triangulated=z(n1, torch.uint8), matches12_out=z(n1, torch.int32),
                  hyp_R=z((8, 9), torch.float32), hyp_t=z((8, 3), torch.float32), hyp_good=z(8, torch.int32), hyp_parallax=z(8, torch.float32),
                  result=z(16, torch.int32), **{k: rv[k] for k in ("pairs", "H", "F", "inl_H", "inl_F")})
        stream = torch.cuda.Stream(device=dev)

        def search():
            ms.SearchForInitializationDevice(sd, n1, n2, post.cols, post.rows, window=100, list_cap=1024, stream=None)

        def ransac():
            m.TwoViewRansacDevice(rv, n1, n2, 1.0, iters)

        def pose():
            m.TwoViewPoseDevice(pv, n1, n2, pm.K4, -1, 1.0, 1.0)

        def timed(*calls):
            t = []
            with torch.cuda.stream(stream):
                for k in range(warm + reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for c in calls:
                        c()
                    b.record()
                    b.synchronize()
                    if k >= warm:
                        t.append(a.elapsed_time(b) * 1e3)
            return np.percentile(t, 50), np.percentile(t, 90)

        chain = timed(search, ransac, pose)
        alone = timed(pose)
        two = timed(ransac, pose)
        res, sres = pv["result"].cpu().numpy(), sd["result"].cpu().numpy()
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            stream.synchronize()
            got = {k: rv[k].cpu().numpy() for k in ("pairs", "H", "F", "inl_H", "inl_F", "result")}
            fam = int(got["result"][4])
            nm = int(got["result"][0])
            out = pm.run_model(sc["xy1"], sc["xy2"], got["pairs"][:nm],
                               (got["inl_H"] if fam else got["inl_F"])[:nm], got["H"] if fam else got["F"], fam, dt=np.float32)
            host.append((time.perf_counter() - t0) * 1e3)
        assert out["status"] == res[0], (out["status"], res)
        lines.append("%5d key-point pairs, %d matched by the search (n1 %d, n2 %d): pose alone p50 %.1f us, p90 %.1f us; RANSAC + pose p50 %.1f us; "
                     "search + RANSAC + pose p50 %.1f us, p90 %.1f us; host p50 %.1f ms; result %s" % (
                         n, sres[0], n1, n2, alone[0], alone[1], two[0], chain[0], chain[1], np.percentile(host, 50), res.tolist()))
    return lines


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "two_view_latency.txt"))
