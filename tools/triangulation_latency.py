"""Latency of one key-frame pair of LocalMapping::createNewMapPoints (LocalMapping.cpp:168-253), both ways in one run, at 2000 x 2000
features:
  device form   orbm_search_for_triangulation_device + orbm_triangulate_matches_device, device time by HIP events
  host form     what a caller has to do between the search and the fuse without the triangulation kernel: wait, read matches12
                back, the numpy loop of tests/triangulation_model.py (float32), upload points / normals / distance ranges / valid /
                descriptors and both has_mp flag arrays; host wall time up to the wait that ends the uploads.  The loop is NUMPY's,
                not the reference's C++: the figure bounds what a host hop costs here, it is not a measurement of Eigen.
The search runs on 2000 x 2000 synthetic descriptors in 16 vocabulary nodes; the triangulation consumes a seeded two-view cloud's
matches (tests/triangulation_model.make_cloud, 1600 matches in 2000 x 2000 key points), so that the gates see real geometry.
p50 (and p90) of 300 calls after 50 warm-up calls, the two forms alternating.  Writes profiles/triangulation_latency.txt (or the path
given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import triangulation_model as tm
    from monoorbslam3_amd import _lib, synth
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    n, n_match, warm, reps, cap_points = 2000, 1600, 50, 300, 4000
    cloud = tm.make_cloud(False, n_match, 31)
    pad = lambda a, fill: np.concatenate([a, np.full(n - len(a), fill, a.dtype)]) if len(a) < n else a[:n]  # noqa: E731
    assert cloud["n1"] <= n and cloud["n2"] == n
    kps1 = np.concatenate([cloud["kps1"], np.zeros(n - cloud["n1"], cloud["kps1"].dtype)])
    cloud.update(kps1=kps1, matches12=pad(cloud["matches12"], -1), n1=n, n_points=0)
    a, b, _ = synth.make_descriptor_pair(n, seed=5)
    cloud["desc2"] = b
    fv1, fv2 = synth.feature_vector_by_prefix(a, 4), synth.feature_vector_by_prefix(b, 4)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rec = lambda k: up(np.frombuffer(k.tobytes(), np.uint8).copy())  # noqa: E731

    def dev_fv(fv):
        nodes, off, idx = fv
        p = lambda x, dt, m: up(np.concatenate([np.asarray(x, dt), np.zeros(max(m - len(x), 0), dt)]))  # noqa: E731
        return (p(nodes, np.uint32, n).view(torch.int32), p(off, np.int32, n + 1), p(idx, np.uint32, n).view(torch.int32),
                torch.tensor([len(nodes)], dtype=torch.int32, device=dev))

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table = dict(n_points=z((1,), torch.int32), points=z((cap_points, 3), torch.float32), valid=z((cap_points,), torch.uint8),
                 normals=z((cap_points, 3), torch.float32), min_dist=z((cap_points,), torch.float32), max_dist=z((cap_points,), torch.float32),
                 desc=z((cap_points, 32), torch.uint8), obs=z((cap_points, 2), torch.int32))
    search = dict(desc1=up(a), kps1=rec(kps1), has_mp1=z((n,), torch.uint8), fv1=dev_fv(fv1), desc2=up(b), kps2=rec(cloud["kps2"]),
                  has_mp2=z((n,), torch.uint8), fv2=dev_fv(fv2), matches12=z((n,), torch.int32), result=z((8,), torch.int32))
    tri = dict(table, pose_R1=up(np.asarray(cloud["R1"]).reshape(9)), pose_t1=up(np.asarray(cloud["t1"])), pose_R2=up(np.asarray(cloud["R2"]).reshape(9)),
               pose_t2=up(np.asarray(cloud["t2"])), kps1=search["kps1"], kps2=search["kps2"], desc2=search["desc2"], matches12=up(cloud["matches12"]),
               mp1=z((n,), torch.int32), mp2=z((n,), torch.int32), has_mp1=search["has_mp1"], has_mp2=search["has_mp2"], result=z((8,), torch.int32))
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher(0.6, False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def reset():
        table["n_points"].zero_()
        search["has_mp1"].zero_()
        search["has_mp2"].zero_()

    def device_form():
        reset()
        e0.record()
        m.SearchForTriangulationDevice(search, n, n)
        m.TriangulateMatchesDevice(cam, tri, n, n, cap_points, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def host_form():
        reset()
        m.SearchForTriangulationDevice(search, n, n)
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                       # the wait the chain has to make
        tri["matches12"].cpu().numpy()                                 # matches12 read-back (the cloud's: the geometry the loop needs)
        e = tm.evaluate(cloud["cam"], None, cloud["R1"], cloud["t1"], cloud["R2"], cloud["t2"], kps1, cloud["kps2"], b, cloud["matches12"])
        k = int(e["result"][0])
        h1, h2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        h1[e["feat1"]], h2[e["feat2"]] = 1, 1
        for key, val in (("points", e["points"]), ("normals", e["normals"]), ("min_dist", e["min_dist"]), ("max_dist", e["max_dist"]),
                         ("valid", np.ones(k, np.uint8)), ("desc", e["desc"])):
            table[key][:k].copy_(torch.from_numpy(np.ascontiguousarray(val)))
        search["has_mp1"].copy_(torch.from_numpy(h1))
        search["has_mp2"].copy_(torch.from_numpy(h2))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    dev_us, host_us = [], []
    for i in range(warm + reps):
        x, y = device_form(), host_form()
        if i >= warm:
            dev_us.append(x)
            host_us.append(y)
    device_form()
    s_res, t_res = search["result"].cpu().numpy().tolist(), tri["result"].cpu().numpy().tolist()
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "one key-frame pair of createNewMapPoints, %d x %d features, %d matches triangulated; p50 / p90 of %d after %d warm-up calls, forms "
        "alternating; kernels %s" % (n, n, n_match, reps, warm, _lib.kernels_sha16()),
        "device form (search + triangulate, device time by HIP events):                          %.1f / %.1f us   search d_result %s, "
        "triangulate d_result %s" % (pct(dev_us, 50), pct(dev_us, 90), s_res, t_res),
        "host form (wait, matches12 read-back, NUMPY float32 loop, eight uploads), host wall time: %.1f / %.1f us   (numpy's loop, not the "
        "reference's C++)" % (pct(host_us, 50), pct(host_us, 90)),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "triangulation_latency.txt"))
