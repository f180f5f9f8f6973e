"""Latency of the stage-2 hand-over of the tracking thread (Tracking.cpp:386-427), both ways in one run, on 2000 key points and 4000
local map points:
  device form   orbba_pose_drop_outliers_device + orbm_project_frustum_device, device time by HIP events
  host form     wait, pose read-back, the numpy loop of tests/projection_model.py, five uploads; host wall time up to the wait
                that ends the uploads
p50 (and p90) of 300 calls after 50 warm-up calls, the two forms alternating.  Writes profiles/projection_queries_latency.txt (or
the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import projection_model as pm
    from monoorbslam3_amd import _lib, ba
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    n_kp, nq, warm, reps = 2000, 4000, 50, 300
    cloud = pm.make_cloud(pm.FRUSTUM, False, nq, 21)
    rng = np.random.RandomState(1)
    frame_mp = np.full(n_kp, -1, np.int32)
    slots = rng.choice(n_kp, 600, replace=False)
    frame_mp[slots] = rng.choice(nq, 600, replace=False)          # 600 matches of stage 1, a quarter of them outliers
    edge_kp = np.sort(slots).astype(np.int32)
    inlier = (rng.uniform(size=600) > 0.25).astype(np.uint8)
    cloud.update(frame_mp=frame_mp, n2=n_kp)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = dict(pose_R=up(np.asarray(cloud["R"]).reshape(9)), pose_t=up(np.asarray(cloud["t"])), points=up(cloud["points"]),
             valid=up(cloud["valid"]), normals=up(cloud["normals"]), min_dist=up(cloud["min_dist"]), max_dist=up(cloud["max_dist"]),
             frame_mp=up(frame_mp), q_xy=torch.zeros((nq, 2), device=dev), q_radius=torch.zeros(nq, device=dev),
             q_level=torch.zeros(nq, dtype=torch.int32, device=dev), q_ok=torch.zeros(nq, dtype=torch.uint8, device=dev),
             view_cos=torch.zeros(nq, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
    d_mp0, d_off, d_ekp, d_inl = up(frame_mp), up(np.array([0, 600], np.int32)), up(edge_kp), up(inlier)
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_form():
        d["frame_mp"].copy_(d_mp0)
        e0.record()
        ba.pose_drop_outliers_device(n_kp, d_off, d_ekp, d_inl, d["frame_mp"])
        m.ProjectFrustumDevice(cam, d, nq, n_kp, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 1.0, 0.5)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def host_form():
        d["frame_mp"].copy_(d_mp0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                       # the wait the chain has to make
        R, t = d["pose_R"].cpu().numpy(), d["pose_t"].cpu().numpy()    # pose read-back
        mp = frame_mp.copy()                                           # (the host's own frame_mp; the outlier drop is a host loop too)
        mp[edge_kp[inlier == 0]] = -1
        e = pm.evaluate(pm.FRUSTUM, cloud["cam"], cloud["bounds"], R, t, cloud["points"], cloud["valid"], normals=cloud["normals"],
                        min_dist=cloud["min_dist"], max_dist=cloud["max_dist"], frame_mp=mp, th=1.0, view_cos_limit=0.5)
        for k in ("q_xy", "q_radius", "q_level", "q_ok", "view_cos"):  # five uploads
            d[k].copy_(torch.from_numpy(e[k]), non_blocking=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    dev_us, host_us = [], []
    for i in range(warm + reps):
        a, b = device_form(), host_form()
        if i >= warm:
            dev_us.append(a)
            host_us.append(b)
    res = d["result"].cpu().numpy().tolist()
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "stage-2 hand-over, %d key points, %d local map points, %d stage-1 matches (%d outliers); p50 / p90 of %d after %d warm-up calls, "
        "forms alternating; kernels %s" % (n_kp, nq, 600, int((inlier == 0).sum()), reps, warm, _lib.kernels_sha16()),
        "device form (drop outliers + frustum builder, 2 launches), device time by HIP events: %.1f / %.1f us   d_result %s" % (
            pct(dev_us, 50), pct(dev_us, 90), res),
        "host form (wait, pose read-back, numpy loop, five uploads), host wall time:           %.1f / %.1f us" % (
            pct(host_us, 50), pct(host_us, 90)),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "projection_queries_latency.txt"))
