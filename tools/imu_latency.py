"""Latency of the inertial prediction of a tracked frame (Tracking.cpp:90-91, :102-104, ORBMatcher.cpp:212-229), both ways in one run:
ten IMU samples into the last frame's and the last key frame's integrator, the predicted pose, the frame form's queries for 1500 map
points.
  device form   orbi_integrate_device (2 jobs x 10 samples) + orbi_predict_device + orbm_project_frame_device, the span between two
                HIP events; once enqueued on an idle stream, once with 20 frames queued back to back (the span per frame)
  host form     what a caller did before: wait, read the last frame's IMU pose back, the numpy loop of tests/imu_model.py (the
                reference's C++ is faster: this is numpy's figure, not the reference's), upload the pose, the builder; host wall time
p50 (and p90) of 300 after 50 warm-up calls.  Writes profiles/imu_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import imu_model as im
    import projection_model as pm
    from monoorbslam3_amd import _lib, imu
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    nq, warm, reps, burst = 1500, 50, 300, 20
    rng = np.random.RandomState(17)
    cal = im.calib()
    ccal = imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])
    bank = im.Bank(2, 64)
    for r in bank.recs:
        r.reset(im.random_bias(rng))
    samples = im.make_stream(10, 42)
    jobs = np.zeros(2, im.JOB)
    for j in range(2):
        jobs[j] = (j, 0, 10, 0, samples["t"][0] - 0.4 / im.RATE, samples["t"][-1] + 0.6 / im.RATE)
    src = np.concatenate([im.rodrigues([0.3, -0.2, 0.5]).reshape(9), [0.4, -1.0, 0.2], [0.5, 0.1, -0.3]]).astype(np.float32)
    cloud = pm.make_cloud(pm.FRAME, False, nq, 23)
    h_bank, h_pool = bank.pack()
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_bank, d_pool, d_jobs, d_samples, d_src = up(h_bank), up(h_pool), up(jobs), up(samples), up(src)
    d_ids, d_bias = up(np.arange(2, dtype=np.int32)), up(np.stack([r.bias for r in bank.recs]))
    d_res, d_res0 = (torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(2))
    d_dst = torch.zeros(15, device=dev)
    q = dict(pose_R=torch.zeros(9, dtype=torch.float64, device=dev), pose_t=torch.zeros(3, dtype=torch.float64, device=dev), points=up(cloud["points"]),
             valid=up(cloud["valid"]), kps1=up(cloud["kps1"]), q_xy=torch.zeros((nq, 2), device=dev), q_radius=torch.zeros(nq, device=dev),
             q_level=torch.zeros(nq, dtype=torch.int32, device=dev), q_angle=torch.zeros(nq, device=dev),
             q_ok=torch.zeros(nq, dtype=torch.uint8, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()

    def reset():                                                       # outside every timed span: the records start empty
        imu.reset_device(d_bank, 2, d_ids, 2, d_res0, d_bias=d_bias)

    def chain():
        imu.integrate_device(ccal, d_bank, d_pool, 2, 64, d_jobs, 2, d_samples, 10, d_res)
        imu.predict_device(ccal, d_bank, 2, 0, d_src, d_dst, q["pose_R"], q["pose_t"])
        m.ProjectFrameDevice(cam, q, nq, cloud["th"])

    def device_idle():
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        chain()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def device_queued():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * burst)]
        torch.cuda.synchronize()
        for k in range(burst):
            reset()
            ev[2 * k].record()
            chain()
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        return [ev[2 * k].elapsed_time(ev[2 * k + 1]) * 1e3 for k in range(1, burst)]

    def host_form():
        recs = [r.copy() for r in bank.recs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                       # the wait the chain has to make
        s = d_src.cpu().numpy()                                        # the last frame's IMU pose and velocity, read back
        for r, job in zip(recs, jobs):
            r.compute_preintegration(cal, samples, job["timestamp"], job["end_time"])
        _, Rcw, tcw = im.predict(cal, recs[0], s)
        q["pose_R"].copy_(torch.from_numpy(Rcw.reshape(9).astype(np.float64)))    # the pose, uploaded
        q["pose_t"].copy_(torch.from_numpy(tcw.astype(np.float64)))
        m.ProjectFrameDevice(cam, q, nq, cloud["th"])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    idle, host, queued = [], [], []
    for i in range(warm + reps):
        a, b = device_idle(), host_form()
        if i >= warm:
            idle.append(a)
            host.append(b)
    for i in range(3 + reps // (burst - 1) + 1):
        v = device_queued()
        if i >= 3:
            queued += v
    queued = queued[:reps]
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    lines = [
        "inertial prediction of a frame: 2 integration jobs x 10 samples, the prediction, the frame form's queries for %d map points; p50 / p90 "
        "of %d after %d warm-up calls; kernels %s" % (nq, reps, warm, _lib.kernels_sha16()),
        "device form (integrate + predict + frame builder, 3 launches), span between two HIP events, idle stream:      %.1f / %.1f us   "
        "d_result %s" % (pct(idle, 50), pct(idle, 90), d_res.cpu().numpy().tolist()),
        "device form, %d frames queued back to back, span per frame:                                                   %.1f / %.1f us" % (
            burst, pct(queued, 50), pct(queued, 90)),
        "host form (wait, read-back, numpy loop of tests/imu_model.py, pose upload, frame builder), host wall time:     %.1f / %.1f us   "
        "(numpy's figure, not the reference's C++)" % (pct(host, 50), pct(host, 90)),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "imu_latency.txt"))
