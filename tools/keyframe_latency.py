"""Latency of the start of a mapper step, both ways in one run: 200 key frames x 2000 slots over 60000 table rows, a tracked frame of 2000
key points with about 300 matched that becomes key frame 200, a recent list of 1500 entries, 400 rows a triangulation appended.
  device form   orbm_insert_keyframe_device -> orbm_build_observations_device -> orbm_cull_map_points_device ->
                orbm_register_new_points_device on one stream, device time between two HIP events; the slots, d_valid, the list and
                the counters are restored by device copies outside the timed span.  Twice: as enqueued from Python on an idle stream,
                where the span also holds the gaps in which the device waits for the next launch, and behind a stream kept busy by large
                fills, so that all launches are queued before the first one starts and the kernels run back to back (caches cold)
  host form     the parent commit's: wait, read frame_mp, the pose, d_valid and the key-frame table back, the loop of processNewKeyFrame (the array model of
                tests/keyframe_model.py), upload the slot row, the pose row, d_n, d_bad and the two pointers; the device build; wait, read the
                slots, the CSR, the list and the three counters back, the culling's and the registration's loops, upload d_valid, the
                slots, the list, the counters and the new rows' fields.  Host wall time up to the wait that ends the last upload.  The
                loops are NUMPY's and Python's, not the reference's C++: the figure bounds what the host hops cost here, it is not a
                measurement of LocalMapping::processNewKeyFrame or MapPointCulling.
p50 (and p90) of `reps` calls after `warm` warm-up calls, every form.  Writes profiles/keyframe_latency.txt (or the path given as the
first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

CUR = 200                                                          # the new key frame's slot and id


def make_scene(n_kf=200, stride=2000, cap0=60000, span=6000, n2=2000, n_matched=300, n_new=400, n_listed=1500, seed=7):
    """key frame k observes rows of [k * step, k * step + span) (tools/local_map_latency.py's world); the frame looks at the window of the
    newest key frames; the list holds rows of the last key frames' windows, created up to four key frames ago"""
    rng = np.random.RandomState(seed)
    cap = cap0 + n_new
    step = (cap0 - span) // (n_kf - 1)
    slots = np.stack([k * step + rng.choice(span, stride, replace=False) for k in range(n_kf)]).astype(np.int32)
    slots[rng.rand(n_kf, stride) < 0.4] = -1
    slots = np.concatenate([slots, rng.randint(-1, cap0, (1, stride)).astype(np.int32)])   # row 200: an earlier use
    n = np.concatenate([np.full(n_kf, stride), [17]]).astype(np.int32)
    bad = np.concatenate([np.zeros(n_kf), [1]]).astype(np.uint8)
    valid = np.concatenate([rng.rand(cap0) < 0.97, np.ones(n_new, bool)]).astype(np.uint8)
    window = (n_kf - 3) * step + np.arange(span)
    fm = np.full(n2, -1, np.int32)
    fm[rng.choice(n2, n_matched, replace=False)] = rng.choice(window, n_matched, replace=False)
    listed = rng.choice(window, n_listed, replace=False).astype(np.int32)
    first_kf = (CUR - rng.randint(0, 5, cap)).astype(np.int32)
    visible = rng.randint(1, 30, cap).astype(np.int32)
    found = np.minimum(visible, rng.randint(0, 12, cap)).astype(np.int32)
    recent = np.concatenate([listed, np.full(n_new + 8, -3, np.int32)])
    return dict(n_kf=n_kf + 1, stride=stride, cap=cap, cap0=cap0, n=n, bad=bad, slots=slots, valid=valid, frame_mp=fm, recent=recent, n_recent=n_listed,
                first_kf=first_kf, found=found, visible=visible, ref_kf=rng.randint(0, n_kf, cap).astype(np.int32),
                pose_R=rng.randn(n_kf + 1, 9), pose_t=rng.randn(n_kf + 1, 3), frame_R=rng.randn(9), frame_t=rng.randn(3))


def main(out_path):
    import torch
    import keyframe_model as km
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import ORBMatcher
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 20, 300
    sc = make_scene()
    n_kf, stride, cap, cap0, n2, K = sc["n_kf"], sc["stride"], sc["cap"], sc["cap0"], len(sc["frame_mp"]), sc["n_kf"] - 1
    cap_obs = int((sc["slots"] >= 0).sum()) + n2
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    one = lambda x: up(np.array([x], np.int32))  # noqa: E731
    frame_kps, frame_desc = torch.zeros(n2 * 8, dtype=torch.int32, device=dev), torch.zeros(n2 * 32, dtype=torch.uint8, device=dev)
    d = {k: up(sc[k]) for k in ("n", "bad", "slots", "valid", "frame_mp", "recent", "first_kf", "found", "visible", "ref_kf", "pose_R", "pose_t")}
    d.update(frame_pose_R=up(sc["frame_R"]), frame_pose_t=up(sc["frame_t"]), kps=torch.zeros(n_kf, dtype=torch.int64, device=dev),
             desc=torch.zeros(n_kf, dtype=torch.int64, device=dev), n_recent=one(sc["n_recent"]), n_points=one(cap), n_registered=one(cap0),
             obs_off=zi(cap + 1), obs_kf=zi(cap_obs), obs_kp=zi(cap_obs), code=zi(len(sc["recent"])))
    restored = ("n", "bad", "slots", "valid", "recent", "first_kf", "found", "visible", "ref_kf", "n_recent", "n_registered")
    keep = {k: d[k].clone() for k in restored}
    res = dict(insert=zi(8), build=zi(8), cull=zi(8), register=zi(8))
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def restore():
        for k in restored:
            d[k].copy_(keep[k])

    busy = torch.empty(64 << 20, dtype=torch.int32, device=dev)            # 256 MB: eight fills outlast the launches many times

    def device_form(behind_busy=False):
        if behind_busy:
            for _ in range(8):
                busy.zero_()
        e0.record()
        m.InsertKeyFrameDevice(dict(d, result=res["insert"]), K, stride, cap, n2, frame_kps, frame_desc)
        m.BuildObservationsDevice(dict(d, result=res["build"]), n_kf, stride, cap, cap_obs)
        m.CullMapPointsDevice(dict(d, result=res["cull"]), CUR, n_kf, stride, cap, cap_obs)
        m.RegisterNewPointsDevice(dict(d, result=res["register"]), K, CUR, cap)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    c = lambda x: x.cpu().numpy()  # noqa: E731

    def host_form():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        table = dict(pose_R=c(d["pose_R"]), pose_t=c(d["pose_t"]), bad=c(d["bad"]), kps=c(d["kps"]), desc=c(d["desc"]), n=c(d["n"]),
                     slots=c(d["slots"]).reshape(n_kf, stride))
        valid = c(d["valid"])
        ins = km.insert_keyframe(table, K, valid, cap, c(d["frame_mp"]), c(d["frame_pose_R"]), c(d["frame_pose_t"]), frame_kps.data_ptr(),
                                 frame_desc.data_ptr())
        d["slots"].view(n_kf, stride)[K].copy_(torch.from_numpy(ins["slots"][K]))
        d["pose_R"][K].copy_(torch.from_numpy(ins["pose_R"][K]))
        d["pose_t"][K].copy_(torch.from_numpy(ins["pose_t"][K]))
        for k in ("n", "bad", "kps", "desc"):
            d[k][K:K + 1].copy_(torch.from_numpy(ins[k][K:K + 1]))
        m.BuildObservationsDevice(dict(d, result=res["build"]), n_kf, stride, cap, cap_obs)
        torch.cuda.synchronize()
        w = dict(n_kf=n_kf, stride=stride, cap_points=cap, n=ins["n"], bad=ins["bad"], slots=c(d["slots"]).reshape(n_kf, stride), valid=valid,
                 obs_off=c(d["obs_off"]), obs_kf=c(d["obs_kf"]), obs_kp=c(d["obs_kp"]))
        first_kf, found, visible = c(d["first_kf"]), c(d["found"]), c(d["visible"])
        cull = km.cull_map_points(w, c(d["recent"]), int(c(d["n_recent"])[0]), CUR, first_kf, found, visible)
        reg = km.register_new_points(int(c(d["n_points"])[0]), int(c(d["n_registered"])[0]), cull["n_recent"], K, CUR, cap, c(d["ref_kf"]), first_kf,
                                     found, visible, cull["recent"])
        a, b = int(reg["result"][km.G_FROM]), int(reg["result"][km.G_TO])
        d["valid"].copy_(torch.from_numpy(cull["valid"]))
        d["slots"].copy_(torch.from_numpy(cull["slots"]))
        d["recent"].copy_(torch.from_numpy(reg["recent"]))
        for k in ("ref_kf", "first_kf", "found", "visible"):
            d[k][a:b].copy_(torch.from_numpy(reg[k][a:b]))
        d["n_recent"].copy_(torch.from_numpy(np.array([reg["n_recent"]], np.int32)))
        d["n_registered"].copy_(torch.from_numpy(np.array([reg["n_registered"]], np.int32)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, ins, cull, reg

    t = dict(device=[], queued=[], host=[])
    for key, behind_busy in (("device", False), ("queued", True)):
        for i in range(warm + reps):
            restore()
            a = device_form(behind_busy)
            if i >= warm:
                t[key].append(a)
    for i in range(warm + reps):
        restore()
        us, ins, cull, reg = host_form()
        if i >= warm:
            t["host"].append(us)
    host_state = {k: c(d[k]) for k in restored}
    restore()
    device_form()
    same = all(np.array_equal(c(d[k]), host_state[k]) for k in restored) and all(
        np.array_equal(c(res[k]), want["result"]) for k, want in (("insert", ins), ("cull", cull), ("register", reg)))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "the start of a mapper step: %d key-frame slots x %d slots, %d table rows, %d observations, a frame of %d key points, a list of %d; "
        "d_result of the insert %s, of the build %s, of the culling %s, of the registration %s; kernels %s"
        % (n_kf, stride, cap, int(c(res["build"])[0]), n2, sc["n_recent"], ins["result"].tolist(), c(res["build"]).tolist(), cull["result"].tolist(),
           reg["result"].tolist(), _lib.kernels_sha16()),
        "device form (orbm_insert_keyframe_device -> orbm_build_observations_device -> orbm_cull_map_points_device -> "
        "orbm_register_new_points_device, device time by HIP events), p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us enqueued from "
        "Python on an idle stream (the waits for the next launch included), %.1f / %.1f us with the launches queued behind a busy stream "
        "(back to back, caches cold)" % (reps, warm, pct(t["device"], 50), pct(t["device"], 90), pct(t["queued"], 50), pct(t["queued"], 90)),
        "host form (wait, frame_mp / pose / d_valid / key-frame table read-back, the insert's PYTHON loop, row K uploaded, the device build, wait, slots / CSR / list / "
        "counters read-back, the culling's and the registration's PYTHON loops, d_valid / slots / list / counters / fields uploaded), host wall "
        "time, p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us   (numpy's and Python's loops, not the reference's C++)"
        % (reps, warm, pct(t["host"], 50), pct(t["host"], 90)),
        "both forms gave the same bytes: %s" % same,
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keyframe_latency.txt"))
