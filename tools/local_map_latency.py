"""Latency of the local-map step of one tracked frame, both ways in one run: 200 key frames x 2000 slots over 60000 table rows, a camera
moving along the table so that covisibility is local, a frame of 2000 key points with about 300 matched and about 40 voted key frames.
  device form   orbm_local_map_device -> orbm_project_frustum_device (d_valid = the mask, nq = the table's rows) ->
                orbm_track_counters_device (1 | 2) on one stream, device time between two HIP events; d_frame_mp and d_visible are
                restored by device copies outside the timed span.  Twice: as enqueued from Python on an idle stream, where the span also
                holds the gaps in which the device waits for the next launch, and behind a stream kept busy by large fills, so that
                all launches are queued before the first one starts and the kernels run back to back (with the caches the fills left: cold)
  host form     the parent commit's: wait, read frame_mp, the slot arrays, d_n, d_bad, d_valid, the CSR and the graph's lists and
                parents back, the array model of tests/local_map_model.py (`local_map`: numpy and Python loops), upload the mask.  Host
                wall time up to the wait that ends the upload.  The loops are NUMPY's and Python's, not the reference's C++: the figure
                bounds what the host hop costs here, it is not a measurement of Tracking::updateLocalMap.
p50 (and p90) of `reps` calls after `warm` warm-up calls, every form.  Writes profiles/local_map_latency.txt (or the path given as the
first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def make_scene(n_kf=200, stride=2000, cap=60000, span=6000, n2=2000, n_matched=300, near=40, seed=7):
    """key frame k observes rows of [k * step, k * step + span); its list is its `near` nearest key frames by shared window, its parent
    the one before it (graph_model.update's Python loops over 200 x 2000 slots would take minutes: the lists are written directly)"""
    import graph_model as gm
    import observations_model as om
    import projection_model as pm
    rng = np.random.RandomState(seed)
    step = (cap - span) // (n_kf - 1)
    slots = np.stack([k * step + rng.choice(span, stride, replace=False) for k in range(n_kf)]).astype(np.int32)
    slots[rng.rand(n_kf, stride) < 0.4] = -1
    n = np.full(n_kf, stride, np.int32)
    bad = np.zeros(n_kf, np.uint8)
    valid = (rng.rand(cap) < 0.97).astype(np.uint8)
    g = gm.new_graph(n_kf)
    for k in range(n_kf):
        order = np.argsort(np.abs(np.arange(n_kf) - k), kind="stable")[1:near + 1]
        g["ord_kf"][k, :near], g["ord_n"][k], g["parent"][k] = order, near, k - 1
    off, okf, okp, _ = om.build(n, bad, slots, stride, valid, cap, 1 << 30)
    at = n_kf - 25                                                 # the frame looks at the window of key frame `at`
    rows = at * step + rng.choice(span, n_matched, replace=False)
    fm = np.full(n2, -1, np.int32)
    fm[rng.choice(n2, n_matched, replace=False)] = rows
    parts = [pm.make_cloud(pm.FRUSTUM, False, cap // 3, seed + i) for i in range(3)]       # the table: three clouds under one pose
    cloud = dict(parts[0], **{k: np.concatenate([c[k] for c in parts]) for k in ("points", "normals", "min_dist", "max_dist")})
    w = dict(n_kf=n_kf, stride=stride, cap_points=cap, n=n, bad=bad, slots=slots, valid=valid, obs_off=off, obs_kf=okf, obs_kp=okp, g=g)
    return dict(w=w, frame_mp=fm, recent=np.arange(n_kf - 10, n_kf, dtype=np.int32), cloud=cloud)


def main(out_path):
    import torch
    import local_map_model as lm
    import projection_model as pm
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import CovisGraph, ORBMatcher, ProjCamera
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 20, 300
    sc = make_scene()
    w, cloud = sc["w"], sc["cloud"]
    n_kf, stride, cap, n2, n_obs = w["n_kf"], w["stride"], w["cap_points"], len(sc["frame_mp"]), len(w["obs_kf"])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    g = {k: up(w["g"][k]) for k in ("weight", "ord_kf", "ord_n", "parent")}
    graph = CovisGraph.make(g["weight"], g["ord_kf"], g["ord_n"], g["parent"])
    cap_local_kf, cap_rows = n_kf, cap
    d = {k: up(w[k]) for k in ("n", "bad", "slots", "valid", "obs_off", "obs_kf", "obs_kp")}
    d.update(pose_R=up(np.asarray(cloud["R"], np.float64).reshape(9)), pose_t=up(np.asarray(cloud["t"], np.float64)),
             **{k: up(cloud[k]) for k in ("points", "normals", "min_dist", "max_dist")})
    frame0, visible0 = up(sc["frame_mp"]), zi(cap)
    d.update(frame_mp=frame0.clone(), visible=visible0.clone(), found=zi(cap), ref=zi(1), work=zi(cap + n_kf), local_kf=zi(cap_local_kf),
             rows=zi(cap_rows), local_mask=torch.zeros(cap, dtype=torch.uint8, device=dev), q_ok=torch.zeros(cap, dtype=torch.uint8, device=dev),
             q_xy=zf(cap, 2), q_radius=zf(cap), q_level=zi(cap))
    res = dict(local=zi(16), frustum=zi(8), counters=zi(8))
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def restore():
        d["frame_mp"].copy_(frame0)
        d["visible"].copy_(visible0)

    busy = torch.empty(64 << 20, dtype=torch.int32, device=dev)            # 256 MB: eight fills outlast the launches many times

    def device_form(behind_busy=False):
        if behind_busy:
            for _ in range(8):
                busy.zero_()
        e0.record()
        m.LocalMapDevice(graph, dict(d, result=res["local"]), n2, n_kf, stride, cap, n_obs, sc["recent"], cap_local_kf, cap_rows)
        m.ProjectFrustumDevice(cam, dict(d, valid=d["local_mask"], result=res["frustum"]), cap, n2, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 1.0)
        m.TrackCountersDevice(dict(d, result=res["counters"]), n2, cap, cap, 1 | 2)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    mask_dev = torch.zeros(cap, dtype=torch.uint8, device=dev)

    def host_form():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        hw = {k: d[k].cpu().numpy() for k in ("n", "bad", "valid", "obs_off", "obs_kf", "obs_kp")}
        hw["slots"] = d["slots"].cpu().numpy().reshape(n_kf, stride)
        hg = dict(ord_kf=g["ord_kf"].cpu().numpy().reshape(n_kf, n_kf), ord_n=g["ord_n"].cpu().numpy(), parent=g["parent"].cpu().numpy())
        out = lm.local_map(dict(hw, n_kf=n_kf, stride=stride, cap_points=cap, g=hg), frame0.cpu().numpy(), sc["recent"])
        mask_dev.copy_(torch.from_numpy(out["mask"]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    t = dict(device=[], queued=[], host=[])
    for key, behind_busy in (("device", False), ("queued", True)):
        for i in range(warm + reps):
            restore()
            a = device_form(behind_busy)
            if i >= warm:
                t[key].append(a)
    for i in range(warm + reps):
        us, want = host_form()
        if i >= warm:
            t["host"].append(us)
    restore()
    device_form()
    c = lambda x: x.cpu().numpy()  # noqa: E731
    n_rows = len(want["rows"])
    same = (np.array_equal(c(res["local"]), want["result"]) and np.array_equal(c(d["local_mask"]), want["mask"])
            and np.array_equal(c(d["rows"])[:n_rows], want["rows"]) and np.array_equal(c(d["local_kf"])[:len(want["local_kf"])], want["local_kf"])
            and int(c(d["ref"])[0]) == want["ref"] and np.array_equal(c(d["frame_mp"]), want["frame_mp"]))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "the local-map step of one tracked frame: %d key frames x %d slots, %d table rows, %d observations, a frame of %d slots; d_result of the "
        "local map %s, of the frustum builder %s, of the counters %s; kernels %s"
        % (n_kf, stride, cap, n_obs, n2, want["result"].tolist(), c(res["frustum"]).tolist(), c(res["counters"]).tolist(), _lib.kernels_sha16()),
        "device form (orbm_local_map_device -> orbm_project_frustum_device -> orbm_track_counters_device, device time by HIP events), "
        "p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us enqueued from Python on an idle stream (the waits for the next launch included), "
        "%.1f / %.1f us with the launches queued behind a busy stream (back to back, caches cold)"
        % (reps, warm, pct(t["device"], 50), pct(t["device"], 90), pct(t["queued"], 50), pct(t["queued"], 90)),
        "host form (wait, frame_mp / slots / d_n / d_bad / d_valid / CSR / lists / parents read-back, the model's PYTHON loops, the mask uploaded), "
        "host wall time, p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us   (numpy's and Python's loops, not the reference's C++)"
        % (reps, warm, pct(t["host"], 50), pct(t["host"], 90)),
        "both forms gave the same bytes: %s" % same,
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "local_map_latency.txt"))
