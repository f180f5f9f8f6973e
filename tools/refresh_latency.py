"""Latency of refreshing a device-resident map-point table after a fuse or a bundle adjustment, and of the median-depth test of
LocalMapping.cpp:163-165, both ways in one run: 3000 points x 6 observations over 20 key frames of 2000 features.
  device form   orbm_refresh_points_device (normals, distance ranges, descriptors, covisibility counts) and
                orbm_scene_median_depth_device (20 key frames), device time by HIP events
  host form     what a caller has to do today: wait, read the points back, MapPoint::update() in numpy (vectorised over the points,
                float32), gather the observations' descriptor rows on the host and call orbm_distinctive_descriptors, upload normals /
                min_dist / max_dist / descriptors; for the median: wait, read the points back, numpy's sort per key frame.  Host wall
                time up to the wait that ends the uploads.  The loops are NUMPY's, not the reference's C++: the figures bound what a
                host hop costs here, they are not a measurement of Eigen.
p50 (and p90) of 300 calls after 50 warm-up calls, the forms alternating.  Also records the kernels' VGPRs / LDS / occupancy from the
code object's notes.  Writes profiles/refresh_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def resources():
    import kernel_resources
    lines = []
    for name, vgpr, sgpr, lds, scratch, wg in kernel_resources.table(os.path.join(ROOT, "monoorbslam3_amd", "lib", "liborbx.so")):
        if not any(k in name for k in ("k_refreshE", "k_median_depth")):
            continue
        vg, ld, threads = int(vgpr), int(lds), int(wg)
        waves_wg = threads // 64
        by_vgpr = min(8, 512 // ((vg + 7) // 8 * 8))                           # waves per SIMD the registers allow
        wgs = min(by_vgpr * 4 // waves_wg, 160 * 1024 // max(ld, 1), 32 // waves_wg)
        lines.append("%s: %d VGPRs, %s SGPRs, %d B LDS per workgroup of %d threads, scratch %s; registers allow %d waves per SIMD, LDS %d "
                     "workgroups per CU: %d workgroups = %d waves per CU" % ("k_refresh" if "k_refreshE" in name else "k_median_depth", vg, sgpr,
                                                                            ld, threads, scratch, by_vgpr, 160 * 1024 // max(ld, 1), wgs,
                                                                            wgs * waves_wg))
    return lines


def main(out_path):
    import torch
    import refresh_model as rm
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    n_kf, n_feat, n_pts, n_per, warm, reps = 20, 2000, 3000, 6, 50, 300
    sc = rm.make_scene(5, n_kf=n_kf, feats=(n_feat, n_feat), n_rows=n_pts, lengths=(), typical=(n_per, n_per), spare_rows=0)
    sc["valid"][:] = 1
    sc["bad"][:] = 0
    # observations of a point in distinct key frames, as a map holds them; every index in range
    rng = np.random.RandomState(6)
    sc["obs_kf"] = np.concatenate([rng.permutation(n_kf)[:n_per] for _ in range(n_pts)]).astype(np.int32)
    sc["obs_kp"] = rng.randint(0, n_feat, n_pts * n_per).astype(np.int32)
    sc["ref_kf"] = sc["obs_kf"][::n_per].copy()
    sel = np.arange(n_pts, dtype=np.int32)
    want = rm.refresh(sc, sel, n_pts, kf_self=0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rec = lambda k: up(np.frombuffer(k.tobytes(), np.uint8).copy())  # noqa: E731
    kf = KfTable.make(up(sc["pose_R"]), up(sc["pose_t"]), up(sc["bad"]), [rec(k) for k in sc["kps"]], [up(d) for d in sc["kf_desc"]], up(sc["n"]))
    d = {k: up(sc[k]) for k in ("points", "valid", "normals", "min_dist", "max_dist", "desc", "obs_off", "obs_kf", "obs_kp", "ref_kf")}
    d.update(sel=up(sel), covis=torch.zeros(n_kf, dtype=torch.int32, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
    slots = np.full((n_kf, n_feat), -1, np.int32)                              # a key frame's slots: the points that observe it
    for p in range(n_pts):
        slots[sc["obs_kf"][p * n_per:(p + 1) * n_per], sc["obs_kp"][p * n_per:(p + 1) * n_per]] = p
    md = dict(pose_R=up(sc["pose_R"]), pose_t=up(sc["pose_t"]), slots=up(slots), n=up(sc["n"]), points=d["points"],
              median=torch.zeros(n_kf, dtype=torch.float32, device=dev), count=torch.zeros(n_kf, dtype=torch.int32, device=dev),
              baseline=torch.zeros(n_kf, dtype=torch.float32, device=dev))
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    msf = float(rm.MAX_SCALE_FACTOR)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    dev_refresh = lambda: timed(lambda: m.RefreshPointsDevice(kf, d, n_pts, n_pts, n_pts * n_per, msf, kf_self=0))  # noqa: E731
    dev_median = lambda: timed(lambda: m.SceneMedianDepthDevice(md, n_kf, n_feat, n_pts, cur=0))  # noqa: E731
    # host copies a caller on the host form keeps anyway: key-frame records, poses, observations
    O = rm.camera_centres(sc["pose_R"], sc["pose_t"])
    desc_all = np.stack(sc["kf_desc"])                                          # [n_kf][n_feat][32]
    size_all = np.stack([k["size"] for k in sc["kps"]])
    okf, okp = sc["obs_kf"].reshape(n_pts, n_per), sc["obs_kp"].reshape(n_pts, n_per)
    ref_at = np.argmax(okf == sc["ref_kf"][:, None], axis=1)
    off = sc["obs_off"][:n_pts + 1]
    R32, t32 = sc["pose_R"].reshape(n_kf, 3, 3).astype(np.float32), sc["pose_t"].astype(np.float32)

    def host_refresh():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                               # the wait the chain has to make
        P = d["points"].cpu().numpy()
        v = P[:, None, :] - O[okf]
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        dirs = v / ln[..., None]
        s = np.zeros((n_pts, 3), np.float32)
        for j in range(n_per):
            s = s + dirs[:, j]
        normals = s / np.float32(n_per)
        span = ln[np.arange(n_pts), ref_at] * size_all[sc["ref_kf"], okp[np.arange(n_pts), ref_at]]
        max_d, min_d = np.float32(1.2) * span, np.float32(0.8) * (span / rm.MAX_SCALE_FACTOR)
        rows = desc_all[okf.reshape(-1), okp.reshape(-1)]                      # the host gather
        best = m.ComputeDistinctiveDescriptors(rows, off)
        new_desc = rows[off[:-1] + best]
        for key, val in (("normals", normals), ("min_dist", min_d), ("max_dist", max_d), ("desc", new_desc)):
            d[key].copy_(torch.from_numpy(np.ascontiguousarray(val)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, (normals, min_d, max_d, new_desc)

    def host_median():
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        P = d["points"].cpu().numpy()
        med = np.zeros(n_kf, np.float32)
        for k in range(n_kf):
            s = slots[k][slots[k] >= 0]
            z = ((R32[k, 2, 0] * P[s, 0] + R32[k, 2, 1] * P[s, 1]) + R32[k, 2, 2] * P[s, 2]) + t32[k, 2]
            med[k] = np.sort(z)[len(z) // 2]
        v = O[0][None, :] - O
        base = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return (time.perf_counter() - t0) * 1e6, (med, base)

    t = dict(dev_refresh=[], dev_median=[], host_refresh=[], host_median=[])
    for i in range(warm + reps):
        a, b, (c, _), (e, _) = dev_refresh(), dev_median(), host_refresh(), host_median()
        if i >= warm:
            for key, val in zip(("dev_refresh", "dev_median", "host_refresh", "host_median"), (a, b, c, e)):
                t[key].append(val)
    # both forms computed the same thing
    _, (normals, min_d, max_d, new_desc) = host_refresh()
    _, (med, base) = host_median()
    dev_refresh()
    dev_median()
    torch.cuda.synchronize()
    g = lambda x: x.cpu().numpy()  # noqa: E731
    same = (np.array_equal(g(d["normals"]), normals) and np.array_equal(g(d["min_dist"]), min_d) and np.array_equal(g(d["max_dist"]), max_d) and
            np.array_equal(g(d["desc"]), new_desc) and np.array_equal(g(d["normals"]), want["normals"]) and np.array_equal(g(d["desc"]), want["desc"]) and
            np.array_equal(g(md["median"]), med) and np.array_equal(g(md["baseline"]), base))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "refresh of %d map points x %d observations over %d key frames of %d features, and the scene median depth of the %d key frames; "
        "p50 / p90 of %d after %d warm-up calls, forms alternating; kernels %s" % (n_pts, n_per, n_kf, n_feat, n_kf, reps, warm, _lib.kernels_sha16()),
        "refresh, device form (orbm_refresh_points_device, device time by HIP events):                 %.1f / %.1f us   d_result %s" % (
            pct(t["dev_refresh"], 50), pct(t["dev_refresh"], 90), g(d["result"]).tolist()),
        "refresh, host form (wait, points read-back, NUMPY update(), host gather + orbm_distinctive_descriptors, four uploads), host wall "
        "time: %.1f / %.1f us   (numpy's loop, not the reference's C++)" % (pct(t["host_refresh"], 50), pct(t["host_refresh"], 90)),
        "median depth, device form (orbm_scene_median_depth_device, %d key frames, device time):        %.1f / %.1f us   counts %d .. %d" % (
            n_kf, pct(t["dev_median"], 50), pct(t["dev_median"], 90), int(g(md["count"]).min()), int(g(md["count"]).max())),
        "median depth, host form (wait, points read-back, numpy sort per key frame), host wall time:    %.1f / %.1f us" % (
            pct(t["host_median"], 50), pct(t["host_median"], 90)),
        "both forms gave the same bytes: %s" % same,
    ] + resources()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refresh_latency.txt"))
