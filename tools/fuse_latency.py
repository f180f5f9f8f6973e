"""Latency of one target key frame of the fuse (LocalMapping::searchInNeighbors -> the static SearchByProjection), both ways in one run:
a key frame of 2000 key points, 4000 candidate map points (half of them project onto a key point with a matching descriptor), 1000
more rows that occupy every other slot of the key frame, eight key frames in the table.
  device form   orbm_project_fuse_device -> orbm_search_fuse_device -> orbm_fuse_apply_device on one stream, device time between two
                HIP events; the apply's in / out arrays are restored by device copies outside the timed span
  host form     today's: builder and search on the device, then wait, read d_best_idx, the slot arrays, d_valid and d_found back, the
                array model of tests/fuse_model.py (`apply`, a Python loop over the entries with numpy inside), upload the slots, d_valid
                and d_found.  Host wall time up to the wait that ends the uploads.  The loop is NUMPY's and Python's, not the
                reference's C++: the figure bounds what a host hop costs here, it is not a measurement of MapPoint::replace.
p50 (and p90) of `reps` calls after `warm` warm-up calls (the host form fewer times: it is slow).  Also records the kernel's VGPRs /
LDS from the code object's notes.  Writes profiles/fuse_latency.txt (or the path given as the first argument)."""
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
        if "k_fuse_apply" in name:
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def main(out_path):
    import torch
    import fuse_model as fm
    import projection_model as pm
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps, host_reps = 20, 200, 5
    sc = fm.make_projected_scene()
    cap, stride, n_kf = sc["cap_points"], sc["stride"], len(sc["n"])
    csr = fm.fresh_csr(sc)
    n_obs = len(csr[1])
    post = FramePost(sc["w"], sc["h"], *sc["cam"])
    _, kpu, start, items = post(sc["kps"])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    sigma2 = (pm.SCALE_FACTORS * pm.SCALE_FACTORS).astype(np.float32)
    begin = {k: up(sc[k]) for k in ("slots", "valid", "found")}
    d = {k: v.clone() for k, v in begin.items()}
    d.update(pose_R=up(np.eye(3).reshape(9)), pose_t=up(np.zeros(3)), points=up(sc["points"]), normals=up(sc["normals"]),
             min_dist=up(sc["min_dist"]), max_dist=up(sc["max_dist"]), q_xy=torch.zeros((cap, 2), dtype=torch.float32, device=dev),
             q_radius=torch.zeros(cap, dtype=torch.float32, device=dev), q_level=zi(cap), q_ok=torch.zeros(cap, dtype=torch.uint8, device=dev),
             q_desc=up(sc["q_desc"]), kps=up(np.frombuffer(np.ascontiguousarray(kpu).tobytes(), np.uint8).copy()), desc=up(sc["desc"]),
             cell_start=up(start.astype(np.int32)), cell_items=up(np.concatenate([items, np.zeros(1, items.dtype)]).astype(np.int32)),
             sigma2=up(sigma2), best_idx=zi(cap), best_dist=zi(cap), n=up(sc["n"]), bad=up(sc["bad"]), obs_off=up(csr[0]), obs_kf=up(csr[1]),
             obs_kp=up(csr[2]), visible=up(sc["visible"]), work=zi(cap), code=zi(cap), refresh_sel=zi(cap))
    res = {k: zi(8) for k in ("project", "search", "apply")}
    cam = ProjCamera.make(sc["cam"], (0.0, float(sc["w"]), 0.0, float(sc["h"])))
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def restore():
        for k, v in begin.items():
            d[k].copy_(v)

    def search():
        m.ProjectFuseDevice(cam, dict(d, result=res["project"]), cap, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 3.0)
        m.SearchFuseDevice(dict(d, result=res["search"]), cap, post.cols, post.rows, list_cap=48)

    def device_form():
        e0.record()
        search()
        m.FuseApplyDevice(dict(d, result=res["apply"]), cap, n_kf, sc["K"], stride, cap, n_obs)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def host_form():
        t0 = time.perf_counter()
        search()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        now = dict(sc, best_idx=d["best_idx"].cpu().numpy(), slots=d["slots"].cpu().numpy(), valid=d["valid"].cpu().numpy(),
                   found=d["found"].cpu().numpy())
        out = fm.apply(now, csr)
        for k in ("slots", "valid", "found"):
            d[k].copy_(torch.from_numpy(np.ascontiguousarray(out[k])))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    t = dict(device=[], host=[])
    for i in range(warm + reps):
        restore()
        a = device_form()
        if i >= warm:
            t["device"].append(a)
    restore()
    e0.record()
    search()
    e1.record()
    e1.synchronize()
    search_us = e0.elapsed_time(e1) * 1e3
    for _ in range(host_reps):
        restore()
        us, want = host_form()
        t["host"].append(us)
    restore()
    device_form()
    g = lambda x: x.cpu().numpy()  # noqa: E731
    got = g(res["apply"])
    same = (np.array_equal(got, want["result"]) and np.array_equal(g(d["code"]), want["code"]) and np.array_equal(g(d["refresh_sel"]), want["refresh_sel"])
            and all(np.array_equal(g(d[k]).reshape(-1), np.asarray(want[k]).reshape(-1)) for k in ("slots", "valid", "found")))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "the fuse into one key frame of %d key points: %d table rows (%d candidates), %d key frames, %d observations; d_result of the search %s, "
        "of the apply %s; kernels %s" % (stride, cap, cap - stride // 2, n_kf, n_obs, g(res["search"])[:2].tolist(), got.tolist(), _lib.kernels_sha16()),
        "device form (orbm_project_fuse_device -> orbm_search_fuse_device -> orbm_fuse_apply_device, device time by HIP events), p50 / p90 of %d "
        "after %d warm-up calls: %.1f / %.1f us   (builder + search alone, once: %.1f us)" % (reps, warm, pct(t["device"], 50), pct(t["device"], 90), search_us),
        "host form (builder + search, wait, d_best_idx / slots / d_valid / d_found read-back, the model's PYTHON loop, three uploads), host wall "
        "time, p50 of %d: %.1f us   (numpy's and Python's loop, not the reference's C++)" % (host_reps, pct(t["host"], 50)),
        "both forms gave the same bytes: %s" % same,
    ] + resources()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fuse_latency.txt"))
