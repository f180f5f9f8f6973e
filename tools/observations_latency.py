"""Latency of rebuilding the observation lists of a device-resident map-point table and of KeyFrameCulling, both ways in one run:
25 key frames of 2000 features, 6000 map points seen by 6 key frames each (36000 observations).
  device form   orbm_build_observations_device (five launches) and orbm_cull_keyframes_device (one workgroup) on the slot arrays,
                device time by HIP events; the cull's in / out arrays are restored by device copies outside the timed span
  host form     what a caller has to do without them: wait, read the slot arrays, d_valid and d_bad back, the numpy model of
                tests/observations_model.py (`build`, vectorised; `cull`, its Python loop over candidates x slots x lists), upload the
                CSR / the edited slots, d_valid, d_bad and d_ref_kf.  Host wall time up to the wait that ends the uploads.  The loops
                are NUMPY's and Python's, not the reference's C++: the figures bound what a host hop costs here, they are not a
                measurement of std::map.
p50 (and p90) of `reps` calls after `warm` warm-up calls, the forms alternating (the host cull fewer times: it is slow).  Also records
the kernels' VGPRs / LDS from the code object's notes.  Writes profiles/observations_latency.txt (or the path given as the first
argument)."""
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
        if any(k in name for k in ("k_obs_", "k_cull")):
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def make_scene(n_kf=25, n_feat=2000, n_pts=6000, n_per=6, seed=4):
    """every point in n_per distinct key frames, octaves at random; two key frames are redundant and get culled"""
    from projection_model import KP_DTYPE, N_LEVELS
    rng = np.random.RandomState(seed)
    slots = np.full((n_kf, n_feat), -1, np.int32)
    used = np.zeros(n_kf, np.int64)
    for p in range(n_pts):
        ks = rng.permutation(n_kf)[:n_per]
        slots[ks, used[ks]] = p
        used[ks] += 1
    assert used.max() <= n_feat
    kps = []
    for k in range(n_kf):
        kp = np.zeros(n_feat, KP_DTYPE)
        kp["octave"], kp["class_id"] = rng.randint(0, N_LEVELS, n_feat), -1
        if k in (5, 12):                                                       # coarse features only: every other observer counts, culled
            kp["octave"] = N_LEVELS - 1
        kps.append(kp)
    return dict(n=np.full(n_kf, n_feat, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=n_feat, valid=np.ones(n_pts, np.uint8),
                cap_points=n_pts, kps=kps, ref_kf=rng.randint(0, n_kf, n_pts).astype(np.int32), recent=np.arange(n_kf, dtype=np.int32),
                timestamps=0.05 * np.arange(n_kf), first_kf=0)


def main(out_path):
    import torch
    import observations_model as om
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps, host_cull_reps = 20, 200, 5
    sc = make_scene()
    n_kf, stride, cap = len(sc["n"]), sc["stride"], sc["cap_points"]
    off, okf, okp, res = om.build(sc["n"], sc["bad"], sc["slots"], stride, sc["valid"], cap, 1 << 30)
    n_obs = len(okf)
    want = om.cull(sc, off, okf, okp)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rec = lambda k: up(np.frombuffer(k.tobytes(), np.uint8).copy())  # noqa: E731
    z = torch.zeros(1, dtype=torch.float64, device=dev)
    start = {k: up(sc[k]) for k in ("bad", "slots", "valid", "ref_kf")}
    d = {k: v.clone() for k, v in start.items()}
    d.update(n=up(sc["n"]), obs_off=torch.zeros(cap + 1, dtype=torch.int32, device=dev), obs_kf=torch.zeros(n_obs, dtype=torch.int32, device=dev),
             obs_kp=torch.zeros(n_obs, dtype=torch.int32, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev),
             code=torch.zeros(n_kf, dtype=torch.int32, device=dev), num_mp=torch.zeros(n_kf, dtype=torch.int32, device=dev),
             num_redundant=torch.zeros(n_kf, dtype=torch.int32, device=dev))
    kf = KfTable.make(z, z, d["bad"], [rec(k) for k in sc["kps"]], torch.zeros(n_kf, dtype=torch.int64, device=dev), d["n"])
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def restore():
        for k, v in start.items():
            d[k].copy_(v)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    dev_build = lambda: timed(lambda: m.BuildObservationsDevice(d, n_kf, stride, cap, n_obs))  # noqa: E731
    dev_cull = lambda: timed(lambda: m.CullKeyFramesDevice(kf, d, stride, cap, n_obs, sc["recent"], sc["timestamps"], first_kf=sc["first_kf"]))  # noqa: E731

    def host_build():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                               # the wait the chain has to make
        slots, valid, bad = d["slots"].cpu().numpy(), d["valid"].cpu().numpy(), d["bad"].cpu().numpy()
        o, a, b, _ = om.build(sc["n"], bad, slots, stride, valid, cap, n_obs)
        d["obs_off"].copy_(torch.from_numpy(o))
        d["obs_kf"][:len(a)].copy_(torch.from_numpy(a))
        d["obs_kp"][:len(b)].copy_(torch.from_numpy(b))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def host_cull():
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        now = dict(sc, slots=d["slots"].cpu().numpy(), valid=d["valid"].cpu().numpy(), bad=d["bad"].cpu().numpy(), ref_kf=d["ref_kf"].cpu().numpy())
        out = om.cull(now, off, okf, okp)
        for k in ("bad", "slots", "valid", "ref_kf"):
            d[k].copy_(torch.from_numpy(np.ascontiguousarray(out[k])))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    t = dict(dev_build=[], dev_cull=[], host_build=[], host_cull=[])
    for i in range(warm + reps):
        restore()
        a = dev_build()
        b = dev_cull()
        restore()
        c = host_build()
        if i >= warm:
            t["dev_build"].append(a), t["dev_cull"].append(b), t["host_build"].append(c)
    for _ in range(host_cull_reps):
        restore()
        t["host_cull"].append(host_cull()[0])
    # both forms computed the same thing
    restore()
    dev_build()
    dev_cull()
    torch.cuda.synchronize()
    g = lambda x: x.cpu().numpy()  # noqa: E731
    same = (np.array_equal(g(d["obs_off"]), off) and np.array_equal(g(d["obs_kf"]), okf) and np.array_equal(g(d["obs_kp"]), okp) and
            all(np.array_equal(g(d[k]).reshape(-1), np.asarray(want[k]).reshape(-1)) for k in ("bad", "slots", "valid", "ref_kf", "code", "num_mp",
                                                                                             "num_redundant", "result")))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "observation lists of %d map points x %d observations over %d key frames of %d features (%d entries), and KeyFrameCulling over the %d "
        "key frames; p50 / p90 of %d after %d warm-up calls, forms alternating; kernels %s" % (cap, n_obs // cap, n_kf, stride, n_obs, n_kf, reps, warm,
                                                                                              _lib.kernels_sha16()),
        "build, device form (orbm_build_observations_device, device time by HIP events):          %.1f / %.1f us" % (
            pct(t["dev_build"], 50), pct(t["dev_build"], 90)),
        "build, host form (wait, slots / d_valid / d_bad read-back, NUMPY build, three uploads), host wall time: %.1f / %.1f us" % (
            pct(t["host_build"], 50), pct(t["host_build"], 90)),
        "cull, device form (orbm_cull_keyframes_device, device time by HIP events):               %.1f / %.1f us   d_result %s" % (
            pct(t["dev_cull"], 50), pct(t["dev_cull"], 90), g(d["result"]).tolist()),
        "cull, host form (wait, read-back, the model's PYTHON loop, four uploads), host wall time, p50 of %d: %.1f us   (Python's loop, not "
        "the reference's C++)" % (host_cull_reps, pct(t["host_cull"], 50)),
        "both forms gave the same bytes: %s" % same,
    ] + resources()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "observations_latency.txt"))
