"""Latency of one local bundle adjustment on the device-resident map (Optimize::localBundleAdjustment), both ways in one run, at a
mapper-like size: 20 local and 10 fixed key frames of 2000 features, about 3000 local points seen by three to six key frames each.
  device form   orbm_local_ba_problem_device -> one 32-byte read-back -> orbba_local_bundle_adjustment_device ->
                orbm_local_ba_apply_device on one stream; host wall time (the LM waits once per trial, so device events alone would
                leave the waits out); the in / out arrays are restored by device copies outside the timed span
  host form     the parent commit's: wait, read the slots, d_valid, the CSR, the table and the poses back, the array model's gathering
                loop (tests/local_ba_model.py `problem`), orbba_local_bundle_adjustment on host pointers, the model's `apply`, upload
                the slots, d_valid, d_ref_kf, the positions and the poses.  Host wall time.  The loops are NUMPY's and Python's, not the
                reference's C++: the figure bounds what the host hop costs here, it is not a measurement of the reference.
Median and the 10th / 90th percentile of `reps` calls after `warm` warm-up calls (the host form fewer times: it is slow).  Writes
profiles/local_ba_latency.txt (or the path given as the first argument)."""
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
        if "k_lba_" in name or "k_lmi_" in name:
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def make_scene(n_local=20, n_fixed=10, stride=2000, n_points=3000, seed=7):
    import local_ba_model as lm
    from projection_model import KP_DTYPE, N_LEVELS, SCALE_FACTORS
    rng = np.random.RandomState(seed)
    n_kf, cap = n_local + n_fixed, n_points + 200
    pose_R = np.tile(np.eye(3).reshape(9), (n_kf, 1))
    pose_t = rng.uniform(-0.5, 0.5, (n_kf, 3)).astype(np.float32).astype(np.float64)
    truth = np.stack([rng.uniform(-3, 3, cap), rng.uniform(-2, 2, cap), rng.uniform(5, 10, cap)], 1)
    kps = []
    for _ in range(n_kf):
        kp = np.zeros(stride, KP_DTYPE)
        kp["octave"], kp["class_id"] = rng.randint(0, N_LEVELS, stride), -1
        kp["size"] = SCALE_FACTORS[kp["octave"]]
        kps.append(kp)
    slots = np.full((n_kf, stride), -1, np.int32)
    used = np.zeros(n_kf, np.int64)
    ref_kf = np.zeros(cap, np.int32)
    for p in range(n_points):
        ks = rng.permutation(n_kf)[:rng.randint(3, 7)]
        if ks.min() >= n_local:
            ks[0] = rng.randint(0, n_local)
        ref_kf[p] = ks[0]
        for j, k in enumerate(ks):
            i = used[k]
            used[k] += 1
            slots[k, i] = p
            Pc = truth[p] + pose_t[k]
            noise = rng.normal(0, 0.5, 2) if rng.uniform() > 0.03 else rng.uniform(40, 60, 2)
            kps[k]["x"][i], kps[k]["y"][i] = lm._project(lm.PINHOLE, Pc) + noise
    valid = (np.arange(cap) < n_points).astype(np.uint8)
    points = (truth + rng.normal(0, 0.02, truth.shape)).astype(np.float32)
    return dict(n=np.full(n_kf, stride, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=stride, valid=valid, points=points,
                cap_points=cap, pose_R=pose_R, pose_t=pose_t, kps=kps, local=np.arange(n_local, dtype=np.int32), first_kf=n_local, ref_kf=ref_kf,
                cam=lm.PINHOLE)


def main(out_path):
    import torch
    import local_ba_model as lm
    from monoorbslam3_amd import _lib, ba, matcher
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps, host_reps = 5, 30, 3
    sc = make_scene()
    csr = lm.fresh_csr(sc)
    cap, stride, n_kf, n_obs = sc["cap_points"], sc["stride"], len(sc["n"]), len(csr[1])
    up = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy() if x.dtype.fields else np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    begin = dict(slots=up(sc["slots"]), valid=up(sc["valid"]), ref_kf=up(sc["ref_kf"]), points=up(sc["points"]), kf_pose_R=up(sc["pose_R"]),
                 kf_pose_t=up(sc["pose_t"]))
    d = {k: v.clone() for k, v in begin.items()}
    d.update(n=up(sc["n"]), bad=up(sc["bad"]), obs_off=up(csr[0]), obs_kf=up(csr[1]), obs_kp=up(csr[2]), local=up(sc["local"]))
    kps = [up(k) for k in sc["kps"]]
    kft = matcher.KfTable.make(d["kf_pose_R"], d["kf_pose_t"], d["bad"], kps, kps, d["n"])
    cp, cl, ce = n_kf, cap, n_obs
    d.update(work=z(cap + n_kf, torch.int32), pose_R=z(cp * 9, torch.float64), pose_t=z(cp * 3, torch.float64), pose_fixed=z(cp, torch.uint8),
             ba_points=z(cl * 3, torch.float64), edge_pose=z(ce, torch.int32), edge_point=z(ce, torch.int32), edge_z=z(ce * 2, torch.float64),
             edge_inv_sigma2=z(ce, torch.float64), edge_kf=z(ce, torch.int32), edge_kp=z(ce, torch.int32), edge_off=z(cl + 1, torch.int32),
             point_row=z(cl, torch.int32), pose_kf=z(cp, torch.int32), est_pose_R=z(cp * 9, torch.float64), est_pose_t=z(cp * 3, torch.float64),
             est_points=z(cl * 3, torch.float64), chi2=z(ce, torch.float64), outlier=z(ce, torch.uint8))
    res = dict(problem=z(16, torch.int32), apply=z(8, torch.int32))
    m = matcher.ORBMatcher()

    def restore():
        for k, v in begin.items():
            d[k].copy_(v)
        torch.cuda.synchronize()

    def device_form():
        t0 = time.perf_counter()
        m.LocalBaProblemDevice(kft, dict(d, result=res["problem"]), stride, cap, n_obs, len(sc["local"]), sc["first_kf"], cp, cl, ce)
        head = res["problem"][:8].cpu().numpy()                            # the one 32-byte read-back
        assert head[lm.P_REFUSED] == 0
        info = ba.local_bundle_adjustment_device(sc["cam"], d, int(head[0]), int(head[1]), int(head[2]))
        m.LocalBaApplyDevice(dict(d, result=res["apply"]), n_kf, stride, cap, n_obs, int(head[3]), int(head[1]), int(head[2]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, head, info

    def host_form():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        g = lambda k: d[k].cpu().numpy()  # noqa: E731
        now = dict(sc, slots=g("slots"), valid=g("valid"), points=g("points"), pose_R=g("kf_pose_R"), pose_t=g("kf_pose_t"), ref_kf=g("ref_kf"))
        now_csr = (g("obs_off"), g("obs_kf"), g("obs_kp"))
        prob = lm.problem(now, now_csr)
        out = ba.local_bundle_adjustment(sc["cam"], prob["pose_R"], prob["pose_t"], prob["pose_fixed"], prob["ba_points"], prob["edge_pose"],
                                         prob["edge_point"], prob["edge_z"], prob["edge_inv_sigma2"])
        new = lm.apply(now, now_csr, prob, out["pose_R"].reshape(-1, 9), out["pose_t"], out["points"], out["outlier"].astype(np.uint8))
        for k, mk in (("slots", "slots"), ("valid", "valid"), ("ref_kf", "ref_kf"), ("points", "points"), ("kf_pose_R", "pose_R"), ("kf_pose_t", "pose_t")):
            d[k].copy_(torch.from_numpy(np.ascontiguousarray(new[mk])))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, new

    t = dict(device=[], host=[])
    for i in range(warm + reps):
        restore()
        us, head, info = device_form()
        if i >= warm:
            t["device"].append(us)
    got = {k: d[k].cpu().numpy().copy() for k in begin}
    for _ in range(host_reps):
        restore()
        us, want = host_form()
        t["host"].append(us)
    same = all(got[k].tobytes() == np.ascontiguousarray(want[mk]).tobytes() for k, mk in
               (("slots", "slots"), ("valid", "valid"), ("ref_kf", "ref_kf"), ("points", "points"), ("kf_pose_R", "pose_R"), ("kf_pose_t", "pose_t")))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "local BA on %d local + %d fixed key frames of %d features: %d poses, %d points, %d edges; %d iterations, %d trials; d_result of the "
        "apply %s; kernels %s" % (len(sc["local"]), n_kf - len(sc["local"]), stride, head[0], head[1], head[2], info["iterations"], info["trials"],
                                  res["apply"].cpu().numpy().tolist(), _lib.kernels_sha16()),
        "device form (assemble -> 32-byte read-back -> LM on device arrays -> apply), host wall time, median (p10 / p90) of %d after %d warm-up "
        "calls: %.1f (%.1f / %.1f) us" % (reps, warm, pct(t["device"], 50), pct(t["device"], 10), pct(t["device"], 90)),
        "host form (wait, read-backs, the model's PYTHON gathering loop, orbba_local_bundle_adjustment, the model's apply, uploads), host wall "
        "time, median (min / max) of %d: %.1f (%.1f / %.1f) us   (numpy's and Python's loops, not the reference's C++)"
        % (host_reps, pct(t["host"], 50), min(t["host"]), max(t["host"])),
        "both forms gave the same bytes: %s" % same,
    ] + resources()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "local_ba_latency.txt"))
