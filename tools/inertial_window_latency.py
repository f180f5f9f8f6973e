"""Latency of the inertial local BA window's assembly ALONE (orbm_inertial_window_problem_device: steps 1 and 3 of
Optimize::localFullBundleAdjustment on the device-resident map), both ways in one run, at the shapes of tools/vw_step_latency.py: 10 and
25 window key frames of 2000 slots with 8 fixed key frames, about 3000 local points seen by three to six key frames each.
  device form   one launch; p50 (p10 / p90) of `reps` spans between two events on the chain's stream after `warm` warm-up calls
  host form     what a caller does without this call: wait, read the slots, d_valid, the positions, the CSR and the key points back,
                the array model's assembly (tests/inertial_window_model.py `problem`), upload the EdgeMono arrays and the job lists.
                Host wall time.  The loops are NUMPY's and Python's, not the reference's C++: the figure bounds what the host hop costs
                here, it is not a measurement of the reference.
There is no pass bar and no throughput claim: the work is a few thousand slots and short lists.  Writes
profiles/inertial_window_latency.txt (or the path given as the first argument)."""
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
        if "k_iw_" in name:
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def measure(torch, dev, n_window, n_fixed=8, warm=10, reps=200, host_reps=3):
    import inertial_window_model as wm
    import local_ba_model as lm
    from local_ba_latency import make_scene
    from monoorbslam3_amd import matcher
    sc = wm.with_imu(make_scene(n_local=n_window, n_fixed=n_fixed), list(range(n_window)))
    csr = lm.fresh_csr(sc)
    cap, stride, n_kf, n_obs = sc["cap_points"], sc["stride"], len(sc["n"]), len(csr[1])
    up = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy() if x.dtype.fields else np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    d = dict(slots=up(sc["slots"]), valid=up(sc["valid"]), points=up(sc["points"]), n=up(sc["n"]), bad=up(sc["bad"]), obs_off=up(csr[0]),
             obs_kf=up(csr[1]), obs_kp=up(csr[2]), window=up(sc["window"]), kf_imu=up(sc["kf_imu"]), kf_pose_R=up(sc["pose_R"]), kf_pose_t=up(sc["pose_t"]))
    kps = [up(k) for k in sc["kps"]]
    kft = matcher.KfTable.make(d["kf_pose_R"], d["kf_pose_t"], d["bad"], kps, kps, d["n"])
    cs, cl, ce = n_kf, cap, n_obs
    sizes = dict(ba_points=(cl * 3, torch.float64), point_row=(cl, torch.int32), edge_off=(cl + 1, torch.int32), edge_state=(ce, torch.int32),
                 edge_point=(ce, torch.int32), edge_z=(ce * 2, torch.float64), edge_inv_sigma2=(ce, torch.float64), edge_kf=(ce, torch.int32),
                 edge_kp=(ce, torch.int32), state_kf=(cs, torch.int32), init_jobs=(cs * 3, torch.int32), fixed=(cs, torch.uint8),
                 inertial_edges=(n_window * 4, torch.int32), prior_jobs=(3, torch.int32), recover_jobs=(n_window * 3, torch.int32),
                 bias_ids=(n_window, torch.int32), prior_info_jobs=(n_window * 3, torch.int32))
    d.update({k: z(*v) for k, v in sizes.items()})
    d.update(work=z(cap + 2 * n_kf, torch.int32), result=z(16, torch.int32))
    m = matcher.ORBMatcher()
    chain = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def device_form():
        m.InertialWindowProblemDevice(kft, d, stride, cap, n_obs, n_window, sc["n_src"], sc["cap_bank"], sc["n_priors"], sc["max_fixed"], cs, cl, ce,
                                      stream=chain.cuda_stream)

    spans = []
    with torch.cuda.stream(chain):
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(chain)
            device_form()
            b.record(chain)
            b.synchronize()
            if i >= warm:
                spans.append(a.elapsed_time(b) * 1e3)
    head = d["result"].cpu().numpy()
    assert head[wm.W_REFUSED] == 0
    got = {k: d[k].cpu().numpy().copy() for k in wm.OUT}

    def host_form():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        g = lambda k: d[k].cpu().numpy()  # noqa: E731
        now = dict(sc, slots=g("slots").reshape(n_kf, stride), valid=g("valid"), points=g("points").reshape(-1, 3),
                   kps=[np.frombuffer(k.cpu().numpy().tobytes(), sc["kps"][0].dtype) for k in kps])
        prob = wm.problem(now, (g("obs_off"), g("obs_kf"), g("obs_kp")))
        for k in wm.OUT:
            flat = torch.from_numpy(np.ascontiguousarray(prob[k]).reshape(-1))
            d[k][:flat.numel()].copy_(flat)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, prob

    host = []
    for _ in range(host_reps):
        us, want = host_form()
        host.append(us)
    same = all(got[k][:np.asarray(want[k]).size].tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in wm.OUT) and \
        head.tobytes() == want["result"].tobytes()
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    return [
        "%d window + %d fixed key frames of %d slots: %d states, %d points, %d edges" % (n_window, n_fixed, stride, head[0], head[1], head[2]),
        "  device form (one launch), span between two events on the chain's stream, p50 (p10 / p90) of %d after %d warm-up calls: "
        "%.1f (%.1f / %.1f) us" % (reps, warm, pct(spans, 50), pct(spans, 10), pct(spans, 90)),
        "  host form (wait, read-backs, the model's PYTHON assembly, uploads), host wall time, median (min / max) of %d: %.0f (%.0f / %.0f) us   "
        "(numpy's and Python's loops, not the reference's C++)" % (host_reps, pct(host, 50), min(host), max(host)),
        "  both forms gave the same bytes: %s" % same,
    ]


def main(out_path):
    import torch
    from monoorbslam3_amd import _lib
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["the inertial window's assembly alone (orbm_inertial_window_problem_device); kernels %s" % _lib.kernels_sha16()]
    for n_window in (10, 25):
        lines += measure(torch, dev, n_window)
    lines += resources()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "inertial_window_latency.txt"))
