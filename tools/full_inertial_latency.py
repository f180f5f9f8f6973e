"""Latency of fullInertialOptimize's iteration on the device (include/orbfi.h) at 17 key frames -- LocalMapping runs the IMU
initialisation at key frame id 16 -- and 400 map points:
  one linearisation  orbfi_linearize_device (mode 0)
  one trial chain    orbvw_reduce_device (d_off_edges, d_H_off) -> orbvw_solve_device -> orbvw_backsub_device -> orbi_graph_oplus_device ->
                     orbfi_linearize_device (mode 1) -> orbvw_linearize_device (mode 1), enqueued on one stream behind the pop of the trial before
  device form   p50 (p10 / p90) of `reps` spans between two events on the chain's stream after `warm` warm-up calls
  host form     the parent's form, without these calls: wait, read the vertices, the points and the records back, the numpy model's
                iteration (tests/full_inertial_model.py), upload the vertices and the points again.  Host wall time.  The loops are NUMPY's
                and Python's, not the reference's C++: the figure bounds what the host hop costs here, it is not a measurement of the reference.
There is no pass bar and no throughput claim: the case for these calls is the removed round trip.  Writes
profiles/full_inertial_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from imu_init_latency import _spans  # noqa: E402


def resources():
    import kernel_resources
    lines = []
    for name, vgpr, sgpr, lds, scratch, wg in kernel_resources.table(os.path.join(ROOT, "monoorbslam3_amd", "lib", "liborbx.so")):
        if "k_fi_" in name:
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def measure(torch, dev, n_kf=17, n_points=400, lam=1e-5, warm=10, reps=200, host_reps=3):
    import full_inertial_model as fim
    from monoorbslam3_amd import imu
    from test_full_inertial_gpu import _Fi
    sc = fim.scene(n_kf, n_points, common_bias=True)
    d = _Fi(torch, dev, sc)
    i, w = d.i, d.w
    chain = torch.cuda.Stream(device=dev)
    st = chain.cuda_stream
    live = [i.Rwb, i.twb, i.v, i.bg, i.ba, i.it]
    saved = [t.clone() for t in live]
    torch.cuda.synchronize()
    with torch.cuda.stream(chain):
        imu.edge_information_device(i.bank, i.cap, i.edges, i.ne, i.info, i.walk, i.result, stream=st)
        w.lam.fill_(lam)
        d.linearize(0, st)
        w.linearize(0, H_diag=i.H_diag, b=i.b, stream=st)

    def trial():
        for s, t in zip(saved, live):                               # the pop of the trial before: every trial starts from the same estimate
            t.copy_(s)
        w.reduce(H_diag=i.H_diag, H_off=d.H_off, b=i.b, stream=st)
        w.solve(b=i.b, stream=st)
        w.backsub(stream=st)
        imu.graph_oplus_device(i.graph, w.dx, i.it, i.result, stream=st)
        d.linearize(1, st)
        w.linearize(1, points=w.points_out, stream=st)

    tri = _spans(torch, chain, trial, warm, reps)
    torch.cuda.synchronize()
    dev_totals = (float(i.total.cpu()[1]), float(w.total.cpu()[1]))
    with torch.cuda.stream(chain):
        for s, t in zip(saved, live):
            t.copy_(s)
    lin = _spans(torch, chain, lambda: d.linearize(0, st), warm, reps)
    torch.cuda.synchronize()
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        back = [t.cpu().numpy() for t in live] + [w.points.cpu().numpy(), i.bank.cpu().numpy()]      # the read-backs
        it = fim.iterate(sc, lam)
        for t, a in zip(live + [w.points], back):                   # the upload
            t.copy_(torch.from_numpy(a).to(dev))
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    m_totals = (it["inertial1"]["total"][1], it["visual1"]["total"][1])
    dev_rel = max(abs(a - b) for a, b in zip(dev_totals, m_totals)) / sum(m_totals)
    d.finish()
    return ["%d key frames and the carrier: %d inertial edges, %d points, %d EdgeMono, N = %d, lambda %g" % (n_kf, i.ne, w.np_, w.ne, 15 * (n_kf + 1), lam),
            "  one linearisation (orbfi_linearize_device, mode 0, two launches), span between two events on the chain's stream, p50 (p10 / p90) of %d after %d warm-up calls: %.1f (%.1f / %.1f) us"
            % (reps, warm, lin[0], lin[1], lin[2]),
            "  one trial chain (pop, reduce, solve, backsub, oplus, both linearisations in mode 1), likewise: %.1f (%.1f / %.1f) us" % (tri[0], tri[1], tri[2]),
            "  host form (wait, read-backs, the model's PYTHON iteration, upload), host wall time, median (min / max) of %d: %.0f (%.0f / %.0f) us"
            "   (numpy's and Python's loops, not the reference's C++)" % (host_reps, np.median(host), min(host), max(host)),
            "  the device's two trial totals against the model's, relative to their sum (a free-running trial at lambda %g, not a stage): %.3g" % (lam, dev_rel)]


def main():
    import torch
    from monoorbslam3_amd import _lib
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["fullInertialOptimize's iteration (orbfi.h): one trial chain and one linearisation; kernels %s" % _lib.kernels_sha16()]
    lines += measure(torch, dev)
    lines += resources()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "full_inertial_latency.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
