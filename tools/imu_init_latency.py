"""Latency of the IMU initialisation's steps on the device (include/orbii.h), at 16 and 100 key frames -- the first initialisation
(LocalMapping runs it at key frame 16) and a late one:
  one trial chain    orbii_damp_device -> orbvw_solve_device -> orbii_oplus_device -> orbii_linearize_device (mode 1), enqueued on one stream
  one linearisation  orbii_linearize_device (mode 0)
  device form   p50 (p10 / p90) of `reps` spans between two events on the chain's stream after `warm` warm-up calls
  host form     what a caller does without these calls: wait, read the state rows, the pose table and the records back, the numpy model's
                linearisation and trial (tests/imu_init_model.py), upload the state rows again.  Host wall time.  The loops are NUMPY's and
                Python's, not the reference's C++: the figure bounds what the host hop costs here, it is not a measurement of the reference.
There is no pass bar and no throughput claim: the case for these calls is the removed round trip.  Writes profiles/imu_init_latency.txt
(or the path given as the first argument)."""
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
        if "k_ii_" in name or "k_rescale_" in name:
            lines.append("%s: %s VGPRs, %s SGPRs, %s B static LDS per workgroup of %s threads, scratch %s" % (name, vgpr, sgpr, lds, wg, scratch))
    return lines


def _spans(torch, chain, fn, warm, reps):
    spans = []
    with torch.cuda.stream(chain):
        for k in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(chain)
            fn()
            b.record(chain)
            b.synchronize()
            if k >= warm:
                spans.append(a.elapsed_time(b) * 1000.0)
    return np.percentile(spans, [50, 10, 90])


def measure(torch, dev, n_kf, warm=10, reps=200, host_reps=3):
    import factors_model as fm
    import imu_init_model as mm
    import vw_model as wm
    from monoorbslam3_amd import imu, imu_init, vw
    kind, pg, pa, lam = mm.KIND_GS, 1e6, 1e12, 1e3
    sc = mm.make_scene(n_kf, seed=7, sample_counts=(100,), tilt=0.2, scale=1.1)
    g, N, ne = sc["graph"], mm.system_size(n_kf), n_kf - 1
    bank = fm.im.Bank(len(sc["recs"]), 100)
    bank.recs = [r.copy() for r in sc["recs"]]
    up = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy() if x.dtype.fields else np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    d_bank, d_state, d_pose_R, d_pose_t = up(bank.pack()[0]), up(sc["state"]), up(sc["pose_R"]), up(sc["pose_t"])
    t = dict(v=up(g.v.reshape(-1)), shared=up(g.shared), it=z(1, torch.int32), Rwb=up(g.Rwb.reshape(-1)), twb=up(g.twb.reshape(-1)), Oc=up(g.Oc.reshape(-1)),
             Pcb=up(g.Pcb.reshape(-1)))
    graph = imu_init.Graph.make(t["v"], t["shared"], t["it"], t["Rwb"], t["twb"], t["Oc"], t["Pcb"], n_kf)
    saved = [t["v"].clone(), t["shared"].clone(), t["it"].clone()]
    edges, info, walk = up(sc["edges"]), z(81 * ne), z(18 * ne)
    work, err, chi2, chi2_prior, total = z(mm.EDGE_WORK * ne), z(9 * ne), z(ne), z(2), z(1)
    H, b, S, rhs, dx, out, lam_d, result = z(N * N), z(N), z(N * N), z(N), z(N), z(3), z(1), z(8, torch.int32)
    ib = imu_init.Bias.make(sc["initial_bias"])
    chain = torch.cuda.Stream(device=dev)
    st = chain.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(chain):
        imu.edge_information_device(d_bank, len(sc["recs"]), edges, ne, info, walk, result, stream=st)
        lam_d.fill_(lam)

    def linearise(mode=0):
        imu_init.linearize_device(graph, d_bank, len(sc["recs"]), sc["cal"]["gravity"], edges, info, ib, pg, pa, kind, work, err, chi2, chi2_prior, total, result,
                                  mode=mode, d_H=None if mode else H, d_b=None if mode else b, stream=st)

    def trial():
        for s, live in zip(saved, (t["v"], t["shared"], t["it"])):      # the pop of the trial before: every trial starts from the same estimate
            live.copy_(s)
        imu_init.damp_device(n_kf, kind, H, b, lam_d, S, rhs, out, result, stream=st)
        vw.solve_device(N // 15, S, rhs, b, lam_d, dx, out, result, stream=st)
        imu_init.oplus_device(graph, kind, dx, result, stream=st)
        linearise(1)

    lin = _spans(torch, chain, linearise, warm, reps)
    tri = _spans(torch, chain, trial, warm, reps)
    torch.cuda.synchronize()
    dev_total, dev_scale = float(total.cpu()[0]), float(out.cpu()[0])
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        state, _, _, _ = d_state.cpu().numpy(), d_pose_R.cpu().numpy(), d_pose_t.cpu().numpy(), d_bank.cpu().numpy()     # the read-backs
        be = mm.ModelInit(sc, kind, pg, pa)
        be.linearize()
        ok, m_scale, _, g1 = be.trial_outputs(lam)
        m_total = float(be._lin(g1, 1)["total"][0])
        d_state.copy_(torch.from_numpy(state).to(dev))                   # the upload
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    same = abs(dev_total - m_total) <= 1e-9 * abs(m_total) and abs(dev_scale - m_scale) <= 1e-9 * (abs(m_scale) + 1e-3)
    return ["%d key frames: %d edges, N = %d" % (n_kf, ne, N),
            "  one linearisation (mode 0, two launches), span between two events on the chain's stream, p50 (p10 / p90) of %d after %d warm-up calls: %.1f (%.1f / %.1f) us"
            % (reps, warm, lin[0], lin[1], lin[2]),
            "  one trial chain (pop, damp, solve, oplus, linearise mode 1), likewise: %.1f (%.1f / %.1f) us" % (tri[0], tri[1], tri[2]),
            "  host form (wait, read-backs, the model's PYTHON linearisation and trial, upload), host wall time, median (min / max) of %d: %.0f (%.0f / %.0f) us"
            "   (numpy's and Python's loops, not the reference's C++)" % (host_reps, np.median(host), min(host), max(host)),
            "  the device's trial total and d_out[0] are the model's to 1e-9: %s" % same]


def main():
    import torch
    from monoorbslam3_amd import _lib
    assert torch.cuda.is_available(), "this tool measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["the IMU initialisation's steps (orbii.h): one trial chain and one linearisation; kernels %s" % _lib.kernels_sha16()]
    for n_kf in (16, 100):
        lines += measure(torch, dev, n_kf)
    lines += resources()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "imu_init_latency.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
