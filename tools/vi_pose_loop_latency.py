"""Latency of the WHOLE per-frame optimisation of the inertial phase, poseFullOptimize on the tracker's graph (2 states, 1 inertial edge, 3
priors), at 200 and at 2000 visual edges, three ways in one run:
  (a) orbvi_pose_optimize_device (include/orbvi_loop.h): one launch; the span between two HIP events on its stream
  (b) the form before it: the staged chain of include/orbvi.h closed by a HOST loop with one read-back per trial -- the loop is PYTHON's
      (tests/inertial_loop.py's DevicePose and pose_full), so the figure is wall clock and is not g2o's time: it shows what the launches,
      the waits and an interpreter cost, not what the reference's optimiser costs
  (c) for scale, orbba_pose_optimize_batch_device (the visual-only poseOptimize, one launch) on the same visual edges from the same pose
p50 (and p90) of 200 after 20 warm-up runs ((b): of 20 after 3, it takes tens of milliseconds); the graph and d_active are set back before
every run, outside the span.  The trial counts stand beside the times.  There is no pass bar: this is a record.
Writes profiles/vi_pose_loop_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import imu_model as im
    import inertial_loop as il
    import vi_model as vm
    from monoorbslam3_amd import _lib, ba, imu, vi
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 20, 200
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    lines = ["the whole of poseFullOptimize (4 rounds of up to 10 iterations of up to 10 trials) on the tracker's graph; p50 / p90; kernels %s" % _lib.kernels_sha16()]
    for ne_vis in (200, 2000):
        sc = vm.pose_full_scene(ne_vis, sample_counts=il.LOOP_WINDOW["sample_counts"])
        n, ne, recs, cal, cam = sc["graph"].n, len(sc["edges"]), sc["recs"], sc["cal"], sc["cam"]
        bank = im.Bank(len(recs), max(len(r.meas) for r in recs))
        bank.recs = recs
        h_bank, _ = bank.pack()
        cap = len(recs)
        ccal = imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])
        ccam = vi.Camera.make(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["model"], cam["k"])
        d_bank, d_src, d_init, d_edges, d_fixed = up(h_bank), up(sc["src"]), up(sc["init_jobs"]), up(sc["edges"]), up(sc["graph"].fixed)
        d_priors, d_pjobs = up(sc["priors"]), up(sc["pjobs"])
        a = {k: f64(s) for k, s in dict(Rwb=9 * n, twb=3 * n, v=3 * n, bg=3 * n, ba=3 * n, info=81 * ne, walk=18 * ne, chi2=ne_vis,
                                        work=ne_vis * vi.LOOP_EDGE_WORK + vi.LOOP_FIXED_WORK, trace=512 * vi.LOOP_TRACE, summary=vi.LOOP_SUMMARY).items()}
        g = imu.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], d_fixed, n)
        d_res, d_it, d_nin = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        d_active = torch.ones(ne_vis, dtype=torch.uint8, device=dev)
        d_gs, d_off, d_P, d_z, d_w = up(sc["group_state"]), up(sc["edge_off"]), up(sc["points"].reshape(-1)), up(sc["z"].reshape(-1)), up(sc["w"])
        opts = vi.LoopOptions.make(cal["gravity"])

        def reset():
            imu.graph_init_device(g, d_bank, cap, d_src, n, d_init, n, d_res)
            d_it.zero_()
            d_active.fill_(1)

        def one_launch():
            vi.pose_optimize_device(g, d_it, d_bank, cap, d_edges, ne, a["info"], a["walk"], d_priors, 1, d_pjobs, 1, ccal, ccam, ne_vis, d_gs, d_off, d_P, d_z, d_w,
                                    d_active, opts, a["work"], a["chi2"], d_nin, a["trace"], 512, a["summary"], d_res)

        # (c): the frame's T_cw as the visual-only optimiser takes it
        gr = sc["graph"]
        s = int(sc["group_state"][0])
        Rcb, tcb = np.asarray(cal["Rcb"], np.float64).reshape(3, 3), np.asarray(cal["tcb"], np.float64)
        Rcw = Rcb @ gr.Rwb[s].T
        d_R, d_t = up(Rcw.reshape(-1)), up(tcb - Rcw @ gr.twb[s])
        d_Ro, d_to, d_inl, d_c2 = f64(9), f64(3), torch.zeros(ne_vis, dtype=torch.uint8, device=dev), f64(ne_vis)

        def visual_only():
            ba.pose_optimize_batch_device((cam["fx"], cam["fy"], cam["cx"], cam["cy"]), d_R, d_t, d_off, d_P, d_z, d_w, d_Ro, d_to, d_inl, d_nin, d_c2)

        def spans(fn, count, warm_up):
            out = []
            for i in range(warm_up + count):
                reset()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= warm_up:
                    out.append(e0.elapsed_time(e1) * 1e3)
            return out

        reset()
        imu.edge_information_device(d_bank, cap, d_edges, ne, a["info"], a["walk"], d_res)
        t_a = spans(one_launch, reps, warm)
        sm = a["summary"].cpu().numpy()
        trials_a = [int(sm[6 * k + 1]) for k in range(4)]
        t_c = spans(visual_only, reps, warm)
        # (b): Python's loop over the staged calls; a fresh back-end per run (its uploads outside the clock)
        t_b, trials_b = [], None
        for i in range(3 + 20):
            be = il.DevicePose(torch, dev, sc, visual=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rounds = il.pose_full(be)
            torch.cuda.synchronize()
            if i >= 3:
                t_b.append((time.perf_counter() - t0) * 1e6)
            trials_b = [len(r["trace"]) for r in rounds]
        lines += ["%d visual edges" % ne_vis,
                  "  (a) orbvi_pose_optimize_device, one launch, HIP events:                         %9.1f / %9.1f us   trials per round %s, inliers %d" % (
                      pct(t_a, 50), pct(t_a, 90), trials_a, int(sm[23])),
                  "  (b) the staged chain closed by Python's loop, a read-back per trial, wall clock: %9.1f / %9.1f us   trials per round %s (Python's time, not g2o's)" % (
                      pct(t_b, 50), pct(t_b, 90), trials_b),
                  "  (c) orbba_pose_optimize_batch_device, visual edges only, one launch, HIP events:  %9.1f / %9.1f us   inliers %d" % (
                      pct(t_c, 50), pct(t_c, 90), int(d_nin.cpu().numpy()[0]))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vi_pose_loop_latency.txt"))
