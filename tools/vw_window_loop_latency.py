"""Latency of the WHOLE optimisation of the inertial mapper step, localFullBundleAdjustment's optimize(10) and its classification, on
two windows -- 17 key frames in the window, 2 fixed, 400 points (the sizes of tools/full_inertial_latency.py) and "window 3+2 1025" of
tests/inertial_loop.py -- two ways in one run:
  (a) orbwl_window_optimize_device (include/orbwl.h): the host closes the loop over the staged calls and waits once per trial, so the
      figure is WALL CLOCK around the call, the stream idle before it
  (b) the form before it: tests/inertial_loop.py's DeviceWindow and local_full, PYTHON's loop over the same staged calls with one
      read-back per trial and six torch copies per push / pop; wall clock.  It is Python's time, not g2o's: it shows what the interpreter,
      the read-backs and the copies cost, not what the reference's optimiser costs
p50 (p10 / p90) of 200 runs after 20 warm-up runs ((b): of 20 after 3); the graph, d_iter and the points are set back before every run,
outside the clock.  The trial counts stand beside the times.  There is no pass bar: this is a record.
Writes profiles/vw_window_loop_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def measure(torch, dev, label, sc, iterations, lambda_init, warm=20, reps=200):
    import inertial_loop as il
    from monoorbslam3_amd import imu, vw
    from test_factors_gpu import _Dev
    from test_projection_queries_gpu import _up
    from test_vw_gpu import _Win
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    d = _Dev(torch, dev, sc, sc["graph"], n_priors=1, n_pjobs=1)
    d.priors.copy_(_up(torch, dev, sc["priors"]))
    pjobs = _up(torch, dev, sc["pjobs"])
    w = _Win(torch, dev, sc)
    it = torch.zeros(d.n, dtype=torch.int32, device=dev)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    n_work = vw.window_work_doubles(d.n, w.ns, w.np_, w.ne, d.ne, 1)
    work, trace, summary = f64(n_work), f64(512 * vw.LOOP_TRACE), f64(vw.LOOP_SUMMARY)
    live = [d.Rwb, d.twb, d.v, d.bg, d.ba, w.points]
    start = [t.clone() for t in live]
    opts = vw.WindowLoopOptions.make(sc["cal"]["gravity"], iterations=iterations, lambda_init=lambda_init)
    chain = torch.cuda.Stream(device=dev)
    st = chain.cuda_stream
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
    t_a = []
    for i in range(warm + reps):
        with torch.cuda.stream(chain):
            for s, t in zip(start, live):
                t.copy_(s)
            it.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vw.window_optimize_device(d.graph, it, d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.priors, 1, pjobs, 1, w.cal, w.cam, w.ns, w.np_, w.ne, w.points,
                                  w.edge_state, w.edge_point, w.z, w.w, None, opts, work, w.chi2, w.outlier, trace, 512, summary, d.result, stream=st)
        if i >= warm:
            t_a.append((time.perf_counter() - t0) * 1e6)                # the call has waited for its last kernel
    sm = summary.cpu().numpy()
    t_b, trials_b = [], None
    for i in range(3 + 20):
        be = il.DeviceWindow(torch, dev, sc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rounds = il.local_full(be, iterations=iterations, be_large=lambda_init < 1.0)
        torch.cuda.synchronize()
        if i >= 3:
            t_b.append((time.perf_counter() - t0) * 1e6)
        trials_b = len(rounds[0]["trace"])
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    return ["%s: %d solve states + %d fixed, %d inertial edges, %d points, %d EdgeMono, N = %d; optimize(%d), lambda init %g" % (
                label, w.ns, d.n - w.ns, d.ne, w.np_, w.ne, 15 * w.ns, iterations, lambda_init),
            "  (a) orbwl_window_optimize_device, wall clock around the call, p50 (p10 / p90) of %d:                       %9.1f (%9.1f / %9.1f) us   %d iterations, %d trials (%d accepted), %d outliers"
            % (reps, pct(t_a, 50), pct(t_a, 10), pct(t_a, 90), int(sm[0]), int(sm[1]), int(sm[2]), int(sm[5])),
            "      per trial of (a): %.1f us" % (pct(t_a, 50) / max(int(sm[1]), 1)),
            "  (b) the staged chain closed by Python's loop (tests/inertial_loop.py), wall clock, p50 (p10 / p90) of 20:  %9.1f (%9.1f / %9.1f) us   %d trials (Python's time, not g2o's)"
            % (pct(t_b, 50), pct(t_b, 10), pct(t_b, 90), trials_b)]


def main(out_path):
    import torch
    import inertial_loop as il
    import vw_model as wm
    from monoorbslam3_amd import _lib
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    lines = ["the whole of localFullBundleAdjustment's optimisation (up to 10 iterations of up to 10 trials, then the classification); kernels %s" % _lib.kernels_sha16()]
    lines += measure(torch, dev, "17 key frames, 400 points", wm.window_scene(17, 2, 400), 10, 1e0)
    lines += measure(torch, dev, "window 3+2 1025", il.scene("window 3+2 1025"), 10, 1e0)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vw_window_loop_latency.txt"))
