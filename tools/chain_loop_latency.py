"""Latency of the WHOLE optimisation of localInertialBundleAdjustment (optimize(10) on a chain of key frames with every pose fixed), at 10
and at 20 key frames -- the reference's window without and with beLarge --, two ways in one run:
  (a) orbil_chain_optimize_device (include/orbil.h): one launch; the span between two HIP events on its stream
  (b) the staged chain closed by a HOST loop with one read-back per trial: orbi_linearize_device, orbil_chain_solve_device,
      orbi_graph_oplus_device, orbi_linearize_device in mode 1.  The loop is PYTHON's (tests/inertial_loop.py's DevicePose and optimize, with
      the chain solve in place of the dense one), so the figure is wall clock and is not g2o's time: it shows what the launches, the waits
      and an interpreter cost, not what the reference's optimiser costs
and, for scale, one orbil_chain_solve_device alone.  The scenes are tests/inertial_chain.py's "chain 10" and "chain 20" (ten accepted
iterations each) with one prior job of mask 0, which applies nothing: the staged back-end passes one job to every linearisation.
p50 (and p90) of 100 after 10 warm-up runs ((b): of 10 after 2); the graph is set back before every run, outside the span.  There is no
pass bar: this is a record.  Writes profiles/chain_loop_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import factors_model as fm
    import imu_model as im
    import inertial_chain as ic
    import inertial_loop as il
    from monoorbslam3_amd import _lib, chain, imu
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 10, 100
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    lines = ["the whole of localInertialBundleAdjustment's optimize(10) on a chain of key frames; p50 / p90; kernels %s" % _lib.kernels_sha16()]

    class StagedChain(il.DevicePose):
        """tests/inertial_loop.py's staged back-end with the solve of a chain"""

        def _solve(self, lam):
            d = self.d
            self.lam.fill_(lam)
            chain.chain_solve_device(d.n, d.fixed, d.edges, d.ne, d.cap, d.H_diag, d.H_off, d.b, self.lam, self.band, self.dx, self.out, d.result, stream=self.st)

    for name in ("chain 10", "chain 20"):
        sc = dict(ic.scene(name), pjobs=np.zeros(1, fm.PRIOR_JOB))
        g0 = sc["graph"]
        n, ne, recs, cal = g0.n, len(sc["edges"]), sc["recs"], sc["cal"]
        bank = im.Bank(len(recs), max(len(r.meas) for r in recs))
        bank.recs = recs
        h_bank, _ = bank.pack()
        cap = len(recs)
        d_bank, d_edges, d_fixed, d_priors, d_pjobs = up(h_bank), up(sc["edges"]), up(g0.fixed), up(sc["priors"]), up(sc["pjobs"])
        start = {k: up(getattr(g0, k).reshape(-1)) for k in il.STATE}
        a = {k: f64(s) for k, s in dict(Rwb=9 * n, twb=3 * n, v=3 * n, bg=3 * n, ba=3 * n, info=81 * ne, walk=18 * ne, work=chain.LOOP_WORK,
                                        trace=128 * chain.LOOP_TRACE, summary=chain.SUMMARY).items()}
        g = imu.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], d_fixed, n)
        d_res, d_it = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        opts = chain.ChainOptions.make(cal["gravity"], iterations=ic.ITERATIONS, max_trials=il.MAX_TRIALS, tau=il.TAU)

        def reset():
            for k in il.STATE:
                a[k].copy_(start[k])
            d_it.zero_()

        def one_launch():
            chain.chain_optimize_device(g, d_it, d_bank, cap, d_edges, ne, a["info"], a["walk"], d_priors, 1, d_pjobs, 1, opts, a["work"], a["trace"], 128, a["summary"], d_res)

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

        imu.edge_information_device(d_bank, cap, d_edges, ne, a["info"], a["walk"], d_res)
        t_a = spans(one_launch, reps, warm)
        sm = a["summary"].cpu().numpy()
        # (b): Python's loop over the staged calls; a fresh back-end per run (its uploads outside the clock)
        t_b, trials_b, be = [], None, None
        for i in range(2 + 10):
            be = StagedChain(torch, dev, sc, visual=False)
            be.band = f64(chain.solve_work(n))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = il.optimize(be, ic.ITERATIONS)
            torch.cuda.synchronize()
            if i >= 2:
                t_b.append((time.perf_counter() - t0) * 1e6)
            trials_b = (r["iterations"], len(r["trace"]))
        d = be.d
        d.linearize(sc, 0.0, 0, be.pjobs, 1, 1, None)
        t_s = spans(lambda: be._solve(1.0), reps, warm)
        lines += ["%d key frames (%d unknowns, %d free)" % (n, 15 * n, 9 * (n - 1)),
                  "  (a) orbil_chain_optimize_device, one launch, HIP events:                          %9.1f / %9.1f us   %d iterations, %d trials" % (
                      pct(t_a, 50), pct(t_a, 90), int(sm[0]), int(sm[5])),
                  "  (b) the staged chain closed by Python's loop, a read-back per trial, wall clock: %9.1f / %9.1f us   %d iterations, %d trials (Python's time, not g2o's)" % (
                      pct(t_b, 50), pct(t_b, 90), trials_b[0], trials_b[1]),
                  "  orbil_chain_solve_device alone, HIP events:                                      %9.1f / %9.1f us" % (pct(t_s, 50), pct(t_s, 90))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chain_loop_latency.txt"))
