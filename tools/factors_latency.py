"""Latency of one linearisation of the inertial factors (include/orbi.h, "Inertial factors linearised on the device"), both ways in
one run, for the tracker's graph (2 states, 1 edge, 3 priors: poseFullOptimize's inertial part) and for a 25-state chain with walks
(a local window):
  device form   orbi_graph_init_device + orbi_edge_information_device + orbi_linearize_device (mode 0) + orbi_graph_recover_device,
                the span between two HIP events on an idle stream
  host form     what a caller did before: wait, read the 1232-byte records and the states back, the host loop of
                tests/factors_model.py (the reference's g2o is faster: this is numpy's figure, not g2o's); host wall time
p50 (and p90) of 200 after 30 warm-up calls (the host form: of 20 after 3).  There is no pass bar: the case for the change is the removed wait and read-back.
Writes profiles/factors_latency.txt (or the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def records_from_bank(im, hb):
    """imu_model records from the bytes of a bank"""
    out = []
    for k in range(len(hb)):
        r = im.Rec(np.float32)
        for f in im.FIELDS:
            v = hb[f][k]
            setattr(r, f, v.reshape(3, 3).copy() if f in im.MATS else v.reshape(15, 15).copy() if f == "C" else v.copy())
        out.append(r)
    return out


def main(out_path):
    import torch
    import factors_model as fm
    import imu_model as im
    from monoorbslam3_amd import _lib, imu
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 30, 200
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    lines = ["one linearisation of the inertial factors: init + edge information + linearise (mode 0) + recover, 5 launches (6 where the edges span several workgroups); p50 / p90 of %d after "
             "%d warm-up calls; kernels %s" % (reps, warm, _lib.kernels_sha16())]
    for name, sc in (("tracker's graph (2 states, 1 edge, 3 priors)", fm.make_tracker_graph()), ("25-state chain with walks (24 edges)", fm.make_chain(24))):
        n, ne, recs, cal = sc["graph"].n, len(sc["edges"]), sc["recs"], sc["cal"]
        if "priors" not in sc:
            sc["priors"], _, _ = fm.make_priors(sc, [0])
            sc["pjobs"] = np.array([(0, 0, 7)], fm.PRIOR_JOB)
        bank = im.Bank(len(recs), max(len(r.meas) for r in recs))
        bank.recs = recs
        h_bank, _ = bank.pack()
        ccal = imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])
        d_bank, d_src, d_init, d_edges, d_fixed = up(h_bank), up(sc["src"]), up(sc["init_jobs"]), up(sc["edges"]), up(sc["graph"].fixed)
        d_priors, d_pjobs = up(sc["priors"]), up(sc["pjobs"])
        arrays = {k: f64(s) for k, s in dict(Rwb=9 * n, twb=3 * n, v=3 * n, bg=3 * n, ba=3 * n, info=81 * ne, walk=18 * ne, work=imu.EDGE_WORK * ne, err=9 * ne,
                                              chi2=3 * ne, chi2_prior=3 * len(sc["pjobs"]), total=2, H_diag=225 * n, H_off=225 * ne, b=15 * n).items()}
        g = imu.Graph.make(arrays["Rwb"], arrays["twb"], arrays["v"], arrays["bg"], arrays["ba"], d_fixed, n)
        d_res = torch.zeros(8, dtype=torch.int32, device=dev)
        rjobs = up(np.array([(s, s, 0) for s in range(n)], np.int32))
        d_dst, d_bias = torch.zeros(15 * n, device=dev), torch.zeros(6 * n, device=dev)

        def chain():
            imu.graph_init_device(g, d_bank, len(recs), d_src, n, d_init, n, d_res)
            imu.edge_information_device(d_bank, len(recs), d_edges, ne, arrays["info"], arrays["walk"], d_res)
            imu.linearize_device(g, d_bank, len(recs), cal["gravity"], d_edges, ne, arrays["info"], arrays["walk"], arrays["work"], arrays["err"], arrays["chi2"],
                                 arrays["total"], d_res, d_priors, len(sc["priors"]), d_pjobs, len(sc["pjobs"]), arrays["chi2_prior"], fm.HUBER_DELTA, 0,
                                 arrays["H_diag"], arrays["H_off"], arrays["b"])
            imu.graph_recover_device(g, ccal, rjobs, n, d_dst, n, d_bias, d_res)

        def device_idle():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            chain()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        def host_form():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.cuda.synchronize()                                   # the wait the chain has to make
            hb = np.frombuffer(d_bank.cpu().numpy().tobytes(), im.RECORD)          # the records, read back
            src = d_src.cpu().numpy().reshape(n, 15)                   # and the states
            host_recs = records_from_bank(im, hb)
            hg = fm.Graph(n)
            hg.fixed[:] = sc["graph"].fixed
            fm.graph_init(hg, host_recs, src, sc["init_jobs"])
            info, walk, _ = fm.edge_information(host_recs, sc["edges"])
            fm.linearize(hg, host_recs, cal["gravity"], sc["edges"], info, walk, sc["priors"], sc["pjobs"], fm.HUBER_DELTA)
            fm.recover(hg, cal, np.array([(s, s, 0) for s in range(n)]), src.copy(), False)
            return (time.perf_counter() - t0) * 1e6

        idle, host = [], []
        for i in range(warm + reps):
            a = device_idle()
            if i >= warm:
                idle.append(a)
        for i in range(3 + 20):
            b = host_form()
            if i >= 3:
                host.append(b)
        total = arrays["total"].cpu().numpy()
        lines += ["%s" % name,
                  "  device form, span between two HIP events, idle stream:                           %.1f / %.1f us   d_result %s  total chi2 %.6g" % (
                      pct(idle, 50), pct(idle, 90), d_res.cpu().numpy().tolist(), total[0]),
                  "  host form (wait, read-back, numpy loop of tests/factors_model.py), host wall time, p50 / p90 of 20: %.1f / %.1f us   "
                  "(numpy's figure, not g2o's)" % (pct(host, 50), pct(host, 90))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "factors_latency.txt"))
