"""Latency of one Levenberg-Marquardt iteration of poseFullOptimize on the tracker's graph (2 states, 1 inertial edge, 3 priors) with 400
visual edges (include/orbvi.h), both ways in one run, each the span between two HIP events on the chain's stream:
  device form   orbi_linearize_device + orbvi_linearize_device (mode 0) -> orbvi_solve_device -> orbi_graph_oplus_device ->
                orbi_linearize_device + orbvi_linearize_device (mode 1): nothing leaves the stream
  host form     what a caller did before orbvi_solve_device: the same linearisations, then wait, read d_H_diag, d_H_off and d_b back,
                assemble and solve in numpy (tests/vi_model.py's assembly, np.linalg.solve), upload dx, then oplus and the trial's
                errors.  The host figure is numpy's; g2o's dense solve of 18 unknowns is faster than that.
p50 (and p90) of 300 after 30 warm-up iterations; the graph is re-initialised before every iteration, outside the span.  Also the two
new calls alone.  There is no pass bar: the case for the change is the removed wait and copies.
Writes profiles/vi_step_latency.txt (or the path given as the first argument)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import imu_model as im
    import vi_model as vm
    from monoorbslam3_amd import _lib, imu, vi
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps, ne_vis = 30, 300, 400
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    sc = vm.pose_full_scene(ne_vis)
    n, ne, recs, cal, cam = sc["graph"].n, len(sc["edges"]), sc["recs"], sc["cal"], sc["cam"]
    bank = im.Bank(len(recs), max(len(r.meas) for r in recs))
    bank.recs = recs
    h_bank, _ = bank.pack()
    cap = len(recs)
    ccal = imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])
    ccam = vi.Camera.make(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["model"], cam["k"])
    d_bank, d_src, d_init, d_edges, d_fixed = up(h_bank), up(sc["src"]), up(sc["init_jobs"]), up(sc["edges"]), up(sc["graph"].fixed)
    d_priors, d_pjobs = up(sc["priors"]), up(sc["pjobs"])
    a = {k: f64(s) for k, s in dict(Rwb=9 * n, twb=3 * n, v=3 * n, bg=3 * n, ba=3 * n, info=81 * ne, walk=18 * ne, work=imu.EDGE_WORK * ne, err=9 * ne, chi2=3 * ne,
                                    chi2_prior=3, total=2, H_diag=225 * n, H_off=225 * ne, b=15 * n, vwork=vi.EDGE_WORK * ne_vis, verr=2 * ne_vis,
                                    vchi2=ne_vis, vtotal=2, dx=15 * n, out=3).items()}
    g = imu.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], d_fixed, n)
    d_res, d_it = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    d_gs, d_off, d_P, d_z, d_w = up(sc["group_state"]), up(sc["edge_off"]), up(sc["points"].reshape(-1)), up(sc["z"].reshape(-1)), up(sc["w"])
    d_lam = up(np.array([4.0e9]))

    def inertial(mode):
        imu.linearize_device(g, d_bank, cap, cal["gravity"], d_edges, ne, a["info"], a["walk"], a["work"], a["err"], a["chi2"], a["total"], d_res, d_priors, 1,
                             d_pjobs, 1, a["chi2_prior"], 0.0, mode, a["H_diag"], a["H_off"], a["b"])

    def visual(mode):
        vi.linearize_device(g, ccal, ccam, 1, ne_vis, d_gs, d_off, d_P, d_z, d_w, a["verr"], a["vchi2"], d_res, mode=mode, d_total=a["vtotal"],
                            d_H_diag=a["H_diag"], d_b=a["b"], d_work=a["vwork"])

    def solve():
        vi.solve_device(n, d_fixed, d_edges, ne, cap, a["H_diag"], a["H_off"], a["b"], d_lam, a["dx"], a["out"], d_res)

    def trial():
        imu.graph_oplus_device(g, a["dx"], d_it, d_res)
        inertial(1)
        visual(1)

    def device_form():
        inertial(0)
        visual(0)
        solve()
        trial()

    def host_form():
        inertial(0)
        visual(0)
        torch.cuda.synchronize()                                       # the wait
        H, Ho, b = a["H_diag"].cpu().numpy(), a["H_off"].cpu().numpy(), a["b"].cpu().numpy()   # 2 x 225 + 225 + 30 doubles back
        A, rhs, _, _, _ = vm.assemble(sc["graph"].fixed, sc["edges"], cap, H, Ho, b, 4.0e9)
        a["dx"].copy_(torch.from_numpy(np.linalg.solve(A, rhs)))       # 30 doubles up
        trial()

    def spans(fn, count, warm_up):
        out = []
        for i in range(warm_up + count):
            imu.graph_init_device(g, d_bank, cap, d_src, n, d_init, n, d_res)
            d_it.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warm_up:
                out.append(e0.elapsed_time(e1) * 1e3)
        return out

    imu.graph_init_device(g, d_bank, cap, d_src, n, d_init, n, d_res)
    imu.edge_information_device(d_bank, cap, d_edges, ne, a["info"], a["walk"], d_res)
    dev_t, host_t = spans(device_form, reps, warm), spans(host_form, reps, warm)
    inertial(0)
    lin_t, sol_t = spans(lambda: visual(0), reps, warm), spans(solve, reps, warm)
    imu.graph_init_device(g, d_bank, cap, d_src, n, d_init, n, d_res)
    d_it.zero_()
    device_form()
    totals = (a["total"].cpu().numpy()[1], a["vtotal"].cpu().numpy()[1], a["out"].cpu().numpy().tolist())
    lines = ["one Levenberg-Marquardt iteration of poseFullOptimize: the tracker's graph (2 states, 1 inertial edge, 3 priors) and %d visual edges; spans between two "
             "HIP events on the chain's stream, p50 / p90 of %d after %d warm-up iterations; kernels %s" % (ne_vis, reps, warm, _lib.kernels_sha16()),
             "  device form (linearise x 2, orbvi_solve_device, oplus, errors at the trial x 2; 8 launches, no wait):   %.1f / %.1f us" % (pct(dev_t, 50), pct(dev_t, 90)),
             "  host form (the same with wait, read-back of H and b, numpy assembly and solve, upload of dx):           %.1f / %.1f us   (numpy's figure, not g2o's)" % (
                 pct(host_t, 50), pct(host_t, 90)),
             "  orbvi_linearize_device (mode 0, %d edges, one 1024-thread workgroup) alone:                            %.1f / %.1f us" % (ne_vis, pct(lin_t, 50), pct(lin_t, 90)),
             "  orbvi_solve_device (18 free of 30 unknowns) alone:                                                       %.1f / %.1f us" % (pct(sol_t, 50), pct(sol_t, 90)),
             "  one more device iteration from the initial estimate, at the trial point: inertial robust total %.6g, visual robust total %.6g, d_out %s, d_result %s" % (totals + (d_res.cpu().numpy().tolist(),))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vi_step_latency.txt"))
