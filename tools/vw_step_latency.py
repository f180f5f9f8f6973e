"""Latency of one Levenberg-Marquardt iteration of localFullBundleAdjustment on a window of 10 and of 25 solve states (tests/vw_model.py's
window_scene: a chain with walks, three priors, 8 fixed key frames, 2000 map points seen by 1 to 6 states each) with include/orbvw.h,
both ways in one run, each the span between two HIP events on the chain's stream:
  device form   orbi_linearize_device + orbvw_linearize_device (mode 0) -> orbvw_reduce_device -> orbvw_solve_device ->
                orbvw_backsub_device -> orbi_graph_oplus_device -> orbi_linearize_device + orbvw_linearize_device (mode 1) on the trial
                points: nothing leaves the stream
  host form     what a caller did before this header: the inertial linearisation on the device, then wait, read d_H_diag, d_H_off and
                d_b back, and with the visual edges held on the host (tests/vw_model.py's linearize, then a plain numpy Schur
                complement over a dense H_pl, np.linalg.solve and the back-substitution) upload dx, then oplus and the inertial
                errors at the trial point; the visual errors at the trial point are left out of the host's span.  The host figure
                is numpy's, not g2o's.
p50 (and p90) of 200 after 20 warm-up iterations; the graph is re-initialised before every iteration, outside the span.  Also the four
new calls alone.  There is no pass bar: the case for the change is the removed wait, the copies and the host's Schur complement.
Writes profiles/vw_step_latency.txt (or the path given as the first argument)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def measure(n_solve, warm, reps, host_reps):
    import torch
    import imu_model as im
    import vi_model as vm
    import vw_model as wm
    from monoorbslam3_amd import imu, vi, vw
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy() if a.dtype.fields else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    pct = lambda v, k: float(np.percentile(v, k))  # noqa: E731
    sc = wm.window_scene(n_solve, 8, 2000, 2, 0)
    g0, recs, cal, cam = sc["graph"], sc["recs"], sc["cal"], sc["cam"]
    n, ne, npt, nv, N = g0.n, len(sc["edges"]), sc["n_points"], len(sc["w"]), 15 * n_solve
    bank = im.Bank(len(recs), max(len(r.meas) for r in recs))
    bank.recs = recs
    h_bank, _ = bank.pack()
    cap = len(recs)
    ccal = imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])
    ccam = vi.Camera.make(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["model"], cam["k"])
    d_bank, d_src, d_init, d_edges, d_fixed = up(h_bank), up(sc["src"]), up(sc["init_jobs"]), up(sc["edges"]), up(g0.fixed)
    d_priors, d_pjobs = up(sc["priors"]), up(sc["pjobs"])
    a = {k: f64(s) for k, s in dict(info=81 * ne, walk=18 * ne, work=imu.EDGE_WORK * ne, err=9 * ne, chi2=3 * ne, chi2_prior=3, total=2, H_diag=225 * n, H_off=225 * ne,
                                    b=15 * n, vwork=vw.EDGE_WORK * nv, verr=2 * nv, vchi2=nv, vtotal=2, Hll=9 * npt, bl=3 * npt, Hlp=18 * nv, S=N * N, rhs=N,
                                    inv=9 * npt, tl=3 * npt, out=3, dx=15 * n, xl=3 * npt, trial=3 * npt, out_points=1).items()}
    a.update(Rwb=up(g0.Rwb.reshape(-1)), twb=up(g0.twb.reshape(-1)), v=up(g0.v.reshape(-1)), bg=up(g0.bg.reshape(-1)), ba=up(g0.ba.reshape(-1)))
    g = imu.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], d_fixed, n)
    d_res, d_it, d_off = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(npt + 1, dtype=torch.int32, device=dev)
    d_P, d_es, d_ep, d_z, d_w = up(sc["points"].reshape(-1)), up(sc["edge_state"]), up(sc["edge_point"]), up(sc["z"].reshape(-1)), up(sc["w"])
    lam = 1.0
    d_lam = up(np.array([lam]))

    def inertial(mode):
        imu.linearize_device(g, d_bank, cap, cal["gravity"], d_edges, ne, a["info"], a["walk"], a["work"], a["err"], a["chi2"], a["total"], d_res, d_priors, 1,
                             d_pjobs, 1, a["chi2_prior"], 0.0, mode, a["H_diag"], a["H_off"], a["b"])

    def visual(mode, points=d_P):
        z = mode != 0
        vw.linearize_device(g, ccal, ccam, n_solve, npt, nv, points, d_es, d_ep, d_z, d_w, d_off, a["verr"], a["vchi2"], d_res, mode=mode, d_total=a["vtotal"],
                            d_work=None if z else a["vwork"], d_H_diag=None if z else a["H_diag"], d_b=None if z else a["b"], d_Hll=None if z else a["Hll"],
                            d_bl=None if z else a["bl"], d_Hlp=None if z else a["Hlp"])

    def reduce():
        vw.reduce_device(n_solve, d_fixed, d_edges, ne, cap, a["H_diag"], a["H_off"], a["b"], d_lam, npt, nv, d_off, d_es, a["Hll"], a["bl"], a["Hlp"], a["S"], a["rhs"],
                         a["inv"], a["tl"], a["out"], d_res)

    def solve():
        vw.solve_device(n_solve, a["S"], a["rhs"], a["b"], d_lam, a["dx"], a["out"], d_res)

    def backsub():
        vw.backsub_device(n_solve, npt, nv, d_off, d_es, a["Hlp"], a["inv"], a["bl"], a["dx"], d_lam, d_P, a["xl"], a["trial"], a["out_points"], d_res)

    def device_form():
        inertial(0), visual(0), reduce(), solve(), backsub()
        imu.graph_oplus_device(g, a["dx"], d_it, d_res)
        inertial(1), visual(1, a["trial"])

    ep, es = sc["edge_point"].astype(np.int64), sc["edge_state"].astype(np.int64)
    on = es < n_solve

    def host_form():
        inertial(0)
        torch.cuda.synchronize()                                       # the wait
        H, Ho, b = a["H_diag"].cpu().numpy(), a["H_off"].cpu().numpy(), a["b"].cpu().numpy()
        gm = g0.copy()
        gm.Rwb, gm.twb = a["Rwb"].cpu().numpy().reshape(n, 3, 3), a["twb"].cpu().numpy().reshape(n, 3)
        ov = wm.linearize(gm, cal, cam, n_solve, sc["points"], sc["edge_state"], sc["edge_point"], sc["z"], sc["w"], mode=0, H_diag=H, b=b)
        A, rhs, _, _, _ = vm.assemble(g0.fixed[:n_solve], sc["edges"], cap, ov["H_diag"][:n_solve], Ho, ov["b"][:n_solve], lam)
        inv = np.linalg.inv(ov["Hll"].reshape(npt, 3, 3) + lam * np.eye(3))
        E = np.zeros((n_solve, 6, npt, 3))                              # H_pl, dense: a window's is small
        E[es[on], :, ep[on], :] = ov["Hlp"].reshape(nv, 3, 6)[on].transpose(0, 2, 1)
        E = E.reshape(6 * n_solve, 3 * npt)
        EI = np.einsum("plk,lkj->plj", E.reshape(-1, npt, 3), inv).reshape(6 * n_solve, 3 * npt)
        pose = (np.arange(N) % 15) < 6
        A[np.ix_(pose, pose)] -= EI @ E.T
        rhs[pose] -= EI @ ov["bl"].reshape(-1)
        dx = np.zeros((n, 15))
        dx[:n_solve] = np.linalg.solve(A, rhs).reshape(n_solve, 15)
        xl = np.einsum("lkj,lj->lk", inv, ov["bl"] - (E.T @ dx[:n_solve, :6].reshape(-1)).reshape(npt, 3))
        a["dx"].copy_(torch.from_numpy(dx.reshape(-1)))                 # 15 n doubles up; the trial points stay on the host
        imu.graph_oplus_device(g, a["dx"], d_it, d_res)
        inertial(1)
        return xl

    def spans(fn, count, warm_up, prepare=None):
        out = []
        for i in range(warm_up + count):
            imu.graph_init_device(g, d_bank, cap, d_src, n_solve, d_init, n_solve, d_res)
            d_it.zero_()
            if prepare:
                prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warm_up:
                out.append(e0.elapsed_time(e1) * 1e3)
        return out

    imu.graph_init_device(g, d_bank, cap, d_src, n_solve, d_init, n_solve, d_res)
    imu.edge_information_device(d_bank, cap, d_edges, ne, a["info"], a["walk"], d_res)
    dev_t, host_t = spans(device_form, reps, warm), spans(host_form, host_reps, 2)
    lin_t = spans(lambda: visual(0), reps, warm, lambda: inertial(0))
    red_t = spans(reduce, reps, warm, lambda: (inertial(0), visual(0)))
    sol_t = spans(solve, reps, warm, lambda: (inertial(0), visual(0), reduce()))
    bck_t = spans(backsub, reps, warm, lambda: (inertial(0), visual(0), reduce(), solve()))
    imu.graph_init_device(g, d_bank, cap, d_src, n_solve, d_init, n_solve, d_res)
    d_it.zero_()
    inertial(0), visual(0)
    before = (a["total"].cpu().numpy()[1], a["vtotal"].cpu().numpy()[1])
    reduce(), solve(), backsub()
    imu.graph_oplus_device(g, a["dx"], d_it, d_res)
    inertial(1), visual(1, a["trial"])
    after = (a["total"].cpu().numpy()[1], a["vtotal"].cpu().numpy()[1])
    return ["  %d solve states + 8 fixed, %d points, %d EdgeMono, %d unknowns in the reduced system (p50 / p90 of %d after %d warm-up iterations):" % (n_solve, npt, nv, N, reps, warm),
            "    device form (linearise x 2, reduce, solve, backsub, oplus, errors at the trial x 2; 22 launches, no wait):   %.1f / %.1f us" % (pct(dev_t, 50), pct(dev_t, 90)),
            "    host form (wait, read-back of H and b, numpy EdgeMono, Schur complement, solve and backsub, upload of dx; %d runs): %.1f / %.1f us   (numpy's figure, not g2o's)" % (
                host_reps, pct(host_t, 50), pct(host_t, 90)),
            "    orbvw_linearize_device (mode 0) alone: %.1f / %.1f us;  orbvw_reduce_device: %.1f / %.1f us;  orbvw_solve_device: %.1f / %.1f us;  orbvw_backsub_device: %.1f / %.1f us" % (
                pct(lin_t, 50), pct(lin_t, 90), pct(red_t, 50), pct(red_t, 90), pct(sol_t, 50), pct(sol_t, 90), pct(bck_t, 50), pct(bck_t, 90)),
            "    one device iteration at lambda 1: robust totals (inertial, visual) %.6g, %.6g -> %.6g, %.6g; d_out %s, d_out_points %.6g" % (
                before + after + (a["out"].cpu().numpy().tolist(), float(a["out_points"].cpu().numpy()[0])))]


def main(out_path):
    import torch
    from monoorbslam3_amd import _lib
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["one Levenberg-Marquardt iteration of localFullBundleAdjustment with include/orbvw.h; spans between two HIP events on the chain's stream; kernels %s" % _lib.kernels_sha16()]
    for n_solve in (10, 25):
        lines += measure(n_solve, 20, 200, 200)
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vw_step_latency.txt"))
