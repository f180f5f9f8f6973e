"""orbwl_window_optimize_device on the MI355X: localFullBundleAdjustment's Levenberg-Marquardt loop closed by the library (include/orbwl.h),
on the window scenes of inertial_loop.SCENES, built with the helpers inertial_loop.DeviceWindow uses, every buffer between guard elements.
  1  against the model loop (inertial_loop.model_run), through test_inertial_loop_gpu._compare: the bars are that file's and are not restated
  2  against the staged chain closed by the host (inertial_loop.device_backend): the first trial bit for bit, the decisions
  3  a run that ends on a rejected trial holds the bytes of the run cut just before that iteration
  4  the refused solve: lambda forced to 0 on a window whose velocities and biases have no block
  5  the stop flag
  6  two runs, a NULL stream, a trace shorter than the run
  7  the mapper step on a device-resident map: assembly -> the call on the ASSEMBLED arrays -> recover -> apply -> the priors"""
import ctypes as C
import time

import numpy as np
import pytest

import inertial_loop as il
from test_factors_gpu import _Dev, _calib
from test_inertial_loop_gpu import _compare, _device_run
from test_projection_queries_gpu import _up
from test_vi_gpu import _camera
from test_vw_gpu import _Win

pytestmark = pytest.mark.gpu

NAN = float("nan")
WINDOW_SCENES = [n for n, s in il.SCENES.items() if s[0] == "local_full"]
REJECTING = "window 4+3 65 large"
CAP_TRACE = 320                                          # 25 iterations x 10 trials fit, with room
STATE_KEYS = ("Rwb", "twb", "v", "bg", "ba", "it", "points")
_cache = {}


def _bare(sc):
    """the scene without its inertial edges and prior jobs: velocity and biases have no block, so the system is singular at lambda 0"""
    bare = {k: v for k, v in sc.items() if k not in ("info", "walk")}
    bare["edges"], bare["pjobs"] = sc["edges"][:0], sc["pjobs"][:0]
    return bare


class _Loop:
    """the device memory of one orbwl_window_optimize_device call on a window scene, padded, and the call"""

    def __init__(self, torch, dev, name, cap_trace=CAP_TRACE, bare=False):
        from monoorbslam3_amd import vw
        self.torch, self.dev, self.vw, self.name = torch, dev, vw, name
        _, _, kw = il.SCENES[name]
        sc = self.sc = il.scene(name)
        self.iterations, self.lambda_init = kw["iterations"], 1e-2 if kw.get("be_large") else 1e0
        d = self.d = _Dev(torch, dev, sc, sc["graph"], n_priors=1, n_pjobs=1)
        d.priors.copy_(_up(torch, dev, sc["priors"]))
        d.it = d._pad("it", np.zeros(d.n, np.int32), -3)
        self.pjobs = _up(torch, dev, sc["pjobs"])
        self.n_iedges, self.n_pjobs = (0, 0) if bare else (d.ne, 1)
        w = self.w = _Win(torch, dev, sc)
        self.cap_trace = cap_trace
        self.n_work = vw.window_work_doubles(d.n, w.ns, w.np_, w.ne, self.n_iedges, self.n_pjobs)
        assert self.n_work > 0
        self.work = d._pad("loop work", np.full(self.n_work, NAN), -1.5)
        self.trace = d._pad("trace", np.full(max(cap_trace, 1) * vw.LOOP_TRACE, NAN), -1.5)
        self.summary = d._pad("summary", np.full(vw.LOOP_SUMMARY, NAN), -1.5)

    def call(self, stream=None, iterations=None, max_trials=il.MAX_TRIALS, lambda_init=None, stop=None):
        d, w, vw = self.d, self.w, self.vw
        o = vw.WindowLoopOptions.make(self.sc["cal"]["gravity"], iterations=iterations or self.iterations, lambda_init=lambda_init or self.lambda_init,
                                      max_trials=max_trials)
        vw.window_optimize_device(d.graph, d.it, d.bank, d.cap, d.edges, self.n_iedges, d.info, d.walk, d.priors, 1, self.pjobs, self.n_pjobs, w.cal, w.cam,
                                  w.ns, w.np_, w.ne, w.points, w.edge_state, w.edge_point, w.z, w.w, None, o, self.work, w.chi2, w.outlier,
                                  self.trace if self.cap_trace else None, self.cap_trace, self.summary, d.result, stop=stop, stream=stream)

    def finish(self):
        self.d.finish()
        self.w.finish()

    def raw(self):
        """every output as bytes-comparable arrays"""
        d, w = self.d, self.w
        return dict(trace=self.trace.cpu().numpy().copy(), summary=self.summary.cpu().numpy().copy(), result=d.res(), Rwb=d.get("Rwb").copy(),
                    twb=d.get("twb").copy(), v=d.get("v").copy(), bg=d.get("bg").copy(), ba=d.get("ba").copy(), it=d.it.cpu().numpy().copy(),
                    points=w.get("points"), chi2=w.get("chi2")[:w.ne], outlier=w.get("outlier")[:w.ne])


def _rows(trace, n):
    t = trace.reshape(-1, 13)[:n]
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]), bool(r[7]), float(r[8]), float(r[9]), float(r[10]),
             float(r[11]), bool(r[12])) for r in t]


def _form(lp, raw, seconds=0.0):
    """a call's outputs in the form inertial_loop.run gives (rounds, estimate, refused)"""
    sm, n, cap = raw["summary"], lp.d.n, lp.cap_trace
    total = int(sm[1])
    rows = _rows(raw["trace"], min(total, cap))
    assert int(sm[6]) == max(total - cap, 0), sm
    r = dict(iterations=int(sm[0]), lam=float(sm[4]), trace=rows, accepted=int(sm[2]), refused=int(sm[3]),
             classification=dict(outlier=raw["outlier"], n_outliers=int(sm[5]), chi2=raw["chi2"]))
    if cap >= total:
        assert r["accepted"] == sum(t[-1] for t in rows) and r["refused"] == sum(not t[7] for t in rows), sm
    res = raw["result"]
    assert res[0] == r["accepted"] and res[2] == total - r["accepted"] and res[3] == r["refused"] and res[5] == r["classification"]["n_outliers"], (res, sm)
    est = dict(Rwb=raw["Rwb"].reshape(n, 3, 3), twb=raw["twb"].reshape(n, 3), v=raw["v"].reshape(n, 3), bg=raw["bg"].reshape(n, 3), ba=raw["ba"].reshape(n, 3),
               iter=raw["it"], points=raw["points"].reshape(-1, 3))
    return dict(rounds=[r], estimate=est, refused=r["refused"], n_trials=total, seconds=seconds, dx_zero=[], raw=raw)


def _run(name, stream_kind="explicit", cap_trace=CAP_TRACE, cached=True, bare=False, **call):
    """one optimisation behind orbi_edge_information_device, every guard checked"""
    import torch
    key = (name, stream_kind, cap_trace, bare, tuple(sorted((k, v.value if k == "stop" else v) for k, v in call.items())))
    if key in _cache and cached:
        return _cache[key]
    dev = torch.device("cuda", 0)
    lp = _Loop(torch, dev, name, cap_trace, bare)
    st = il._chain_stream(torch, dev, stream_kind)
    d = lp.d
    d.imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
    t0 = time.perf_counter()
    lp.call(st, **call)
    seconds = time.perf_counter() - t0
    lp.finish()
    out = _form(lp, lp.raw(), seconds)
    _cache[key] = out
    return out


def _same_bytes(a, b, skip=()):
    for k in a["raw"]:
        if k not in skip:
            assert a["raw"][k].tobytes() == b["raw"][k].tobytes(), k


def _start_bytes(name):
    sc = il.scene(name)
    g = sc["graph"]
    return dict({k: np.ascontiguousarray(getattr(g, k)).reshape(-1).tobytes() for k in il.STATE}, it=np.zeros(g.n, np.int32).tobytes(),
                points=np.ascontiguousarray(sc["points"]).reshape(-1).tobytes())


def _untouched(name, run):
    want = _start_bytes(name)
    for k in STATE_KEYS:
        assert run["raw"][k].tobytes() == want[k], (k, "moved")


def _fixed_kept(name, run):
    """fixed vertices and the states >= n_solve hold the bytes of the scene"""
    import factors_model as fm
    sc = il.scene(name)
    g, ns = sc["graph"], sc["n_solve"]
    for k, bit, width in zip(il.STATE, (fm.FIX_POSE, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC), (9, 3, 3, 3, 3)):
        keep = ((g.fixed & bit) != 0) | (np.arange(g.n) >= ns)
        got, want = run["raw"][k].reshape(g.n, width), np.ascontiguousarray(getattr(g, k)).reshape(g.n, width)
        assert got[keep].tobytes() == want[keep].tobytes(), (name, k)
    assert not run["raw"]["it"][ns:].any()


# ---- 1
@pytest.mark.parametrize("name", WINDOW_SCENES)
def test_the_library_loop_is_the_models(name):
    """decisions, iteration counts and refused flags equal (up to flat_from() on the converged scene); every trial's lambda, totals and
    scales, the estimate, the classification away from the threshold, d_iter and the fixed vertices as test_inertial_loop_gpu._compare
    holds the staged device loop"""
    dev = _run(name)
    _compare(name, dev)
    _fixed_kept(name, dev)
    res, sm = dev["raw"]["result"], dev["raw"]["summary"]
    assert res[1] == 0 and res[4] == 0 and res[6] == 0 and res[7] == 0 and sm[7] == 0, (res, sm)


# ---- 2
@pytest.mark.parametrize("name", WINDOW_SCENES)
def test_the_first_trial_has_the_bytes_of_the_staged_chain(name):
    """trial 0 of iteration 0 has no policy arithmetic ahead of it: lambda, current, temp, scale and both totals are the staged calls'
    bytes; the decisions of the whole run are the staged loop's (up to flat_from() on the converged scene)"""
    one, staged = _run(name), _device_run(name)
    a, b = one["rounds"][0]["trace"][0], staged["rounds"][0]["trace"][0]
    for key in ("lam", "current", "temp", "scale", "total_inertial", "total_visual", "scale_pose", "scale_points"):
        i = il.FIELDS.index(key)
        assert np.float64(a[i]).tobytes() == np.float64(b[i]).tobytes(), (name, key, a[i], b[i])
    x, y = one["rounds"][0], staged["rounds"][0]
    flat = il.flat_from(y["trace"]) if name in il.CONVERGED else len(y["trace"])
    dx, dy = il.decisions([x])[0], il.decisions([y])[0]
    assert dx[:flat] == dy[:flat], (name, dx, dy)
    if name not in il.CONVERGED:
        assert dx == dy and x["iterations"] == y["iterations"], name


# ---- 3
def test_a_run_that_ends_on_a_rejected_trial_holds_the_bytes_before_that_iteration():
    """the first iteration with a rejection: m rejected trials, then an accepted one.  With max_trials = m the optimisation ends there,
    through qmax == max_trials, on a rejected trial; the graph, d_iter and the live points are those of the run cut before that
    iteration's first trial (iterations one less, the same max_trials)"""
    full = _run(REJECTING)
    trace = full["rounds"][0]["trace"]
    assert any(not t[-1] for t in trace)
    it_r = next(t[0] for t in trace if not t[-1])
    of_it = [t for t in trace if t[0] == it_r]
    m = next(k for k, t in enumerate(of_it) if t[-1]) if any(t[-1] for t in of_it) else len(of_it)
    assert m >= 1 and it_r >= 1 and all(sum(1 for t in trace if t[0] == i) < m for i in range(it_r)), (it_r, m)
    ends_rejected = _run(REJECTING, iterations=it_r + 1, max_trials=m)
    before = _run(REJECTING, iterations=it_r, max_trials=m)
    last = ends_rejected["rounds"][0]["trace"]
    assert len(last) == len(before["rounds"][0]["trace"]) + m and not any(t[-1] for t in last[-m:]) and last[-1][0] == it_r
    assert ends_rejected["rounds"][0]["iterations"] == it_r + 1 and before["rounds"][0]["iterations"] == it_r
    assert last[:len(last) - m] == before["rounds"][0]["trace"] == trace[:len(last) - m]
    for k in STATE_KEYS:
        assert ends_rejected["raw"][k].tobytes() == before["raw"][k].tobytes(), (k, "a popped estimate is not the pushed one")
    assert before["raw"]["Rwb"].tobytes() != _start_bytes(REJECTING)["Rwb"]       # and that estimate has moved
    for run in (full, ends_rejected, before):
        _fixed_kept(REJECTING, run)


# ---- 4
def test_a_refused_solve_is_a_rejected_trial_and_the_estimate_stays():
    """ "window 3+2 63" without inertial edges and prior jobs: the model (tests/vw_model.py) refuses every solve of it at lambda 0.  With
    lambda_init < 0 the call runs one iteration of max_trials trials, each refused and rejected at lambda 0, leaves the graph, d_iter
    and the points untouched byte for byte, and still writes the classification"""
    name = "window 3+2 63"
    sc = il.scene(name)
    be = il.ModelWindow(_bare(sc))
    ref = il.optimize(be, 10, user_lambda_init=1.0, forced_lambda_init=0.0)
    assert be.refused == il.MAX_TRIALS == len(ref["trace"]) and ref["iterations"] == 1 and not any(t[7] for t in ref["trace"])
    dev = _run(name, bare=True, lambda_init=-1.0)
    r = dev["rounds"][0]
    assert r["iterations"] == 1 and len(r["trace"]) == il.MAX_TRIALS and r["refused"] == il.MAX_TRIALS and r["accepted"] == 0 and r["lam"] == 0.0
    assert all(t[2] == 0.0 and t[4] == il.DBL_MAX and not t[7] and not t[-1] for t in r["trace"])
    assert [t[:2] for t in r["trace"]] == [(0, k) for k in range(il.MAX_TRIALS)]
    _untouched(name, dev)
    want = be.classify()
    assert np.array_equal(dev["raw"]["outlier"], want["outlier"]) and r["classification"]["n_outliers"] == want["n_outliers"]
    assert np.allclose(dev["raw"]["chi2"], want["chi2"], rtol=il.BAR, atol=0.0)


# ---- 5
def _classified_input(name):
    """mode 2 of the staged visual linearisation on the scene as it is"""
    import torch
    w = _Win(torch, torch.device("cuda", 0), il.scene(name))
    w.linearize(2)
    w.finish()
    return w.get("chi2")[:w.ne], w.get("outlier")[:w.ne], w.get("result")


def test_a_raised_stop_flag_ends_the_call_before_the_first_iteration():
    name = "window 3+2 63"
    dev = _run(name, stop=C.c_int32(1))
    sm, res = dev["raw"]["summary"], dev["raw"]["result"]
    assert sm[0] == 0 and sm[1] == 0 and sm[2] == 0 and sm[3] == 0 and sm[6] == 0 and sm[7] == 1, sm
    _untouched(name, dev)
    chi2, outlier, lin = _classified_input(name)
    assert dev["raw"]["chi2"].tobytes() == chi2.tobytes() and dev["raw"]["outlier"].tobytes() == outlier.tobytes()
    assert sm[5] == lin[5] == res[5] and res[0] == 0 and res[2] == 0 and res[3] == 0 and res[6] == 0, (sm, res, lin)
    assert np.isnan(dev["raw"]["trace"]).all()


def test_a_flag_that_stays_down_gives_the_bytes_of_no_flag():
    name = "window 3+2 63"
    _same_bytes(_run(name), _run(name, stop=C.c_int32(0)))


# ---- 6
def test_two_runs_of_the_1025_point_window_give_the_same_bytes():
    _same_bytes(_run("window 3+2 1025"), _run("window 3+2 1025", cached=False))


def test_the_null_stream_gives_the_bytes_of_an_explicit_one():
    _same_bytes(_run("window 3+2 63"), _run("window 3+2 63", "null"))


def test_a_trace_shorter_than_the_run_counts_what_it_drops():
    name = "window 3+2 63"
    full = _run(name)
    cap = full["n_trials"] // 2
    assert cap >= 2
    short = _run(name, cap_trace=cap)                       # _run's finish() holds the guards behind the trace
    assert short["raw"]["summary"][1] == full["n_trials"] and short["raw"]["summary"][6] == full["n_trials"] - cap
    assert short["raw"]["trace"][:13 * cap].tobytes() == full["raw"]["trace"][:13 * cap].tobytes()
    _same_bytes(short, full, skip=("trace", "summary"))
    assert short["raw"]["summary"][:6].tobytes() == full["raw"]["summary"][:6].tobytes()


# ---- 7
def test_the_mapper_step_on_a_device_resident_map():
    """build -> assembly -> one 32-byte read-back -> orbi_graph_init_device -> orbi_edge_information_device -> the call ON THE ASSEMBLED
    ARRAYS (the scene the helpers size their buffers from is poison) -> recover -> orbm_local_ba_apply_device with the call's d_outlier ->
    set_bias -> prior information -> the velocity prior: the decisions are those of test_inertial_window_gpu's caller loop, and the
    key-frame table, the state rows, the biases, the point table, the bank and the priors equal the model tail applied to the device's
    own estimate, byte for byte"""
    import torch
    import inertial_window_model as wm
    import test_inertial_window_gpu as tw
    from monoorbslam3_amd import imu, matcher, vw
    dev = torch.device("cuda", 0)
    sc, csr, a, ws = tw._loop_map()
    _, caller_rounds, _, _ = tw._chain_once()
    n_kf, stride, cap, ns = len(sc["n"]), sc["stride"], sc["cap_points"], len(sc["window"])
    cap_obs = len(csr[1]) + 40
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    st = il._chain_stream(torch, dev, "explicit")
    t = tw._table(torch, dev, sc, csr)
    t["obs_off"], t["obs_kf"], t["obs_kp"] = z(cap + 1, torch.int32), z(cap_obs, torch.int32), z(cap_obs, torch.int32)
    m = matcher.ORBMatcher()
    res = {k: torch.full((16,), 77, dtype=torch.int32, device=dev) for k in ("build", "problem", "recover", "apply", "set_bias", "prior", "velocity")}
    m.BuildObservationsDevice(dict(t, result=res["build"]), n_kf, stride, cap, cap_obs, stream=st)
    caps = tw._caps(a["result"])
    sizes = tw._sizes(ns, caps["states"], caps["points"], caps["edges"])
    d = dict(t, result=res["problem"], work=z(cap + 2 * n_kf, torch.int32))
    for k, dt in tw.OUT_TYPES.items():
        d[k] = _up(torch, dev, np.full(max(sizes[tw.PER.get(k, "edges")], 1) * tw.WIDTH.get(k, 1), tw.FILL[dt], dt))
    matcher.inertial_window_problem_device(m, t["kft"], d, stride, cap, cap_obs, ns, sc["n_src"], sc["cap_bank"], sc["n_priors"], sc["max_fixed"],
                                           caps["states"], caps["points"], caps["edges"], stream=st)
    head = res["problem"][:8].cpu().numpy()                               # the one 32-byte read-back
    assert head.tobytes() == a["result"][:8].tobytes() and head[wm.W_REFUSED] == 0
    n_states, n_points, n_edges, n_solve = (int(v) for v in head[:4])
    src = _up(torch, dev, sc["src"])
    # the caller's state (bank, priors, calibration) is uploaded; the problem is the assembly's, and the scene the helper sizes from is poison
    poison_graph = ws["graph"].copy()
    poison_graph.fixed[:] = 15
    poison_edges = ws["edges"].copy()
    for field in poison_edges.dtype.names:
        poison_edges[field] = -7
    i = _Dev(torch, dev, dict(ws, graph=poison_graph, edges=poison_edges), None, n_priors=sc["n_priors"], n_pjobs=1)
    i.priors.copy_(_up(torch, dev, sc["priors"]))
    assert i.n == n_states and i.ne == n_solve - 1
    graph = imu.Graph.make(i.Rwb, i.twb, i.v, i.bg, i.ba, d["fixed"], n_states)
    it = i._pad("it", np.zeros(n_states, np.int32), -3)
    n_work = vw.window_work_doubles(n_states, n_solve, n_points, n_edges, n_solve - 1, 1)
    work, trace, summary = i._pad("loop work", np.full(n_work, NAN), -1.5), i._pad("trace", np.full(CAP_TRACE * 13, NAN), -1.5), i._pad("summary", np.full(8, NAN), -1.5)
    chi2, outlier = i._pad("loop chi2", np.full(n_edges, NAN), -1.5), i._pad("outlier", np.full(n_edges, 0xEE, np.uint8), 0xA5)
    points = d["ba_points"][:3 * n_points]
    cal, cam = _calib(ws["cal"]), _camera(ws["cam"])
    kw = il.SCENES[tw.LOOP_SCENE][2]
    imu.graph_init_device(graph, i.bank, i.cap, src, sc["n_src"], d["init_jobs"], n_states, i.result, stream=st)
    imu.edge_information_device(i.bank, i.cap, d["inertial_edges"], n_solve - 1, i.info, i.walk, i.result, stream=st)
    o = vw.WindowLoopOptions.make(ws["cal"]["gravity"], iterations=kw["iterations"], lambda_init=1e-2 if kw.get("be_large") else 1e0)
    vw.window_optimize_device(graph, it, i.bank, i.cap, d["inertial_edges"], n_solve - 1, i.info, i.walk, i.priors, sc["n_priors"], d["prior_jobs"], 1, cal, cam,
                              n_solve, n_points, n_edges, points, d["edge_state"], d["edge_point"], d["edge_z"], d["edge_inv_sigma2"], None, o, work, chi2, outlier,
                              trace, CAP_TRACE, summary, i.result, stream=st)
    loop_result = i.res()
    bias, est_R, est_t = z(6 * n_solve, torch.float32), z(9 * n_solve, torch.float64), z(3 * n_solve, torch.float64)
    imu.graph_recover_device(graph, cal, d["recover_jobs"], n_solve, src, sc["n_src"], bias, res["recover"], d_pose_R=est_R, d_pose_t=est_t, stream=st)
    matcher.local_ba_apply_device(m, dict(t, pose_kf=d["state_kf"], point_row=d["point_row"], edge_off=d["edge_off"], edge_kf=d["edge_kf"], edge_kp=d["edge_kp"],
                                          est_pose_R=est_R, est_pose_t=est_t, est_points=points, outlier=outlier, result=res["apply"]),
                                  n_kf, stride, cap, cap_obs, n_solve, n_points, n_edges, stream=st)
    imu.set_bias_device(cal, i.bank, i.pool, i.cap, i.cap_meas, d["bias_ids"], bias, n_solve, res["set_bias"], stream=st)
    imu.prior_information_device(i.priors, sc["n_priors"], i.bank, i.cap, d["prior_info_jobs"], n_solve - 1, res["prior"], d_src=src, n_src=sc["n_src"], stream=st)
    matcher.inertial_window_velocity_prior_device(m, dict(priors=i.priors, src=src, recover_jobs=d["recover_jobs"], prior_jobs=d["prior_jobs"],
                                                          result=res["velocity"]), sc["n_priors"], sc["n_src"], stream=st)
    i.finish()
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    sm, rows = g(summary), None
    total = int(sm[1])
    rows = _rows(g(trace), total)
    assert total <= CAP_TRACE and sm[6] == 0 and sm[7] == 0 and loop_result[0] == sm[2] and loop_result[1] == 0
    # ---- the decisions are the caller loop's
    y = caller_rounds[0]
    flat = il.flat_from(y["trace"])
    assert len(rows) >= flat and [r[-1] for r in rows[:flat]] == [r[-1] for r in y["trace"][:flat]] and flat >= 5
    out = g(outlier)
    assert sm[5] == (out != 0).sum() == loop_result[5]
    # ---- the tail: the models on the device's own estimate, byte for byte
    est = dict(Rwb=g(i.Rwb).reshape(n_states, 3, 3), twb=g(i.twb).reshape(n_states, 3), v=g(i.v).reshape(n_states, 3), bg=g(i.bg).reshape(n_states, 3),
               ba=g(i.ba).reshape(n_states, 3), iter=g(it), points=g(points).reshape(-1, 3))
    want = wm.tail(sc, csr, a, est, out, [r.copy() for r in ws["recs"]])
    held = dict(slots=g(t["slots"]), valid=g(t["valid"]), ref_kf=g(t["ref_kf"]), points=g(t["points"]), pose_R=g(t["kf_pose_R"]), pose_t=g(t["kf_pose_t"]),
                src=g(src), bias=g(bias), est_pose_R=g(est_R), est_pose_t=g(est_t))
    for k, v in want["results"].items():
        key = dict(recover="recover", apply="apply", set_bias="set_bias", prior_information="prior", velocity_prior="velocity")[k]
        assert g(res[key])[:8].tobytes() == np.asarray(v, np.int32)[:8].tobytes(), k
    for k in held:
        assert held[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    bank, pool = want["bank"].pack()
    assert g(i.bank).tobytes() == bank.tobytes() and g(i.pool).tobytes() == pool.tobytes() and g(i.priors).tobytes() == want["priors"].tobytes()
    assert (want["pose_R"][sc["window"]] != sc["pose_R"][sc["window"]]).any() and (want["points"] != sc["points"]).any()
