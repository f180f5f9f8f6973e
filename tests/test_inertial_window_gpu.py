"""The inertial local BA window assembled on the device-resident map on the MI355X (include/orbm.h, "The inertial local BA window on the
device-resident map"): the assembly against the array model of tests/inertial_window_model.py BYTE FOR BYTE (integers and exact
conversions only), its refusals, its job lists driving the existing calls of the inertial and the visual side, and the inertial mapper
chain with tests/inertial_loop.py as the caller of the loop."""
import numpy as np
import pytest

import inertial_window_model as wm
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401 (GUARD: the padding _padded puts around every array)
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
SLACK = 5                                # capacity beyond the counts
NAN = float("nan")
OUT_TYPES = dict(ba_points=np.float64, point_row=np.int32, edge_off=np.int32, edge_state=np.int32, edge_point=np.int32, edge_z=np.float64,
                 edge_inv_sigma2=np.float64, edge_kf=np.int32, edge_kp=np.int32, state_kf=np.int32, init_jobs=np.int32, fixed=np.uint8,
                 inertial_edges=np.int32, prior_jobs=np.int32, recover_jobs=np.int32, bias_ids=np.int32, prior_info_jobs=np.int32)
WIDTH = dict(ba_points=3, edge_z=2, init_jobs=3, inertial_edges=4, prior_jobs=3, recover_jobs=3, prior_info_jobs=3)
PER = dict(ba_points="points", point_row="points", edge_off="points+1", state_kf="states", init_jobs="states", fixed="states",
           inertial_edges="solve-1", prior_jobs="one", recover_jobs="solve", bias_ids="solve", prior_info_jobs="solve-1")
FILL = {np.float64: NAN, np.int32: -9, np.uint8: 0xF7}


def _scene(name):
    """(scene, CSR, model problem): computed once, shared, never changed"""
    if name not in _cache:
        sc, csr = wm.make(name)
        _cache[name] = (sc, csr, wm.problem(sc, csr))
    return _cache[name]


def _table(torch, dev, sc, csr):
    """the map as a caller holds it on the device"""
    from monoorbslam3_amd.matcher import KfTable
    d = dict(slots=_up(torch, dev, sc["slots"]), valid=_up(torch, dev, sc["valid"]), points=_up(torch, dev, sc["points"]),
             ref_kf=_up(torch, dev, sc["ref_kf"]), n=_up(torch, dev, sc["n"]), bad=_up(torch, dev, sc["bad"]),
             kf_pose_R=_up(torch, dev, sc["pose_R"]), kf_pose_t=_up(torch, dev, sc["pose_t"]), obs_off=_up(torch, dev, csr[0]),
             obs_kf=_up(torch, dev, np.concatenate([csr[1], np.zeros(1, np.int32)])), obs_kp=_up(torch, dev, np.concatenate([csr[2], np.zeros(1, np.int32)])),
             window=_up(torch, dev, sc["window"]), kf_imu=_up(torch, dev, sc["kf_imu"]))
    d["kps"] = [_up(torch, dev, k) for k in sc["kps"]]
    d["kft"] = KfTable.make(d["kf_pose_R"], d["kf_pose_t"], d["bad"], d["kps"], d["kps"], d["n"])   # descriptors are not read here
    return d


def _caps(counts, cut=None):
    caps = dict(states=int(counts[wm.W_STATES]) + SLACK, points=int(counts[wm.W_POINTS]) + SLACK, edges=int(counts[wm.W_EDGES]) + SLACK)
    if cut:
        caps[cut] -= SLACK + 1
    return caps


def _sizes(n_window, states, points, edges):
    return {"states": states, "points": points, "points+1": points + 1, "edges": edges, "solve": n_window, "solve-1": n_window - 1, "one": 1}


def _assemble(torch, dev, sc, csr, t, caps, stream_kind):
    """one orbm_inertial_window_problem_device on outputs filled with NaN / -9 between guard pads -> (the arrays on the device, d_result
    as numpy, the outputs as numpy)"""
    from monoorbslam3_amd import matcher
    n_window = len(sc["window"])
    sizes = _sizes(n_window, caps["states"], caps["points"], caps["edges"])
    pads = {}
    for k, dt in OUT_TYPES.items():
        n = max(sizes[PER.get(k, "edges")], 1) * WIDTH.get(k, 1)             # a list of n_window - 1 = 0 entries still has an address
        pads[k] = _padded(torch, dev, np.full(n, FILL[dt], dt), 17)
    pads["result"] = _padded(torch, dev, np.full(16, 77, np.int32), 17)
    pads["work"] = _padded(torch, dev, np.full(sc["cap_points"] + 2 * len(sc["n"]), -5, np.int32), 17)
    d = dict(t, **{k: v[1] for k, v in pads.items()})
    st = _stream(torch, dev, stream_kind)
    matcher.inertial_window_problem_device(matcher.ORBMatcher(), t["kft"], d, sc["stride"], sc["cap_points"], len(csr[1]), n_window, sc["n_src"],
                                           sc["cap_bank"], sc["n_priors"], sc["max_fixed"], caps["states"], caps["points"], caps["edges"], stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], 17), k
    return d, d["result"].cpu().numpy(), {k: d[k].cpu().numpy() for k in OUT_TYPES}


def _untouched(a):
    fill = FILL[a.dtype.type]
    return np.isnan(a).all() if a.dtype == np.float64 else (a == fill).all()


def _equals_model(got, want, n_window):
    res = want["result"]
    counts = _sizes(n_window, res[wm.W_STATES], res[wm.W_POINTS], res[wm.W_EDGES])
    for k in OUT_TYPES:
        n = counts[PER.get(k, "edges")] * WIDTH.get(k, 1)
        assert got[k][:n].tobytes() == np.ascontiguousarray(want[k]).reshape(-1).tobytes(), k
        if PER.get(k) in ("solve-1", "solve", "one"):
            assert _untouched(got[k][n:]), k                                  # nothing behind a list of n_window - 1 or n_window entries


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", wm.SCENES)
def test_the_assembly_equals_the_model(name, stream_kind):
    """8 key frames of 96 slots and 200 table rows: a window of 3 with four fixed key frames and a row with a key frame twice in its
    list; a window of 1; slots edited behind the CSR; max_fixed = 1, 2 (reached exactly at a point boundary) and 3 (reached in mid-scene)
    with the edges behind the cap dropped and counted; a forged CSR offset and entries out of range; 2 key frames x 600 slots, so that
    the numbering crosses a tile of the block scan; a point of 260 edges.  Every output array up to its count and d_result byte for
    byte, guards intact, inputs as passed; a second run gives the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, want = _scene(name)
    t = _table(torch, dev, sc, csr)
    d, res, got = _assemble(torch, dev, sc, csr, t, _caps(want["result"]), stream_kind)
    print("device d_result %s, model %s" % (res.tolist(), want["result"].tolist()))
    assert res.tobytes() == want["result"].tobytes() and res[wm.W_REFUSED] == 0
    _equals_model(got, want, len(sc["window"]))
    _, res2, again = _assemble(torch, dev, sc, csr, t, _caps(want["result"]), stream_kind)
    assert res2.tobytes() == res.tobytes()
    for k in OUT_TYPES:
        assert again[k].tobytes() == got[k].tobytes(), k
    for key in ("slots", "valid", "points", "window", "kf_imu"):              # inputs as passed
        assert t[key].cpu().numpy().tobytes() == np.ascontiguousarray(sc[key]).tobytes(), key


def _refusal_case(case):
    """-> (scene, CSR, model output, capacities)"""
    sc, csr, full = _scene("window3")
    w, res = [int(k) for k in sc["window"]], full["result"]
    if case in ("states", "points", "edges"):
        caps = _caps(res, case)
        want = wm.problem(sc, csr, cap_states=caps["states"], cap_local_points=caps["points"], cap_edges=caps["edges"])
        assert want["result"][wm.W_REFUSED] == dict(states=wm.REFUSE_STATES, points=wm.REFUSE_POINTS, edges=wm.REFUSE_EDGES)[case]
        assert (want["result"][:5] == res[:5]).all()                        # the FULL counts
        return sc, csr, want, caps
    if case.startswith("window"):
        window = dict(window_out_of_range=[w[0], len(sc["n"]), w[2]], window_negative=[-1, w[1], w[2]], window_bad=[w[0], w[1], sc["roles"]["bad"]],
                      window_repeated=[w[1], w[0], w[1]])[case]
        sc = dict(sc, window=np.array(window, np.int32))
        want = wm.problem(sc, csr)
        assert want["result"][wm.W_REFUSED] == wm.REFUSE_WINDOW and want["result"][wm.W_WINDOW_UNUSABLE] == 1
    elif case.startswith("imu"):
        k, c, v = dict(imu_row=(w[1], 0, sc["n_src"]), imu_record=(w[0], 1, -1), imu_prior=(w[2], 2, sc["n_priors"]),
                       imu_fixed_row=(int(full["state_kf"][4]), 0, -2))[case]
        imu = sc["kf_imu"].copy()
        imu[k, c] = v
        sc = dict(sc, kf_imu=imu)
        want = wm.problem(sc, csr)
        assert want["result"][wm.W_REFUSED] == wm.REFUSE_IMU and (want["result"][:5] == res[:5]).all()
    else:
        sc = dict(sc, valid=np.zeros_like(sc["valid"]))
        want = wm.problem(sc, csr)
        assert want["result"][wm.W_REFUSED] == wm.REFUSE_NO_EDGE
    return sc, csr, want, _caps(res)


@pytest.mark.parametrize("case", ["states", "points", "edges", "window_out_of_range", "window_negative", "window_bad", "window_repeated", "imu_row",
                                  "imu_record", "imu_prior", "imu_fixed_row", "no_edge"])
def test_a_refused_assembly_keeps_the_full_counts_and_its_capacities(case):
    """one capacity one below the count; a window entry out of range, bad or repeated; each d_kf_imu index of a window key frame and the
    state row of a fixed one out of range; no edge: d_result equals the model's, full counts included, the guards behind every array
    cut to its capacity are intact, the job lists are not written, and an unusable window leaves every output as it was"""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, want, caps = _refusal_case(case)
    _, res, got = _assemble(torch, dev, sc, csr, _table(torch, dev, sc, csr), caps, "explicit")
    print("device d_result %s, model %s" % (res.tolist(), want["result"].tolist()))
    assert res.tobytes() == want["result"].tobytes()
    for k in ("edge_z", "edge_inv_sigma2") + wm.INERTIAL_OUT:
        assert _untouched(got[k]), k
    if case.startswith("window"):
        for k in OUT_TYPES:
            assert _untouched(got[k]), k


# ---- the job lists in use: a loop scene of tests/inertial_loop.py laid out as a map ---------------------------------------------------------
LOOP_SCENE = "window 3+2 63 converging"


def _loop_map():
    """(the map the scene was laid out as, its CSR, the model assembly, the window scene in the assembly's order): computed once, shared"""
    if "loop" not in _cache:
        import inertial_loop as il
        import local_ba_model as lm
        sc = wm.map_from_window_scene(il.scene(LOOP_SCENE))
        csr = lm.fresh_csr(sc)
        a = wm.problem(sc, csr)
        wm.reproduces(sc, a)
        rng = np.random.RandomState(90)                                   # what the refresh reads and writes beside the map
        rows = sc["cap_points"] + 4
        sc["kf_desc"] = [rng.randint(0, 256, (sc["stride"], 32)).astype(np.uint8) for _ in sc["n"]]
        sc["table"] = dict(normals=rng.uniform(-1, 1, (rows, 3)).astype(np.float32), min_dist=rng.uniform(1, 2, rows).astype(np.float32),
                           max_dist=rng.uniform(20, 30, rows).astype(np.float32), desc=rng.randint(0, 256, (rows, 32)).astype(np.uint8))
        _cache["loop"] = (sc, csr, a, wm.window_scene_of(sc, a))
    return _cache["loop"]


def _stage_calls(torch, dev, sc, ws, lists, stream=None):
    """orbi_graph_init_device, orbi_edge_information_device, one mode-0 orbi_linearize_device and the visual-window linearise on the job
    lists and edge arrays `lists` (device tensors) -> every output as numpy"""
    from monoorbslam3_amd import imu
    from test_factors_gpu import _Dev
    from test_vw_gpu import _Win
    res, n_states, ns = sc["model"]["result"], len(ws["graph"].fixed), ws["n_solve"]
    i = _Dev(torch, dev, ws, None, n_priors=sc["n_priors"], n_pjobs=1)
    i.priors.copy_(_up(torch, dev, sc["priors"]))
    graph = imu.Graph.make(i.Rwb, i.twb, i.v, i.bg, i.ba, lists["fixed"], n_states)
    src = _up(torch, dev, sc["src"])
    out = {}
    imu.graph_init_device(graph, i.bank, i.cap, src, sc["n_src"], lists["init_jobs"], n_states, i.result, stream=stream)
    out["init result"] = i.res()
    imu.edge_information_device(i.bank, i.cap, lists["inertial_edges"], ns - 1, i.info, i.walk, i.result, stream=stream)
    out["information result"] = i.res()
    i.edges, i.graph = lists["inertial_edges"], graph
    i.linearize(ws, 0.0, 0, lists["prior_jobs"], 1, sc["n_priors"], stream)
    out["linearize result"] = i.res()
    w = _Win(torch, dev, ws)
    w.graph, w.edge_state, w.edge_point, w.z, w.w = graph, lists["edge_state"], lists["edge_point"], lists["edge_z"], lists["edge_inv_sigma2"]
    assert (w.np_, w.ne) == (int(res[wm.W_POINTS]), int(res[wm.W_EDGES]))
    w.linearize(0, points=lists["ba_points"], H_diag=i.H_diag, b=i.b, stream=stream)
    for k in ("Rwb", "twb", "v", "bg", "ba", "info", "walk", "err", "chi2", "chi2_prior", "total", "H_diag", "H_off", "b", "J", "flt"):
        out[k] = i.get(k).copy()
    for k in ("point_off", "err", "chi2", "total", "Hll", "bl", "Hlp", "result"):
        out["visual " + k] = w.get(k)
    i.finish()
    w.finish()
    return out


def test_the_job_lists_drive_the_existing_calls():
    """the calls of the inertial side and the visual-window linearise on the ASSEMBLED device arrays give the bytes of the same calls on
    the model's assembled arrays uploaded: the same kernels on the same inputs.  Every job is carried out and every edge kept."""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, a, ws = _loop_map()
    sc = dict(sc, model=a)
    d, res, got = _assemble(torch, dev, sc, csr, _table(torch, dev, sc, csr), _caps(a["result"]), "explicit")
    assert res.tobytes() == a["result"].tobytes()
    _equals_model(got, a, len(sc["window"]))
    on_device = _stage_calls(torch, dev, sc, ws, d)
    uploaded = _stage_calls(torch, dev, sc, ws, {k: _up(torch, dev, np.ascontiguousarray(a[k]).reshape(-1)) for k in OUT_TYPES})
    n_states, ns = int(res[wm.W_STATES]), int(res[wm.W_SOLVE])
    assert on_device["init result"][0] == n_states and on_device["information result"][0] == ns - 1
    assert on_device["linearize result"][0] == ns - 1 and on_device["linearize result"][4] == 1     # ORBI_R_DONE edges, ORBI_R_PRIOR_DONE
    assert on_device["visual result"][0] == res[wm.W_EDGES] and np.isfinite(on_device["H_diag"]).all() and np.isfinite(on_device["visual Hlp"]).all()
    for k in on_device:
        assert on_device[k].tobytes() == uploaded[k].tobytes(), k
    g = ws["graph"]                                                       # and the graph is the scene's
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        assert on_device[k].tobytes() == np.ascontiguousarray(getattr(g, k)).tobytes(), k


def _assembled_window(torch, dev, sc, ws, d, src, st):
    """tests/inertial_loop.py's DeviceWindow over DEVICE ARRAYS: the graph comes from orbi_graph_init_device on d_init_jobs, the edges, the
    prior job, the fixed masks and the EdgeMono arrays are the assembly's.  _Dev and _Win size their buffers from a scene and upload
    its problem; the scene they get here is POISON (NaN points, measurements and weights, edges and states out of range, every vertex
    fixed), so a field this class forgot to replace by the assembly's would fail the loop, not pass on equal bytes.  The bank, the
    priors and the calibration are the caller's state, not the problem, and are uploaded."""
    import inertial_loop as il
    from monoorbslam3_amd import imu, vw
    from test_factors_gpu import _Dev
    from test_vw_gpu import _Win

    class AssembledWindow(il.DeviceWindow):
        def __init__(self):
            self.torch, self.sc, self.imu, self.vw = torch, ws, imu, vw
            poison_graph = ws["graph"].copy()
            poison_graph.fixed[:] = 15
            poison_edges = ws["edges"].copy()
            for name in poison_edges.dtype.names:
                poison_edges[name] = -7
            poison = dict(ws, graph=poison_graph, edges=poison_edges, points=np.full_like(ws["points"], NAN), z=np.full_like(ws["z"], NAN),
                          w=np.full_like(ws["w"], NAN), edge_state=np.full_like(ws["edge_state"], -7), edge_point=np.full_like(ws["edge_point"], -7))
            i = _Dev(torch, dev, poison, None, n_priors=sc["n_priors"], n_pjobs=1)
            i.priors.copy_(_up(torch, dev, sc["priors"]))
            i.fixed, i.edges = d["fixed"], d["inertial_edges"]
            i.graph = imu.Graph.make(i.Rwb, i.twb, i.v, i.bg, i.ba, i.fixed, i.n)
            stage = i.linearize                                           # the prior job names a slot of the WHOLE prior array
            i.linearize = lambda s, delta, mode, pjobs, n_pjobs, n_priors, stream: stage(s, delta, mode, pjobs, n_pjobs, sc["n_priors"], stream)
            w = _Win(torch, dev, poison)
            w.graph, w.fixed, w.edges = i.graph, i.fixed, i.edges
            w.edge_state, w.edge_point, w.z, w.w = d["edge_state"], d["edge_point"], d["edge_z"], d["edge_inv_sigma2"]
            w.points = d["ba_points"][:3 * w.np_]
            self.w, self.pjobs, self.st = w, d["prior_jobs"], st
            imu.graph_init_device(i.graph, i.bank, i.cap, src, sc["n_src"], d["init_jobs"], i.n, i.result, stream=st)
            self._init_state(i, False)
            self.pts, self.cur = [w.points, w.points_out], 0
            imu.edge_information_device(i.bank, i.cap, i.edges, i.ne, i.info, i.walk, i.result, stream=st)

    return AssembledWindow()


def _chain(torch, dev, stream_kind):
    """the inertial mapper chain of include/orbm.h's section on one stream -> (what the device holds afterwards, the loop's rounds, its
    estimate, the assembly's d_result)"""
    import inertial_loop as il
    import refresh_model as rm
    from monoorbslam3_amd import imu, matcher
    from test_factors_gpu import _calib
    sc, csr, a, ws = _loop_map()
    n_kf, stride, cap, ns = len(sc["n"]), sc["stride"], sc["cap_points"], len(sc["window"])
    cap_obs = len(csr[1]) + 40
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    st = il._chain_stream(torch, dev, stream_kind)
    t = _table(torch, dev, sc, csr)
    t["obs_off"], t["obs_kf"], t["obs_kp"] = z(cap + 1, torch.int32), z(cap_obs, torch.int32), z(cap_obs, torch.int32)
    m = matcher.ORBMatcher()
    res = {k: torch.full((16,), 77, dtype=torch.int32, device=dev)
           for k in ("build", "problem", "recover", "apply", "set_bias", "prior", "velocity", "build2", "refresh")}
    tab = {k: _up(torch, dev, v) for k, v in sc["table"].items()}
    desc_kf = [_up(torch, dev, x) for x in sc["kf_desc"]]
    kft_desc = matcher.KfTable.make(t["kf_pose_R"], t["kf_pose_t"], t["bad"], t["kps"], desc_kf, t["n"])
    m.BuildObservationsDevice(dict(t, result=res["build"]), n_kf, stride, cap, cap_obs, stream=st)
    caps = _caps(a["result"])
    sizes = _sizes(ns, caps["states"], caps["points"], caps["edges"])
    d = dict(t, result=res["problem"], work=z(cap + 2 * n_kf, torch.int32))
    for k, dt in OUT_TYPES.items():
        d[k] = _up(torch, dev, np.full(max(sizes[PER.get(k, "edges")], 1) * WIDTH.get(k, 1), FILL[dt], dt))
    matcher.inertial_window_problem_device(m, t["kft"], d, stride, cap, cap_obs, ns, sc["n_src"], sc["cap_bank"], sc["n_priors"], sc["max_fixed"],
                                           caps["states"], caps["points"], caps["edges"], stream=st)
    head = res["problem"][:8].cpu().numpy()                               # the one 32-byte read-back
    assert head.tobytes() == a["result"][:8].tobytes() and head[wm.W_REFUSED] == 0
    n_states, n_points, n_edges, n_solve = (int(v) for v in head[:4])
    src = _up(torch, dev, sc["src"])
    be = _assembled_window(torch, dev, sc, ws, d, src, st)
    rounds = il.local_full(be, **il.SCENES[LOOP_SCENE][2])                # the caller's loop and mode 2
    estimate = be.estimate()
    i, w = be.d, be.w
    bias, est_R, est_t = z(6 * n_solve, torch.float32), z(9 * n_solve, torch.float64), z(3 * n_solve, torch.float64)
    cal = _calib(ws["cal"])
    imu.graph_recover_device(i.graph, cal, d["recover_jobs"], n_solve, src, sc["n_src"], bias, res["recover"], d_pose_R=est_R, d_pose_t=est_t, stream=st)
    matcher.local_ba_apply_device(m, dict(t, pose_kf=d["state_kf"], point_row=d["point_row"], edge_off=d["edge_off"], edge_kf=d["edge_kf"], edge_kp=d["edge_kp"],
                                          est_pose_R=est_R, est_pose_t=est_t, est_points=be.pts[be.cur], outlier=w.outlier, result=res["apply"]),
                                  n_kf, stride, cap, cap_obs, n_solve, n_points, n_edges, stream=st)
    imu.set_bias_device(cal, i.bank, i.pool, i.cap, i.cap_meas, d["bias_ids"], bias, n_solve, res["set_bias"], stream=st)
    imu.prior_information_device(i.priors, sc["n_priors"], i.bank, i.cap, d["prior_info_jobs"], n_solve - 1, res["prior"], d_src=src, n_src=sc["n_src"], stream=st)
    matcher.inertial_window_velocity_prior_device(m, dict(priors=i.priors, src=src, recover_jobs=d["recover_jobs"], prior_jobs=d["prior_jobs"],
                                                          result=res["velocity"]), sc["n_priors"], sc["n_src"], stream=st)
    m.BuildObservationsDevice(dict(t, result=res["build2"]), n_kf, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft_desc, dict(t, **tab, sel=d["point_row"], result=res["refresh"]), n_points, cap, cap_obs, float(rm.MAX_SCALE_FACTOR),
                          stream=st)                                      # mp->update() of the local points: d_sel = d_point_row
    torch.cuda.synchronize()                                              # the one wait behind the loop
    be.finish()
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    held = dict(slots=g(t["slots"]), valid=g(t["valid"]), ref_kf=g(t["ref_kf"]), points=g(t["points"]), pose_R=g(t["kf_pose_R"]), pose_t=g(t["kf_pose_t"]),
                src=g(src), bias=g(bias), est_pose_R=g(est_R), est_pose_t=g(est_t), bank=g(i.bank), pool=g(i.pool), priors=g(i.priors),
                obs_off=g(t["obs_off"]), obs_kf=g(t["obs_kf"]), outlier=g(w.outlier)[:n_edges], **{k: g(v) for k, v in tab.items()}, **{"result " + k: g(v)[:8] for k, v in res.items()})
    return held, rounds, estimate, head


def _chain_once(stream_kind="explicit"):
    if ("chain", stream_kind) not in _cache:
        import torch
        _cache[("chain", stream_kind)] = _chain(torch, torch.device("cuda", 0), stream_kind)
    return _cache[("chain", stream_kind)]


def test_the_inertial_mapper_chain():
    """build -> assembly -> one 32-byte read-back -> orbi_graph_init_device -> orbi_edge_information_device -> the caller's loop
    (tests/inertial_loop.py over device arrays) -> mode 2 -> recover -> orbm_local_ba_apply_device -> set_bias -> prior information ->
    the velocity prior -> build -> orbm_refresh_points_device (d_sel = d_point_row), against the model chain: decisions and classifications equal, the estimate within the bars of
    tests/test_inertial_loop_gpu.py, and everything the tail writes equal to the model tail applied to the device's own estimate,
    byte for byte; the oldest key frame's velo_priori is updated, its bias_priori and its three information matrices are not.  The
    rebuilt CSR and the refreshed normals, distances and descriptors of the local points equal the models' on the applied map."""
    import factors_model as fm
    import inertial_loop as il
    import observations_model as om
    import vi_model as vm
    from test_inertial_loop_gpu import _bar
    sc, csr, a, ws = _loop_map()
    held, rounds, est, head = _chain_once()
    ref = il.run(LOOP_SCENE, il.ModelWindow(ws))
    # ---- decisions and classifications
    x, y = rounds[0], ref["rounds"][0]
    flat = il.flat_from(y["trace"])
    assert len(x["trace"]) >= flat and [t[-1] for t in x["trace"][:flat]] == [t[-1] for t in y["trace"][:flat]] and flat >= 5
    c, mdl = x["classification"], y["classification"]
    near = np.abs(mdl["chi2"] - vm.CHI2_MONO) <= 1e-6 * vm.CHI2_MONO
    assert near.mean() <= 0.01 and np.array_equal(c["outlier"][~near], mdl["outlier"][~near]) and c["n_outliers"] == (c["outlier"] != 0).sum()
    # ---- the estimate, within the bars the loop's own GPU test uses
    for o in il.STATE + ("points",):
        scale = np.abs(ref["estimate"][o]).max()
        dev_ = float(np.abs(est[o] - ref["estimate"][o]).max() / scale)
        print("%s: largest deviation %.3g of %.3g allowed" % (o, dev_, _bar(LOOP_SCENE, o)))
        assert dev_ <= _bar(LOOP_SCENE, o), (o, dev_)
    # ---- the tail: the models on the device's own estimate, byte for byte
    recs = [r.copy() for r in ws["recs"]]
    want = wm.tail(sc, csr, a, est, held["outlier"], recs)
    for k, v in want["results"].items():
        key = dict(recover="recover", apply="apply", set_bias="set_bias", prior_information="prior", velocity_prior="velocity")[k]
        print(k, held["result " + key].tolist(), v.tolist())
        assert held["result " + key].tobytes() == np.asarray(v, np.int32)[:8].tobytes(), k
    for k in ("slots", "valid", "ref_kf", "points", "pose_R", "pose_t", "src", "bias", "est_pose_R", "est_pose_t"):
        assert held[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    bank, pool = want["bank"].pack()
    assert held["bank"].tobytes() == bank.tobytes() and held["pool"].tobytes() == pool.tobytes()
    assert held["priors"].tobytes() == want["priors"].tobytes()
    n_solve = int(head[wm.W_SOLVE])
    assert want["results"]["apply"][7] == n_solve and want["results"]["apply"][4] >= 60 and want["results"]["set_bias"][0] == n_solve
    assert (want["pose_R"][sc["window"]] != sc["pose_R"][sc["window"]]).any() and (want["points"] != sc["points"]).any()
    # ---- the oldest key frame's prior: velo_priori moved to the recovered velocity, nothing else of the slot
    before = sc["priors"]
    after = np.frombuffer(held["priors"].tobytes(), fm.PRIOR)
    oldest, row = int(a["prior_jobs"][0, 1]), int(a["recover_jobs"][0, 1])
    assert after[oldest]["velo_priori"].tobytes() == held["src"].reshape(-1, 15)[row, 12:15].tobytes()
    assert after[oldest]["velo_priori"].tobytes() != before[oldest]["velo_priori"].tobytes()
    for k in ("bias_priori", "velo_info", "gyro_info", "acc_info"):
        assert after[oldest][k].tobytes() == before[oldest][k].tobytes(), k
    for s in range(1, n_solve):                                           # the others were chained: every field written
        slot = int(a["prior_info_jobs"][s - 1, 0])
        assert after[slot]["gyro_info"].tobytes() != before[slot]["gyro_info"].tobytes() and after[slot]["bias_priori"].tobytes() == held["bias"].reshape(-1, 6)[s - 1].tobytes()
    # ---- the CSR rebuilt behind the tail is the applied map's, and the refresh of the local points (d_sel = d_point_row) the model's on it
    import refresh_model as rm
    off2, okf2, okp2, bres2 = om.build(sc["n"], sc["bad"], want["slots"], sc["stride"], want["valid"], sc["cap_points"], 1 << 30)
    assert held["obs_off"].tobytes() == off2.tobytes() and held["obs_kf"][:len(okf2)].tobytes() == okf2.tobytes()
    assert held["result build2"].tobytes() == bres2.tobytes()
    rs = dict(n=sc["n"], bad=sc["bad"], pose_R=want["pose_R"], pose_t=want["pose_t"], kps=sc["kps"], kf_desc=sc["kf_desc"], points=want["points"],
              valid=want["valid"], obs_off=off2, obs_kf=okf2, obs_kp=okp2, ref_kf=want["ref_kf"], **sc["table"])
    fresh = rm.refresh(rs, a["point_row"], sc["cap_points"])
    print("refresh", held["result refresh"].tolist(), fresh["result"].tolist())
    assert np.array_equal(held["result refresh"], fresh["result"]) and fresh["result"][0] >= 60
    assert np.array_equal(held["normals"].reshape(-1, 3), fresh["normals"])          # by value: -0 equals +0
    for k in ("min_dist", "max_dist"):
        assert held[k].view(np.uint32).tobytes() == fresh[k].view(np.uint32).tobytes(), k
    assert np.array_equal(held["desc"].reshape(-1, 32), fresh["desc"])
    assert (fresh["normals"] != sc["table"]["normals"]).any() and (fresh["desc"] != sc["table"]["desc"]).any()


def test_two_runs_of_the_chain_give_the_same_bytes():
    import torch
    first, rounds1, est1, _ = _chain_once()
    second, rounds2, est2, _ = _chain(torch, torch.device("cuda", 0), "explicit")
    assert [r["trace"] for r in rounds1] == [r["trace"] for r in rounds2]
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    for k in est1:
        assert est1[k].tobytes() == est2[k].tobytes(), k
