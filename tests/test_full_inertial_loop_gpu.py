"""fullInertialOptimize's Levenberg-Marquardt loop closed on the MI355X: tests/full_inertial_loop.py's device back-end runs FREE -- its
own decisions from its own read-backs, no state uploaded after the start -- against the model loop of the same scene, by the rules of
tests/test_inertial_loop_gpu.py.  The accept / reject sequence and the iteration counts are equal (up to inertial_loop.flat_from() on the
scenes that reach their minimum); every trial's read-backs and the final estimate lie within 4 x MEASURED_SPREAD
of tests/test_full_inertial_cpu.py per output -- the model's own sensitivity to a stage error of
1e-9, never the device's result -- and no bar is tighter than 1e-9, the stage bar.  Every buffer sits between guard elements.
Behind them the whole step on a small device-resident map: the chain of include/orbfi.h from the window assembly to the refresh, its loop
over the assembled device arrays, against the model chain."""
import time

import numpy as np
import pytest

import factors_model as fm
import full_inertial_loop as fl
import inertial_loop as il
from test_full_inertial_cpu import MEASURED_SPREAD
from test_inertial_loop_cpu import TRIAL, trial_deviation

pytestmark = pytest.mark.gpu

_cache = {}
NAN = float("nan")


def _bar(name, key):
    """4 x the model's measured spread of that output, never below the stage bar.  A trial's read-backs are held to their OWN spread ("trial
    lam" / "trial total" / "trial scale"), as tests/test_inertial_loop_gpu.py holds its beLarge scene: lambda starts at 1e-5 against an inertial
    information of 1e14 -- and without a fixed key frame lambda alone holds the gauge -- so a trial in the middle of the route is far more
    sensitive than the total at its end (9.2e-4 against 1.4e-5 under the 1e-9 perturbation on the scene without a fixed key frame)."""
    return max(4 * MEASURED_SPREAD[name][key], il.BAR)


def _device_run(name, stream_kind="explicit", audit=False):
    import torch
    key = (name, stream_kind, audit)
    if key not in _cache:
        be = fl.device_backend(torch, torch.device("cuda", 0), name, stream_kind, audit)
        t0 = time.perf_counter()
        r = fl.run(name, be)
        r["seconds"], r["n_trials"], r["dx_zero"], r["kf_bias_zero"] = time.perf_counter() - t0, be.n_trials, be.dx_zero, be.kf_bias_zero
        be.finish()                                                          # the guards of every buffer of the loop
        _cache[key] = r
    return _cache[key]


def _compare(name, dev):
    ref, sc = fl.model_run(name), fl.scene(name)
    conv = name in fl.CONVERGED
    worst = dict.fromkeys(TRIAL, 0.0)
    x, y = dev["rounds"][0], ref["rounds"][0]
    flat = il.flat_from(y["trace"]) if conv else len(y["trace"])
    assert len(x["trace"]) >= flat, (name, len(x["trace"]), flat)
    for k, (a, b) in enumerate(zip(x["trace"][:flat], y["trace"][:flat])):
        where = "%s, trial %d (iteration %d, trial %d of it)" % (name, k, b[0], b[1])
        assert a[:2] == b[:2] and a[7] == b[7], (where, a, b)
        for key, dv in zip(TRIAL, trial_deviation(a, b)):
            worst[key] = max(worst[key], dv)
            assert dv <= _bar(name, key), (where, key, dv, _bar(name, key), dict(zip(il.FIELDS, a)), dict(zip(il.FIELDS, b)))
        assert a[-1] == b[-1], (where, "accepted" if a[-1] else "rejected", "rho %.6g, the model's %.6g" % (a[6], b[6]))
    if not conv:
        assert x["iterations"] == y["iterations"] and len(x["trace"]) == len(y["trace"]), name
    est, want = dev["estimate"], ref["estimate"]
    for o in il.STATE + ("points",):
        scale = np.abs(want[o]).max()
        worst[o] = float(np.abs(est[o] - want[o]).max() / scale) if scale else float(np.abs(est[o]).max())
        assert worst[o] <= _bar(name, o), (name, o, worst[o], _bar(name, o))
    last = lambda r: min([t[4] for t in r["rounds"][-1]["trace"] if t[-1]] + [r["rounds"][-1]["trace"][0][3]])  # noqa: E731
    worst["total"] = abs(last(dev) - last(ref)) / last(ref)
    assert worst["total"] <= _bar(name, "total"), (name, worst["total"])
    if MEASURED_SPREAD[name]["lam"] is not None:
        worst["lam"] = abs(x["lam"] - y["lam"]) / y["lam"]
        assert worst["lam"] <= _bar(name, "lam"), (name, worst["lam"])
    assert dev["refused"] == ref["refused"] or conv
    # the counters: (accepted updates mod 3) per free pose; what is fixed keeps its bytes -- the fixed key frame never moves, the key frames'
    # bg and ba stay the zeros of "no such vertex", the carrier's pose and velocity stay the last key frame's
    g = sc["graph"]
    free_pose = (g.fixed & fm.FIX_POSE) == 0
    assert np.array_equal(est["iter"], np.where(free_pose, x["accepted"] % 3, 0)), (name, est["iter"], x["accepted"])
    for o, bit in zip(il.STATE, (fm.FIX_POSE, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC)):
        fx = (g.fixed & bit) != 0
        assert est[o][fx].tobytes() == getattr(g, o)[fx].tobytes(), (name, o, "a fixed vertex moved")
    if not sc["per_state"]:
        n_kf = sc["n_kf"]
        assert not est["bg"][:n_kf].any() and not est["ba"][:n_kf].any() and est["bg"][n_kf].tobytes() != g.bg[n_kf].tobytes(), name
    print("%s: %d trials in %.2f s, %s" % (name, dev["n_trials"], dev["seconds"], " ".join(il.decisions(dev["rounds"]))))
    print("    largest deviation " + ", ".join("%s %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", list(fl.SCENES))
def test_the_free_running_device_loop_is_the_models(name):
    _compare(name, _device_run(name))


@pytest.mark.parametrize("name,stream_kind", [("full 4 63", "explicit"), ("full 3 65 free", "null")])
def test_a_rejected_trial_leaves_the_graph_the_counters_and_the_live_points_as_they_were(name, stream_kind):
    """the loop once more with the estimate read back around every trial: after every pop the vertices, d_iter and the live point buffer
    hold the bytes they held before the push (the assertion names the trial); at every trial the key frames' bg and ba are zero"""
    dev = _device_run(name, stream_kind, audit=True)
    assert sum(not t[-1] for t in dev["rounds"][0]["trace"]) >= 5
    _compare(name, dev)
    assert not any(dev["dx_zero"]) and all(dev["kf_bias_zero"]) and len(dev["kf_bias_zero"]) == dev["n_trials"]
    plain = _device_run(name, "explicit")
    assert [t for t in dev["rounds"][0]["trace"]] == [t for t in plain["rounds"][0]["trace"]]       # the audit and the stream change no byte
    for k, v in dev["estimate"].items():
        assert v.tobytes() == plain["estimate"][k].tobytes(), k


# ---- the whole step on a small device-resident map ------------------------------------------------------------------------------------------------
def _assembled_full(torch, dev, cm, d, lists, src, st):
    """tests/full_inertial_loop.py's DeviceFull over DEVICE ARRAYS: the vertices come from orbi_graph_init_device on orbfi_jobs_device's
    d_init_out, the fixed masks and the edges are that call's, the EdgeMono arrays the assembly's.  _Fi sizes its buffers from a scene and
    uploads its problem; the scene it gets here is POISON (NaN vertices, points, measurements, weights and information, edges and states out
    of range, every vertex fixed), so a field this class forgot to replace would fail the loop, not pass on equal bytes.  The bank and the
    calibration are the caller's state, and bias_state and prior_rec the caller's host ints."""
    from monoorbslam3_amd import imu, vw
    from test_full_inertial_gpu import _Fi
    mp, fs = cm["map"], cm["fs"]

    class AssembledFull(fl.DeviceFull):
        def __init__(self):
            self.torch, self.sc, self.imu, self.vw, self.per_state = torch, fs, imu, vw, False
            g = fs["graph"].copy()
            for k in il.STATE:
                getattr(g, k)[:] = NAN
            g.fixed[:] = 15
            edges = fs["edges"].copy()
            for key in edges.dtype.names:
                edges[key] = -7
            poison = dict(fs, graph=g, edges=edges, info=np.full((len(edges), 81), NAN), points=np.full_like(fs["points"], NAN), z=np.full_like(fs["z"], NAN),
                          w=np.full_like(fs["w"], NAN), edge_state=np.full_like(fs["edge_state"], -7), edge_point=np.full_like(fs["edge_point"], -7))
            self.f = f = _Fi(torch, dev, poison)
            i, w = f.i, f.w
            i.fixed, i.edges = lists["fixed"], lists["edges"]
            i.graph = imu.Graph.make(i.Rwb, i.twb, i.v, i.bg, i.ba, i.fixed, i.n)
            w.graph, w.fixed = i.graph, i.fixed
            w.edge_state, w.edge_point, w.z, w.w = d["edge_state"], d["edge_point"], d["edge_z"], d["edge_inv_sigma2"]
            w.points = d["ba_points"][:3 * w.np_]
            self.w, self.st = w, st
            imu.graph_init_device(i.graph, i.bank, i.cap, src, mp["n_src"], lists["init"], i.n, i.result, stream=st)
            self._init_state(i, False)
            self.kf_bias_zero = []
            self.pts, self.cur = [w.points, w.points_out], 0
            imu.edge_information_device(i.bank, i.cap, i.edges, i.ne, i.info, i.walk, i.result, stream=st)

    return AssembledFull()


def _chain(torch, dev, name):
    """the chain of include/orbfi.h on one stream -> (what the device holds afterwards, the loop's run in the form of _device_run)"""
    import inertial_window_model as iw
    import refresh_model as rm
    from monoorbslam3_amd import full_inertial, imu, matcher
    from test_factors_gpu import _calib
    from test_inertial_window_gpu import FILL, OUT_TYPES, PER, WIDTH, _caps, _sizes, _table
    from test_projection_queries_gpu import _up
    cm = fl.chain_map(name)
    mp, csr, a, fs = cm["map"], cm["csr"], cm["a"], cm["fs"]
    n_table, stride, cap, n_kf = len(mp["n"]), mp["stride"], mp["cap_points"], fl.CHAIN_KF
    cap_obs = len(csr[1]) + 40
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    st = il._chain_stream(torch, dev, "explicit")
    rng = np.random.RandomState(91)                                      # what the refresh reads and writes beside the map
    rows = cap + 4
    kf_desc = [rng.randint(0, 256, (stride, 32)).astype(np.uint8) for _ in mp["n"]]
    table = dict(normals=rng.uniform(-1, 1, (rows, 3)).astype(np.float32), min_dist=rng.uniform(1, 2, rows).astype(np.float32),
                 max_dist=rng.uniform(20, 30, rows).astype(np.float32), desc=rng.randint(0, 256, (rows, 32)).astype(np.uint8))
    t = _table(torch, dev, mp, csr)
    t["obs_off"], t["obs_kf"], t["obs_kp"] = z(cap + 1, torch.int32), z(cap_obs, torch.int32), z(cap_obs, torch.int32)
    m = matcher.ORBMatcher()
    res = {k: torch.full((16,), 77, dtype=torch.int32, device=dev)
           for k in ("build", "problem", "jobs", "recover", "apply", "set_bias", "prior", "velocity", "build2", "refresh")}
    tab = {k: _up(torch, dev, v) for k, v in table.items()}
    kft_desc = matcher.KfTable.make(t["kf_pose_R"], t["kf_pose_t"], t["bad"], t["kps"], [_up(torch, dev, x) for x in kf_desc], t["n"])
    # ---- the window assembly with all key frames, and the one 32-byte read-back
    m.BuildObservationsDevice(dict(t, result=res["build"]), n_table, stride, cap, cap_obs, stream=st)
    caps = _caps(a["result"])
    sizes = _sizes(n_kf, caps["states"], caps["points"], caps["edges"])
    d = dict(t, result=res["problem"], work=z(cap + 2 * n_table, torch.int32))
    for k, dt in OUT_TYPES.items():
        d[k] = _up(torch, dev, np.full(max(sizes[PER.get(k, "edges")], 1) * WIDTH.get(k, 1), FILL[dt], dt))
    matcher.inertial_window_problem_device(m, t["kft"], d, stride, cap, cap_obs, n_kf, mp["n_src"], mp["cap_bank"], mp["n_priors"], mp["max_fixed"],
                                           caps["states"], caps["points"], caps["edges"], stream=st)
    head = res["problem"][:8].cpu().numpy()
    assert head.tobytes() == a["result"][:8].tobytes() and head[iw.W_REFUSED] == 0
    n_states, n_points, n_edges, n_solve = (int(v) for v in head[:4])
    assert n_states == n_solve == n_kf                                    # every point is local, no key frame is left over to be fixed
    # ---- this graph's job lists, the vertices, the information
    lists = dict(fixed=_up(torch, dev, np.full(n_kf + 1, 0xF7, np.uint8)), init=_up(torch, dev, np.full(3 * (n_kf + 1), -9, np.int32)),
                 edges=_up(torch, dev, np.full(4 * (n_kf - 1), -9, np.int32)), recover=_up(torch, dev, np.full(3 * n_kf, -9, np.int32)),
                 prior_rec=_up(torch, dev, np.full(1, -9, np.int32)))
    full_inertial.jobs_device(d["init_jobs"], d["inertial_edges"], d["recover_jobs"], n_kf, True, mp["n_src"], mp["cap_bank"], lists["fixed"], lists["init"],
                              lists["edges"], lists["recover"], lists["prior_rec"], res["jobs"], stream=st)
    src = _up(torch, dev, mp["src"])
    be = _assembled_full(torch, dev, cm, d, lists, src, st)
    # ---- the caller's loop
    t0 = time.perf_counter()
    r = fl.run(name, be)
    r["seconds"], r["n_trials"] = time.perf_counter() - t0, be.n_trials
    # ---- the tail
    i, w = be.d, be.w
    bias, est_R, est_t = z(6 * n_kf, torch.float32), z(9 * n_kf, torch.float64), z(3 * n_kf, torch.float64)
    outlier = z(max(caps["edges"], 1), torch.uint8)                       # this optimiser classifies nothing
    priors = _up(torch, dev, mp["priors"])
    cal = _calib(fs["cal"])
    full_inertial.recover_device(i.graph, cal, fs["bias_state"], lists["recover"], n_kf, src, mp["n_src"], bias, res["recover"], d_pose_R=est_R, d_pose_t=est_t,
                                 stream=st)
    matcher.local_ba_apply_device(m, dict(t, pose_kf=d["state_kf"], point_row=d["point_row"], edge_off=d["edge_off"], edge_kf=d["edge_kf"], edge_kp=d["edge_kp"],
                                          est_pose_R=est_R, est_pose_t=est_t, est_points=be.pts[be.cur], outlier=outlier, result=res["apply"]),
                                  n_table, stride, cap, cap_obs, n_solve, n_points, n_edges, stream=st)
    imu.set_bias_device(cal, i.bank, i.pool, i.cap, i.cap_meas, d["bias_ids"], bias, n_kf, res["set_bias"], stream=st)
    imu.prior_information_device(priors, mp["n_priors"], i.bank, i.cap, d["prior_info_jobs"], n_kf - 1, res["prior"], d_src=src, n_src=mp["n_src"], stream=st)
    matcher.inertial_window_velocity_prior_device(m, dict(priors=priors, src=src, recover_jobs=d["recover_jobs"], prior_jobs=d["prior_jobs"], result=res["velocity"]),
                                                  mp["n_priors"], mp["n_src"], stream=st)
    m.BuildObservationsDevice(dict(t, result=res["build2"]), n_table, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft_desc, dict(t, **tab, sel=d["point_row"], result=res["refresh"]), n_points, cap, cap_obs, float(rm.MAX_SCALE_FACTOR), stream=st)
    torch.cuda.synchronize()                                              # the one wait behind the loop
    be.finish()
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    held = dict(slots=g(t["slots"]), valid=g(t["valid"]), ref_kf=g(t["ref_kf"]), points=g(t["points"]), pose_R=g(t["kf_pose_R"]), pose_t=g(t["kf_pose_t"]),
                src=g(src), bias=g(bias), est_pose_R=g(est_R), est_pose_t=g(est_t), bank=g(i.bank), pool=g(i.pool), priors=g(priors), obs_off=g(t["obs_off"]),
                obs_kf=g(t["obs_kf"]), outlier=g(outlier), kf_desc=kf_desc, table=table, **{"list " + k: g(v) for k, v in lists.items()},
                **{k: g(v) for k, v in tab.items()}, **{"result " + k: g(v)[:8] for k, v in res.items()})
    return held, r


@pytest.mark.parametrize("name", list(fl.CHAIN_SCENES))
def test_the_whole_step_on_a_device_resident_map(name):
    """build -> the window assembly with ALL key frames -> one 32-byte read-back -> orbfi_jobs_device -> orbi_graph_init_device ->
    orbi_edge_information_device -> the caller's loop (a few iterations over device arrays) -> orbfi_recover_device ->
    orbm_local_ba_apply_device with an all-zero d_outlier -> orbi_set_bias_device -> orbi_prior_information_device -> the velocity prior ->
    build -> orbm_refresh_points_device, on one stream with one wait at the end besides the loop's scalars; 6 key frames and 65 / 1025
    points, the sizes of tests/test_imu_init_gpu.py's whole step.  Against the model chain: the job lists byte for byte, the loop by the
    rules of the tests above, and everything the tail writes -- the key-frame table, the state rows, the records and their biases, the prior
    slots and the point table -- equal to the model tail applied to the device's own estimate, byte for byte."""
    import torch
    import observations_model as om
    import refresh_model as rm
    cm = fl.chain_map(name)
    mp, csr, a, fs, jobs = cm["map"], cm["csr"], cm["a"], cm["fs"], cm["jobs"]
    n_kf = fl.CHAIN_KF
    held, dev = _chain(torch, torch.device("cuda", 0), name)
    # ---- the job lists, from the device's own assembly
    print("jobs", held["result jobs"].tolist(), jobs["result"].tolist())
    assert held["result jobs"].tobytes() == jobs["result"].tobytes()
    for k, want in (("fixed", jobs["fixed"]), ("init", jobs["init"]), ("edges", jobs["edges"]), ("recover", jobs["recover"]), ("prior_rec", jobs["prior_rec"])):
        assert held["list " + k].tobytes() == np.ascontiguousarray(want).tobytes(), k
    # ---- the loop: decisions, every trial's read-backs, the estimate, the counters, what is fixed
    _compare(name, dev)
    assert dev["rounds"][0]["accepted"] >= 3 and dev["refused"] == 0
    # ---- the tail: the models on the device's own estimate, byte for byte
    est = dev["estimate"]
    want = fl.chain_tail(cm, est, [r.copy() for r in fs["recs"]])
    for k, v in want["results"].items():
        key = dict(recover="recover", apply="apply", set_bias="set_bias", prior_information="prior", velocity_prior="velocity")[k]
        print(k, held["result " + key].tolist(), np.asarray(v).tolist())
        assert held["result " + key].tobytes() == np.asarray(v, np.int32)[:8].tobytes(), k
    assert not held["outlier"].any()
    for k in ("slots", "valid", "ref_kf", "points", "pose_R", "pose_t", "src", "bias", "est_pose_R", "est_pose_t"):
        assert held[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    bank, pool = want["bank"].pack()
    assert held["bank"].tobytes() == bank.tobytes() and held["pool"].tobytes() == pool.tobytes()
    assert held["priors"].tobytes() == want["priors"].tobytes()
    assert want["results"]["recover"][0] == n_kf and want["results"]["apply"][7] == n_kf and want["results"]["apply"][4] == len(a["point_row"])
    assert want["results"]["set_bias"][0] == n_kf and want["results"]["prior_information"][0] == n_kf - 1
    # ---- what the step changed: every key frame behind the fixed first one moved, every point moved, and every record holds the ONE bias
    w = mp["window"]
    moved = [(want["pose_R"][k] != mp["pose_R"][k]).any() or (want["pose_t"][k] != mp["pose_t"][k]).any() for k in w]
    assert all(moved[1:]) and (want["points"][a["point_row"]] != mp["points"][a["point_row"]]).any(1).all()
    one = np.concatenate([est["bg"][n_kf], est["ba"][n_kf]]).astype(np.float32)
    assert (held["bias"].reshape(n_kf, 6) == one).all() and one.tobytes() != fs["recs"][fs["prior_rec"]].updated_bias.tobytes()
    for rec in a["bias_ids"]:
        assert want["bank"].recs[rec].updated_bias.tobytes() == one.tobytes(), rec
    before, after = mp["priors"], np.frombuffer(held["priors"].tobytes(), fm.PRIOR)
    oldest, row = int(a["prior_jobs"][0, 1]), int(a["recover_jobs"][0, 1])
    assert after[oldest]["velo_priori"].tobytes() == held["src"].reshape(-1, 15)[row, 12:15].tobytes()
    for s in range(1, n_kf):
        slot = int(a["prior_info_jobs"][s - 1, 0])
        assert after[slot]["gyro_info"].tobytes() != before[slot]["gyro_info"].tobytes() and after[slot]["bias_priori"].tobytes() == one.tobytes()
    # ---- the CSR rebuilt behind the tail is the applied map's, and the refresh of the points the model's on it
    off2, okf2, okp2, bres2 = om.build(mp["n"], mp["bad"], want["slots"], mp["stride"], want["valid"], mp["cap_points"], 1 << 30)
    assert held["obs_off"].tobytes() == off2.tobytes() and held["obs_kf"][:len(okf2)].tobytes() == okf2.tobytes()
    assert held["result build2"].tobytes() == bres2.tobytes()
    rs = dict(n=mp["n"], bad=mp["bad"], pose_R=want["pose_R"], pose_t=want["pose_t"], kps=mp["kps"], kf_desc=held["kf_desc"], points=want["points"],
              valid=want["valid"], obs_off=off2, obs_kf=okf2, obs_kp=okp2, ref_kf=want["ref_kf"], **held["table"])
    fresh = rm.refresh(rs, a["point_row"], mp["cap_points"])
    print("refresh", held["result refresh"].tolist(), fresh["result"].tolist())
    assert np.array_equal(held["result refresh"], fresh["result"]) and fresh["result"][0] == len(a["point_row"])
    assert np.array_equal(held["normals"].reshape(-1, 3), fresh["normals"])           # by value: -0 equals +0
    for k in ("min_dist", "max_dist"):
        assert held[k].view(np.uint32).tobytes() == fresh[k].view(np.uint32).tobytes(), k
    assert np.array_equal(held["desc"].reshape(-1, 32), fresh["desc"])
