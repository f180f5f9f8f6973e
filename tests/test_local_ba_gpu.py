"""Local bundle adjustment on the device-resident map on the MI355X (include/orbm.h, "Local bundle adjustment on the device-resident
map"; include/orbba.h, orbba_local_bundle_adjustment_device): the assembly and the apply against the array model of
tests/local_ba_model.py byte for byte (integers and exact conversions only), the device form of the LM against the host entry point bit
for bit (same kernels, same order, same index arrays), and the chain build -> assemble -> LM -> apply -> build -> refresh -> cull."""
import numpy as np
import pytest

import local_ba_model as lm
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401 (GUARD: the padding _padded puts around every array)
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
SLACK = 5                                # capacity beyond the counts
OUT_TYPES = dict(pose_R=np.float64, pose_t=np.float64, pose_fixed=np.uint8, ba_points=np.float64, edge_pose=np.int32, edge_point=np.int32,
                 edge_z=np.float64, edge_inv_sigma2=np.float64, edge_kf=np.int32, edge_kp=np.int32, edge_off=np.int32, point_row=np.int32,
                 pose_kf=np.int32)
WIDTH = dict(pose_R=9, pose_t=3, ba_points=3, edge_z=2)
PER = dict(pose_R="poses", pose_t="poses", pose_fixed="poses", pose_kf="poses", ba_points="points", point_row="points", edge_off="points+1")


def _scene(name, cam=lm.PINHOLE):
    """(scene, fresh CSR, model problem): computed once, shared, never changed"""
    key = (name, cam)
    if key not in _cache:
        sc = lm.make_scene(cam=cam, **lm.SCENES[name])
        csr = lm.fresh_csr(sc)
        _cache[key] = (sc, csr, lm.problem(sc, csr))
    return _cache[key]


def _table(torch, dev, sc, csr):
    """the map as a caller holds it on the device"""
    from monoorbslam3_amd.matcher import KfTable
    d = dict(slots=_up(torch, dev, sc["slots"]), valid=_up(torch, dev, sc["valid"]), points=_up(torch, dev, sc["points"]),
             ref_kf=_up(torch, dev, sc["ref_kf"]), n=_up(torch, dev, sc["n"]), bad=_up(torch, dev, sc["bad"]),
             kf_pose_R=_up(torch, dev, sc["pose_R"]), kf_pose_t=_up(torch, dev, sc["pose_t"]), obs_off=_up(torch, dev, csr[0]),
             obs_kf=_up(torch, dev, np.concatenate([csr[1], np.zeros(1, np.int32)])), obs_kp=_up(torch, dev, np.concatenate([csr[2], np.zeros(1, np.int32)])),
             local=_up(torch, dev, sc["local"]))
    d["kps"] = [_up(torch, dev, k) for k in sc["kps"]]
    d["kft"] = KfTable.make(d["kf_pose_R"], d["kf_pose_t"], d["bad"], d["kps"], d["kps"], d["n"])   # descriptors are not read here
    return d


def _caps(counts, cut=None):
    caps = dict(poses=int(counts[lm.P_POSES]) + SLACK, points=int(counts[lm.P_POINTS]) + SLACK, edges=int(counts[lm.P_EDGES]) + SLACK)
    if cut:
        caps[cut] -= SLACK + 1
    return caps


def _assemble(torch, dev, sc, csr, t, caps, stream_kind):
    """one orbm_local_ba_problem_device on padded outputs -> (the arrays on the device, d_result as numpy)"""
    from monoorbslam3_amd import matcher
    sizes = {"poses": caps["poses"], "points": caps["points"], "points+1": caps["points"] + 1, "edges": caps["edges"]}
    pads = {}
    for k, dt in OUT_TYPES.items():
        n = sizes[PER.get(k, "edges")] * WIDTH.get(k, 1)
        fill = 91 if dt == np.uint8 else -91
        pads[k] = _padded(torch, dev, np.full(n, fill, dt), 17)
    pads["result"] = _padded(torch, dev, np.full(16, 77, np.int32), 17)
    pads["work"] = _padded(torch, dev, np.full(sc["cap_points"] + len(sc["n"]), -5, np.int32), 17)
    d = dict(t, **{k: v[1] for k, v in pads.items()})
    st = _stream(torch, dev, stream_kind)
    matcher.local_ba_problem_device(matcher.ORBMatcher(), t["kft"], d, sc["stride"], sc["cap_points"], len(csr[1]), len(sc["local"]),
                                    sc["first_kf"], caps["poses"], caps["points"], caps["edges"], stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], 17), k
    return d, d["result"].cpu().numpy()


def _equals_model(d, want):
    res = want["result"]
    counts = {"poses": res[lm.P_POSES], "points": res[lm.P_POINTS], "points+1": res[lm.P_POINTS] + 1, "edges": res[lm.P_EDGES]}
    for k in OUT_TYPES:
        n = counts[PER.get(k, "edges")] * WIDTH.get(k, 1)
        got = d[k].cpu().numpy()[:n]
        assert got.tobytes() == np.ascontiguousarray(want[k]).reshape(-1).tobytes(), k


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_the_assembly_equals_the_model(name, stream_kind):
    """8 key frames of 96 slots, 200 table rows, about 150 points and 500 edges; d_local with a bad, an out-of-range and a duplicate
    entry; first_kf local / not local; a row twice in a key frame, invalid rows, d_n > stride.  Every output array up to its count and
    d_result byte for byte, guards intact, a second run the same bytes; then the same map behind a CSR that is stale and spoilt."""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, want = _scene(name)
    t = _table(torch, dev, sc, csr)
    d, res = _assemble(torch, dev, sc, csr, t, _caps(want["result"]), stream_kind)
    print("device d_result %s, model %s" % (res.tolist(), want["result"].tolist()))
    assert res.tobytes() == want["result"].tobytes()
    _equals_model(d, want)
    again, res2 = _assemble(torch, dev, sc, csr, t, _caps(want["result"]), stream_kind)
    assert res2.tobytes() == res.tobytes()
    for k in OUT_TYPES:
        assert again[k].cpu().numpy().tobytes() == d[k].cpu().numpy().tobytes(), k
    for key in ("slots", "valid", "points"):                              # inputs as passed
        assert t[key].cpu().numpy().tobytes() == np.ascontiguousarray(sc[key]).tobytes(), key
    stale, spoilt, junk = lm.stale_scene(sc, csr)
    want2 = lm.problem(stale, spoilt)
    assert want2["result"][lm.P_NO_EDGE] == 1 and want2["result"][lm.P_CSR_DROPPED] == junk
    d2, res2 = _assemble(torch, dev, stale, spoilt, _table(torch, dev, stale, spoilt), _caps(want2["result"]), stream_kind)
    assert res2.tobytes() == want2["result"].tobytes()
    _equals_model(d2, want2)


@pytest.mark.parametrize("cut", ["poses", "points", "edges", "no_free_pose"])
def test_a_refused_assembly_keeps_the_full_counts_and_its_capacities(cut):
    """one capacity one below the count, or first_kf as the only local key frame: d_result equals the model's, full counts included,
    and the guards behind every array cut to its capacity are intact"""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, full = _scene("first_local")
    if cut == "no_free_pose":
        sc = dict(sc, local=np.array([sc["first_kf"], -4], np.int32))
        want = lm.problem(sc, csr)
        caps = _caps(want["result"])
        assert want["result"][lm.P_REFUSED] == lm.REFUSE_NO_FREE_POSE
    else:
        caps = _caps(full["result"], cut)
        want = lm.problem(sc, csr, cap_poses=caps["poses"], cap_local_points=caps["points"], cap_edges=caps["edges"])
        assert want["result"][lm.P_REFUSED] in (lm.REFUSE_POSES, lm.REFUSE_POINTS, lm.REFUSE_EDGES) and (want["result"][:5] == full["result"][:5]).all()
    _, res = _assemble(torch, dev, sc, csr, _table(torch, dev, sc, csr), caps, "explicit")
    print("device d_result %s, model %s" % (res.tolist(), want["result"].tolist()))
    assert res.tobytes() == want["result"].tobytes()


def _download(d, res):
    """the assembled problem as numpy arrays cut to the counts"""
    counts = {"poses": res[lm.P_POSES], "points": res[lm.P_POINTS], "points+1": res[lm.P_POINTS] + 1, "edges": res[lm.P_EDGES]}
    return {k: d[k].cpu().numpy()[:counts[PER.get(k, "edges")] * WIDTH.get(k, 1)].copy() for k in OUT_TYPES}


def _lm_outputs(torch, dev, n_poses, n_points, n_edges):
    z = lambda n, dt, fill: torch.full((n,), fill, dtype=dt, device=dev)  # noqa: E731
    return dict(est_pose_R=z(n_poses * 9, torch.float64, -3.0), est_pose_t=z(n_poses * 3, torch.float64, -3.0),
                est_points=z(n_points * 3, torch.float64, -3.0), chi2=z(n_edges, torch.float64, -3.0), outlier=z(n_edges, torch.uint8, 9))


def _host_ba(cam, prob_arrays):
    from monoorbslam3_amd import ba
    p = prob_arrays
    return ba.local_bundle_adjustment(cam, p["pose_R"], p["pose_t"], p["pose_fixed"], p["ba_points"], p["edge_pose"], p["edge_point"],
                                      p["edge_z"], p["edge_inv_sigma2"])


def _bits_equal(dev_out, info, host):
    g = lambda k: dev_out[k].cpu().numpy()  # noqa: E731
    assert g("est_pose_R").tobytes() == host["pose_R"].tobytes() and g("est_pose_t").tobytes() == host["pose_t"].tobytes()
    assert g("est_points").tobytes() == host["points"].tobytes() and g("chi2").tobytes() == host["chi2"].tobytes()
    assert np.array_equal(g("outlier"), host["outlier"].astype(np.uint8))
    assert (info["iterations"], info["trials"]) == (host["iterations"], host["trials"])
    assert np.float64(info["lam"]).tobytes() == np.float64(host["lam"]).tobytes()
    assert np.float64(info["chi2_initial"]).tobytes() == np.float64(host["chi2_initial"]).tobytes()
    assert np.float64(info["chi2_final"]).tobytes() == np.float64(host["chi2_final"]).tobytes()


@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
def test_the_device_lm_equals_the_host_entry_point_bit_for_bit(model, chol):
    """the assembled problem downloaded and given to orbba_local_bundle_adjustment: poses, points, chi2, outlier, iterations, trials,
    lambda and both chi2 sums of orbba_local_bundle_adjustment_device equal it BIT FOR BIT -- the same kernels in the same order on
    index arrays that the device built and the host built.  No tolerance: a difference is a bug in the index structures."""
    import torch
    from monoorbslam3_amd import ba
    dev = torch.device("cuda", 0)
    cam = lm.PINHOLE if model == "pinhole" else lm.FISHEYE
    sc, csr, want = _scene("first_local", cam)
    d, res = _assemble(torch, dev, sc, csr, _table(torch, dev, sc, csr), _caps(want["result"]), "explicit")
    assert res.tobytes() == want["result"].tobytes() and res[lm.P_REFUSED] == 0
    n_poses, n_points, n_edges = (int(v) for v in res[:3])
    ba.set_variant("chol", chol)
    try:
        host = _host_ba(cam, _download(d, res))
        out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
        info = ba.local_bundle_adjustment_device(cam, dict(d, **out), n_poses, n_points, n_edges)
        torch.cuda.synchronize()
    finally:
        ba.set_variant("chol", "lds")
    print("iterations %d trials %d lambda %.6g chi2 %.6g -> %.6g outliers %d" % (info["iterations"], info["trials"], info["lam"],
                                                                               info["chi2_initial"], info["chi2_final"], int(host["outlier"].sum())))
    assert host["outlier"].sum() >= 3 and info["iterations"] >= 3
    _bits_equal(out, info, host)


@pytest.mark.parametrize("chol", ["lds", "global"])
def test_the_device_lm_equals_the_host_entry_point_where_trials_are_rejected(chol):
    """the scene of tests/test_ba_lm_paths.py whose first round rejects a trial (admitted there on the CPU, and the host form held against
    the oracle): push(), pop() and the lambda schedule on the index arrays the device built -- bit for bit again, counts and lambda included"""
    import torch
    from monoorbslam3_amd import ba
    from test_ba_lm_paths import _local_ba_args, _local_ba_oracle
    dev = torch.device("cuda", 0)
    cam, R, t, fixed, P, ep, el, z, w = _local_ba_args()
    prob = dict(pose_R=np.ascontiguousarray(R, np.float64).reshape(-1, 9), pose_t=np.ascontiguousarray(t, np.float64),
                pose_fixed=np.ascontiguousarray(fixed, np.uint8), ba_points=np.ascontiguousarray(P, np.float64),
                edge_pose=np.ascontiguousarray(ep, np.int32), edge_point=np.ascontiguousarray(el, np.int32),
                edge_z=np.ascontiguousarray(z, np.float64), edge_inv_sigma2=np.ascontiguousarray(w, np.float64))
    n_poses, n_points, n_edges = len(prob["pose_t"]), len(prob["ba_points"]), len(prob["edge_pose"])
    ba.set_variant("chol", chol)
    try:
        host = _host_ba(cam, prob)
        out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
        info = ba.local_bundle_adjustment_device(cam, dict({k: _up(torch, dev, v) for k, v in prob.items()}, **out), n_poses, n_points, n_edges)
        torch.cuda.synchronize()
    finally:
        ba.set_variant("chol", "lds")
    ref = _local_ba_oracle()
    print("iterations %d trials %d lambda %.6g chi2 %.6g -> %.6g outliers %d" % (info["iterations"], info["trials"], info["lam"],
                                                                               info["chi2_initial"], info["chi2_final"], int(host["outlier"].sum())))
    assert info["trials"] > info["iterations"] and info["trials"] == ref["first_round"]["trials"] + ref["trials"]
    assert np.array_equal(host["outlier"], ref["outlier"])
    _bits_equal(out, info, host)


def test_the_device_lm_refuses_what_the_host_form_refuses():
    """a key frame observing a point twice, and an edge index out of range: ORBX_E_ARG, found on the device, outputs as passed"""
    import torch
    from monoorbslam3_amd import _lib, ba
    dev = torch.device("cuda", 0)
    sc, csr, want = _scene("first_local")
    n_poses, n_points, n_edges = (int(v) for v in want["result"][:3])
    free = int(np.flatnonzero(want["pose_fixed"] == 0)[0])
    x = next(x for x in range(n_points) if want["edge_off"][x + 1] - want["edge_off"][x] >= 2)
    twice = want["edge_pose"].copy()
    twice[want["edge_off"][x]:want["edge_off"][x] + 2] = free
    beyond = want["edge_pose"].copy()
    beyond[n_edges // 2] = n_poses
    for edge_pose in (twice, beyond):
        d = {k: _up(torch, dev, want[k]) for k in ("pose_R", "pose_t", "pose_fixed", "ba_points", "edge_point", "edge_z", "edge_inv_sigma2")}
        d["edge_pose"] = _up(torch, dev, edge_pose)
        out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
        before = {k: v.cpu().numpy().copy() for k, v in out.items()}
        with pytest.raises(_lib.OrbxError) as err:
            ba.local_bundle_adjustment_device(lm.PINHOLE, dict(d, **out), n_poses, n_points, n_edges)
        torch.cuda.synchronize()
        print(err.value)
        with pytest.raises(_lib.OrbxError):
            ba.local_bundle_adjustment(lm.PINHOLE, want["pose_R"], want["pose_t"], want["pose_fixed"], want["ba_points"], edge_pose,
                                       want["edge_point"], want["edge_z"], want["edge_inv_sigma2"])
        for k, v in out.items():
            assert v.cpu().numpy().tobytes() == before[k].tobytes(), k


IN_OUT = ("slots", "valid", "ref_kf", "points", "kf_pose_R", "kf_pose_t")


def _apply(torch, dev, sc, csr, prob, est, stream_kind):
    from monoorbslam3_amd import matcher
    start = dict(slots=sc["slots"], valid=sc["valid"], ref_kf=sc["ref_kf"], points=sc["points"], kf_pose_R=sc["pose_R"], kf_pose_t=sc["pose_t"],
                 n=sc["n"], bad=sc["bad"], obs_off=csr[0], obs_kf=csr[1], obs_kp=csr[2], pose_kf=prob["pose_kf"], point_row=prob["point_row"],
                 edge_off=prob["edge_off"], edge_kf=prob["edge_kf"], edge_kp=prob["edge_kp"], est_pose_R=est[0], est_pose_t=est[1],
                 est_points=est[2], outlier=est[3], result=np.full(8, 64, np.int32))
    pads = {k: _padded(torch, dev, v, 23) for k, v in start.items()}
    d = {k: v[1] for k, v in pads.items()}
    st = _stream(torch, dev, stream_kind)
    res = prob["result"]
    matcher.local_ba_apply_device(matcher.ORBMatcher(), d, len(sc["n"]), sc["stride"], sc["cap_points"], len(csr[1]), int(res[lm.P_LOCAL]),
                                  int(res[lm.P_POINTS]), int(res[lm.P_EDGES]), stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], 23), k
    return {k: v.cpu().numpy() for k, v in d.items()}, start


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_the_apply_equals_the_model(name, stream_kind):
    """the model fed the DEVICE LM's outputs: slots, validity, reference key frames, positions, key-frame poses and d_result byte for
    byte, inputs as passed, guards intact; the outliers move a reference key frame, send points bad with their cascade, and one finds
    its point bad.  Then with a spoilt CSR and maps holding indices out of range: dropped and counted."""
    import torch
    from monoorbslam3_amd import ba
    dev = torch.device("cuda", 0)
    sc, csr, prob = _scene(name)
    n_poses, n_points, n_edges = (int(v) for v in prob["result"][:3])
    out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
    ba.local_bundle_adjustment_device(sc["cam"], dict({k: _up(torch, dev, prob[k]) for k in OUT_TYPES}, **out), n_poses, n_points, n_edges)
    est = tuple(out[k].cpu().numpy() for k in ("est_pose_R", "est_pose_t", "est_points", "outlier"))
    est = (est[0].reshape(-1, 9), est[1].reshape(-1, 3), est[2].reshape(-1, 3), est[3])
    want = lm.apply(sc, csr, prob, *est)
    assert want["result"][lm.A_MOVED] >= 1 and want["result"][lm.A_POINTS_BAD] >= 2 and want["result"][lm.A_CLEARED] >= 4 and want["found_bad"] >= 1
    got, start = _apply(torch, dev, sc, csr, prob, est, stream_kind)
    print("device d_result %s, model %s" % (got["result"].tolist(), want["result"].tolist()))

    def check(got, start, want):
        assert got["result"].tobytes() == want["result"].tobytes()
        for key, mk in zip(IN_OUT, ("slots", "valid", "ref_kf", "points", "pose_R", "pose_t")):
            assert got[key].tobytes() == np.ascontiguousarray(want[mk]).tobytes(), key
        for key in start:
            if key not in IN_OUT + ("result",):
                assert got[key].tobytes() == np.ascontiguousarray(start[key]).tobytes(), key
    check(got, start, want)
    stale, spoilt, junk = lm.stale_scene(sc, csr)
    broken = dict(prob, point_row=prob["point_row"].copy(), edge_kf=prob["edge_kf"].copy(), edge_kp=prob["edge_kp"].copy(), pose_kf=prob["pose_kf"].copy())
    broken["point_row"][[3, 7]] = (-2, sc["cap_points"])
    outl = np.flatnonzero(est[3])
    broken["edge_kf"][outl[0]], broken["edge_kp"][outl[1]] = len(sc["n"]), sc["stride"] + 5
    broken["pose_kf"][1] = -1
    want = lm.apply(stale, spoilt, broken, *est)
    assert want["result"][lm.A_CSR_DROPPED] == junk and want["result"][lm.A_MAP_DROPPED] >= 4
    got, start = _apply(torch, dev, stale, spoilt, broken, est, stream_kind)
    check(got, start, want)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_mapper_chain_around_the_local_ba(stream_kind):
    """orbm_build_observations_device -> orbm_local_ba_problem_device -> (one 32-byte read-back) -> orbba_local_bundle_adjustment_device
    -> orbm_local_ba_apply_device -> build -> orbm_refresh_points_device (d_sel = d_point_row) -> orbm_cull_keyframes_device on one
    stream: every table equals the same chain done with the models and the host BA, and the slots and flags the refresh and the
    culling see are the applied ones."""
    import torch
    import observations_model as om
    import refresh_model as rm
    from monoorbslam3_amd import ba, matcher
    dev = torch.device("cuda", 0)
    sc, csr0, _ = _scene("first_fixed")
    rng = np.random.RandomState(90)
    cap, stride, n_kf = sc["cap_points"], sc["stride"], len(sc["n"])
    cap_obs = len(csr0[1]) + 40
    kf_desc = [rng.randint(0, 256, (stride + 8, 32)).astype(np.uint8) for _ in range(n_kf)]
    table = dict(normals=rng.uniform(-1, 1, (cap + 4, 3)).astype(np.float32), min_dist=rng.uniform(1, 2, cap + 4).astype(np.float32),
                 max_dist=rng.uniform(20, 30, cap + 4).astype(np.float32), desc=rng.randint(0, 256, (cap + 4, 32)).astype(np.uint8))
    roles = sc["roles"]
    recent = np.array([roles["fix"][0], roles["fix"][1], roles["conn"][0], roles["conn"][1], roles["conn"][2], roles["cur"]], np.int32)
    timestamps = np.arange(len(recent)) * 0.3
    kps = [np.concatenate([k, np.zeros(8, k.dtype)]) for k in sc["kps"]]      # d_n[cur] > stride: records exist for every feature
    # ---- the models and the host BA
    off, okf, okp, bres = om.build(sc["n"], sc["bad"], sc["slots"], stride, sc["valid"], cap, cap_obs)
    csr = (off, okf, okp)
    prob = lm.problem(sc, csr)
    host = _host_ba(sc["cam"], prob)
    est = (host["pose_R"].reshape(-1, 9), host["pose_t"], host["points"], host["outlier"].astype(np.uint8))
    applied = lm.apply(sc, csr, prob, *est)
    off2, okf2, okp2, bres2 = om.build(sc["n"], sc["bad"], applied["slots"], stride, applied["valid"], cap, cap_obs)
    rs = dict(n=sc["n"], bad=sc["bad"], pose_R=applied["pose_R"], pose_t=applied["pose_t"], kps=kps, kf_desc=kf_desc, points=applied["points"],
              valid=applied["valid"], obs_off=off2, obs_kf=okf2, obs_kp=okp2, ref_kf=applied["ref_kf"], **table)
    sel = np.full(cap, -1, np.int32)
    sel[:len(prob["point_row"])] = prob["point_row"]
    fresh = rm.refresh(rs, sel, cap)
    cs = dict(sc, kps=kps, slots=applied["slots"], valid=applied["valid"], ref_kf=applied["ref_kf"], recent=recent, timestamps=timestamps)
    culled = om.cull(cs, off2, okf2, okp2)
    assert applied["result"][lm.A_POINTS_BAD] >= 2 and fresh["result"][0] >= 100 and culled["result"][om.CULLED] + culled["result"][om.KEPT] >= 2
    # ---- the device chain
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    t = _table(torch, dev, dict(sc, kps=kps), (off, np.zeros(cap_obs, np.int32), np.zeros(cap_obs, np.int32)))
    t["obs_off"], t["obs_kf"], t["obs_kp"] = z(cap + 1, torch.int32), z(cap_obs, torch.int32), z(cap_obs, torch.int32)
    t["desc_kf"] = [_up(torch, dev, x) for x in kf_desc]
    kft = matcher.KfTable.make(t["kf_pose_R"], t["kf_pose_t"], t["bad"], t["kps"], t["desc_kf"], t["n"])
    caps = _caps(prob["result"])
    work = dict(work=z(cap + n_kf, torch.int32), pose_R=z(caps["poses"] * 9, torch.float64), pose_t=z(caps["poses"] * 3, torch.float64),
                pose_fixed=z(caps["poses"], torch.uint8), ba_points=z(caps["points"] * 3, torch.float64), edge_pose=z(caps["edges"], torch.int32),
                edge_point=z(caps["edges"], torch.int32), edge_z=z(caps["edges"] * 2, torch.float64), edge_inv_sigma2=z(caps["edges"], torch.float64),
                edge_kf=z(caps["edges"], torch.int32), edge_kp=z(caps["edges"], torch.int32), edge_off=z(caps["points"] + 1, torch.int32),
                point_row=torch.full((cap,), -1, dtype=torch.int32, device=dev), pose_kf=z(caps["poses"], torch.int32))
    res = {k: torch.full((16,), 77, dtype=torch.int32, device=dev) for k in ("build", "problem", "apply", "build2", "refresh", "cull")}
    tab = {k: _up(torch, dev, v) for k, v in table.items()}
    m = matcher.ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    m.BuildObservationsDevice(dict(t, result=res["build"]), n_kf, stride, cap, cap_obs, stream=st)
    n_obs = cap_obs                                                           # the CSR's arrays' length: the offsets bound the lists
    matcher.local_ba_problem_device(m, kft, dict(t, **work, result=res["problem"]), stride, cap, n_obs, len(sc["local"]), sc["first_kf"],
                                    caps["poses"], caps["points"], caps["edges"], stream=st)
    head = res["problem"][:8].cpu().numpy()                                   # the one 32-byte read-back
    assert head[lm.P_REFUSED] == 0
    n_poses, n_points, n_edges, n_local = (int(v) for v in head[:4])
    out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
    info = ba.local_bundle_adjustment_device(sc["cam"], dict(work, **out), n_poses, n_points, n_edges, stream=st)
    matcher.local_ba_apply_device(m, dict(t, **work, **out, result=res["apply"]), n_kf, stride, cap, n_obs, n_local, n_points, n_edges, stream=st)
    m.BuildObservationsDevice(dict(t, result=res["build2"]), n_kf, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft, dict(t, **tab, sel=work["point_row"], result=res["refresh"]), cap, cap, cap_obs, float(rm.MAX_SCALE_FACTOR), stream=st)
    code, num_mp, num_red = z(len(recent), torch.int32), z(len(recent), torch.int32), z(len(recent), torch.int32)
    m.CullKeyFramesDevice(kft, dict(t, code=code, num_mp=num_mp, num_redundant=num_red, result=res["cull"]), stride, cap, cap_obs, recent, timestamps,
                          first_kf=sc["first_kf"], stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    g = lambda x: x.cpu().numpy()  # noqa: E731
    print("problem %s apply %s refresh %s cull %s" % (g(res["problem"]).tolist(), g(res["apply"])[:8].tolist(), g(res["refresh"])[:8].tolist(),
                                                      g(res["cull"])[:8].tolist()))
    assert g(res["build"])[:8].tobytes() == bres.tobytes() and g(res["problem"]).tobytes() == prob["result"].tobytes()
    _bits_equal(out, info, host)
    assert g(res["apply"])[:8].tobytes() == applied["result"].tobytes() and g(res["build2"])[:8].tobytes() == bres2.tobytes()
    assert g(t["obs_off"]).tobytes() == off2.tobytes() and g(t["obs_kf"])[:len(okf2)].tobytes() == okf2.tobytes()
    assert np.array_equal(g(res["refresh"])[:8], fresh["result"])
    assert np.array_equal(g(tab["normals"]), fresh["normals"])                # by value: -0 equals +0
    for key in ("min_dist", "max_dist"):
        assert g(tab[key]).view(np.uint32).tobytes() == fresh[key].view(np.uint32).tobytes(), key
    assert np.array_equal(g(tab["desc"]), fresh["desc"])
    assert g(res["cull"])[:8].tobytes() == culled["result"].tobytes() and np.array_equal(g(code), culled["code"])
    for key, mk in (("slots", "slots"), ("valid", "valid"), ("ref_kf", "ref_kf"), ("bad", "bad")):
        assert g(t[key]).tobytes() == np.ascontiguousarray(culled[mk]).tobytes(), key
    assert g(t["points"]).tobytes() == applied["points"].tobytes() and g(t["kf_pose_R"]).tobytes() == applied["pose_R"].tobytes()
    assert g(t["kf_pose_t"]).tobytes() == applied["pose_t"].tobytes()
