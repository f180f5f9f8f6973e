"""The tracker's local map on the MI355X (include/orbm.h, "The tracker's local map on the device") against the array model of
tests/local_map_model.py, byte for byte: integers only, so no tolerance and no exclusion."""
import numpy as np
import pytest

import local_map_model as lm
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401 (GUARD: the padding _padded puts around every array)
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
REF0 = -7                                 # *d_ref before every call
FILL = dict(local_kf=-21, rows=-23, local_mask=91, result=31, work=32, count=33)
GUARDS = dict(frame_mp=-20, local_kf=-22, rows=-24, local_mask=92, ref=-25, result=-26, work=-27, count=-28)
SLACK = 3                                 # capacity beyond the model's counts
WORLD_KEYS = ("n", "bad", "slots", "valid", "obs_off", "obs_kf", "obs_kp")


def cached(key, make):
    """a scene, a world or a model output made once, shared, never changed"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _device_graph(torch, dev, g):
    """the model's lists and parents in padded device arrays -> (CovisGraph, pads); d_weight, which these calls do not read, is zeros"""
    from monoorbslam3_amd.matcher import CovisGraph
    cap = g["cap_kf"]
    pads = {k: _padded(torch, dev, g[k], -12) for k in ("ord_kf", "ord_n", "parent")}
    weight = torch.zeros(cap * cap, dtype=torch.int32, device=dev)
    return CovisGraph.make(weight, *(pads[k][1] for k in ("ord_kf", "ord_n", "parent"))), pads


def _device_world(torch, dev, w):
    t = {k: _up(torch, dev, w[k]) for k in WORLD_KEYS}
    if len(w["obs_kf"]) == 0:                                                     # a pointer even where there is no observation
        t["obs_kf"] = t["obs_kp"] = torch.zeros(1, dtype=torch.int32, device=dev)
    graph, gpads = _device_graph(torch, dev, w["g"])
    return t, graph, gpads


def _world_untouched(w, t, gpads):
    for k in WORLD_KEYS:
        if len(w[k]):
            assert t[k].cpu().numpy().tobytes() == np.ascontiguousarray(w[k]).tobytes(), k
    for k, (whole, mid) in gpads.items():
        assert _guards_intact(whole, -12) and mid.cpu().numpy().tobytes() == np.ascontiguousarray(w["g"][k]).tobytes(), k


def _local_map(torch, dev, m, w, t, graph, call, cap_local_kf, cap_rows, stream_kind, min_obs=3):
    """orbm_local_map_device and, behind it on the same stream with no read-back, orbm_num_tracked_points_device on the d_ref it left;
    every output in a padded array; -> what the calls wrote, as numpy arrays"""
    cap = w["cap_points"]
    fm = np.ascontiguousarray(call["frame_mp"], np.int32)
    pads = dict(frame_mp=_padded(torch, dev, fm, GUARDS["frame_mp"]), ref=_padded(torch, dev, np.full(1, REF0, np.int32), GUARDS["ref"]),
                local_kf=_padded(torch, dev, np.full(cap_local_kf, FILL["local_kf"], np.int32), GUARDS["local_kf"]),
                rows=_padded(torch, dev, np.full(cap_rows, FILL["rows"], np.int32), GUARDS["rows"]),
                local_mask=_padded(torch, dev, np.full(cap, FILL["local_mask"], np.uint8), GUARDS["local_mask"]),
                result=_padded(torch, dev, np.full(16, FILL["result"], np.int32), GUARDS["result"]),
                work=_padded(torch, dev, np.full(cap + w["n_kf"], FILL["work"], np.int32), GUARDS["work"]),
                count=_padded(torch, dev, np.full(4, FILL["count"], np.int32), GUARDS["count"]))
    d = dict(t, **{k: v[1] for k, v in pads.items()})
    st = _stream(torch, dev, stream_kind)
    m.LocalMapDevice(graph, d, len(fm), w["n_kf"], w["stride"], cap, len(w["obs_kf"]), call["recent"], cap_local_kf, cap_rows,
                     n_neigh=call.get("n_neigh", lm.N_NEIGH), max_kf=call.get("max_kf", lm.MAX_KF), stream=st)
    m.NumTrackedPointsDevice(d, w["n_kf"], w["stride"], cap, len(w["obs_kf"]), min_obs, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k, fill in GUARDS.items():
        assert _guards_intact(pads[k][0], fill), k
    return {k: v[1].cpu().numpy() for k, v in pads.items()}


def _equals_model(w, got, want, cap_local_kf, cap_rows, min_obs=3):
    """every output and every d_result entry; on a refusal the full counts, an all-zero mask, d_ref as passed, and nothing at or past a
    capacity (the arrays end there: the guards were compared).  d_count against the model on the d_ref the call left."""
    res = want["result"]
    assert got["result"].tobytes() == res.tobytes(), (got["result"].tolist(), res.tolist())
    assert got["frame_mp"].tobytes() == want["frame_mp"].tobytes()
    assert got["local_mask"].tobytes() == want["mask"].tobytes() and int(got["ref"][0]) == want["ref"]
    if res[lm.R_REFUSED]:
        assert not got["local_mask"].any() and int(got["ref"][0]) == REF0
        assert res[lm.R_KF] == len(want["local_kf"]) and res[lm.R_ROWS] == len(want["rows"])
    else:
        for key in ("local_kf", "rows"):
            n = len(want[key])
            assert got[key][:n].tobytes() == want[key].tobytes() and (got[key][n:] == FILL[key]).all(), key
    assert got["count"].tobytes() == lm.num_tracked(w, want["ref"], min_obs).tobytes()


def _caps(call, want):
    return call.get("cap_local_kf", len(want["local_kf"]) + SLACK), call.get("cap_rows", len(want["rows"]) + SLACK)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_every_call_of_a_tagged_scene_equals_the_model(name, stream_kind):
    """40 key frames x 32 slots over 600 rows, 120 x 96 over 2400: every call of the scene (66: frames without a match, with five and
    with 22 / 120 matched rows, among them bad rows and rows named twice; no recent key frame, one, ten; n_neigh 0, 1, 10; max_kf 80, 0, 1
    and the ones that meet the limit exactly; each capacity one short) -- the cases tests/local_map_model.py's check_scene asserts.  Every
    output and every d_result entry equals the model's, d_count of orbm_num_tracked_points_device on the d_ref just left too (no vote:
    d_ref stays -7 and the flag is set); the map, the CSR and the graph are as passed; guards intact; a second run gives the same bytes."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    sc = cached(("scene", name), lambda: lm.make_scene(name))
    lm.check_scene(sc)
    w = sc["world"]
    t, graph, gpads = _device_world(torch, dev, w)
    m = ORBMatcher()
    print(name, "d_result sums", np.stack([o["result"] for o in sc["outs"]]).sum(0).tolist())
    for call, want in zip(sc["calls"], sc["outs"]):
        caps = _caps(call, want)
        runs = [_local_map(torch, dev, m, w, t, graph, call, *caps, stream_kind) for _ in range(2)]
        _equals_model(w, runs[0], want, *caps)
        for k in runs[0]:
            if k != "work":                                                       # a work array's contents after a call are unspecified
                assert runs[1][k].tobytes() == runs[0][k].tobytes(), k
    _world_untouched(w, t, gpads)


# n_kf: 1, 2, around the wave (the child ballot), past one pass of the workgroup over the votes, the full pitch; n2: 0, 1, around the
# workgroup; n_recent 0, 1, 32; max_kf 0, 1, 80 (300 at the full pitch) with a list that reaches it where `end` says so; then strides with
# which the point pass crosses a 1024-slot tile inside a key frame (1500, 2049) and exactly between two (1024)
SIZES = [dict(n_kf=1, n2=0, stride=16, cap=40, matched=0, n_recent=0, max_kf=80, end=lm.END_RAN_OUT),
         dict(n_kf=1, n2=1, stride=16, cap=40, matched=1, n_recent=1, max_kf=0, end=lm.END_SIZE_LIMIT),
         dict(n_kf=2, n2=1, stride=16, cap=40, matched=1, n_recent=1, max_kf=1, end=None),
         dict(n_kf=63, n2=1023, stride=32, cap=600, matched=40, n_recent=32, max_kf=80, end=None),
         dict(n_kf=64, n2=1024, stride=32, cap=600, matched=40, n_recent=0, max_kf=80, end=None),
         dict(n_kf=65, n2=1025, stride=32, cap=600, matched=60, n_recent=32, max_kf=1, end=lm.END_SIZE_LIMIT),
         dict(n_kf=200, n2=300, stride=64, cap=3000, matched=20, n_recent=10, max_kf=80, end=lm.END_SIZE_LIMIT, clean=True),
         dict(n_kf=1025, n2=1025, stride=24, cap=6000, matched=20, n_recent=10, max_kf=80, end=lm.END_SIZE_LIMIT, clean=True),
         dict(n_kf=4096, n2=1024, stride=16, cap=15000, matched=40, n_recent=32, max_kf=300, end=lm.END_SIZE_LIMIT, clean=True),
         dict(n_kf=6, n2=64, stride=1500, cap=4000, matched=30, n_recent=2, max_kf=80, end=None),
         dict(n_kf=5, n2=64, stride=1024, cap=3000, matched=30, n_recent=2, max_kf=80, end=None),
         dict(n_kf=5, n2=64, stride=2049, cap=5000, matched=30, n_recent=2, max_kf=80, end=None)]


def _sized(cfg):
    n_kf = cfg["n_kf"]
    extra = dict(p_bad=0.02, p_stray=0.0) if cfg.get("clean") else {}              # parents that are list heads: the walk goes on
    if cfg["stride"] >= 1024:
        extra["p_full"] = 0.8
    w = lm.make_direct_world(n_kf, n_kf, cfg["stride"], cfg["cap"], 4096 if n_kf == 4096 else None, **extra)
    fm = lm.direct_frame(w, 3, cfg["n2"], cfg["matched"])
    if n_kf > 1024:                                                               # a vote for the last key frame
        last = np.flatnonzero((w["obs_kf"] == n_kf - 1) & (w["bad"][n_kf - 1] == 0))
        fm[0] = np.searchsorted(w["obs_off"], last[0], side="right") - 1
    call = dict(frame_mp=fm, max_kf=cfg["max_kf"],
                recent=np.random.RandomState(1).choice(n_kf, min(cfg["n_recent"], n_kf), replace=False).astype(np.int32))
    return w, call, lm.local_map(w, **call)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("cfg", SIZES, ids=lambda c: "kf%d-n2_%d-stride%d" % (c["n_kf"], c["n2"], c["stride"]))
def test_one_call_at_the_sizes_where_the_code_changes_path(cfg, stream_kind):
    """a world whose graph is written directly, one call: everything equals the model, a second run gives the same bytes"""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    w, call, want = cached(("size", cfg["n_kf"], cfg["n2"], cfg["stride"]), lambda: _sized(cfg))
    res = want["result"]
    print(cfg, "model d_result", res.tolist())
    assert cfg["end"] is None or res[lm.R_END] == cfg["end"]
    if cfg["n_kf"] > 1024:
        assert cfg["n_kf"] - 1 in want["local_kf"][:res[lm.R_VOTED] + cfg["n_recent"]]   # a vote past the workgroup's first pass
    if cfg["stride"] >= 1024:                                                      # full key frames in the list: the tiles are crossed
        assert (w["n"][want["local_kf"][:-1]] >= cfg["stride"]).any() and res[lm.R_ROWS] > 1024
    if cfg["n2"] > 0 and cfg["matched"]:
        assert 0 <= call["frame_mp"][-1] < cfg["cap"]                              # the frame's last slot takes part
    t, graph, gpads = _device_world(torch, dev, w)
    m = ORBMatcher()
    caps = _caps(call, want)
    runs = [_local_map(torch, dev, m, w, t, graph, call, *caps, stream_kind) for _ in range(2)]
    _equals_model(w, runs[0], want, *caps)
    for k in runs[0]:
        if k != "work":
            assert runs[1][k].tobytes() == runs[0][k].tobytes(), k
    _world_untouched(w, t, gpads)


def _garbage_world():
    """the small scene's world with what the distrust rules are for: list lengths negative and over n_kf, list entries and parents out
    of range, CSR offsets descending and past n_obs.  Inputs the header defines, not attempts to provoke a fault."""
    w = lm.make_scene("small")["world"]
    n_kf, rng = w["n_kf"], np.random.RandomState(77)
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w["g"].items()}
    g["ord_kf"][g["ord_kf"] == lm.gm.LIST_FILL] = n_kf + 9                         # what lies past every list
    g["ord_n"][[3, 11]] = -4
    g["ord_n"][[5, 18, 30]] = n_kf + 50
    g["ord_n"][[6, 19]] = 1 << 30
    for k in rng.choice(n_kf, 12, replace=False):
        g["ord_kf"][k, rng.randint(0, 4)] = (-1, n_kf, -(1 << 31), (1 << 31) - 1)[k % 4]
    g["parent"][[2, 9, 17, 25, 33]] = (-5, n_kf, 1 << 30, n_kf + 2, -(1 << 31))
    off = w["obs_off"].copy()
    rows = rng.choice(w["cap_points"] - 2, 40, replace=False) + 1
    off[rows[:20]] += 7                                                            # descending against the next offset here and there
    off[rows[20:30]] = len(w["obs_kf"]) + 5
    off[rows[30:]] = -3
    return dict(w, g=g, obs_off=off)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_garbage_in_the_graph_and_the_csr_is_dropped_and_counted(stream_kind):
    """d_ord_n negative and over n_kf, list entries and d_parent out of range, CSR offsets descending, past n_obs and negative, d_kf out
    of range: every call of the small scene on that world equals the model, the dropped entries are counted, the guards are intact"""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    w = cached("garbage", _garbage_world)
    sc = cached(("scene", "small"), lambda: lm.make_scene("small"))
    calls = [c for c in sc["calls"] if "cap_local_kf" not in c and "cap_rows" not in c][::3]
    wants = cached("garbage_outs", lambda: [lm.local_map(w, **c) for c in calls])
    total = np.stack([o["result"] for o in wants]).sum(0)
    print("d_result sums", total.tolist())
    assert total[lm.R_LIST_DROPPED] >= 3 and total[lm.R_MAX_VOTES] > 0
    t, graph, gpads = _device_world(torch, dev, w)
    m = ORBMatcher()
    for call, want in zip(calls, wants):
        caps = _caps(call, want)
        _equals_model(w, _local_map(torch, dev, m, w, t, graph, call, *caps, stream_kind), want, *caps)
    # d_kf out of range, either side, and a key frame whose rows' lists the forged offsets cut
    for kf in (-1, w["n_kf"], 1 << 30, 4):
        for min_obs in (0, 1, 3):
            count = _padded(torch, dev, np.full(4, FILL["count"], np.int32), GUARDS["count"])
            st = _stream(torch, dev, stream_kind)
            m.NumTrackedPointsDevice(dict(t, ref=_up(torch, dev, np.array([kf], np.int32)), count=count[1]), w["n_kf"], w["stride"], w["cap_points"],
                                     len(w["obs_kf"]), min_obs, stream=st)
            torch.cuda.synchronize()
            torch.cuda.set_stream(torch.cuda.default_stream(dev))
            assert _guards_intact(count[0], GUARDS["count"]) and count[1].cpu().numpy().tobytes() == lm.num_tracked(w, kf, min_obs).tobytes(), (kf, min_obs)
    _world_untouched(w, t, gpads)


def _chain_scene():
    """the mid scene's world and its first call with a vote and ten neighbours, a table of positions, normals and distance ranges over
    its 2400 rows, a pose; and the models chained: observations_model.build -> local_map -> projection_model (Pinhole, valid = the mask)
    -> track_counters (1 | 2) -> num_tracked on the reference key frame"""
    import observations_model as om
    import projection_model as pm
    sc = lm.make_scene("mid")
    w = sc["world"]
    cap = w["cap_points"]
    call = next(c for c, o in zip(sc["calls"], sc["outs"]) if o["result"][lm.R_MAX_KF] >= 0 and c["n_neigh"] == lm.N_NEIGH and not o["result"][lm.R_REFUSED]
                and o["result"][lm.R_CLEARED])
    cloud = pm.make_cloud(pm.FRUSTUM, False, cap, 31)
    off, okf, okp, bres = om.build(w["n"], w["bad"], w["slots"], w["stride"], w["valid"], cap, 1 << 30)
    w2 = dict(w, obs_off=off, obs_kf=okf, obs_kp=okp)
    local = lm.local_map(w2, **call)
    e32 = pm.evaluate(pm.FRUSTUM, cloud["cam"], cloud["bounds"], cloud["R"], cloud["t"], cloud["points"], local["mask"], normals=cloud["normals"],
                      min_dist=cloud["min_dist"], max_dist=cloud["max_dist"], frame_mp=local["frame_mp"], th=1.0)
    rng = np.random.RandomState(8)
    visible0 = rng.randint(0, 50, cap).astype(np.int32)
    fm, visible, _, counters = lm.track_counters(local["frame_mp"], w["valid"], cap, e32["q_ok"], 1 | 2, visible0, np.zeros(cap, np.int32))
    return dict(w=w2, call=call, cloud=cloud, build=bres, local=local, e32=e32, visible0=visible0, visible=visible, counters=counters, frame_mp=fm,
                count=lm.num_tracked(w2, local["ref"], 3))


def _chain_on_device(torch, dev, cs, stream_kind):
    import projection_model as pm
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    w, call, cloud, local = cs["w"], cs["call"], cs["cloud"], cs["local"]
    cap, n_kf, n2 = w["cap_points"], w["n_kf"], len(call["frame_mp"])
    cap_obs = len(w["obs_kf"]) + 40
    t = {k: _up(torch, dev, w[k]) for k in ("n", "bad", "slots", "valid")}
    t.update(pose_R=_up(torch, dev, np.asarray(cloud["R"], np.float64).reshape(9)), pose_t=_up(torch, dev, np.asarray(cloud["t"], np.float64)),
             **{k: _up(torch, dev, cloud[k]) for k in ("points", "normals", "min_dist", "max_dist")})
    graph, gpads = _device_graph(torch, dev, w["g"])
    ints = dict(obs_off=cap + 1, obs_kf=cap_obs, obs_kp=cap_obs, work=cap + n_kf, local_kf=len(local["local_kf"]) + SLACK, rows=len(local["rows"]) + SLACK,
                q_level=cap, r_build=8, r_local=16, r_frustum=8, r_counters=8, count=4)
    pads = {k: _padded(torch, dev, np.zeros(n, np.int32) if k in ("obs_kf", "obs_kp") else np.full(n, -51, np.int32), 41) for k, n in ints.items()}
    pads.update(frame_mp=_padded(torch, dev, call["frame_mp"], 41), ref=_padded(torch, dev, np.full(1, REF0, np.int32), 41),
                visible=_padded(torch, dev, cs["visible0"], 41), local_mask=_padded(torch, dev, np.full(cap, 91, np.uint8), 41),
                q_ok=_padded(torch, dev, np.full(cap, 7, np.uint8), 41), q_xy=_padded(torch, dev, np.full(2 * cap, 7.5, np.float32), 41),
                q_radius=_padded(torch, dev, np.full(cap, 7.5, np.float32), 41))
    d = dict(t, **{k: v[1] for k, v in pads.items()})
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    m.BuildObservationsDevice(dict(d, result=d["r_build"]), n_kf, w["stride"], cap, cap_obs, stream=st)
    m.LocalMapDevice(graph, dict(d, result=d["r_local"]), n2, n_kf, w["stride"], cap, cap_obs, call["recent"], ints["local_kf"], ints["rows"], stream=st)
    m.ProjectFrustumDevice(cam, dict(d, valid=d["local_mask"], result=d["r_frustum"]), cap, n2, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 1.0, stream=st)
    m.TrackCountersDevice(dict(d, result=d["r_counters"]), n2, cap, cap, 1 | 2, stream=st)
    m.NumTrackedPointsDevice(d, n_kf, w["stride"], cap, cap_obs, 3, stream=st)
    torch.cuda.synchronize()                                                      # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], 41), k
    return {k: v[1].cpu().numpy() for k, v in pads.items()}


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_chain_from_the_observations_to_the_tracked_points_with_one_wait(stream_kind):
    """orbm_build_observations_device -> orbm_local_map_device -> orbm_project_frustum_device (Pinhole, d_valid = the mask, nq = the
    table's 2400 rows) -> orbm_track_counters_device (1 | 2) -> orbm_num_tracked_points_device on d_ref: one stream, no read-back between
    the calls, ONE wait at the end, on the mid scene's world (120 key frames x 96 slots).  The CSR, the mask, d_rows, q_ok, the builder's
    d_result, d_visible, d_ref and the count equal observations_model, the model here and projection_model chained the same way; q_ok
    does not pass through logf, so nothing is excluded.  A second run gives the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    cs = cached("chain", _chain_scene)
    w, local, e32 = cs["w"], cs["local"], cs["e32"]
    print("build %s local map %s frustum %s counters %s count %s" % (cs["build"].tolist(), local["result"].tolist(), e32["result"].tolist(),
                                                                     cs["counters"].tolist(), cs["count"].tolist()))
    assert local["result"][lm.R_ROWS] >= 300 and e32["result"][0] >= 50 and e32["result"][2] >= 10 and local["result"][lm.R_CLEARED] >= 1
    assert cs["counters"][lm.C_VISIBLE_QUERIES] == e32["result"][0] and cs["counters"][lm.C_CLEARED] == 0 and cs["count"][0] >= 5
    runs = [_chain_on_device(torch, dev, cs, stream_kind) for _ in range(2)]
    got = runs[0]
    n_obs = len(w["obs_kf"])
    assert got["r_build"].tobytes() == cs["build"].tobytes() and got["obs_off"].tobytes() == w["obs_off"].tobytes()
    assert got["obs_kf"][:n_obs].tobytes() == w["obs_kf"].tobytes() and got["obs_kp"][:n_obs].tobytes() == w["obs_kp"].tobytes()
    assert got["r_local"].tobytes() == local["result"].tobytes() and got["local_mask"].tobytes() == local["mask"].tobytes()
    for key in ("local_kf", "rows"):
        n = len(local[key])
        assert got[key][:n].tobytes() == local[key].tobytes() and (got[key][n:] == -51).all(), key
    assert int(got["ref"][0]) == local["ref"] and got["frame_mp"].tobytes() == cs["frame_mp"].tobytes()
    assert got["q_ok"].tobytes() == e32["q_ok"].tobytes() and got["r_frustum"].tobytes() == e32["result"].tobytes()
    assert got["visible"].tobytes() == cs["visible"].tobytes() and got["r_counters"].tobytes() == cs["counters"].tobytes()
    assert got["count"].tobytes() == cs["count"].tobytes()
    for k in got:
        if k != "work":
            assert runs[1][k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_counters_bit_by_bit(stream_kind):
    """each bit alone, 1 | 2, 1 | 4 and all three, on a frame of 1025 slots with bad rows, rows named twice, -1 and junk, and 600
    queries: d_frame_mp, d_visible, d_found (accumulated on what they held) and d_result equal the model's, the array a bit does not
    name is untouched; d_q_ok == NULL with bit 2 clear is taken, with bit 2 set it is an argument error"""
    import torch
    from monoorbslam3_amd._lib import OrbxError
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    w = cached(("scene", "small"), lambda: lm.make_scene("small"))["world"]
    cap, n2 = w["cap_points"], 1025
    rng = np.random.RandomState(4)
    fm = rng.randint(0, cap, n2).astype(np.int32)                                   # 1025 draws from 600 rows: many twice, about a tenth bad
    fm[rng.rand(n2) < 0.3] = -1
    fm[rng.rand(n2) < 0.02] = cap
    q_ok = (rng.rand(cap) < 0.4).astype(np.uint8)
    visible0, found0 = rng.randint(0, 90, cap).astype(np.int32), rng.randint(0, 90, cap).astype(np.int32)
    valid = _up(torch, dev, w["valid"])
    m = ORBMatcher()
    for what, with_q in ((1, True), (2, True), (4, True), (3, True), (5, False), (4, False), (7, True)):
        want = lm.track_counters(fm, w["valid"], cap, q_ok, what, visible0, found0)
        pads = dict(frame_mp=_padded(torch, dev, fm, 41), visible=_padded(torch, dev, visible0, 42), found=_padded(torch, dev, found0, 43),
                    result=_padded(torch, dev, np.full(8, 31, np.int32), 44))
        d = dict({k: v[1] for k, v in pads.items()}, valid=valid, q_ok=_up(torch, dev, q_ok) if with_q else None)
        st = _stream(torch, dev, stream_kind)
        m.TrackCountersDevice(d, n2, cap, cap if with_q else 0, what, stream=st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        print("what", what, "d_result", pads["result"][1].cpu().numpy().tolist())
        for (k, fill), model in zip((("frame_mp", 41), ("visible", 42), ("found", 43), ("result", 44)), want):
            assert _guards_intact(pads[k][0], fill) and pads[k][1].cpu().numpy().tobytes() == model.tobytes(), (what, k)
    assert want[3][lm.C_CLEARED] >= 20 and want[3][lm.C_FOUND] >= 300
    with pytest.raises(OrbxError) as e:
        m.TrackCountersDevice(dict(d, q_ok=None), n2, cap, cap, 2)
    assert e.value.code == -1
