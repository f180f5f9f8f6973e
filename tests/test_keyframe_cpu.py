"""The two restatements of tests/keyframe_model.py against each other on every call of the seeded scenes, the parallel claim of the
map-point culling, the cases the scenes were built for, and the three entry points' symbols, bindings and argument checks through the
library.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import keyframe_model as km

_cache = {}


def scene(name):
    """a scene made once, shared, never changed"""
    if name not in _cache:
        _cache[name] = km.make_scene(name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(km.SCENES))
def test_the_scenes_hold_every_case_they_were_built_for(name):
    sc = scene(name)
    km.check_scene(sc)
    print(name, "cull", sc["cull_out"]["result"].tolist(), "inserts", np.stack([o["result"] for o in sc["insert_outs"]]).sum(0).tolist(),
          "registers", [o["result"][:2].tolist() for o in sc["register_outs"]])


@pytest.mark.parametrize("name", sorted(km.SCENES))
def test_the_inserted_key_frame_equals_the_objects(name):
    """per call: the KeyFrame constructed from the Frame and run through the loop of processNewKeyFrame holds the map points the model's
    row K holds, the frame's own are untouched, the observations added number (slots holding a point) - (second slots of a row), and
    every other row of the table is as passed"""
    sc = scene(name)
    w = sc["cull"]["world"]
    cap, stride = w["cap_points"], w["stride"]
    for call, out in zip(sc["inserts"], sc["insert_outs"]):
        point_map = km.Map()
        mps = [km.MapPoint(p, not w["valid"][p], point_map) for p in range(cap)]
        fm = call["frame_mp"][:stride]                             # a frame is no longer than the stride in the reference
        frame = km.Frame([mps[p] if 0 <= p < cap else None for p in fm.tolist()], call["frame_R"], call["frame_t"], call["frame_kps"], call["frame_desc"])
        before = list(frame.map_points)
        kf = km.KeyFrame.from_frame(call["K"], frame)
        added = km.process_new_key_frame(kf)
        K, res = call["K"], out["result"]
        assert [mp.row if mp else -1 for mp in kf.map_points] == out["slots"][K, :len(fm)].tolist() and (out["slots"][K, len(fm):] == -1).all()
        assert frame.map_points == before and added == res[km.I_HELD] - res[km.I_TWICE]
        assert all(mp.observations == ({kf: min(np.flatnonzero(out["slots"][K] == mp.row))} if mp.row in out["slots"][K] else {}) for mp in mps)
        assert res[km.I_RANGE] == sum(1 for p in fm.tolist() if p != -1 and not 0 <= p < cap) and res[km.I_CUT] == max(len(call["frame_mp"]) - stride, 0)
        assert out["pose_R"][K].tobytes() == np.asarray(kf.R_cw).tobytes() and out["pose_t"][K].tobytes() == np.asarray(kf.t_cw).tobytes()
        assert (out["bad"][K], out["n"][K], out["kps"][K], out["desc"][K]) == (0, len(call["frame_mp"]), kf.key_points, kf.descriptors)
        others = np.arange(w["n_kf"]) != K
        for key in km.TABLE_KEYS:
            assert out[key][others].tobytes() == sc["table"][key][others].tobytes(), key


@pytest.mark.parametrize("name", sorted(km.SCENES))
def test_the_registered_rows_equal_the_constructed_points(name):
    """per call that is not refused: MapPoint objects constructed in creation order and pushed to recent_map_points carry the fields the
    model wrote and the list holds their rows behind what it held; a refused call leaves everything as passed"""
    sc = scene(name)
    state = sc["state"]
    for call, out in zip(sc["registers"], sc["register_outs"]):
        res = out["result"]
        if res[km.G_REFUSED]:
            for key in ("ref_kf", "first_kf", "found", "visible", "recent"):
                assert out[key].tobytes() == state[key].tobytes(), key
            assert (out["n_registered"], out["n_recent"]) == (call["n_registered"], call["n_recent"]) and res[km.G_ROWS] == 0
            continue
        a, b, r = int(res[km.G_FROM]), int(res[km.G_TO]), int(res[km.G_RECENT]) - int(res[km.G_ROWS])
        last_kf, cur_kf = km.KeyFrame(99, num_kps=b - a + 1), km.KeyFrame(call["K"], kf_id=call["kf_id"], num_kps=b - a + 1)
        recent = [km.MapPoint(int(p)) for p in state["recent"][:r]]
        made = km.bookkeeping_of_new_points(last_kf, cur_kf, [(t, t) for t in range(b - a)], a, km.Map(), recent)
        assert [mp.row for mp in recent] == out["recent"][:out["n_recent"]].tolist() and out["n_registered"] == b and len(made) == res[km.G_ROWS]
        assert [mp.reference_kf.slot for mp in made] == out["ref_kf"][a:b].tolist() and [mp.first_kf_id for mp in made] == out["first_kf"][a:b].tolist()
        assert [mp.num_found for mp in made] == out["found"][a:b].tolist() and [mp.num_visible for mp in made] == out["visible"][a:b].tolist()
        for key in ("ref_kf", "first_kf", "found", "visible"):
            assert out[key][:a].tobytes() == state[key][:a].tobytes() and out[key][b:].tobytes() == state[key][b:].tobytes(), key
        assert out["recent"][out["n_recent"]:].tobytes() == state["recent"][out["n_recent"]:].tobytes()


@pytest.mark.parametrize("name", sorted(km.SCENES))
def test_the_culled_list_equals_the_objects_and_the_parallel_run_the_sequential_one(name):
    """MapPointCulling as written on objects built from the slots in ascending (k, i): the list that remains, the points gone bad, the
    points handed to Map::eraseMapPoint, every key frame's map_points and the two counts of the reference's log line equal the model's;
    and the model run entry by entry equals the model run with every entry classified on the arrays as passed"""
    sc = scene(name)
    c, out = sc["cull"], sc["cull_out"]
    w, n = c["world"], c["n_recent"]
    cap = w["cap_points"]
    kfs, mps, point_map = km.world_objects(w, c["first_kf"], c["found"], c["visible"])
    recent = [mps[p] for p in c["recent"][:n].tolist() if 0 <= p < cap]          # no object stands for a value that is no row
    num_found_ratio, num_bad = km.map_point_culling(recent, km.KeyFrame(0, kf_id=c["cur"]))
    res = out["result"]
    assert [mp.row for mp in recent] == out["recent"][:out["n_recent"]].tolist() and out["n_recent"] == res[km.P_KEPT]
    assert (num_found_ratio, num_bad) == (res[km.P_RATIO], res[km.P_BAD])
    assert [not mp.is_bad for mp in mps] == (out["valid"] != 0).tolist()
    assert point_map.erased == [int(p) for p, k in zip(c["recent"][:n], out["code"][:n]) if k in (2, 3)]
    assert km.object_slots(kfs, w).tobytes() == out["slots"].tobytes()
    par = km.run_cull(c, sequential=False)
    for key in ("recent", "valid", "slots", "code", "result"):
        assert par[key].tobytes() == out[key].tobytes(), key
    assert par["n_recent"] == out["n_recent"]
    twice = sc["twice_out"]                                                       # the refusal: everything as passed
    assert twice["recent"].tobytes() == sc["twice"]["recent"].tobytes() and twice["n_recent"] == n and twice["code"].tobytes() == c["code0"].tobytes()
    assert twice["valid"].tobytes() == w["valid"].tobytes() and twice["slots"].tobytes() == w["slots"].tobytes()


# ---- the library: symbols, bindings, argument and limit checks ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


NAMES = ("orbm_insert_keyframe_device", "orbm_register_new_points_device", "orbm_cull_map_points_device")


def test_the_library_exports_the_three_entry_points_and_the_bindings_resolve(mlib):
    L, matcher = mlib
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p and fn.restype is C.c_int, name
    for method in ("InsertKeyFrameDevice", "RegisterNewPointsDevice", "CullMapPointsDevice"):
        assert callable(getattr(matcher.ORBMatcher, method)), method


P = 0x1000                # a fake device pointer: never dereferenced, every call below fails before a launch
E_ARG, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -4


def _insert(L, **over):
    a = dict(K=3, cap_kf=8, pose_R=P, pose_t=P, bad=P, kps=P, desc=P, n=P, slots=P, stride=64, valid=P, cap_points=500, frame_mp=P, n2=60,
             frame_R=P, frame_t=P, frame_kps=P, frame_desc=P, result=P)
    a.update(over)
    return L.orbm_insert_keyframe_device(None, a["K"], a["cap_kf"], a["pose_R"], a["pose_t"], a["bad"], a["kps"], a["desc"], a["n"], a["slots"],
                                         a["stride"], a["valid"], a["cap_points"], a["frame_mp"], a["n2"], a["frame_R"], a["frame_t"],
                                         a["frame_kps"], a["frame_desc"], a["result"], None)


def _register(L, **over):
    a = dict(n_points=P, n_registered=P, K=2, kf_id=5, cap_points=500, ref_kf=P, first_kf=P, found=P, visible=P, recent=P, cap_recent=90,
             n_recent=P, result=P)
    a.update(over)
    return L.orbm_register_new_points_device(None, a["n_points"], a["n_registered"], a["K"], a["kf_id"], a["cap_points"], a["ref_kf"], a["first_kf"],
                                             a["found"], a["visible"], a["recent"], a["cap_recent"], a["n_recent"], a["result"], None)


def _cull(L, **over):
    a = dict(recent=P, n_recent=P, cap_recent=90, cur=7, first_kf=P, found=P, visible=P, valid=P, cap_points=500, n_kf=6, n=P, bad=P, slots=P,
             stride=64, obs_off=P, obs_kf=P, obs_kp=P, n_obs=800, code=P, result=P)
    a.update(over)
    return L.orbm_cull_map_points_device(None, a["recent"], a["n_recent"], a["cap_recent"], a["cur"], a["first_kf"], a["found"], a["visible"],
                                         a["valid"], a["cap_points"], a["n_kf"], a["n"], a["bad"], a["slots"], a["stride"], a["obs_off"], a["obs_kf"],
                                         a["obs_kp"], a["n_obs"], a["code"], a["result"], None)


def test_the_entry_points_check_their_arguments_before_any_device_call(mlib):
    """every ORBX_E_ARG and ORBX_E_UNSUPPORTED case of the header's section, returned with a NULL handle and fake pointers: before the
    device is asked for; an argument error wins over a limit; without a device a valid call fails with ORBX_E_NO_DEVICE"""
    L, _ = mlib
    import torch
    for key in ("cap_kf", "stride", "cap_points", "n2", "K"):
        assert _insert(L, **{key: -1}) == E_ARG, key
    assert _insert(L, K=8) == E_ARG and _insert(L, K=8, stride=8193) == E_ARG          # the argument error first
    for key in ("pose_R", "pose_t", "bad", "kps", "desc", "n", "slots", "valid", "frame_mp", "frame_R", "frame_t", "result"):
        assert _insert(L, **{key: None}) == E_ARG, key
    assert _insert(L, kps=P + 4) == E_ARG and _insert(L, desc=P + 2) == E_ARG           # the pointer arrays, pointer aligned
    assert _insert(L, stride=8193) == E_UNSUPPORTED and _insert(L, cap_points=524289) == E_UNSUPPORTED
    for key in ("cap_points", "cap_recent", "K", "kf_id"):
        assert _register(L, **{key: -1}) == E_ARG, key
    for key in ("n_points", "n_registered", "ref_kf", "first_kf", "found", "visible", "recent", "n_recent", "result"):
        assert _register(L, **{key: None}) == E_ARG, key
    assert _register(L, cap_points=524289) == E_UNSUPPORTED
    for key in ("cap_recent", "cur", "cap_points", "n_kf", "stride", "n_obs"):
        assert _cull(L, **{key: -1}) == E_ARG, key
    for key in ("recent", "n_recent", "first_kf", "found", "visible", "valid", "n", "bad", "slots", "obs_off", "obs_kf", "obs_kp", "code", "result"):
        assert _cull(L, **{key: None}) == E_ARG, key
    assert _cull(L, stride=8193) == E_UNSUPPORTED and _cull(L, cap_points=524289) == E_UNSUPPORTED
    assert _cull(L, cur=-1, stride=8193) == E_ARG and L.orbx_last_error()
    if not torch.cuda.is_available():
        assert _insert(L) == E_NO_DEVICE and _insert(L, n2=0, frame_mp=None) == E_NO_DEVICE and _insert(L, n2=9000, stride=8192) == E_NO_DEVICE
        assert _insert(L, frame_kps=None, frame_desc=None) == E_NO_DEVICE          # the frame's record pointers are values, not dereferenced
        assert _register(L) == E_NO_DEVICE and _register(L, cap_recent=0, recent=None) == E_NO_DEVICE
        assert _cull(L) == E_NO_DEVICE and _cull(L, n_obs=0, obs_kf=None, obs_kp=None) == E_NO_DEVICE and _cull(L, cap_points=524288) == E_NO_DEVICE
