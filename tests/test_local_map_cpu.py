"""The two restatements of the tracker's local map in tests/local_map_model.py against each other on every call of the seeded scenes, the
cases the scenes were built for, and the three entry points' argument and limit checks through the library.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import local_map_model as lm

_cache = {}


def scene(name):
    """a scene made once, shared, never changed"""
    if name not in _cache:
        _cache[name] = lm.make_scene(name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_the_array_form_and_the_objects_agree_on_every_call(name):
    """per call: the local key frames and the local map points in order, the reference key frame, the frame's cleared slots; then the
    counters of searchLocalPoints and trackLocalMap on the same objects (visible, found per row) and getNumTrackedMapPoint of the new
    reference key frame for minObs 0 .. 4; the scene holds every case it was built for"""
    sc = scene(name)
    lm.check_scene(sc)
    w = sc["world"]
    cap = w["cap_points"]
    print(name, len(sc["calls"]), "calls; cases", sorted(sc["tags"]))
    rng = np.random.RandomState(9)
    for t, (c, out) in enumerate(zip(sc["calls"], sc["outs"])):
        kfs, mps = lm.world_objects(w)
        frame = lm.frame_object(1000 + t, c["frame_mp"], mps)
        start = lm.KeyFrame(-7)                                    # reference_kf before the call
        local_kfs, ref = lm.update_local_key_frames(frame, [kfs[k] for k in c["recent"]], start, c["n_neigh"], c["max_kf"])
        local_mps = lm.update_local_map_points(frame, local_kfs)
        assert [kf.id for kf in local_kfs] == out["local_kf"].tolist(), t
        assert [mp.row for mp in local_mps] == out["rows"].tolist(), t
        assert np.flatnonzero(out["mask"]).tolist() == (sorted(out["rows"].tolist()) if not out["result"][lm.R_REFUSED] else []), t
        assert ref.id == (out["result"][lm.R_MAX_KF] if out["result"][lm.R_MAX_KF] >= 0 else -7), t
        assert [mp.row if mp is not None else -1 for mp in frame.map_points] == [p if 0 <= p < cap else -1 for p in out["frame_mp"].tolist()], t
        if out["result"][lm.R_REFUSED]:
            continue
        # the counters: q_ok as the frustum builder leaves it over the mask (valid, not already in the frame, in view)
        in_view = rng.rand(cap) < 0.6
        in_frame = np.zeros(cap, bool)
        fm = out["frame_mp"]
        in_frame[fm[(fm >= 0) & (fm < cap)]] = True
        q_ok = ((out["mask"] != 0) & ~in_frame & in_view).astype(np.uint8)
        fm2, visible, found, r12 = lm.track_counters(fm, w["valid"], cap, q_ok, 1 | 2, np.zeros(cap, np.int32), np.zeros(cap, np.int32))
        fm3, visible, found, r4 = lm.track_counters(fm2, w["valid"], cap, None, 4, visible, found)
        lm.search_local_points_counters(frame, local_mps, in_view)
        lm.increase_found(frame)
        assert [mp.visible for mp in mps] == visible.tolist() and [mp.found for mp in mps] == found.tolist(), t
        assert r12[lm.C_CLEARED] == 0 and r4[lm.C_FOUND] == r12[lm.C_VISIBLE_FRAME] and np.array_equal(fm2, fm) and np.array_equal(fm3, fm)
        for min_obs in range(5 if ref is not start else 0):
            assert ref.get_num_tracked_map_point(min_obs) == lm.num_tracked(w, ref.id, min_obs)[0], (t, min_obs)


def test_the_counters_on_a_frame_with_bad_and_repeated_rows():
    """bit 1 clears a bad row and counts the others, a row named twice counts twice; bit 4 alone does not test for bad; all three bits: a
    slot bit 1 cleared is not found; against the objects"""
    w = scene("small")["world"]
    cap = w["cap_points"]
    good, bad = np.flatnonzero(w["valid"])[:6], np.flatnonzero(w["valid"] == 0)[:2]
    fm = np.array([good[0], -1, bad[0], good[1], good[0], cap + 2, bad[1], good[2], -5, good[0]], np.int32)
    zero = np.zeros(cap, np.int32)
    q_ok = np.zeros(cap, np.uint8)
    q_ok[good[3:6]] = 1
    f1, v1, _, r1 = lm.track_counters(fm, w["valid"], cap, None, 1, zero, zero)
    assert r1[:4].tolist() == [5, 0, 0, 2] and v1[good[0]] == 3 and (f1[[2, 6]] == -1).all() and f1[5] == cap + 2
    _, _, n4, r4 = lm.track_counters(fm, w["valid"], cap, None, 4, zero, zero)
    assert r4[:4].tolist() == [0, 0, 7, 0] and n4[bad[0]] == 1
    f7, v7, n7, r7 = lm.track_counters(fm, w["valid"], cap, q_ok, 7, zero, zero)
    assert r7[:4].tolist() == [5, 3, 5, 2] and n7[bad[0]] == 0
    kfs, mps = lm.world_objects(w)
    frame = lm.frame_object(1, fm, mps)
    lm.search_local_points_counters(frame, [mps[p] for p in good[3:6]], np.ones(cap, bool))
    lm.increase_found(frame)
    assert [mp.visible for mp in mps] == v7.tolist() and [mp.found for mp in mps] == n7.tolist()


# ---- the argument and limit checks, through the library ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


P = 0x1000                # a fake device pointer: never dereferenced, every call below fails before a launch
E_ARG, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -4


def _graph(matcher, cap=64, **over):
    f = dict(cap_kf=cap, d_weight=P, d_ord_kf=P, d_ord_n=P, d_parent=P)
    f.update(over)
    return matcher.CovisGraph(f["cap_kf"], f["d_weight"], f["d_ord_kf"], f["d_ord_n"], f["d_parent"])


def _local_map(L, g, recent=(1, 2, 3), **over):
    a = dict(frame_mp=P, n2=100, valid=P, cap_points=500, obs_off=P, obs_kf=P, obs_kp=P, n_obs=900, n_kf=32, n=P, bad=P, slots=P, stride=64,
             n_neigh=10, max_kf=80, cap_local_kf=200, cap_rows=500, work=P, local_kf=P, rows=P, mask=P, ref=P, result=P)
    a["n_recent"] = len(recent)
    a.update(over)
    rec = (C.c_int32 * 40)(*(list(recent) + [0] * (40 - len(recent))))
    return L.orbm_local_map_device(None, a["frame_mp"], a["n2"], a["valid"], a["cap_points"], a["obs_off"], a["obs_kf"], a["obs_kp"], a["n_obs"], a["n_kf"],
                                   a["n"], a["bad"], a["slots"], a["stride"], C.byref(g) if g is not None else None, C.cast(rec, C.c_void_p),
                                   a["n_recent"], a["n_neigh"], a["max_kf"], a["cap_local_kf"], a["cap_rows"], a["work"], a["local_kf"], a["rows"],
                                   a["mask"], a["ref"], a["result"], None)


def _counters(L, **over):
    a = dict(frame_mp=P, n2=100, valid=P, cap_points=500, q_ok=P, nq=500, what=7, visible=P, found=P, result=P)
    a.update(over)
    return L.orbm_track_counters_device(None, a["frame_mp"], a["n2"], a["valid"], a["cap_points"], a["q_ok"], a["nq"], a["what"], a["visible"],
                                        a["found"], a["result"], None)


def _tracked(L, **over):
    a = dict(kf=P, min_obs=3, n_kf=32, n=P, bad=P, slots=P, stride=64, cap_points=500, obs_off=P, obs_kf=P, obs_kp=P, n_obs=900, count=P)
    a.update(over)
    return L.orbm_num_tracked_points_device(None, a["kf"], a["min_obs"], a["n_kf"], a["n"], a["bad"], a["slots"], a["stride"], a["cap_points"],
                                            a["obs_off"], a["obs_kf"], a["obs_kp"], a["n_obs"], a["count"], None)


def test_the_entry_points_check_their_arguments_before_any_device_call(mlib):
    """every ORBX_E_ARG and ORBX_E_UNSUPPORTED case of the header's section, returned with a NULL handle and fake pointers: before the
    device is asked for; an argument error wins over a limit; without a device a valid call fails with ORBX_E_NO_DEVICE"""
    L, matcher = mlib
    import torch
    g = _graph(matcher)
    assert _local_map(L, None) == E_ARG and _local_map(L, _graph(matcher, d_parent=None)) == E_ARG
    assert _local_map(L, g, n_kf=65) == E_ARG and _local_map(L, g, n_kf=-1) == E_ARG
    for key in ("n2", "cap_points", "n_obs", "stride", "n_neigh", "max_kf", "cap_local_kf", "cap_rows"):
        assert _local_map(L, g, **{key: -1}) == E_ARG, key
    for key in ("frame_mp", "valid", "obs_off", "obs_kf", "obs_kp", "n", "bad", "slots", "work", "local_kf", "rows", "mask", "ref", "result"):
        assert _local_map(L, g, **{key: None}) == E_ARG, key
    assert _local_map(L, g, recent=tuple(range(33)), n_kf=64) == E_ARG                 # more than 32
    assert _local_map(L, g, recent=(1, 32)) == E_ARG and _local_map(L, g, recent=(-1,)) == E_ARG
    assert _local_map(L, g, recent=(4, 5, 4)) == E_ARG and b"twice" in L.orbx_last_error()
    assert _local_map(L, g, recent=(4, 5, 4), stride=8193) == E_ARG                    # the argument error first
    assert _local_map(L, _graph(matcher, cap=4097)) == E_UNSUPPORTED
    assert _local_map(L, g, stride=8193) == E_UNSUPPORTED and _local_map(L, g, n2=8193) == E_UNSUPPORTED
    assert _local_map(L, g, cap_points=524289) == E_UNSUPPORTED
    for key in ("n2", "cap_points", "nq"):
        assert _counters(L, **{key: -1}) == E_ARG, key
    assert _counters(L, what=8) == E_ARG and _counters(L, what=-1) == E_ARG
    assert _counters(L, q_ok=None) == E_ARG and _counters(L, nq=501) == E_ARG          # bit 2 with NULL; queries past the table
    for key in ("frame_mp", "valid", "visible", "found", "result"):
        assert _counters(L, **{key: None}) == E_ARG, key
    assert _counters(L, n2=8193) == E_UNSUPPORTED and _counters(L, cap_points=524289, nq=0) == E_UNSUPPORTED
    for key in ("n_kf", "stride", "cap_points", "n_obs"):
        assert _tracked(L, **{key: -1}) == E_ARG, key
    for key in ("kf", "n", "bad", "slots", "obs_off", "obs_kf", "obs_kp", "count"):
        assert _tracked(L, **{key: None}) == E_ARG, key
    assert _tracked(L, stride=8193) == E_UNSUPPORTED and _tracked(L, cap_points=524289) == E_UNSUPPORTED
    assert L.orbx_last_error()
    if not torch.cuda.is_available():
        assert _local_map(L, g) == E_NO_DEVICE and _local_map(L, _graph(matcher, cap=4096), n_kf=4096, stride=8192, n2=8192) == E_NO_DEVICE
        assert _local_map(L, g, recent=(), n_kf=0, n2=0) == E_NO_DEVICE
        assert _counters(L) == E_NO_DEVICE and _counters(L, q_ok=None, what=5) == E_NO_DEVICE and _counters(L, found=None, what=3) == E_NO_DEVICE
        assert _tracked(L) == E_NO_DEVICE and _tracked(L, min_obs=-2) == E_NO_DEVICE
