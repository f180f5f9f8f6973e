"""orbm_insert_keyframe_device / orbm_register_new_points_device / orbm_cull_map_points_device on the MI355X (include/orbm.h, "Key frames
inserted and recent map points culled on the device") against the array model of tests/keyframe_model.py, byte for byte: integers
only (the one float division of the culling is IEEE on both sides), so no tolerance and no exclusion."""
import numpy as np
import pytest

import keyframe_model as km
import local_map_model as lm
import observations_model as om
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401 (GUARD: the padding _padded puts around every array)
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
WORLD_IN = ("n", "bad", "obs_off", "obs_kf", "obs_kp")                # what the culling reads of the world and must leave as passed


def cached(key, make):
    """a scene or a model output made once, shared, never changed"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _fill(a):
    return 177 if a.dtype == np.uint8 else -77


def _run(arrays, stream_kind, call):
    """every array of the call in a padded device array; call(matcher, d, stream); ONE wait; the guards; -> the arrays as the call left them"""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    arrays = {k: np.ascontiguousarray(a) for k, a in arrays.items()}
    pads = {k: _padded(torch, dev, a, _fill(a)) for k, a in arrays.items()}
    st = _stream(torch, dev, stream_kind)
    call(ORBMatcher(), {k: v[1] for k, v in pads.items()}, st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k, a in arrays.items():
        assert _guards_intact(pads[k][0], _fill(a)), k
    return {k: v[1].cpu().numpy() for k, v in pads.items()}


def _same(got, arrays, want):
    """every array equals the model's where the model has one of that name, and is as passed otherwise"""
    for k, a in arrays.items():
        exp = np.ascontiguousarray(want[k] if k in want else a).reshape(-1)
        assert got[k].tobytes() == exp.astype(np.ascontiguousarray(a).dtype).tobytes(), k


def _one(x):
    return np.array([x], np.int32)


# ---- the insert ---------------------------------------------------------------------------------------------------------------------------
# n2 of 0, 1, stride - 1, stride, stride + 5 at stride 64; one call at the largest stride (tiles of 1024 inside the row, a frame longer and
# one shorter than it); the smallest table and the largest (the 64 KB mask)
INSERTS = [dict(stride=64, cap_points=300, sizes=(0, 1, 63, 64, 69)), dict(stride=8192, cap_points=300, sizes=(8197, 5000)),
           dict(stride=64, cap_points=1, sizes=(64, 3)), dict(stride=64, cap_points=524288, sizes=(64,))]


def _insert_case(cfg):
    rng = np.random.RandomState(cfg["cap_points"] + cfg["stride"])
    valid = (rng.rand(cfg["cap_points"]) > 0.15).astype(np.uint8)
    valid[0] = 1
    table, calls = km.make_insert_calls(5, cfg["cap_points"], valid, cfg["stride"], 6, cfg["sizes"])
    return valid, table, calls, [km.run_insert(table, c, valid, cfg["cap_points"]) for c in calls]


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("cfg", INSERTS, ids=lambda c: "stride%d-cap%d" % (c["stride"], c["cap_points"]))
def test_an_inserted_key_frame_equals_the_model(cfg, stream_kind):
    """a table of six key frames full of an earlier use: row K -- pose bit for bit (a NaN payload and -0 among the values), d_bad, d_n, the
    two record pointers, EVERY slot -- and d_result equal the model's; the other rows, d_valid and the frame are as passed; guards intact;
    a second run gives the same bytes"""
    valid, table, calls, wants = cached(("insert", cfg["stride"], cfg["cap_points"]), lambda: _insert_case(cfg))
    if cfg["cap_points"] == 300 and cfg["stride"] == 64:
        km.check_insert_calls(wants)
    for c, want in zip(calls, wants):
        arrays = dict(table, valid=valid, frame_mp=c["frame_mp"], frame_pose_R=c["frame_R"], frame_pose_t=c["frame_t"], result=np.full(8, 31, np.int32))
        runs = [_run(arrays, stream_kind, lambda m, d, st: m.InsertKeyFrameDevice(d, c["K"], cfg["stride"], cfg["cap_points"], len(c["frame_mp"]),
                                                                                 c["frame_kps"], c["frame_desc"], stream=st)) for _ in range(2)]
        print("n2", len(c["frame_mp"]), "K", c["K"], "d_result", runs[0]["result"].tolist())
        _same(runs[0], arrays, want)
        _same(runs[1], arrays, want)


# ---- the registration -----------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)                  # wave and tile edges, of a registered range and of a recent list


def _register_arrays(state, call, cap_recent=None):
    recent = state["recent"] if cap_recent is None else np.resize(state["recent"], cap_recent)
    return dict(n_points=_one(call["n_points"]), n_registered=_one(call["n_registered"]), n_recent=_one(call["n_recent"]), ref_kf=state["ref_kf"],
                first_kf=state["first_kf"], found=state["found"], visible=state["visible"], recent=recent, result=np.full(8, 31, np.int32))


def _register(arrays, call, stream_kind):
    want = km.register_new_points(call["n_points"], call["n_registered"], call["n_recent"], call["K"], call["kf_id"], call["cap_points"],
                                  arrays["ref_kf"], arrays["first_kf"], arrays["found"], arrays["visible"], arrays["recent"])
    want = dict(want, n_registered=_one(want["n_registered"]), n_recent=_one(want["n_recent"]))
    got = _run(arrays, stream_kind, lambda m, d, st: m.RegisterNewPointsDevice(d, call["K"], call["kf_id"], call["cap_points"], stream=st))
    _same(got, arrays, want)
    return want["result"]


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("length", LENGTHS)
def test_a_registered_range_with_the_list_exactly_full_and_one_short(length, stream_kind):
    """rows a .. a + length - 1 behind a list of 9 entries: with cap_recent = 9 + length everything the model writes, the three device
    ints included; with one entry less refusal 1, and every in / out array is as passed"""
    cap = max(300, length + 50)
    state, _ = cached(("register", cap), lambda: km.make_register_calls(11, cap, cap_recent=9 + 2049))
    call = dict(n_points=cap - 20, n_registered=cap - 20 - length, n_recent=9, K=4, kf_id=7, cap_points=cap)
    res = _register(_register_arrays(state, call, 9 + length), call, stream_kind)
    assert res.tolist() == [length, 0, cap - 20 - length, cap - 20, 9 + length, 0, 0, 0]
    if length:
        res = _register(_register_arrays(state, call, 9 + length - 1), call, stream_kind)
        assert res[:2].tolist() == [0, 1]


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("cap", [1, 300, 524288])
def test_registration_distrusts_its_counters(cap, stream_kind):
    """the calls of the model's scene at the smallest, a common and the largest table: counters negative and above their capacity are
    clamped, *d_n_registered > *d_n_points is refusal 2, a full list refusal 1, and a refused call writes d_result alone"""
    state, calls = cached(("register_calls", cap), lambda: km.make_register_calls(12, cap))
    if cap == 1:                                                                  # the one row registered, refused twice, and nothing to do
        calls = [dict(c, **dict(zip(("n_points", "n_registered", "n_recent"), v))) for c, v in zip(calls, ((1, 0, 39), (0, 1, 3), (1, 0, 40), (1, 1, 40)))]
    results = [_register(_register_arrays(state, c), c, stream_kind) for c in calls]
    print(cap, [r[:5].tolist() for r in results])
    refusals = [int(r[km.G_REFUSED]) for r in results]
    assert 2 in refusals and 1 in refusals and 0 in refusals


# ---- the culling ------------------------------------------------------------------------------------------------------------------------------
def _cull_arrays(sc):
    w = sc["world"]
    arrays = {k: w[k] for k in WORLD_IN + ("slots", "valid")}
    if len(w["obs_kf"]) == 0:                                                     # a pointer even where there is no observation
        arrays["obs_kf"] = arrays["obs_kp"] = np.zeros(1, np.int32)
    return dict(arrays, recent=sc["recent"], n_recent=_one(sc["n_recent"]), first_kf=sc["first_kf"], found=sc["found"], visible=sc["visible"],
                code=sc["code0"], result=np.full(8, 31, np.int32))


def _cull(sc, want, stream_kind, runs=1):
    w = sc["world"]
    arrays = _cull_arrays(sc)
    want = dict(want, n_recent=_one(want["n_recent"]))
    for _ in range(runs):
        got = _run(arrays, stream_kind, lambda m, d, st: m.CullMapPointsDevice(d, sc["cur"], w["n_kf"], w["stride"], w["cap_points"], len(w["obs_kf"]),
                                                                               stream=st))
        _same(got, arrays, want)
    return got


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(km.SCENES))
def test_the_culling_of_a_designed_scene_equals_the_model(name, stream_kind):
    """6 key frames x 64 slots over 300 rows with a list of 60, 9 x 160 over 900 with 200: every code, the found ratios 1/4, 1/5, 0/0, 3/0,
    1/-4 and the pair above 2^24, ages 0 .. 3 and a first id above the current one, lists with stale, bad-key-frame and forged entries --
    the cases tests/keyframe_model.py's check_cull_scene asserts.  d_recent (compacted in place, the rest as passed), *d_n_recent, d_valid,
    d_slots, d_code and d_result equal the model's; what the call only reads is as passed; a second run gives the same bytes.  Then the
    same list with one row twice: d_result = {0, 1, 0 ...} and every array as passed."""
    sc = cached(("scene", name), lambda: km.make_scene(name))
    km.check_scene(sc)
    print(name, "d_result", sc["cull_out"]["result"].tolist())
    _cull(sc["cull"], sc["cull_out"], stream_kind, runs=2)
    _cull(sc["twice"], sc["twice_out"], stream_kind)


def _sized_cull(length):
    stride = 64 if length <= 65 else 512
    sc = km.make_cull_scene(20 + length, length, n_kf=6, stride=stride, cap_points=max(300, length + 50), designed=False,
                            cap_recent=length if length % 2 else length + 5)
    return sc, km.run_cull(sc)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("length", LENGTHS)
def test_the_culling_at_the_wave_and_tile_edges(length, stream_kind):
    """lists of 0 .. 2049 entries over 6 key frames, cap_recent exactly the length for the odd ones; a list longer than a tile keeps entries
    in every tile, so the compaction writes behind entries read in an earlier one"""
    sc, want = cached(("sized", length), lambda: _sized_cull(length))
    res = want["result"]
    print(length, "d_result", res.tolist())
    assert not res[km.P_REFUSED] and res[:6].sum() + (want["code"][:length] == -1).sum() == length
    if length > 1024:
        assert (want["code"][1024:length] == 0).sum() >= (5 if length > 2048 else 0) and 0 < (want["code"][:1024] != 0).sum()
    _cull(sc, want, stream_kind)


def _with_counter(sc, n_recent):
    sc = dict(sc, n_recent=n_recent)
    return sc, km.run_cull(sc)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_culling_distrusts_the_counter_the_list_and_the_csr(stream_kind):
    """*d_n_recent negative (nothing happens, it becomes 0) and above cap_recent (the whole array is the list); a row twice in different
    tiles (refused, everything as passed); CSR offsets descending, past n_obs and negative (empty lists), negative first ids and counts"""
    base, _ = cached(("sized", 1025), lambda: _sized_cull(1025))                  # cap_recent == 1025
    for n_recent in (-3, 1025 + 7, 1 << 30):
        sc, want = cached(("counter", n_recent), lambda: _with_counter(base, n_recent))
        assert want["n_recent"] == (0 if n_recent < 0 else want["result"][km.P_KEPT]) and (n_recent < 0 or want["result"][km.P_KEPT] > 100)
        _cull(sc, want, stream_kind)
    twice = dict(base, recent=base["recent"].copy())
    twice["recent"][1024] = next(p for p in base["recent"][:9] if 0 <= p < base["world"]["cap_points"])
    want = cached("twice_far", lambda: km.run_cull(twice))
    assert want["result"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    _cull(twice, want, stream_kind)

    def garbage():
        sc = km.make_scene("small")["cull"]
        w, rng = sc["world"], np.random.RandomState(5)
        off = w["obs_off"].copy()
        rows = rng.choice(w["cap_points"] - 2, 40, replace=False) + 1
        off[rows[:20]] += 7
        off[rows[20:30]] = len(w["obs_kf"]) + 5
        off[rows[30:]] = -3
        first, found, visible = sc["first_kf"].copy(), sc["found"].copy(), sc["visible"].copy()
        some = rng.choice(w["cap_points"], 60, replace=False)
        first[some[:20]], found[some[20:40]], visible[some[40:]] = -(1 << 31), -5, -(1 << 31)
        sc = dict(sc, world=dict(w, obs_off=off), first_kf=first, found=found, visible=visible)
        return sc, km.run_cull(sc)

    sc, want = cached("garbage", garbage)
    print("garbage d_result", want["result"].tolist())
    assert not want["result"][km.P_REFUSED]
    _cull(sc, want, stream_kind)


@pytest.mark.parametrize("cap", [1, 524288])
def test_the_culling_at_the_smallest_and_the_largest_table(cap):
    """cap_points 1: a list of the one row and two values that are no row; cap_points 524288: the 64 KB mask"""
    sc, want = cached(("cap", cap), lambda: (lambda s: (s, km.run_cull(s)))(
        km.make_cull_scene(9, 3 if cap == 1 else 300, cap_points=cap, designed=False, n_junk=2 if cap == 1 else 4)))
    print(cap, "d_result", want["result"].tolist())
    assert not want["result"][km.P_REFUSED] and (cap == 1 or ((sc["recent"] > 1 << 18) & (sc["recent"] < cap)).any())
    _cull(sc, want, "explicit")


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------------
NEW_ROWS, MIN_OBS = 40, 2


def _chain_scene():
    """the mid scene's world with one more key-frame slot, K, and NEW_ROWS more rows, the ones a triangulation just appended; the models
    chained: register -> insert -> observations_model.build -> cull -> build -> local_map_model.num_tracked on K"""
    base = km.make_scene("mid")["cull"]
    w0 = base["world"]
    rng = np.random.RandomState(2)
    n_kf, stride, cap0 = w0["n_kf"] + 1, w0["stride"], w0["cap_points"]
    K, cap = n_kf - 1, cap0 + NEW_ROWS
    more = lambda a, fill: np.concatenate([a, np.full(NEW_ROWS, fill, a.dtype)])  # noqa: E731
    valid = more(w0["valid"], 1)
    state = dict(ref_kf=rng.randint(0, K, cap).astype(np.int32), first_kf=more(base["first_kf"], -55), found=more(base["found"], -55),
                 visible=more(base["visible"], -55), recent=np.concatenate([np.where(base["recent"] == cap0, -7, base["recent"])[:base["n_recent"]], np.full(NEW_ROWS + 3, -3, np.int32)]))   # cap0 is a row now
    reg = km.register_new_points(cap, cap0, base["n_recent"], K, base["cur"], cap, state["ref_kf"], state["first_kf"], state["found"],
                                 state["visible"], state["recent"])
    table, calls = km.make_insert_calls(4, cap, valid, stride, n_kf, (stride - 7,))
    table.update(n=np.concatenate([w0["n"], [5]]).astype(np.int32), bad=np.concatenate([w0["bad"], [1]]).astype(np.uint8),
                 slots=np.concatenate([w0["slots"], rng.randint(-1, cap, (1, stride)).astype(np.int32)]))
    call = dict(calls[0], K=K)
    call["frame_mp"][-NEW_ROWS // 2:] = np.arange(cap0, cap0 + NEW_ROWS // 2)     # the new key frame observes half of the new rows
    ins = km.run_insert(table, call, valid, cap)
    cap_obs = int((ins["slots"] >= 0).sum()) + 40
    pad = lambda a: np.concatenate([a, np.zeros(cap_obs - len(a), np.int32)])     # noqa: E731  the arrays' tails are zeros on the device too
    off1, kf1, kp1, b1 = om.build(ins["n"], ins["bad"], ins["slots"], stride, valid, cap, cap_obs)
    w1 = dict(n_kf=n_kf, stride=stride, cap_points=cap, n=ins["n"], bad=ins["bad"], slots=ins["slots"], valid=valid, obs_off=off1, obs_kf=pad(kf1),
              obs_kp=pad(kp1))
    cull = km.cull_map_points(w1, reg["recent"], reg["n_recent"], base["cur"], reg["first_kf"], reg["found"], reg["visible"],
                              code=np.full(len(state["recent"]), -9, np.int32))
    off2, kf2, kp2, b2 = om.build(ins["n"], ins["bad"], cull["slots"], stride, cull["valid"], cap, cap_obs)
    kf2f, kp2f = w1["obs_kf"].copy(), w1["obs_kp"].copy()                          # the second build writes its n_obs entries over the first's
    kf2f[:len(kf2)], kp2f[:len(kp2)] = kf2, kp2
    w2 = dict(w1, slots=cull["slots"], valid=cull["valid"], obs_off=off2, obs_kf=kf2f, obs_kp=kp2f)
    return dict(K=K, cap=cap, cap_obs=cap_obs, n_kf=n_kf, stride=stride, cur=base["cur"], valid=valid, state=state, reg=reg, table=table, call=call,
                ins=ins, b1=b1, cull=cull, b2=b2, w2=w2, count=lm.num_tracked(w2, K, MIN_OBS), n_points0=cap0)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_chain_from_a_tracked_frame_to_the_culled_map_with_one_wait(stream_kind):
    """orbm_register_new_points_device -> orbm_insert_keyframe_device -> orbm_build_observations_device -> orbm_cull_map_points_device ->
    orbm_build_observations_device -> orbm_num_tracked_points_device on K: one stream, no read-back between the calls, ONE wait at the
    end, on the mid scene's world (10 key-frame slots x 160, 940 rows, a list of 240).  Every array and every d_result equals the models
    chained the same way, and the second build's d_obs_off shows the culled rows empty."""
    cs = cached("chain", _chain_scene)
    K, cap, cap_obs, n_kf, stride, cull, w2 = cs["K"], cs["cap"], cs["cap_obs"], cs["n_kf"], cs["stride"], cs["cull"], cs["w2"]
    gone = [int(p) for p, c in zip(cs["reg"]["recent"], cull["code"]) if c in (2, 3)]
    print("register %s insert %s build %s cull %s build %s count %s" % tuple(x.tolist() for x in (cs["reg"]["result"], cs["ins"]["result"], cs["b1"],
                                                                                                  cull["result"], cs["b2"], cs["count"])))
    assert cs["reg"]["result"][km.G_ROWS] == NEW_ROWS and cs["ins"]["result"][km.I_HELD] >= 40 and len(gone) >= 20 and cull["result"][km.P_CLEARED] >= 10
    assert (np.diff(w2["obs_off"])[gone] == 0).all() and cs["count"][0] >= 5 and set(cull["code"][:cs["reg"]["n_recent"]].tolist()) >= {0, 1, 2, 3, 4}
    assert sum(p >= cs["n_points0"] for p in cull["recent"][:cull["n_recent"]]) == NEW_ROWS   # the rows just registered are of age 0: all kept
    call = cs["call"]
    arrays = dict(cs["table"], valid=cs["valid"], frame_mp=call["frame_mp"], frame_pose_R=call["frame_R"], frame_pose_t=call["frame_t"],
                  n_points=_one(cap), n_registered=_one(cs["n_points0"]), n_recent=_one(len(cs["state"]["recent"]) - NEW_ROWS - 3), **cs["state"],
                  code=np.full(len(cs["state"]["recent"]), -9, np.int32), obs_off=np.full(cap + 1, -51, np.int32), obs_kf=np.zeros(cap_obs, np.int32),
                  obs_kp=np.zeros(cap_obs, np.int32), ref=_one(K), count=np.full(4, -51, np.int32),
                  **{k: np.full(8, -51, np.int32) for k in ("r_register", "r_insert", "r_build1", "r_cull", "r_build2")})

    def chain(m, d, st):
        m.RegisterNewPointsDevice(dict(d, result=d["r_register"]), K, cs["cur"], cap, stream=st)
        m.InsertKeyFrameDevice(dict(d, result=d["r_insert"]), K, stride, cap, len(call["frame_mp"]), call["frame_kps"], call["frame_desc"], stream=st)
        m.BuildObservationsDevice(dict(d, result=d["r_build1"]), n_kf, stride, cap, cap_obs, stream=st)
        m.CullMapPointsDevice(dict(d, result=d["r_cull"]), cs["cur"], n_kf, stride, cap, cap_obs, stream=st)
        m.BuildObservationsDevice(dict(d, result=d["r_build2"]), n_kf, stride, cap, cap_obs, stream=st)
        m.NumTrackedPointsDevice(d, n_kf, stride, cap, cap_obs, MIN_OBS, stream=st)

    want = dict(cs["ins"], **{k: cs["reg"][k] for k in ("ref_kf", "first_kf", "found", "visible")}, n_registered=_one(cap),
                n_recent=_one(cull["n_recent"]), recent=cull["recent"], code=cull["code"], valid=cull["valid"], slots=cull["slots"],
                obs_off=w2["obs_off"], obs_kf=w2["obs_kf"], obs_kp=w2["obs_kp"], count=cs["count"], r_register=cs["reg"]["result"],
                r_insert=cs["ins"]["result"], r_build1=cs["b1"], r_cull=cull["result"], r_build2=cs["b2"])
    del want["result"]
    runs = [_run(arrays, stream_kind, chain) for _ in range(2)]
    _same(runs[0], arrays, want)
    _same(runs[1], arrays, want)
