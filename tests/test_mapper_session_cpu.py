"""tests/mapper_session.py without a GPU: the session on the composed array models against the session on KeyFrame / MapPoint objects after
every key frame, the events the sessions were designed for, and that the array session is a function of its inputs.  The BA estimate is
oracle/ba_ref.py's LM on the model's problem arrays, the triangulation's floats are triangulation_model.evaluate's in float32."""
import pytest

import local_ba_model as lbm
import mapper_session as ms
import observations_model as om

_cache = {}


def _session(name):
    """the array session and, for the two full sessions, the object session beside it: run once, shared, never changed.
    -> dict(tags, differences: per key frame the list objects_describe_the_arrays returns, logs, bytes: the state's after every key frame)"""
    if name in _cache:
        return _cache[name]
    world = ms.World(name)
    s = ms.initial_state(world)
    with_objects = name in ("main", "kb")
    ow = ms.initial_objects(world) if with_objects else None
    out = dict(world=world, tags={}, differences=[ms.objects_describe_the_arrays(ow, s)] if with_objects else [], logs=[], bytes=[], structures=[])
    seen, memo = [ms.copy_state(s), ms.copy_state(s)], {}
    for K in range(2, world.cfg["n_kf"]):
        frame = world.frame(K, seen[-2])
        be, numbers = ms.ArrayBackend(s), {}

        def after(name, _):
            if name == "build2":                                           # the table's floats as the fuse finds them
                numbers["floats"] = {k: s[k].copy() for k in ("points", "normals", "min_dist", "max_dist", "desc")}

        log = ms.step(be, frame, world, after=after, tags=out["tags"], memo=memo)
        seen.append(ms.copy_state(s))
        out["logs"].append(log)
        out["bytes"].append(ms.state_bytes(s))
        if with_objects:
            numbers.update(prob=be.prob, est=be.est if "ba_solve" in dict(log) else None)
            structure = ms.step_objects(ow, frame, numbers)
            out["structures"].append(structure)
            out["differences"].append(ms.objects_describe_the_arrays(ow, s, be.prob, structure, be.replays))
    out["state"], out["objects"] = s, ow
    _cache[name] = out
    return out


@pytest.mark.parametrize("name", ["main", "kb"])
def test_the_objects_and_the_arrays_describe_the_same_map_after_every_key_frame(name):
    """the observation sets per point, the slots per key frame, bad and valid flags, ref_kf, first_kf and the two counters, the
    covisibility lists and parents, the recent list in order, the local BA's key frames, points and edges, and the Map::eraseMapPoint /
    Map::eraseKeyFrame replays: the object session, which follows LocalMapping.cpp:47-372 and knows nothing of slots, CSR offsets or
    tombstones, and the composed array models agree after the initial map and after each of the key frames behind it"""
    run = _session(name)
    assert len(run["differences"]) == run["world"].cfg["n_kf"] - 1
    for K, diff in zip(range(1, run["world"].cfg["n_kf"]), run["differences"]):
        assert not diff, "session %s, after key frame %d: %s" % (name, K, diff[:8])
    assert sum(st["edges"] is not None for st in run["structures"]) >= len(run["structures"]) - 1 and len(run["objects"]["map"].erased_points) >= 20


def test_the_comparison_of_objects_and_arrays_can_fail():
    """the same main session with MapPoint::eraseObservation leaving reference_kf alone: reported at the first key frame whose culling
    moves one"""
    run = _session("main")
    world = run["world"]
    s, ow = ms.initial_state(world), ms.initial_objects(world)
    seen, found = [ms.copy_state(s), ms.copy_state(s)], None
    for K in range(2, world.cfg["n_kf"]):
        frame = world.frame(K, seen[-2])
        be, numbers = ms.ArrayBackend(s), {}
        log = ms.step(be, frame, world, after=lambda name, _: numbers.update(floats={k: s[k].copy() for k in ("points", "normals", "min_dist", "max_dist", "desc")})
                      if name == "build2" else None)
        seen.append(ms.copy_state(s))
        numbers.update(prob=be.prob, est=be.est if "ba_solve" in dict(log) else None)
        for mp in ow["mps"]:
            mp.erase_observation = _erase_without_the_reference_move.__get__(mp)
        ms.step_objects(ow, frame, numbers)
        diff = ms.objects_describe_the_arrays(ow, s)
        if diff:
            found = (K, diff)
            break
    assert found and found[0] == run["tags"]["kf_cull_cascade"] and any(d.startswith("ref_kf") for d in found[1]), found


def _erase_without_the_reference_move(self, kf):
    if kf in self.observations:
        del self.observations[kf]
        if self.get_num_obs() <= 2:
            self.set_bad()


def test_every_event_occurs_in_the_main_session_and_no_capacity_is_reached():
    run = _session("main")
    tags = run["tags"]
    print(sorted(tags.items(), key=lambda kv: kv[1]))
    assert set(tags) == ms.ALL_TAGS, (ms.ALL_TAGS - set(tags), set(tags) - ms.ALL_TAGS)
    assert all(2 <= K < run["world"].cfg["n_kf"] for K in tags.values())
    for log in run["logs"]:                                                 # every build fits, every triangulation fits, no call refuses
        for name, out in log:
            res = out.get("result")
            if res is None:
                continue
            assert not (name.startswith("build") and res[om.OVERFLOW]) and not (name.startswith("triangulate") and res[1]), name
            assert not (name.startswith("fuse_") and name != "fuse_targets" and res[1]) and not (name == "ba_problem" and res[lbm.P_REFUSED]), name
            assert not (name in ("register", "cull_map_points") and res[1]), name


@pytest.mark.parametrize("name", sorted(ms.OVERFLOW_TAGS))
def test_the_two_short_sessions_hit_their_overflow_where_designed_and_go_on(name):
    """table_full: the point table runs full inside key frame 3's second triangulation -- nothing is written, the third is refused too, and
    the step and key frame 4 run on the rows there are.  csr_overflow: cap_obs overflows at a build of key frame 3 -- behind it every
    list is empty, and the docstring of tests/mapper_session.py says what each call then does; key frame 4 follows."""
    run = _session(name)
    tags, last = run["tags"], run["world"].cfg["n_kf"] - 1
    if name == "csr_overflow_late":
        return _late_overflow(run)
    assert tags.get(name) == 3 and last >= 4 and not (ms.OVERFLOW_TAGS - {name}) & set(tags), tags
    at = dict(run["logs"][tags[name] - 2])
    if name == "table_full":
        tri = [(n, o["result"]) for n, o in run["logs"][1] if n.startswith("triangulate")]
        assert [int(r[1]) for _, r in tri] == [0, 1, 1] and tri[0][1][0] > 0 and all(r[0] == 0 for _, r in tri[1:]), tri
        assert run["state"]["n_points"] <= run["world"].cfg["cap_points"] and at["register"]["result"][0] == tri[0][1][0]
    else:
        import graph_model as gm
        import keyframe_model as km
        import refresh_model as rm
        assert at["build"]["result"][om.OVERFLOW] and at["build"]["result"][om.NOBS] > run["world"].cfg["cap_obs"]   # the step's first build
        held = int(at["insert"]["result"][km.I_HELD])
        assert at["refresh"]["result"][rm.DONE] == 0 and at["refresh"]["result"][rm.NONE] == held > 0       # every list is empty: no row written
        assert at["update"]["result"][gm.U_NOTHING] == 1                                                     # d_covis is all zero
        cull = at["cull_map_points"]["result"]
        assert cull[km.P_FEW] > 0 and cull[km.P_CLEARED] == 0      # getNumObs() == 0: every row of age >= 2 goes bad, and no list names a slot to clear
        assert not at["build2"]["result"][om.OVERFLOW] and at["build2"]["result"][om.SKIP_INVALID] >= cull[km.P_FEW]   # their slots still name them
        later = dict(run["logs"][2])
        assert not any(o["result"][om.OVERFLOW] for n, o in later.items() if n.startswith("build")) and not later["ba_problem"]["result"][lbm.P_REFUSED]


def _late_overflow(run):
    """csr_overflow_late: key frame 2's builds fit ahead of the fuse and overflow behind it, so the second refresh, the second graph update,
    the BA assembly, KeyFrameCulling and the erase run behind empty lists; key frames 3 and 4 follow (3 opens with an overflow of its own)"""
    import graph_model as gm
    import refresh_model as rm
    tags = run["tags"]
    assert tags["csr_overflow_late"] == 2 and tags.get("csr_overflow", 9) > 2 and "table_full" not in tags, tags
    names, at = [n for n, _ in run["logs"][0]], dict(run["logs"][0])
    assert not at["build"]["result"][om.OVERFLOW] and not at["build2"]["result"][om.OVERFLOW] and at["build3"]["result"][om.OVERFLOW]
    assert at["refresh2"]["result"][rm.DONE] == 0 and at["refresh2"]["result"][rm.NONE] > 0 and at["update2"]["result"][gm.U_NOTHING] == 1
    res, local = at["ba_problem"]["result"], at["connected"]["local"]
    n_local = int((local >= 0).sum())
    assert res[lbm.P_REFUSED] == lbm.REFUSE_NO_EDGE and res[lbm.P_POINTS] == 0 and res[lbm.P_EDGES] == 0
    assert res[lbm.P_POSES] == res[lbm.P_LOCAL] == n_local >= 2 and res[lbm.P_FIXED] == 0 and res[lbm.P_LOCAL_DROPPED] == len(local) - n_local
    before = _state_before_the_ba(run)                                      # every valid row a local key frame names, once: no edge
    rows = {int(p) for k in local[:n_local] for p in before["table"]["slots"][k, :before["table"]["n"][k]] if p >= 0 and before["valid"][p]}
    assert res[lbm.P_NO_EDGE] == len(rows) > 50
    assert not {"ba_solve", "ba_apply", "build4", "refresh3"} & set(names) and names[-2:] == ["cull_keyframes", "erase"]
    cull = at["cull_keyframes"]
    valid_slots = sum(1 for p in before["table"]["slots"][1, :before["table"]["n"][1]] if p >= 0 and before["valid"][p])
    assert cull["code"].tolist() == [-1, 0, -1] and cull["num_mp"].tolist() == [0, valid_slots, 0] and not cull["num_redundant"].any()
    assert cull["result"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and not at["erase"]["result"].any()
    assert len(run["logs"]) == 3 and not dict(run["logs"][2])["ba_problem"]["result"][lbm.P_REFUSED]   # the session goes on, and recovers


def _state_before_the_ba(run):
    """the late session's state when key frame 2's BA assembly runs: nothing behind it writes the map in that step"""
    world = run["world"]
    s = ms.initial_state(world)
    ms.step_arrays(s, world.frame(2, ms.copy_state(s)), world)
    return s


def test_the_array_session_twice_gives_the_same_bytes():
    first = _session("main")["bytes"]
    kept = _cache.pop("main")
    try:
        again = _session("main")["bytes"]
    finally:
        _cache["main"] = kept
    assert len(first) == len(again) == 10 and all(a == b for a, b in zip(first, again))


def test_the_session_is_small():
    """the sizes the issue asks for: a stride of 64 to 96, 10 to 14 key frames, a key-frame table a little above them"""
    for name, cfg in ms.SESSIONS.items():
        assert 64 <= cfg["stride"] <= 96 and cfg["n_kf"] < cfg["cap_kf"] <= cfg["n_kf"] + 2, name
    assert 10 <= ms.SESSIONS["main"]["n_kf"] <= 14 and 3 <= ms.SESSIONS["table_full"]["n_kf"] - 2 <= 5 and 3 <= ms.SESSIONS["csr_overflow"]["n_kf"] - 2 <= 5
