"""The two restatements of the inertial window's assembly in tests/inertial_window_model.py against each other on the seeded scenes, the
cap of the fixed key frames where it bites, the refusals and the velocity prior.  No GPU."""
import numpy as np
import pytest

import inertial_window_model as wm

_cache = {}
FRESH = tuple(n for n in wm.SCENES if n not in ("stale", "forged"))     # the object form knows no CSR


def scene(name):
    """(scene, CSR, array form): computed once, shared, never changed"""
    if name not in _cache:
        sc, csr = wm.make(name)
        _cache[name] = (sc, csr, wm.problem(sc, csr))
    return _cache[name]


@pytest.mark.parametrize("name", FRESH)
def test_the_array_form_equals_the_object_form(name):
    """solve states in window order, the fixed key frames as a SET (the array form's are in ascending slot order), local rows in
    first-occurrence order, every row's edges, the edges behind the cap against the reference's null vertices, and the inertial side:
    the edges' states and pre-integrators, the prior's key frame, the chaining of step 7"""
    sc, csr, a = scene(name)
    o = wm.problem_objects(sc)
    res, imu = a["result"], sc["kf_imu"]
    print(name, "d_result", res.tolist())
    n_solve = res[wm.W_SOLVE]
    assert res[wm.W_REFUSED] == 0 and a["state_kf"][:n_solve].tolist() == o["solve"] == sc["window"].tolist()
    assert a["state_kf"][n_solve:].tolist() == sorted(o["fixed"]) and res[wm.W_FIXED] == len(o["fixed"]) and res[wm.W_CAPPED] == o["null"]
    assert a["point_row"].tolist() == o["rows"]
    off = a["edge_off"]
    for x, mine in enumerate(o["edges"]):
        assert list(zip(a["edge_kf"][off[x]:off[x + 1]].tolist(), a["edge_kp"][off[x]:off[x + 1]].tolist())) == mine
        assert (a["edge_point"][off[x]:off[x + 1]] == x).all()
    assert (a["state_kf"][a["edge_state"]] == a["edge_kf"]).all() and (np.diff(a["edge_point"]) >= 0).all() and off[-1] == res[wm.W_EDGES]
    assert [(i, j, imu[k][1], wm.EDGE_WALKS) for i, j, k in o["inertial"]] == [tuple(e) for e in a["inertial_edges"].tolist()]
    assert a["prior_jobs"].tolist() == [[0, imu[o["priors"][0]][2], wm.PRIOR_ALL]] and len(o["priors"]) == 1
    assert a["prior_info_jobs"].tolist() == [[imu[k][2], imu[before][1], imu[k][0]] for k, before in o["chain"]]
    assert a["recover_jobs"].tolist() == [[s, imu[k][0], wm.RECOVER_POSE] for s, k in enumerate(o["solve"])]
    assert a["bias_ids"].tolist() == [imu[k][1] for k in o["solve"]]
    assert a["init_jobs"].tolist() == [[q, imu[k][0], imu[k][1] if q < n_solve else -1] for q, k in enumerate(a["state_kf"])]
    assert a["fixed"].tolist() == [0] * n_solve + [wm.FIX_ALL] * len(o["fixed"])


def test_the_scenes_exercise_what_they_claim():
    """the cap scenes' max_fixed lies below the number of key frames that could be fixed and the others' does not; max_fixed = 2 is
    reached exactly at a point boundary, 3 in mid-scene with edges dropped behind the cap, 1 is overshot by a point with two observers;
    a row with a key frame twice, a row without an edge, CSR entries out of range, a point of 257 edges, more than 1024 window slots"""
    for name in wm.SCENES:
        sc, _, a = scene(name)
        res = a["result"]
        assert (res[wm.W_CANDIDATES] > sc["max_fixed"]) == (name in wm.CAP_SCENES), name
        assert (res[wm.W_CAPPED] > 0) == (name in wm.CAP_SCENES), name
    r = {name: scene(name)[2]["result"] for name in wm.SCENES}
    assert r["cap2"][wm.W_FIXED] == 2 and r["cap3"][wm.W_FIXED] == 3 and r["cap1"][wm.W_FIXED] == 2 and r["window3"][wm.W_FIXED] == 4
    assert r["cap3"][wm.W_EDGES] < r["window3"][wm.W_EDGES] and r["cap3"][wm.W_POINTS] == r["window3"][wm.W_POINTS]
    assert r["window3"][wm.W_SECOND] == 1 and r["stale"][wm.W_NO_EDGE] == 1 and r["stale"][wm.W_CSR_DROPPED] == 30
    assert r["forged"][wm.W_CSR_DROPPED] == 3 and r["forged"][wm.W_NO_EDGE] == 2
    assert r["long"][wm.W_LONG] == 1 and r["long"][wm.W_EDGES] == 260 + 3 and r["window1"][wm.W_SOLVE] == 1
    sc = scene("tiles")[0]
    assert len(sc["window"]) * sc["stride"] > 1024 and r["tiles"][wm.W_POINTS] > 400
    assert scene("window1")[2]["inertial_edges"].shape == (0, 4) and scene("window1")[2]["prior_info_jobs"].shape == (0, 3)


@pytest.mark.parametrize("name", wm.CAP_SCENES)
def test_an_exclusive_cap_would_differ_from_the_reference(name):
    """X taken exclusive leaves out the observers of the point at which the reference breaks: the two forms would differ"""
    sc, csr, a = scene(name)
    wrong = wm.problem(sc, csr, inclusive=False)
    o = wm.problem_objects(sc)
    assert wrong["result"][wm.W_FIXED] < len(o["fixed"]) == a["result"][wm.W_FIXED]


def test_the_refusals():
    """each capacity keeps the full counts; an unusable window entry (out of range, bad, repeated) stops the call at the window; each
    d_kf_imu index of a window key frame and the state row of a fixed one; no edge"""
    sc, csr, a = scene("window3")
    full = a["result"]
    for cap, bit in ((dict(cap_states=full[wm.W_STATES] - 1), wm.REFUSE_STATES), (dict(cap_local_points=full[wm.W_POINTS] - 1), wm.REFUSE_POINTS),
                     (dict(cap_edges=full[wm.W_EDGES] - 1), wm.REFUSE_EDGES)):
        r = wm.problem(sc, csr, **cap)
        assert r["result"][wm.W_REFUSED] == bit and r["ba_points"] is None and (r["result"][:5] == full[:5]).all()
    for window in ([sc["window"][0], len(sc["n"]), sc["window"][2]], [sc["window"][0], sc["roles"]["bad"]], [sc["window"][1], sc["window"][0], sc["window"][1]],
                   [-1]):
        r = wm.problem(dict(sc, window=np.array(window, np.int32)), csr)["result"]
        assert r[wm.W_REFUSED] == wm.REFUSE_WINDOW and r[wm.W_WINDOW_UNUSABLE] == 1 and r[wm.W_SOLVE] == len(window) and r[wm.W_POINTS] == 0
    for k, c, v in ((sc["window"][1], 0, sc["n_src"]), (sc["window"][0], 1, -1), (sc["window"][2], 2, sc["n_priors"]), (a["state_kf"][4], 0, -2)):
        imu = sc["kf_imu"].copy()
        imu[k, c] = v
        r = wm.problem(dict(sc, kf_imu=imu), csr)["result"]
        assert r[wm.W_REFUSED] == wm.REFUSE_IMU and r[wm.W_IMU_RANGE] == 1 and (r[:5] == full[:5]).all()
    imu = sc["kf_imu"].copy()
    imu[a["state_kf"][4], 1:] = -7                                         # a fixed key frame's record and prior slot are not read
    assert wm.problem(dict(sc, kf_imu=imu), csr)["result"][wm.W_REFUSED] == 0
    nothing = dict(sc, valid=np.zeros_like(sc["valid"]))
    assert wm.problem(nothing, csr)["result"][wm.W_REFUSED] == wm.REFUSE_NO_EDGE


def test_the_velocity_prior_touches_three_floats():
    rng = np.random.RandomState(1)
    priors, src = rng.uniform(-1, 1, (5, 36)).astype(np.float32), rng.uniform(-1, 1, (7, 15)).astype(np.float32)
    after, res = wm.velocity_prior(priors, src, [[0, 6, 1]], [[0, 3, 15]])
    assert res.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (after[3, :3] == src[6, 12:]).all()
    after[3, :3] = priors[3, :3]
    assert after.tobytes() == priors.tobytes()
    for jobs in (([[0, 7, 1]], [[0, 3, 15]]), ([[0, 6, 1]], [[0, 5, 15]]), ([[0, -1, 1]], [[0, 0, 15]])):
        after, res = wm.velocity_prior(priors, src, *jobs)
        assert res.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and after.tobytes() == priors.tobytes()


def test_a_loop_scene_laid_out_as_a_map_is_reproduced_by_the_assembly():
    """tests/inertial_loop.py's converging window (3 solve + 2 fixed states, 63 points) as slots, key points, CSR and state rows: both
    forms of the assembly give the scene back up to the stated point order -- the order is a permutation, not the identity -- and the
    window scene rebuilt from the assembly carries a model loop"""
    import inertial_loop as il
    import local_ba_model as lm
    sc = wm.map_from_window_scene(il.scene(il.CONVERGING))
    csr = lm.fresh_csr(sc)
    a = wm.problem(sc, csr)
    perm = wm.reproduces(sc, a)
    assert perm != sorted(perm) and sc["kf_of_state"][:3] != sorted(sc["kf_of_state"][:3])
    o = wm.problem_objects(sc)
    assert o["rows"] == a["point_row"].tolist() and sorted(o["fixed"]) == a["state_kf"][3:].tolist() and o["null"] == 0
    ws = wm.window_scene_of(sc, a)
    r = il.run(il.CONVERGING, il.ModelWindow(ws))
    assert r["rounds"][0]["accepted"] >= 5 and il.flat_from(r["rounds"][0]["trace"]) >= 5
