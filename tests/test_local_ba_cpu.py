"""The two restatements of the local bundle adjustment's assembly and apply in tests/local_ba_model.py against each other, the scenes'
engineered branches (with the numpy LM of oracle/ba_ref.py as the optimiser), the refusals, and the declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

import local_ba_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUBER = float(np.sqrt(np.float32(5.991)))
_cache = {}


def scene(name):
    """(scene, fresh CSR, model problem, oracle LM result, model apply): computed once, shared, never changed"""
    if name not in _cache:
        from oracle import ba_ref
        sc = lm.make_scene(**lm.SCENES[name])
        csr = lm.fresh_csr(sc)
        prob = lm.problem(sc, csr)
        ba = ba_ref.local_bundle_adjustment(sc["cam"], prob["pose_R"].reshape(-1, 3, 3), prob["pose_t"], prob["pose_fixed"], prob["ba_points"],
                                            prob["edge_pose"], prob["edge_point"], prob["edge_z"], prob["edge_inv_sigma2"], HUBER)
        est = (ba["pose_R"].reshape(-1, 9), ba["pose_t"], ba["points"], ba["outlier"].astype(np.uint8))
        _cache[name] = (sc, csr, prob, est, lm.apply(sc, csr, prob, *est))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_the_assembly_equals_the_objects_and_holds_its_branches(name):
    """local key frames, local rows in first-occurrence order and every row's edges equal the object form's; the fixed key frames are
    the same SET, in ascending slot order; the scene has a bad, an out-of-range and a duplicate entry in d_local, first_kf where its
    name says, a row twice in a key frame, invalid rows, about 150 points and 500 edges"""
    sc, csr, prob, _, _ = scene(name)
    res = prob["result"]
    print(name, "d_result", res.tolist())
    local, fixed, rows, edges = lm.problem_objects(sc)
    n_loc = res[lm.P_LOCAL]
    assert prob["pose_kf"][:n_loc].tolist() == local and sorted(fixed) == prob["pose_kf"][n_loc:].tolist()
    assert prob["point_row"].tolist() == rows
    off = prob["edge_off"]
    for x, mine in enumerate(edges):
        assert list(zip(prob["edge_kf"][off[x]:off[x + 1]].tolist(), prob["edge_kp"][off[x]:off[x + 1]].tolist())) == mine
        assert (prob["edge_point"][off[x]:off[x + 1]] == x).all()
    assert (prob["pose_kf"][prob["edge_pose"]] == prob["edge_kf"]).all() and (np.diff(prob["edge_point"]) >= 0).all()
    assert res[lm.P_REFUSED] == 0 and res[lm.P_LOCAL] == 4 and res[lm.P_FIXED] == 3 and res[lm.P_LOCAL_DROPPED] == 3 and res[lm.P_LOCAL_BAD] == 1
    assert res[lm.P_SECOND] == 1 and 130 <= res[lm.P_POINTS] <= 200 and 400 <= res[lm.P_EDGES] <= 700
    first_local = sc["first_kf"] in local
    assert first_local == lm.SCENES[name]["first_local"] and prob["pose_fixed"].sum() == 3 + first_local
    ex = sc["expect"]
    assert ex["only_bad"] not in rows and ex["far"] not in rows and ex["twice"] in rows and not set(np.flatnonzero(sc["valid"] == 0)) & set(rows)
    x = rows.index(ex["twice"])
    assert off[x + 1] - off[x] == 3 and (sc["slots"] == ex["twice"]).sum() == 4


@pytest.mark.parametrize("name", sorted(lm.SCENES))
def test_the_apply_equals_the_objects_and_holds_its_branches(name):
    """slots, validity, reference key frames, positions, poses and counts equal what the objects are left with; the optimiser finds
    the engineered outliers: a reference key frame moves, a point falls to two observations and goes bad, a second outlier edge finds
    its point bad"""
    sc, csr, prob, est, a = scene(name)
    b = lm.apply_objects(sc, prob, *est)
    print(name, "d_result", a["result"].tolist(), "outliers", int(est[3].sum()), "found bad", a["found_bad"])
    for key in ("slots", "valid", "ref_kf", "points", "pose_R", "pose_t"):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    for r in (lm.A_ERASED, lm.A_POINTS_BAD, lm.A_CLEARED, lm.A_MOVED, lm.A_ROWS, lm.A_POSES):
        assert a["result"][r] == b["result"][r], r
    assert (a["found_bad"] > 0) == (b["found_bad"] > 0)
    ex, res = sc["expect"], a["result"]
    assert res[lm.A_ERASED] >= 3 and res[lm.A_POINTS_BAD] >= 2 and res[lm.A_CLEARED] >= 4 and res[lm.A_MOVED] >= 1 and a["found_bad"] >= 1
    assert a["valid"][ex["ref_outlier"]] and a["ref_kf"][ex["ref_outlier"]] != sc["ref_kf"][ex["ref_outlier"]]
    assert (a["slots"] == ex["ref_outlier"]).sum() == 4
    for name_ in ("falls_to_two", "two_outliers"):
        assert not a["valid"][ex[name_]] and (a["slots"][:, :sc["stride"] - 4] == ex[name_]).sum() == 0, name_
    x = prob["point_row"].tolist().index(ex["two_outliers"])
    assert est[3][prob["edge_off"][x]:prob["edge_off"][x + 1]].sum() >= 2
    assert res[lm.A_POSES] == prob["result"][lm.P_LOCAL] and res[lm.A_ROWS] == prob["result"][lm.P_POINTS] - res[lm.A_POINTS_BAD]
    fixed = prob["pose_kf"][prob["result"][lm.P_LOCAL]:]
    assert a["pose_R"][fixed].tobytes() == sc["pose_R"][fixed].tobytes() and (a["pose_R"] != sc["pose_R"]).any() and (a["points"] != sc["points"]).any()


def test_a_stale_csr_and_the_refusals():
    """edits the CSR does not know: a row named by a local key frame without a usable entry is dropped (no edge), a stale entry gives no
    edge, unusable entries are counted; each capacity refusal and the no-free-pose refusal keep the full counts"""
    sc, csr, prob, _, _ = scene("first_local")
    stale, spoilt, junk = lm.stale_scene(sc, csr)
    got = lm.problem(stale, spoilt)
    res = got["result"]
    assert res[lm.P_NO_EDGE] == 1 and res[lm.P_CSR_DROPPED] == junk and res[lm.P_EDGES] == prob["result"][lm.P_EDGES] - 1
    assert stale["expect"]["no_edge"] not in got["point_row"].tolist() and got["point_row"].tolist() == prob["point_row"].tolist()
    full = prob["result"]
    for cap, bit in ((dict(cap_poses=full[lm.P_POSES] - 1), lm.REFUSE_POSES), (dict(cap_local_points=full[lm.P_POINTS] - 1), lm.REFUSE_POINTS),
                     (dict(cap_edges=full[lm.P_EDGES] - 1), lm.REFUSE_EDGES)):
        r = lm.problem(sc, csr, **cap)
        assert r["result"][lm.P_REFUSED] == bit and r["pose_R"] is None and (r["result"][:5] == full[:5]).all()
    alone = dict(sc, local=np.array([sc["first_kf"]], np.int32))
    assert lm.problem(alone, csr)["result"][lm.P_REFUSED] == lm.REFUSE_NO_FREE_POSE
    nothing = dict(sc, valid=np.zeros_like(sc["valid"]))
    assert lm.problem(nothing, csr)["result"][lm.P_REFUSED] & lm.REFUSE_NO_EDGE


def test_the_headers_declare_the_entry_points_and_the_wrappers_exist():
    def declared(header):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(orb(?:m|ba)_[a-z0-9_]+)\s*\(", txt))
    assert {"orbm_local_ba_problem_device", "orbm_local_ba_apply_device"} <= declared("orbm.h")
    assert "orbba_local_bundle_adjustment_device" in declared("orbba.h")
    assert "BA on the host" not in open(os.path.join(ROOT, "include", "orbm.h")).read()
    from monoorbslam3_amd import ba, matcher
    assert callable(matcher.local_ba_problem_device) and callable(matcher.local_ba_apply_device) and callable(ba.local_bundle_adjustment_device)
    assert callable(matcher.ORBMatcher.LocalBaProblemDevice) and callable(matcher.ORBMatcher.LocalBaApplyDevice)
