"""The Levenberg-Marquardt loops of the inertial optimisers closed on the MI355X: tests/inertial_loop.py's device back-ends run FREE --
their own decisions from their own read-backs, no state uploaded after the start -- against the model loop of the same scene.  The
decisions are equal; the final estimate lies within 4 x MEASURED_SPREAD of tests/test_inertial_loop_cpu.py per output and every trial's
read-backs within 4 x its "total" entry (one scene excepted, OWN_TRIAL_SPREAD says why)
(the model's own sensitivity to a stage error of 1e-9, never the device's result), and no bar is tighter than BAR, the stage bar.
On the scenes that reach their minimum the sequence is compared up to inertial_loop.flat_from().  Every buffer sits between guard
elements.  Model runs are computed once per scene and shared.  The largest deviation met and the trial count are printed per scene."""
import time

import numpy as np
import pytest

import factors_model as fm
import inertial_loop as il
import vi_model as vm
from test_inertial_loop_cpu import MEASURED_SPREAD, MEASURED_STATIONARITY, TRIAL, trial_deviation

pytestmark = pytest.mark.gpu

_cache = {}


# The one scene whose per-trial read-backs are held to their own measured spread ("trial lam" / "trial total" / "trial scale") instead of the
# final total's: beLarge starts at lambda 1e-2 and 25 iterations take it down to 2e-5 against an inertial information of 1e14, so a trial
# in the middle of the route is 1e4 times as sensitive as the total at its end (1.9e-2 against 7.0e-7 under the 1e-9 perturbation), and the
# device's rounding alone puts lambda 7.5e-6 and the scale 1.2e-5 off the model's.  Of the seeds 1 to 13 of this shape only two give
# every point three observers, and the other has a decision on |rho| < 1e-3.  Every other scene is held to 4 x the total's spread.
OWN_TRIAL_SPREAD = ("window 4+3 65 large",)


def _bar(name, key):
    """4 x the model's measured spread, never below the stage bar; a trial's read-backs against the spread of the final total"""
    if key in TRIAL and name not in OWN_TRIAL_SPREAD:
        key = "total"
    return max(4 * MEASURED_SPREAD[name][key], il.BAR)


def _device_run(name, stream_kind="explicit", audit=False, cached=True):
    import torch
    key = (name, stream_kind, audit)
    if key in _cache and cached:
        return _cache[key]
    be = il.device_backend(torch, torch.device("cuda", 0), name, stream_kind, audit)
    t0 = time.perf_counter()
    r = il.run(name, be)
    r["seconds"], r["n_trials"], r["dx_zero"] = time.perf_counter() - t0, be.n_trials, be.dx_zero
    be.finish()                                                          # the guards of every buffer of the loop
    _cache[key] = r
    return r


def _same_run(a, b):
    assert [x["trace"] for x in a["rounds"]] == [x["trace"] for x in b["rounds"]]
    for x, y in zip(a["rounds"], b["rounds"]):
        for k, v in (x.get("classification") or {}).items():
            assert np.asarray(v).tobytes() == np.asarray(y["classification"][k]).tobytes(), ("classification", k)
    for k, v in a["estimate"].items():
        assert v.tobytes() == b["estimate"][k].tobytes(), k


def _compare(name, dev):
    """the device loop against the model loop: decisions, every trial's read-backs, the classification, the final estimate, the counters"""
    ref, sc, driver = il.model_run(name), il.scene(name), il.SCENES[name][0]
    worst = dict.fromkeys(TRIAL, 0.0)
    assert len(dev["rounds"]) == len(ref["rounds"])
    for n, (x, y) in enumerate(zip(dev["rounds"], ref["rounds"])):
        flat = il.flat_from(y["trace"]) if name in il.CONVERGED else len(y["trace"])
        assert len(x["trace"]) >= flat, (name, "round", n, len(x["trace"]), flat)
        for k, (a, b) in enumerate(zip(x["trace"][:flat], y["trace"][:flat])):
            where = "%s, round %d, trial %d (iteration %d, trial %d of it)" % (name, n, k, b[0], b[1])
            assert a[:2] == b[:2] and a[7] == b[7], (where, "the solve was refused" if b[7] else "the solve was not refused", a, b)
            for key, dv in zip(TRIAL, trial_deviation(a, b)):
                worst[key] = max(worst[key], dv)
                assert dv <= _bar(name, key), (where, key, dv, _bar(name, key), dict(zip(il.FIELDS, a)), dict(zip(il.FIELDS, b)))
            assert a[-1] == b[-1], (where, "accepted" if a[-1] else "rejected", "rho %.6g, the model's %.6g" % (a[6], b[6]))
        if name not in il.CONVERGED:
            assert x["iterations"] == y["iterations"] and len(x["trace"]) == len(y["trace"]), (name, n)
        c, m = x.get("classification"), y.get("classification")
        if m is not None:
            near = np.abs(m["chi2"] - vm.CHI2_MONO) <= 1e-6 * vm.CHI2_MONO
            assert near.mean() <= 0.01
            key = "outlier" if "outlier" in m else "active"
            assert np.array_equal(c[key][~near], m[key][~near]), (name, "round", n, np.nonzero(c[key] != m[key])[0])
            count = "n_outliers" if "outlier" in m else "n_inliers"
            assert abs(c[count] - m[count]) <= near.sum() and c[count] == (c[key] != 0).sum(), (name, n, c[count], m[count])
    est, want = dev["estimate"], ref["estimate"]
    for o in il.STATE + (("points",) if "points" in want else ()):
        scale = np.abs(want[o]).max()
        worst[o] = float(np.abs(est[o] - want[o]).max() / scale) if scale else float(np.abs(est[o]).max())
        assert worst[o] <= _bar(name, o), (name, o, worst[o], _bar(name, o))
    last = lambda r: min([t[4] for t in r["rounds"][-1]["trace"] if t[-1]] + [r["rounds"][-1]["trace"][0][3]])  # noqa: E731
    worst["total"] = abs(last(dev) - last(ref)) / last(ref)
    assert worst["total"] <= _bar(name, "total"), (name, worst["total"])
    if MEASURED_SPREAD[name]["lam"] is not None:
        worst["lam"] = abs(dev["rounds"][-1]["lam"] - ref["rounds"][-1]["lam"]) / ref["rounds"][-1]["lam"]
        assert worst["lam"] <= _bar(name, "lam"), (name, worst["lam"])
    assert dev["refused"] == ref["refused"] or name in il.CONVERGED
    # the counters: (accepted updates mod 3) per free pose -- of the last round where the pose is reset before each; what is fixed keeps its bytes
    g = sc["graph"]
    accepted = dev["rounds"][-1]["accepted"] if driver == "pose_full" else sum(x["accepted"] for x in dev["rounds"])
    free_pose = (g.fixed & fm.FIX_POSE) == 0
    assert np.array_equal(est["iter"], np.where(free_pose, accepted % 3, 0)), (name, est["iter"], accepted)
    for o, bit in zip(il.STATE, (fm.FIX_POSE, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC)):
        fx = (g.fixed & bit) != 0
        assert est[o][fx].tobytes() == getattr(g, o)[fx].tobytes(), (name, o, "a fixed vertex moved")
    print("%s: %d trials in %.2f s, %s" % (name, dev["n_trials"], dev["seconds"], " ".join(il.decisions(dev["rounds"]))))
    print("    largest deviation " + ", ".join("%s %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", list(il.SCENES))
def test_the_free_running_device_loop_is_the_models(name):
    _compare(name, _device_run(name))


@pytest.mark.parametrize("name,stream_kind", [("window 3+2 65 fisheye", "explicit"), ("window 3+2 63 converging", "null"), ("pose inertial", "explicit"), ("pose refused", "null"), ("pose refused", "explicit")])
def test_a_rejected_trial_leaves_the_graph_the_counters_and_the_live_points_as_they_were(name, stream_kind):
    """the loop once more with the estimate read back around every trial: after every pop the vertices, d_iter and the live point buffer hold the
    bytes they held before the push (the assertion names the trial); the refused solve is a rejected trial with d_dx all zero"""
    dev = _device_run(name, stream_kind, audit=True)
    rejected = sum(not t[-1] for x in dev["rounds"] for t in x["trace"])
    assert rejected >= 1
    _compare(name, dev)
    refused = [k for k, t in enumerate(dev["rounds"][0]["trace"]) if not t[7]]
    assert all(dev["dx_zero"][k] for k in refused) and not any(z for k, z in enumerate(dev["dx_zero"]) if k not in refused)
    if name == "pose refused":
        # ORBI_R_REFUSED in every trial of round 0: each is rejected (the frame's free pose and its d_iter popped) and the loop goes on to the
        # next; lambda * nu stays the 0 it was forced to, so the round ends through max_trials with the estimate it started from.  Round 1
        # takes its lambda from tau * d_out[1] of a solve at lambda 0 that is refused as well, and its first solve succeeds on the same buffers
        first, second = dev["rounds"][0]["trace"], dev["rounds"][1]["trace"]
        assert refused == list(range(il.MAX_TRIALS)) and dev["refused"] == il.MAX_TRIALS and dev["rounds"][0]["iterations"] == 1
        assert all(t[2] == 0.0 and t[4] == il.DBL_MAX and not t[-1] for t in first)
        assert second[0][2] > 0.0 and second[0][7] and second[0][-1] and all(t[7] for x in dev["rounds"][1:] for t in x["trace"])
    else:
        assert not refused


def test_two_runs_of_the_1025_point_loop_give_the_same_bytes():
    _same_run(_device_run("window 3+2 1025"), _device_run("window 3+2 1025", cached=False))


@pytest.mark.parametrize("name", ["window 3+2 63", "pose full 65"])
def test_the_null_stream_gives_the_bytes_of_an_explicit_one(name):
    null = _device_run(name, "null")
    _compare(name, null)
    _same_run(_device_run(name), null)


def test_the_device_loop_ends_at_a_stationary_point_of_the_models_cost():
    """the MODEL's gradient at the DEVICE's final estimate of the converging scene: whatever route the device took behind flat_from()"""
    sc, dev = il.scene(il.CONVERGING), _device_run(il.CONVERGING)
    start = dict({k: getattr(sc["graph"], k) for k in il.STATE}, points=sc["points"])
    g0, g1 = il.window_gradient(sc, start), il.window_gradient(sc, dev["estimate"])
    ratio = float(np.abs(g1).max() / np.abs(g0).max())
    print("gradient |b|_inf %.6g at the start, %.6g at the device's final estimate: %.3g (the model's loops: %.3g)" % (np.abs(g0).max(), np.abs(g1).max(), ratio, MEASURED_STATIONARITY))
    assert dev["rounds"][0]["iterations"] < il.SCENES[il.CONVERGING][2]["iterations"]
    assert ratio <= 4 * MEASURED_STATIONARITY <= il.BAR
