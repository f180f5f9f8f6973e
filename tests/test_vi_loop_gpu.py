"""orbvi_pose_optimize_device on the MI355X: poseFullOptimize / poseInertialOptimize whole in one launch (include/orbvi.h), on the scenes of
inertial_loop.SCENES that carry a pose loop, built with the helpers inertial_loop.DevicePose uses, every buffer between guard elements.
  1  against the model loop (inertial_loop.model_run), through test_inertial_loop_gpu._compare: the bars are that file's and are not restated
  2  against the staged chain closed by the host (inertial_loop.device_backend): the first trial of round 0 bit for bit, the decisions
  3  two runs, and a NULL stream against an explicit one: the same bytes everywhere
  4  a trace shorter than the run
  5  init -> edge information -> the optimisation -> recover on one stream with one wait
The classification of a round before the last is read from a run with options.rounds cut there: the runs are deterministic (3), so its
bytes are those of the full run's intermediate state."""
import time

import numpy as np
import pytest

import factors_model as fm
import inertial_loop as il
from test_factors_gpu import _Dev, _calib
from test_inertial_loop_gpu import _compare, _device_run
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _up
from test_vi_gpu import _Vis, _camera

pytestmark = pytest.mark.gpu

NAN = float("nan")
POSE_SCENES = [n for n, s in il.SCENES.items() if s[0] in ("pose_full", "pose_inertial")]
STAGED_BITS = ["pose full 65", "pose full 1025", "pose full 65 fisheye", "pose inertial"]
CAP_TRACE = 512                                          # 4 rounds x 10 iterations x 10 trials fit, with room
_cache = {}


class _Loop:
    """the device memory of one orbvi_pose_optimize_device call on a loop scene, padded, and the call"""

    def __init__(self, torch, dev, name, cap_trace=CAP_TRACE, graph_from_scene=True):
        from monoorbslam3_amd import vi
        self.torch, self.dev, self.vi, self.name = torch, dev, vi, name
        driver, _, kw = il.SCENES[name]
        sc = self.sc = il.scene(name)
        self.visual, self.ne = driver == "pose_full", sc["n_edges"] if driver == "pose_full" else 0
        d = self.d = _Dev(torch, dev, sc, sc["graph"] if graph_from_scene else None, n_priors=1, n_pjobs=1)
        d.priors.copy_(_up(torch, dev, sc["priors"]))
        d.it = d._pad("it", np.zeros(d.n, np.int32), -3)
        self.pjobs = _up(torch, dev, sc["pjobs"])
        self.cal, self.cam = _calib(sc["cal"]), _camera(sc["cam"])
        self.v = None
        if self.visual:
            self.v = _Vis(torch, dev, sc["graph"], sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], self.ne, sc["points"], sc["z"], sc["w"],
                          active=np.ones(self.ne, np.uint8))
        self.cap_trace = cap_trace
        self.work = d._pad("loop work", np.full(self.ne * vi.LOOP_EDGE_WORK + vi.LOOP_FIXED_WORK, NAN), -1.5)
        self.trace = d._pad("trace", np.full(max(cap_trace, 1) * vi.LOOP_TRACE, NAN), -1.5)
        self.summary = d._pad("summary", np.full(vi.LOOP_SUMMARY, NAN), -1.5)
        self.forced = "forced_lambda_init" in kw
        self.full_rounds = 4 if self.visual else 1

    def options(self, rounds=None):
        return self.vi.LoopOptions.make(self.sc["cal"]["gravity"], rounds=rounds or self.full_rounds, lambda_init=(-1.0 if self.forced else 0.0, 0.0, 0.0, 0.0),
                                        tau=il.TAU, max_trials=il.MAX_TRIALS)

    def call(self, stream=None, rounds=None):
        d, v = self.d, self.v
        self.vi.pose_optimize_device(d.graph, d.it, d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.priors, 1, self.pjobs, 1, self.cal, self.cam, self.ne,
                                     v.group_state if v else None, v.edge_off if v else None, v.points if v else None, v.z if v else None, v.w if v else None,
                                     v.active if v else None, self.options(rounds), self.work, v.chi2 if v else None, v.n_inliers if v else None,
                                     self.trace if self.cap_trace else None, self.cap_trace, self.summary, d.result, stream=stream)

    def finish(self):
        self.d.finish()
        if self.v is not None:
            self.v.finish()

    def raw(self):
        """every output as bytes-comparable arrays"""
        d, v = self.d, self.v
        out = dict(trace=self.trace.cpu().numpy().copy(), summary=self.summary.cpu().numpy().copy(), result=d.res(),
                   Rwb=d.get("Rwb").copy(), twb=d.get("twb").copy(), v=d.get("v").copy(), bg=d.get("bg").copy(), ba=d.get("ba").copy(), it=d.it.cpu().numpy().copy())
        if v is not None:
            out.update(active=v.get("active")[:self.ne].copy(), chi2=v.get("chi2")[:self.ne].copy(), n_inliers=v.get("n_inliers").copy())
        return out


def _rows(trace, n):
    t = trace.reshape(-1, 13)[:n]
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]), bool(r[7]), float(r[8]), float(r[9]), float(r[10]),
             float(r[11]), bool(r[12])) for r in t]


def _run(name, stream_kind="explicit", cap_trace=CAP_TRACE, cached=True):
    """one optimisation in the form inertial_loop.run gives (rounds, estimate, refused), with the raw outputs beside it"""
    import torch
    key = (name, stream_kind, cap_trace)
    if key in _cache and cached:
        return _cache[key]
    dev = torch.device("cuda", 0)
    lp = _Loop(torch, dev, name, cap_trace)
    st = il._chain_stream(torch, dev, stream_kind)
    imu = lp.d.imu
    imu.edge_information_device(lp.d.bank, lp.d.cap, lp.d.edges, lp.d.ne, lp.d.info, lp.d.walk, lp.d.result, stream=st)
    t0 = time.perf_counter()
    lp.call(st)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    lp.finish()
    raw = lp.raw()
    sm, n = raw["summary"], lp.d.n
    total = int(sm[24])
    rows = _rows(raw["trace"], min(total, cap_trace))
    rounds, at = [], 0
    for k in range(lp.full_rounds):
        its, trials, accepted, refused, lam = int(sm[6 * k]), int(sm[6 * k + 1]), int(sm[6 * k + 2]), int(sm[6 * k + 3]), float(sm[6 * k + 4])
        r = dict(iterations=its, lam=lam, trace=rows[at:at + trials], accepted=accepted, refused=refused, n_inliers=int(sm[6 * k + 5]))
        at += trials
        rounds.append(r)
    assert at == total and int(sm[25]) == max(total - cap_trace, 0), (name, sm)
    if cap_trace >= total:
        for r in rounds:
            assert r["accepted"] == sum(t[-1] for t in r["trace"]) and r["refused"] == sum(not t[7] for t in r["trace"]), (name, sm)
    if lp.visual:
        # the classification behind round k: the final outputs of a run of k + 1 rounds
        for k in range(lp.full_rounds):
            if k == lp.full_rounds - 1:
                c = raw
            else:
                cut = _Loop(torch, dev, name, cap_trace)
                imu.edge_information_device(cut.d.bank, cut.d.cap, cut.d.edges, cut.d.ne, cut.d.info, cut.d.walk, cut.d.result, stream=st)
                cut.call(st, rounds=k + 1)
                cut.finish()
                c = cut.raw()
                assert c["summary"][:6 * (k + 1)].tobytes() == sm[:6 * (k + 1)].tobytes(), (name, "a run of %d rounds is the full run's start" % (k + 1))
            rounds[k]["classification"] = dict(active=c["active"], n_inliers=int(c["n_inliers"][0]), chi2=c["chi2"])
            assert rounds[k]["n_inliers"] == int(c["n_inliers"][0])
    est = dict(Rwb=raw["Rwb"].reshape(n, 3, 3), twb=raw["twb"].reshape(n, 3), v=raw["v"].reshape(n, 3), bg=raw["bg"].reshape(n, 3), ba=raw["ba"].reshape(n, 3),
               iter=raw["it"])
    out = dict(rounds=rounds, estimate=est, refused=sum(r["refused"] for r in rounds), n_trials=total, seconds=seconds, dx_zero=[], raw=raw)
    _cache[key] = out
    return out


def _same_bytes(a, b, skip=()):
    for k in a["raw"]:
        if k not in skip:
            assert a["raw"][k].tobytes() == b["raw"][k].tobytes(), k


# ---- 1
@pytest.mark.parametrize("name", POSE_SCENES)
def test_the_one_launch_loop_is_the_models(name):
    """decisions, iteration counts and refused flags equal (up to flat_from() on the converged scene); every trial's lambda, totals and scales,
    the estimate, the classification away from the threshold, d_iter and the fixed vertices as test_inertial_loop_gpu._compare holds the
    staged device loop"""
    dev = _run(name)
    _compare(name, dev)
    res = dev["raw"]["result"]
    accepted, trials = sum(r["accepted"] for r in dev["rounds"]), dev["n_trials"]
    assert res[0] == accepted and res[2] == trials - accepted and res[3] == dev["refused"] and res[1] == 0 and not res[4:].any(), res
    if name == "pose refused":
        sc = il.scene(name)
        first, second = dev["rounds"][0], dev["rounds"][1]
        assert first["iterations"] == 1 and len(first["trace"]) == il.MAX_TRIALS and first["refused"] == il.MAX_TRIALS
        assert all(t[2] == 0.0 and t[4] == il.DBL_MAX and not t[7] and not t[-1] for t in first["trace"])
        assert second["trace"][0][2] > 0.0 and second["trace"][0][7] and second["trace"][0][-1] and all(t[7] for r in dev["rounds"][1:] for t in r["trace"])
        # the estimate behind round 0 is the starting bytes: a run of that round alone
        import torch
        tdev = torch.device("cuda", 0)
        one = _Loop(torch, tdev, name)
        one.d.imu.edge_information_device(one.d.bank, one.d.cap, one.d.edges, one.d.ne, one.d.info, one.d.walk, one.d.result)
        one.call(rounds=1)
        one.finish()
        r1, g = one.raw(), sc["graph"]
        for k in il.STATE:
            assert r1[k].tobytes() == np.ascontiguousarray(getattr(g, k)).reshape(-1).tobytes(), (k, "moved in a round of refused solves")
        assert not r1["it"].any()


# ---- 2
@pytest.mark.parametrize("name", STAGED_BITS)
def test_the_first_trial_has_the_bytes_of_the_staged_chain(name):
    """trial 0 of round 0 has no policy arithmetic beyond tau * the largest diagonal entry: lambda, current, temp, the pose side of
    computeScale and both totals are the staged calls' bytes; the decisions of the whole run are the staged loop's"""
    one, staged = _run(name), _device_run(name)
    a, b = one["rounds"][0]["trace"][0], staged["rounds"][0]["trace"][0]
    for key in ("lam", "current", "temp", "scale_pose", "total_inertial", "total_visual"):
        i = il.FIELDS.index(key)
        assert np.float64(a[i]).tobytes() == np.float64(b[i]).tobytes(), (name, key, a[i], b[i])
    assert len(one["rounds"]) == len(staged["rounds"])
    for n, (x, y) in enumerate(zip(one["rounds"], staged["rounds"])):
        flat = il.flat_from(y["trace"]) if name in il.CONVERGED else len(y["trace"])
        dx, dy = il.decisions([x])[0], il.decisions([y])[0]
        assert dx[:flat] == dy[:flat], (name, "round", n, dx, dy)
        if name not in il.CONVERGED:
            assert dx == dy and x["iterations"] == y["iterations"], (name, "round", n)


# ---- 3
@pytest.mark.parametrize("name", ["pose full 1025", "pose refused"])
def test_two_runs_give_the_same_bytes(name):
    _same_bytes(_run(name), _run(name, cached=False))


@pytest.mark.parametrize("name", ["pose full 65", "pose inertial"])
def test_the_null_stream_gives_the_bytes_of_an_explicit_one(name):
    _same_bytes(_run(name), _run(name, "null"))


# ---- 4
def test_a_trace_shorter_than_the_run_counts_what_it_drops():
    name = "pose full 65"
    full = _run(name)
    cap = full["n_trials"] // 2
    assert cap >= 2
    short = _run(name, cap_trace=cap)                       # _run's finish() holds the guards behind the trace
    assert short["raw"]["summary"][24] == full["n_trials"] and short["raw"]["summary"][25] == full["n_trials"] - cap
    assert short["raw"]["trace"][:13 * cap].tobytes() == full["raw"]["trace"][:13 * cap].tobytes()
    _same_bytes(short, full, skip=("trace", "summary"))
    assert short["raw"]["summary"][:24].tobytes() == full["raw"]["summary"][:24].tobytes()


# ---- 5
def test_the_chain_on_one_stream_with_one_wait():
    """orbi_graph_init_device -> orbi_edge_information_device -> orbvi_pose_optimize_device -> orbi_graph_recover_device with nothing read
    back in the middle: the recovered floats are those of the same chain with a wait behind each call"""
    import torch
    from monoorbslam3_amd import imu
    from test_projection_queries_gpu import _stream
    dev, name = torch.device("cuda", 0), "pose full 65"
    sc = il.scene(name)
    rjobs = np.array([(1, 1, fm.RECOVER_POSE), (0, 0, 0)], np.int32)
    got = {}
    for waits in (False, True):
        lp = _Loop(torch, dev, name, graph_from_scene=False)
        lp.v.graph = lp.d.graph
        src, init_jobs, d_rjobs = _up(torch, dev, sc["src"]), _up(torch, dev, sc["init_jobs"]), _up(torch, dev, rjobs)
        d_dst, d_bias = _padded(torch, dev, sc["src"], np.float32(-2.5)), _padded(torch, dev, np.full(12, -4.0, np.float32), np.float32(-2.5))
        st = _stream(torch, dev, "explicit")
        wait = torch.cuda.synchronize if waits else (lambda: None)
        d = lp.d
        imu.graph_init_device(d.graph, d.bank, d.cap, src, 2, init_jobs, 2, d.result, stream=st)
        wait()
        imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
        wait()
        lp.call(st)
        wait()
        imu.graph_recover_device(d.graph, lp.cal, d_rjobs, 2, d_dst[1], 2, d_bias[1], d.result, stream=st)
        lp.finish()                                          # the one wait
        assert _guards_intact(d_dst[0], np.float32(-2.5)) and _guards_intact(d_bias[0], np.float32(-2.5))
        assert d.res().tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
        got[waits] = (d_dst[1].cpu().numpy().copy(), d_bias[1].cpu().numpy().copy(), lp.raw())
    assert got[False][0].tobytes() == got[True][0].tobytes() and got[False][1].tobytes() == got[True][1].tobytes()
    for k in got[False][2]:
        assert got[False][2][k].tobytes() == got[True][2][k].tobytes(), k
    # and the chain from the float source states is the run from the scene's graph: graph_init's widening is exact
    full = _run(name)
    for k in ("Rwb", "twb", "v", "bg", "ba", "it", "active", "chi2", "trace"):
        assert got[False][2][k].tobytes() == full["raw"][k].tobytes(), k
    assert np.isfinite(got[False][0]).all() and np.isfinite(got[False][1]).all()
