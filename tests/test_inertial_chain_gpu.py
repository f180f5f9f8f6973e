"""localInertialBundleAdjustment on the MI355X (include/orbil.h and include/orbm.h, "The inertial chain on the device-resident map"), on the
scenes of tests/inertial_chain.py, every buffer between guard elements.
  1  orbil_chain_solve_device on the linearisation of every scene at its start: the bytes of orbvi_solve_device for n <= 4, vi_model.solve
     within the stage bar for every n, an edge outside the band, the refused system
  2  orbil_chain_optimize_device against the model loop: decisions, iteration counts and refused flags equal; every trial's lambda, totals
     and scales and the final estimate within max(4 x MEASURED_SPREAD, the stage bar); d_iter and every fixed vertex keep their bytes; the
     counters are the trace's sums
  3  trial 0 has the bytes of the staged chain closed by the host
  4  two runs, a NULL stream against an explicit one, a trace shorter than the run
  5  the whole chain of the mapper step, assembly to velocity priors, on one stream with one wait
Model runs are computed once per scene and shared."""
import time

import numpy as np
import pytest

import factors_model as fm
import inertial_chain as ic
import inertial_chain_model as cm
import inertial_loop as il
import vi_model as vm
from test_factors_gpu import _Dev, _calib
from test_inertial_chain_cpu import MEASURED_SPREAD
from test_inertial_loop_cpu import TRIAL, trial_deviation
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up

pytestmark = pytest.mark.gpu

NAN = float("nan")
CAP_TRACE = 128                                          # 10 iterations x 10 trials fit, with room
NAMES = list(ic.SCENES)
_cache = {}


def _bar(name, key):
    """4 x the model's measured spread of that output, never below the stage bar"""
    return max(4 * MEASURED_SPREAD[name][key], il.BAR)


class _Chain:
    """the device memory of a chain scene, padded: what orbi_linearize_device, both solves and orbil_chain_optimize_device take"""

    def __init__(self, torch, dev, name, cap_trace=CAP_TRACE, graph_from_scene=True):
        from monoorbslam3_amd import chain
        self.torch, self.dev, self.chain, self.name = torch, dev, chain, name
        sc = self.sc = ic.scene(name)
        d = self.d = _Dev(torch, dev, sc, sc["graph"] if graph_from_scene else None, n_priors=1, n_pjobs=0)
        d.it = d._pad("it", np.zeros(d.n, np.int32), -3)
        self.cap_trace = cap_trace
        self.work = d._pad("loop work", np.full(chain.LOOP_WORK, NAN), -1.5)
        self.trace = d._pad("trace", np.full(max(cap_trace, 1) * chain.LOOP_TRACE, NAN), -1.5)
        self.summary = d._pad("summary", np.full(chain.SUMMARY, NAN), -1.5)
        self.band = d._pad("band", np.full(chain.solve_work(d.n), NAN), -1.5)
        self.lam, self.dx, self.out = d._pad("lam", np.full(1, NAN), -1.5), d._pad("dx", np.full(15 * d.n, NAN), -1.5), d._pad("out", np.full(3, NAN), -1.5)

    def options(self):
        return self.chain.ChainOptions.make(self.sc["cal"]["gravity"], iterations=ic.ITERATIONS, max_trials=il.MAX_TRIALS, lambda_init=ic.options(self.name)[0], tau=il.TAU)

    def information(self, stream=None):
        d = self.d
        d.imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=stream)

    def call(self, stream=None):
        d = self.d
        self.chain.chain_optimize_device(d.graph, d.it, d.bank, d.cap, d.edges, d.ne, d.info, d.walk, None, 0, None, 0, self.options(), self.work,
                                         self.trace if self.cap_trace else None, self.cap_trace, self.summary, d.result, stream=stream)

    def solve(self, lam, stream=None, edges=None, n_edges=None, H_off=None):
        d = self.d
        self.lam.fill_(lam)
        self.chain.chain_solve_device(d.n, d.fixed, d.edges if edges is None else edges, d.ne if n_edges is None else n_edges, d.cap, d.H_diag,
                                      d.H_off if H_off is None else H_off, d.b, self.lam, self.band, self.dx, self.out, d.result, stream=stream)

    def raw(self):
        d = self.d
        return dict(trace=self.trace.cpu().numpy().copy(), summary=self.summary.cpu().numpy().copy(), result=d.res(), Rwb=d.get("Rwb").copy(), twb=d.get("twb").copy(),
                    v=d.get("v").copy(), bg=d.get("bg").copy(), ba=d.get("ba").copy(), it=d.it.cpu().numpy().copy())


def _rows(trace, n):
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]), bool(r[7]), float(r[8]), float(r[9]), float(r[10]), float(r[11]),
             bool(r[12])) for r in trace.reshape(-1, 13)[:n]]


def _run(name, stream_kind="explicit", cap_trace=CAP_TRACE, cached=True):
    """one optimisation in the form inertial_chain.run gives (rounds, estimate, refused), with the raw outputs beside it"""
    import torch
    key = (name, stream_kind, cap_trace)
    if key in _cache and cached:
        return _cache[key]
    dev = torch.device("cuda", 0)
    lp = _Chain(torch, dev, name, cap_trace)
    st = il._chain_stream(torch, dev, stream_kind)
    lp.information(st)
    t0 = time.perf_counter()
    lp.call(st)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    lp.d.finish()
    raw = lp.raw()
    sm, n = raw["summary"], lp.d.n
    total = int(sm[5])
    rows = _rows(raw["trace"], min(total, cap_trace))
    assert int(sm[1]) == total and int(sm[6]) == max(total - cap_trace, 0) and sm[7] == 0.0, (name, sm)
    r = dict(iterations=int(sm[0]), lam=float(sm[4]), trace=rows, accepted=int(sm[2]), refused=int(sm[3]))
    if cap_trace >= total:
        assert r["accepted"] == sum(t[-1] for t in rows) and r["refused"] == sum(not t[7] for t in rows), (name, sm)
    est = dict(Rwb=raw["Rwb"].reshape(n, 3, 3), twb=raw["twb"].reshape(n, 3), v=raw["v"].reshape(n, 3), bg=raw["bg"].reshape(n, 3), ba=raw["ba"].reshape(n, 3), iter=raw["it"])
    out = dict(rounds=[r], estimate=est, refused=r["refused"], n_trials=total, seconds=seconds, raw=raw)
    _cache[key] = out
    return out


def _same_bytes(a, b, skip=()):
    for k in a["raw"]:
        if k not in skip:
            assert a["raw"][k].tobytes() == b["raw"][k].tobytes(), k


def _linearized(torch, dev, name):
    """a scene's device memory behind the edge information and one mode-0 linearisation at its start"""
    lp = _Chain(torch, dev, name)
    lp.information()
    lp.d.linearize(lp.sc, 0.0, 0)
    return lp


# ---- 1
@pytest.mark.parametrize("name", NAMES)
def test_the_staged_solve_is_the_models_and_the_dense_solves(name):
    """on the device's own linearisation, read back, as the model's input: dx within the stage bar of vi_model.solve relative to the largest
    |dx|, the scale and the pivot relative to themselves, the largest diagonal entry to the byte; for n <= 4 d_dx and d_out are the bytes of
    orbvi_solve_device on the same buffers"""
    import torch
    from monoorbslam3_amd import vi
    dev = torch.device("cuda", 0)
    lp = _linearized(torch, dev, name)
    d, sc = lp.d, lp.sc
    H_diag, H_off, b = d.get("H_diag"), d.get("H_off"), d.get("b")
    lam = 0.0 if name == ic.REFUSED else il.TAU * vm.solve(sc["graph"].fixed, sc["edges"], d.cap, H_diag, H_off, b, 0.0)[1][1]
    want_dx, want_out, want_res = vm.solve(sc["graph"].fixed, sc["edges"], d.cap, H_diag, H_off, b, lam)
    lp.solve(lam)
    dx, out, res = lp.dx.cpu().numpy().copy(), lp.out.cpu().numpy().copy(), d.res()
    assert np.array_equal(res, want_res), (res, want_res)
    if name == ic.REFUSED:
        assert not dx.any() and out[0] == 0.0 and res[vm.R_REFUSED] == 1 and res[vm.R_DONE] == 0 and out[2] == want_out[2] == 0.0 and out[1] == want_out[1]
    else:
        scale = np.abs(want_dx).max()
        worst = float(np.abs(dx.reshape(-1, 15) - want_dx).max() / scale)
        print("%s: n %d, lambda %.6g, largest deviation of dx %.3g of the largest |dx|, computeScale %.3g, pivot %.3g" %
              (name, d.n, lam, worst, abs(out[0] - want_out[0]) / abs(want_out[0]), abs(out[2] - want_out[2]) / want_out[2]))
        assert res[vm.R_DONE] == 1 and worst <= il.BAR and abs(out[0] - want_out[0]) <= il.BAR * abs(want_out[0]) and abs(out[2] - want_out[2]) <= il.BAR * want_out[2]
        assert out[1] == want_out[1]
    if d.n <= vi.MAX_STATES:
        dx2, out2 = d._pad("dense dx", np.full(15 * d.n, NAN), -1.5), d._pad("dense out", np.full(3, NAN), -1.5)
        vi.solve_device(d.n, d.fixed, d.edges, d.ne, d.cap, d.H_diag, d.H_off, d.b, lp.lam, dx2, out2, d.result)
        assert dx2.cpu().numpy().tobytes() == dx.tobytes() and out2.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(d.res(), res)
    d.finish()


def test_an_edge_outside_the_band_is_dropped_and_counted():
    """chain 3 with a third edge between the states 0 and 2, an edge on one state and an edge with a record outside the bank: each is counted
    in ORBI_R_RANGE and dx, d_out are the bytes of the call without them"""
    import torch
    dev = torch.device("cuda", 0)
    lp = _linearized(torch, dev, "chain 3")
    d, sc = lp.d, lp.sc
    lam = 1.0
    lp.solve(lam)
    dx, out, res = lp.dx.cpu().numpy().copy(), lp.out.cpu().numpy().copy(), d.res()
    assert res[vm.R_DONE] == 1 and res[vm.R_RANGE] == 0
    extra = np.zeros(3, fm.EDGE)
    extra["i"], extra["j"], extra["rec"], extra["flags"] = (0, 1, 1), (2, 1, 2), (0, 0, d.cap), fm.EDGE_WALKS
    edges = np.concatenate([sc["edges"][:1], extra[:1], sc["edges"][1:], extra[1:]])
    H = d.get("H_off").reshape(-1, 225)
    junk = np.random.RandomState(5).uniform(1e3, 1e4, (3, 225))
    H_off = np.concatenate([H[:1], junk[:1], H[1:], junk[1:]])
    lp.dx.fill_(NAN), lp.out.fill_(NAN)
    lp.solve(lam, edges=_up(torch, dev, edges), n_edges=len(edges), H_off=_up(torch, dev, H_off.reshape(-1)))
    res2 = d.res()
    assert res2[vm.R_DONE] == 1 and res2[vm.R_RANGE] == 3, res2
    assert lp.dx.cpu().numpy().tobytes() == dx.tobytes() and lp.out.cpu().numpy().tobytes() == out.tobytes()
    d.finish()


# ---- 2
def _compare(name, dev):
    ref, sc = ic.model_run(name), ic.scene(name)
    x, y = dev["rounds"][0], ref["rounds"][0]
    worst = dict.fromkeys(TRIAL, 0.0)
    assert il.flat_from(y["trace"]) == len(y["trace"])                    # tests/test_inertial_chain_cpu.py: no scene decides on a flat rho
    assert il.decisions(dev["rounds"]) == il.decisions(ref["rounds"]), (name, il.decisions(dev["rounds"]), il.decisions(ref["rounds"]))
    assert x["iterations"] == y["iterations"] and len(x["trace"]) == len(y["trace"]) and dev["refused"] == ref["refused"], name
    for k, (a, b) in enumerate(zip(x["trace"], y["trace"])):
        where = "%s, trial %d (iteration %d, trial %d of it)" % (name, k, b[0], b[1])
        assert a[:2] == b[:2] and a[7] == b[7] and a[-1] == b[-1], (where, a, b)
        assert a[9] == 0.0 and a[11] == 0.0, where                        # no visual total, no points' side of computeScale
        for key, dv in zip(TRIAL, trial_deviation(a, b)):
            worst[key] = max(worst[key], dv)
            assert dv <= _bar(name, key), (where, key, dv, _bar(name, key), dict(zip(il.FIELDS, a)), dict(zip(il.FIELDS, b)))
    est, want = dev["estimate"], ref["estimate"]
    for o in ("v", "bg", "ba"):                                          # every pose is fixed: Rwb and twb are held to their bytes below
        scale = np.abs(want[o]).max()
        worst[o] = float(np.abs(est[o] - want[o]).max() / scale)
        assert worst[o] <= _bar(name, o), (name, o, worst[o], _bar(name, o))
    last = lambda r: min([t[4] for t in r["trace"] if t[-1]] + [r["trace"][0][3]])  # noqa: E731
    worst["total"] = abs(last(x) - last(y)) / last(y)
    assert worst["total"] <= _bar(name, "total"), (name, worst["total"])
    if y["lam"]:
        worst["lam"] = abs(x["lam"] - y["lam"]) / y["lam"]
        assert worst["lam"] <= _bar(name, "lam"), (name, worst["lam"])
    else:
        assert x["lam"] == 0.0
    g = sc["graph"]
    assert not est["iter"].any()                                         # every pose is fixed: no update counter moves
    for o, bit in zip(il.STATE, (fm.FIX_POSE, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC)):
        fx = (g.fixed & bit) != 0
        assert est[o][fx].tobytes() == getattr(g, o)[fx].tobytes(), (name, o, "a fixed vertex moved")
    print("%s: %d trials in %.4f s, %s" % (name, dev["n_trials"], dev["seconds"], il.decisions(dev["rounds"])[0]))
    print("    largest deviation " + ", ".join("%s %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", NAMES)
def test_the_one_launch_loop_is_the_models(name):
    dev = _run(name)
    _compare(name, dev)
    res, tr = dev["raw"]["result"], dev["rounds"][0]["trace"]
    accepted = sum(t[-1] for t in tr)
    assert res.tolist() == [accepted, 0, len(tr) - accepted, sum(not t[7] for t in tr), 0, 0, 0, 0], res
    if name == ic.REJECTING:
        assert "ra" in il.decisions(dev["rounds"])[0]
    if name == ic.REFUSED:
        g = ic.scene(name)["graph"]
        assert dev["rounds"][0]["iterations"] == 1 and len(tr) == il.MAX_TRIALS == dev["refused"]
        assert all(t[2] == 0.0 and t[4] == il.DBL_MAX and not t[7] and not t[-1] for t in tr)
        for k in il.STATE:
            assert dev["raw"][k].tobytes() == np.ascontiguousarray(getattr(g, k)).reshape(-1).tobytes(), (k, "moved in an optimisation of refused solves")


# ---- 3
@pytest.mark.parametrize("name", NAMES)
def test_the_first_trial_has_the_bytes_of_the_staged_chain(name):
    """orbi_linearize_device, orbil_chain_solve_device (once for d_out[1], once at tau * d_out[1]), orbi_graph_oplus_device and
    orbi_linearize_device in mode 1, closed by the host: lambda, current, temp and the pose side of computeScale of trial 0, to the byte"""
    import torch
    dev = torch.device("cuda", 0)
    one = _run(name)["rounds"][0]["trace"][0]
    lp = _linearized(torch, dev, name)
    d = lp.d
    current = float(d.get("total")[1])
    lp.solve(0.0)
    lam = 0.0 if name == ic.REFUSED else il.TAU * float(lp.out.cpu().numpy()[1])
    lp.solve(lam)
    refused = d.res()[vm.R_REFUSED] == 1
    scale_pose = float(lp.out.cpu().numpy()[0])
    d.imu.graph_oplus_device(d.graph, lp.dx, d.it, d.result)
    d.linearize(lp.sc, 0.0, 1)
    temp = il.DBL_MAX if refused else float(d.get("total")[1])
    d.finish()
    for key, v in (("lam", lam), ("current", current), ("temp", temp), ("scale_pose", scale_pose)):
        a = one[il.FIELDS.index(key)]
        assert np.float64(a).tobytes() == np.float64(v).tobytes(), (name, key, a, v)
    assert one[7] == (not refused)


# ---- 4
@pytest.mark.parametrize("name", ["chain 20", ic.REJECTING, ic.REFUSED])
def test_two_runs_give_the_same_bytes(name):
    _same_bytes(_run(name), _run(name, cached=False))


@pytest.mark.parametrize("name", ["chain 3", "chain 10"])
def test_the_null_stream_gives_the_bytes_of_an_explicit_one(name):
    _same_bytes(_run(name), _run(name, "null"))


def test_a_trace_shorter_than_the_run_counts_what_it_drops():
    name = ic.REJECTING
    full = _run(name)
    cap = full["n_trials"] // 2
    assert cap >= 2
    short = _run(name, cap_trace=cap)                       # _run's finish() holds the guards behind the trace
    assert short["raw"]["summary"][5] == full["n_trials"] and short["raw"]["summary"][6] == full["n_trials"] - cap
    assert short["raw"]["trace"][:13 * cap].tobytes() == full["raw"]["trace"][:13 * cap].tobytes()
    _same_bytes(short, full, skip=("trace", "summary"))
    assert short["raw"]["summary"][:6].tobytes() == full["raw"]["summary"][:6].tobytes()


# ---- 5
def _mapper_chain(torch, dev, name, waits, bad_window=False):
    """the assembly -> orbi_graph_init_device -> orbi_edge_information_device -> orbil_chain_optimize_device -> orbi_graph_recover_device ->
    orbi_set_bias_device -> orbm_inertial_chain_velocity_priors_device on one stream, with a wait behind each call or one at the end ->
    what the device holds afterwards"""
    from monoorbslam3_amd import imu, matcher
    sc = ic.scene(name)
    mp = cm.map_from_chain_scene(sc)
    n = sc["graph"].n
    window = mp["window"].copy()
    if bad_window:
        window[1] = mp["bad_kf"]
    lp = _Chain(torch, dev, name, graph_from_scene=False)
    d = lp.d
    for t in (d.Rwb, d.twb, d.v, d.bg, d.ba):
        t.fill_(7.5)                                         # a graph no call has initialised: a refused chain must leave it
    pads = dict(init_jobs=_padded(torch, dev, np.full(3 * n, -9, np.int32), 17), fixed=_padded(torch, dev, np.full(n, 0xF7, np.uint8), 17),
                inertial_edges=_padded(torch, dev, np.full(4 * (n - 1), -9, np.int32), 17), recover_jobs=_padded(torch, dev, np.full(3 * n, -9, np.int32), 17),
                bias_ids=_padded(torch, dev, np.full(n, -9, np.int32), 17), velo_jobs=_padded(torch, dev, np.full(2 * n, -9, np.int32), 17),
                state_kf=_padded(torch, dev, np.full(n, -9, np.int32), 17), src=_padded(torch, dev, mp["src"].reshape(-1), np.float32(-2.5)),
                priors=_padded(torch, dev, mp["priors"].reshape(-1), np.float32(-2.5)), bias=_padded(torch, dev, np.full(6 * n, -4.0, np.float32), np.float32(-2.5)))
    a = {k: v[1] for k, v in pads.items()}
    res = {k: torch.full((8,), 77, dtype=torch.int32, device=dev) for k in ("problem", "init", "information", "recover", "set_bias", "velocity")}
    a.update(bad=_up(torch, dev, mp["bad"]), window=_up(torch, dev, window), kf_imu=_up(torch, dev, mp["kf_imu"]), result=res["problem"])
    st = _stream(torch, dev, "explicit")
    wait = torch.cuda.synchronize if waits else (lambda: None)
    m = matcher.ORBMatcher()
    cal = _calib(sc["cal"])
    matcher.inertial_chain_problem_device(m, a, mp["n_kf"], n, mp["n_src"], mp["cap_bank"], mp["n_priors"], stream=st)
    wait()
    graph = imu.Graph.make(d.Rwb, d.twb, d.v, d.bg, d.ba, a["fixed"], n)
    imu.graph_init_device(graph, d.bank, d.cap, a["src"], mp["n_src"], a["init_jobs"], n, res["init"], stream=st)
    wait()
    imu.edge_information_device(d.bank, d.cap, a["inertial_edges"], n - 1, d.info, d.walk, res["information"], stream=st)
    wait()
    lp.chain.chain_optimize_device(graph, d.it, d.bank, d.cap, a["inertial_edges"], n - 1, d.info, d.walk, None, 0, None, 0, lp.options(), lp.work, lp.trace, lp.cap_trace,
                                   lp.summary, d.result, stream=st)
    wait()
    imu.graph_recover_device(graph, cal, a["recover_jobs"], n, a["src"], mp["n_src"], a["bias"], res["recover"], stream=st)
    wait()
    imu.set_bias_device(cal, d.bank, d.pool, d.cap, d.cap_meas, a["bias_ids"], a["bias"], n, res["set_bias"], stream=st)
    wait()
    matcher.inertial_chain_velocity_priors_device(m, dict(priors=a["priors"], src=a["src"], velo_jobs=a["velo_jobs"], result=res["velocity"]), mp["n_priors"], mp["n_src"], n,
                                                  stream=st)
    d.finish()                                               # the one wait, and the guards of the loop's buffers
    for k, (whole, _) in pads.items():
        assert _guards_intact(whole, np.float32(-2.5) if k in ("src", "priors", "bias") else 17), k
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    held = {k: g(v) for k, v in a.items() if k != "result"}
    held.update({"result " + k: g(v) for k, v in res.items()}, bank=g(d.bank), pool=g(d.pool), **lp.raw())
    return mp, held


def test_the_mapper_chain_on_one_stream_with_one_wait():
    """the recovered floats and velo_priori of every window key frame equal the same chain with a wait behind each call, and the models':
    the assembly's lists to the byte, the optimisation the run from the scene's graph to the byte (graph_init's widening is exact), the
    recovery and the velocity priors the models' on the device's own estimate"""
    import torch
    dev, name = torch.device("cuda", 0), ic.MAP_SCENE
    sc = ic.scene(name)
    mp, one = _mapper_chain(torch, dev, name, False)
    _, each = _mapper_chain(torch, dev, name, True)
    for k in one:
        assert one[k].tobytes() == each[k].tobytes(), k
    want = cm.problem(mp["bad"], mp["window"], mp["kf_imu"], mp["n_src"], mp["cap_bank"], mp["n_priors"])
    n = sc["graph"].n
    assert one["result problem"].tolist() == want["result"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
    for k in cm.OUT:
        assert one[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    assert one["result init"][0] == n and one["result information"][0] == n - 1 and one["result recover"][0] == n and one["result velocity"].tolist()[:2] == [n, 0]
    full = _run(name)
    for k in ("Rwb", "twb", "v", "bg", "ba", "it", "trace", "summary", "result"):
        assert one[k].tobytes() == full["raw"][k].tobytes(), k
    g = sc["graph"].copy()
    for k in il.STATE:
        setattr(g, k, np.array(full["estimate"][k], np.float64))
    src = mp["src"].copy()
    bias, _, _, rres = fm.recover(g, sc["cal"], want["recover_jobs"], src, with_pose=False)
    assert one["src"].tobytes() == src.tobytes() and one["bias"].tobytes() == np.ascontiguousarray(bias, np.float32).tobytes()
    assert (src != mp["src"]).any() and one["result recover"].tolist() == list(rres)
    priors, vres = cm.velocity_priors(mp["priors"], src, want["velo_jobs"])
    assert one["priors"].tobytes() == priors.tobytes() and one["result velocity"].tolist() == vres.tolist()
    for s in range(n):                                       # velo_priori of EVERY window key frame, and nothing else of a slot
        row, slot = want["velo_jobs"][s]
        assert one["priors"].reshape(-1, 36)[slot, :3].tobytes() == one["src"].reshape(-1, 15)[row, 12:15].tobytes()
        assert one["priors"].reshape(-1, 36)[slot, 3:].tobytes() == mp["priors"][slot, 3:].tobytes()


def test_a_window_with_a_bad_key_frame_leaves_every_byte_as_it_was():
    """the refusal honoured on the device, without a read-back: every list is -1, every call behind drops every job, the optimisation finds
    nothing to do, and the state rows, the bank's biases and the priors keep their bytes"""
    import torch
    dev, name = torch.device("cuda", 0), ic.MAP_SCENE
    sc = ic.scene(name)
    n = sc["graph"].n
    mp, held = _mapper_chain(torch, dev, name, False, bad_window=True)
    assert held["result problem"].tolist() == [n, cm.REFUSE_WINDOW, 1, 0, 0, 0, 0, 0]
    for k in cm.OUT:
        assert (held[k] == (15 if k == "fixed" else -1)).all(), k
    fresh = _Chain(torch, dev, name, graph_from_scene=False)
    assert held["src"].tobytes() == mp["src"].tobytes() and held["priors"].tobytes() == mp["priors"].tobytes()
    assert held["bank"].tobytes() == fresh.d.bank.cpu().numpy().tobytes() and held["pool"].tobytes() == fresh.d.pool.cpu().numpy().tobytes()
    # (d_bias is the recover's scratch, not the map's: orbi_graph_recover_device writes the row of a dropped job, and orbi_set_bias_device drops it too)
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        assert (held[k] == 7.5).all(), k
    assert not held["it"].any()
    assert held["result init"][0] == 0 and held["result information"][0] == 0 and held["result recover"][0] == 0 and held["result set_bias"][0] == 0
    assert held["result velocity"].tolist()[:2] == [0, n]
    sm = held["summary"]
    assert sm[0] == 1 and sm[1] == 1 and sm[2] == 0 and sm[3] == 0                       # one trial on an empty system: rho == 0 ends it
