"""The inertial factors on the MI355X (include/orbi.h, "Inertial factors linearised on the device") against tests/factors_model.py.
The float intermediates (dR, dV, dP of the bias vertices cast to float), everything stored as float and every counter: bit for bit.
Every double output: within 1e-9 of the model relative to the largest entry of its own 3x3 block (a vector: of its own 3-vector; a
chi2 or a total: of itself) -- the bar tests/test_ba.py holds the f64 BA kernels to.  Padded arrays, intact guards.  Model outputs
are computed once per scene and shared.  The largest deviation met is printed per output."""
import numpy as np
import pytest

import factors_model as fm
import imu_model as im
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _bits, _stream, _up

pytestmark = pytest.mark.gpu

BAR = 1e-9
_cache = {}
_worst = {}
NAN = float("nan")


def _blocks(a, shape):
    """the array cut into its 3x3 blocks (matrices of `shape`) or 3-vectors (shape None), or scalars (shape ())"""
    a = np.asarray(a, np.float64)
    if shape == ():
        return a.reshape(-1, 1)
    if shape is None:
        return a.reshape(-1, 3)
    r, c = shape
    return a.reshape(-1, r // 3, 3, c // 3, 3).transpose(0, 1, 3, 2, 4).reshape(-1, 9)


def _close(what, got, want, shape):
    g, w = _blocks(got, shape), _blocks(want, shape)
    assert g.shape == w.shape and np.isfinite(g).all(), what
    scale = np.abs(w).max(1)
    dev = np.abs(g - w).max(1)
    zero = scale == 0
    assert not g[zero].any(), (what, "blocks that are zero in the model")
    rel = float((dev[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0
    _worst[what] = max(_worst.get(what, 0.0), rel)
    print("%-12s largest deviation %.3g of its block's largest entry (the worst so far %.3g)" % (what, rel, _worst[what]))
    assert rel <= BAR, (what, rel)


def _same_bits(what, got, want):
    assert _bits(np.ascontiguousarray(got)).tobytes() == _bits(np.ascontiguousarray(want)).tobytes(), what


def _same_floats(what, got, want):
    """floats that are roundings of doubles held to 1e-9: at most one float ulp from the model's"""
    g = np.frombuffer(np.ascontiguousarray(got).tobytes(), np.uint32).astype(np.int64)
    w = np.frombuffer(np.ascontiguousarray(want).tobytes(), np.uint32).astype(np.int64)
    ulp = np.abs(g - w)
    print("%s: %d of %d floats differ from the model, by at most %d ulp" % (what, (ulp != 0).sum(), ulp.size, ulp.max()))
    assert ulp.max() <= 1, what


def _calib(cal):
    from monoorbslam3_amd import imu
    return imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])


def _pack(recs):
    bank = im.Bank(len(recs), max(max(len(r.meas) for r in recs), 1))
    bank.recs = [r.copy() for r in recs]
    return bank


class _Dev:
    """a scene's device memory: the bank, the graph, the edges and every output, padded"""

    def __init__(self, torch, dev, sc, graph=None, n_priors=1, n_pjobs=0):
        from monoorbslam3_amd import imu
        self.torch, self.dev, self.imu = torch, dev, imu
        bank, pool = _pack(sc["recs"]).pack()
        self.cap, self.cap_meas = len(bank), pool.shape[1]
        self.bank, self.pool = _up(torch, dev, bank), _up(torch, dev, pool)
        self.n, self.ne = sc["graph"].n, len(sc["edges"])
        g = graph
        self.pads = {}
        f64 = lambda k, n, v=NAN: self._pad(k, np.full(n, v, np.float64), -1.5)  # noqa: E731
        self.Rwb = f64("Rwb", 9 * self.n) if g is None else self._pad("Rwb", g.Rwb.reshape(-1), -1.5)
        for k in ("twb", "v", "bg", "ba"):
            setattr(self, k, f64(k, 3 * self.n) if g is None else self._pad(k, getattr(g, k).reshape(-1), -1.5))
        self.fixed = _up(torch, dev, sc["graph"].fixed if g is None else g.fixed)
        self.graph = imu.Graph.make(self.Rwb, self.twb, self.v, self.bg, self.ba, self.fixed, self.n)
        self.edges = _up(torch, dev, sc["edges"]) if self.ne else _up(torch, dev, np.zeros(1, fm.EDGE))
        ne, n = max(self.ne, 1), self.n
        self.info, self.walk = f64("info", 81 * ne), f64("walk", 18 * ne)
        self.work, self.err, self.chi2, self.total = f64("work", imu.EDGE_WORK * ne), f64("err", 9 * ne), f64("chi2", 3 * ne), f64("total", 2)
        self.chi2_prior = f64("chi2_prior", 3 * max(n_pjobs, 1))
        self.H_diag, self.H_off, self.b, self.J = f64("H_diag", 225 * n), f64("H_off", 225 * ne), f64("b", 15 * n), f64("J", 270 * ne)
        self.flt = self._pad("flt", np.full(15 * ne, -9.0, np.float32), np.float32(-2.5))
        self.priors = self._pad("priors", np.full(144 * n_priors, 0x5A, np.uint8), 0xA5)
        self.result = self._pad("result", np.full(8, 77, np.int32), -6)
        self.it = _up(torch, dev, np.zeros(n, np.int32))

    def _pad(self, key, a, fill):
        self.pads[key] = (_padded(self.torch, self.dev, a, fill), fill)
        return self.pads[key][0][1]

    def res(self):
        return self.result.cpu().numpy().copy()

    def get(self, key, shape=None):
        a = getattr(self, key).cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def finish(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))
        for key, ((whole, _), fill) in self.pads.items():
            assert _guards_intact(whole, fill), key

    def linearize(self, sc, delta, mode, d_pjobs=None, n_pjobs=0, n_priors=0, stream=None):
        self.imu.linearize_device(self.graph, self.bank, self.cap, sc["cal"]["gravity"], self.edges, self.ne, self.info, self.walk, self.work, self.err,
                                  self.chi2, self.total, self.result, self.priors if n_pjobs else None, n_priors, d_pjobs, n_pjobs,
                                  self.chi2_prior if n_pjobs else None, delta, mode, None if mode else self.H_diag, None if mode else self.H_off,
                                  None if mode else self.b, None if mode else self.J, self.flt, stream=stream)


def _assert_graph(what, d, g):
    """the device's vertices against the model's"""
    _close(what + " Rwb", d.get("Rwb"), g.Rwb, (3, 3))
    for k in ("twb", "v", "bg", "ba"):
        _close(what + " " + k, d.get(k), getattr(g, k), None)


def _assert_linear(what, d, o, mode, n_pjobs=0):
    ne = d.ne
    _same_bits(what + " float dR dV dP", d.get("flt", (ne, 15)), o["flt"])
    _close(what + " err", d.get("err"), o["err"], None)
    _close(what + " chi2", d.get("chi2"), o["chi2"], ())
    _close(what + " total", d.get("total"), o["total"], ())
    if n_pjobs:
        _close(what + " chi2_prior", d.get("chi2_prior")[:3 * n_pjobs], o["chi2_prior"], ())
    assert np.array_equal(d.res(), o["result"]), (what, d.res(), o["result"])
    if mode == 0:
        _close(what + " J", d.get("J"), o["J"], (9, 30))
        _close(what + " H_diag", d.get("H_diag"), o["H_diag"], (15, 15))
        _close(what + " H_off", d.get("H_off"), o["H_off"], (15, 15))
        _close(what + " b", d.get("b"), o["b"], None)
        Hd = d.get("H_diag", (-1, 15, 15))
        _close(what + " H_diag symmetric", Hd, np.transpose(Hd, (0, 2, 1)), (15, 15))


FIXED_CYCLE = (0, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC, 0, fm.FIX_POSE | fm.FIX_GYRO | fm.FIX_ACC, 15)


def _chain_scene(n_edges):
    """the chain with every fixed-mask bit on some state (from four edges on), priors on states 0 and 1, and the model's outputs"""
    if n_edges not in _cache:
        sc = fm.make_chain(n_edges)
        sc["graph"].fixed[:] = [FIXED_CYCLE[(s + 1) % 8] for s in range(n_edges + 1)]
        if n_edges >= 4:
            seen = np.bitwise_or.reduce(sc["graph"].fixed)
            assert seen == 15 and (sc["graph"].fixed == 0).any() and (n_edges < 6 or (sc["graph"].fixed == 15).any())
        slots = [1, 0]                                             # slot 0 from state 1, slot 1 from state 0: the priors' errors are not zero
        sc["priors"], sc["prior_info_jobs"], _ = fm.make_priors(sc, slots)
        sc["pjobs"] = np.array([(0, 0, 7), (1, 1, 7 | fm.PRIOR_ACC_GYRO_INFO), (1, 0, fm.PRIOR_GYRO)], fm.PRIOR_JOB)   # two jobs on state 1's gyro bias
        sc["info"], sc["walk"], sc["info_res"] = fm.edge_information(sc["recs"], sc["edges"])
        sc["out"] = fm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], sc["priors"], sc["pjobs"], fm.HUBER_DELTA)
        inside = sc["out"]["chi2"][:, 0] <= fm.HUBER_DELTA ** 2
        assert n_edges < 3 or (inside.any() and (~inside).any())
        if n_edges >= 5:      # both branches of ExpSO3f and of RightJacobianSO3(JRg * delta_bg): zero and non-zero delta_bias
            th = [float(im.norm3(im.mv(r.JRg, fm.float_deltas(r, sc["graph"].bg[e], sc["graph"].ba[e])[3]))) for e, r in enumerate(sc["recs"][:n_edges])]
            assert min(th) < 1e-6 < max(th), th
        _cache[n_edges] = sc
    return _cache[n_edges]


def _run_chain(torch, dev, sc, stream_kind):
    from monoorbslam3_amd import imu
    d = _Dev(torch, dev, sc, n_priors=2, n_pjobs=3)
    src, init_jobs, pi_jobs, pjobs = (_up(torch, dev, sc[k]) for k in ("src", "init_jobs", "prior_info_jobs", "pjobs"))
    st = _stream(torch, dev, stream_kind)
    results = []
    imu.prior_information_device(d.priors, 2, d.bank, d.cap, pi_jobs, 2, d.result, src, len(sc["src"]), stream=st)
    results.append(d.result.clone())
    imu.graph_init_device(d.graph, d.bank, d.cap, src, len(sc["src"]), init_jobs, d.n, d.result, stream=st)
    results.append(d.result.clone())
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
    results.append(d.result.clone())
    d.linearize(sc, fm.HUBER_DELTA, 0, pjobs, 3, 2, st)
    d.finish()
    return d, [r.cpu().numpy() for r in results]


@pytest.mark.parametrize("n_edges,stream_kind", [(1, "explicit"), (1, "null"), (2, "explicit"), (4, "explicit"), (5, "explicit"), (33, "explicit"), (33, "null")])
def test_a_chain_equals_the_model(n_edges, stream_kind):
    """1, 2 (two edges share the middle state), 4 (one workgroup of four waves), 5 (one edge over) and 33 edges (a multi-workgroup
    chain) with walks, records of 2, 3, 8, 40 and 100 samples with zero and non-zero delta_bias, every fixed-mask bit, three prior
    jobs (two of them on one vertex, one weighted with gyro_info) and the Huber kernel on both of its branches: prior information ->
    init -> edge information -> linearise, every output against the model."""
    import torch
    dev = torch.device("cuda", 0)
    sc = _chain_scene(n_edges)
    d, results = _run_chain(torch, dev, sc, stream_kind)
    what = "chain %d" % n_edges
    assert results[0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and results[1].tolist() == [n_edges + 1, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(results[2], sc["info_res"]) and results[2][0] == n_edges
    _same_floats(what + " priors", d.get("priors"), sc["priors"])
    _assert_graph(what, d, sc["graph"])
    assert np.array_equal(d.get("Rwb"), sc["graph"].Rwb.reshape(-1)) and np.array_equal(d.get("bg"), sc["graph"].bg.reshape(-1))   # widening is exact
    _close(what + " info", d.get("info"), sc["info"], (9, 9))
    _close(what + " walk_info", d.get("walk"), sc["walk"], (3, 3))
    _assert_linear(what, d, sc["out"], 0, 3)


def test_two_runs_of_the_33_edge_chain_give_the_same_bytes():
    import torch
    dev = torch.device("cuda", 0)
    sc = _chain_scene(33)
    runs = []
    for _ in range(2):
        d, _ = _run_chain(torch, dev, sc, "explicit")
        runs.append({k: d.get(k).tobytes() for k in ("info", "walk", "err", "chi2", "chi2_prior", "total", "H_diag", "H_off", "b", "J", "flt", "priors", "result")})
    assert runs[0] == runs[1]


def test_the_trackers_graph():
    """poseFullOptimize's inertial part: 2 states, the first pose fixed, the second without bias vertices (record -1 at init, gyro and
    acc fixed), one edge without walks, three priors; with the default acc prior (acc_info) and with ORBI_PRIOR_ACC_GYRO_INFO"""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    if "tracker" not in _cache:
        sc = fm.make_tracker_graph()
        fm.oplus(sc["graph"], np.random.RandomState(5).normal(0, 1e-4, (2, 15)))   # off the priors
        sc["graph"].iter[:] = 0
        sc["info"], sc["walk"], _ = fm.edge_information(sc["recs"], sc["edges"])
        sc["outs"] = []
        for extra in (0, fm.PRIOR_ACC_GYRO_INFO):
            pj = sc["pjobs"].copy()
            pj["mask"] |= extra
            sc["outs"].append((pj, fm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], sc["priors"], pj)))
        assert not np.array_equal(sc["outs"][0][1]["H_diag"], sc["outs"][1][1]["H_diag"]) and sc["outs"][0][1]["chi2_prior"].all()
        assert not sc["graph"].bg[1].any() and not sc["outs"][0][1]["H_diag"][1][9:].any() and not sc["outs"][0][1]["H_diag"][0][:6].any()
        _cache["tracker"] = sc
    sc = _cache["tracker"]
    for pj, out in sc["outs"]:
        d = _Dev(torch, dev, sc, graph=sc["graph"], n_priors=1, n_pjobs=1)
        d.priors.copy_(_up(torch, dev, sc["priors"]))
        imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result)
        d.linearize(sc, 0.0, 0, _up(torch, dev, pj), 1, 1)
        d.finish()
        _assert_linear("tracker mask %d" % pj["mask"][0], d, out, 0, 1)
        assert not d.get("chi2", (1, 3))[0, 1:].any()
    # the init of a state without bias vertices
    d = _Dev(torch, dev, sc)
    imu.graph_init_device(d.graph, d.bank, d.cap, _up(torch, dev, sc["src"]), 2, _up(torch, dev, sc["init_jobs"]), 2, d.result)
    d.finish()
    assert d.res().tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and not d.get("bg", (2, 3))[1].any() and not d.get("ba", (2, 3))[1].any()
    assert d.get("bg", (2, 3))[0].any()


def _rotation_scene():
    """edge 0: R_wb1 = R_wb2 = I and a record whose gyro equals its bias, so dR = I, tr == 3 and er = 0; edge 1: a rotation error of
    1e-8 rad, the < 1e-6 branches of LogSO3 and InverseRightJacobianSO3"""
    if "rotation" in _cache:
        return _cache["rotation"]
    cal = im.calib()
    rng = np.random.RandomState(21)
    still = fm.make_record(cal, 0, 31, None, rng)
    s = im.make_stream(6, 41, t0=50.0)
    s["w"][:] = still.bias[:3]
    still.compute_preintegration(cal, s, 50.0 - 0.5 / im.RATE, s["t"][-1] + 1.0 / im.RATE)
    assert np.array_equal(still.dR, np.eye(3, dtype=np.float32)) and len(still.meas) == 6
    other = fm.make_record(cal, 8, 32, None, rng)
    recs = [still, other]
    g = fm.Graph(4)
    for k, r in ((0, still), (2, other)):
        g.bg[k], g.ba[k] = r.updated_bias[:3].astype(np.float64), r.updated_bias[3:].astype(np.float64)
        g.bg[k + 1], g.ba[k + 1] = g.bg[k], g.ba[k]
    g.twb, g.v = rng.normal(0, 1.0, (4, 3)), rng.normal(0, 0.5, (4, 3))
    g.Rwb[2] = fm.normalize_rotation(im.rodrigues(rng.normal(0, 0.7, 3)))
    g.Rwb[3] = g.Rwb[2] @ other.dR.astype(np.float64) @ im.rodrigues(1e-8 * np.array([0.6, -0.48, 0.64]))
    edges = np.array([(0, 1, 0, 1), (2, 3, 1, 1)], fm.EDGE)
    sc = dict(cal=cal, recs=recs, graph=g, edges=edges)
    sc["info"], sc["walk"], _ = fm.edge_information(recs, edges)
    sc["out"] = fm.linearize(g, recs, cal["gravity"], edges, sc["info"], sc["walk"])
    er0, er1 = sc["out"]["err"][0, :3], sc["out"]["err"][1, :3]
    assert not er0.any() and np.array_equal(sc["out"]["J"][0, 0:3, 15:18], np.eye(3))
    assert 0.5e-8 < np.linalg.norm(er1) < 2e-8 and np.array_equal(sc["out"]["J"][1, 0:3, 15:18], np.eye(3))
    _cache["rotation"] = sc
    return sc


def test_rotation_edge_cases():
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc = _rotation_scene()
    d = _Dev(torch, dev, sc, graph=sc["graph"])
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result)
    d.linearize(sc, 0.0, 0)
    d.finish()
    _assert_linear("rotation", d, sc["out"], 0)
    err = d.get("err", (2, 9))
    assert not err[0, :3].any()                                                     # tr == 3 exactly: er = 0
    assert np.array_equal(err[1, :3], sc["out"]["err"][1, :3])                      # below 1e-6 no atan2 reaches the result


def _distrust_scene():
    if "distrust" in _cache:
        return _cache["distrust"]
    sc = dict(fm.make_chain(3, seed=9))
    cal = sc["cal"]
    sc["recs"] = sc["recs"] + [fm.make_record(cal, 0, 77)]                          # record 4: no samples, C = 0
    n = sc["graph"].n
    sc["edges"] = np.array([(0, 1, 0, 1), (-1, 1, 1, 1), (1, n, 1, 1), (2, 2, 2, 1), (1, 2, 4, 1), (1, 2, 4, 0), (1, 2, 5, 1), (1, 2, -1, 0), (2, 3, 2, 1),
                            (1, 2, 1, 1)], fm.EDGE)
    sc["info"], sc["walk"], sc["info_res"] = fm.edge_information(sc["recs"], sc["edges"])
    assert sc["info_res"].tolist()[:4] == [6, 2, 0, 2]
    sc["priors"], sc["prior_info_jobs"], _ = fm.make_priors(sc, [0, 1])
    sc["pjobs"] = np.array([(0, 0, 7), (-1, 0, 7), (n, 1, 7), (1, -1, 7), (1, 2, 7), (1, 1, 3)], fm.PRIOR_JOB)
    sc["out"] = fm.linearize(sc["graph"], sc["recs"], cal["gravity"], sc["edges"], sc["info"], sc["walk"], sc["priors"], sc["pjobs"], fm.HUBER_DELTA)
    assert sc["out"]["result"].tolist() == [3, 5, 0, 2, 2, 4, 0, 0]
    _cache["distrust"] = sc
    return sc


def test_distrusted_input_is_dropped_and_counted():
    """Edges with ids -1 and n, i == j, a record index -1 and cap, a record without samples with and without walks (refused by the
    information call, skipped and counted by the linearisation); prior jobs with a state or a slot outside its range; init, prior-
    information and recover jobs out of range, repeated (an earlier job counts whether it was dropped or not) and refused.  What is dropped leaves zeros; the rest equals the model."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc = _distrust_scene()
    d = _Dev(torch, dev, sc, graph=sc["graph"], n_priors=2, n_pjobs=len(sc["pjobs"]))
    d.priors.copy_(_up(torch, dev, sc["priors"]))
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result)
    info_res = d.result.clone()
    d.linearize(sc, fm.HUBER_DELTA, 0, _up(torch, dev, sc["pjobs"]), len(sc["pjobs"]), 2)
    d.finish()
    assert np.array_equal(info_res.cpu().numpy(), sc["info_res"])
    _close("distrust info", d.get("info"), sc["info"], (9, 9))
    _close("distrust walk_info", d.get("walk"), sc["walk"], (3, 3))
    _assert_linear("distrust", d, sc["out"], 0, len(sc["pjobs"]))
    # the job lists of the other calls
    n, cap = d.n, d.cap
    g = fm.Graph(n)
    jobs = np.array([(0, 0, 0), (-1, 0, 0), (n, 0, 0), (1, -1, 0), (1, n, 0), (1, 1, cap), (1, 1, -2), (0, 2, 1), (2, 1, -1), (3, 3, 3)], np.int32)
    want = fm.graph_init(g, sc["recs"], sc["src"], jobs)
    d2 = _Dev(torch, dev, sc, graph=fm.Graph(n))
    imu.graph_init_device(d2.graph, d2.bank, cap, _up(torch, dev, sc["src"]), n, _up(torch, dev, jobs), len(jobs), d2.result)
    d2.finish()
    assert want.tolist() == [3, 6, 1, 0, 0, 0, 0, 0] and np.array_equal(d2.res(), want)
    _assert_graph("distrust init", d2, g)
    pri = np.frombuffer(np.full(144 * 4, 0x5A, np.uint8).tobytes(), fm.PRIOR).copy()
    jobs = np.array([(0, 0, 0), (-1, 0, 0), (4, 0, 0), (1, -1, 0), (1, cap, 0), (1, 1, n), (1, 1, -2), (0, 1, 1), (2, 4, 0), (3, 2, -1)], np.int32)
    want, _ = fm.prior_information(pri, sc["recs"], sc["src"], jobs)
    d3 = _Dev(torch, dev, sc, graph=sc["graph"], n_priors=4)
    imu.prior_information_device(d3.priors, 4, d3.bank, cap, _up(torch, dev, jobs), len(jobs), d3.result, _up(torch, dev, sc["src"]), n)
    d3.finish()
    assert want.tolist() == [2, 6, 1, 1, 0, 0, 0, 0] and np.array_equal(d3.res(), want)
    _same_floats("distrust priors", d3.get("priors"), pri)                          # the refused slot and the velo_priori of source -1 stay as passed
    assert d3.get("priors")[144:3 * 144].tobytes() == pri[1:3].tobytes() and d3.get("priors")[3 * 144:3 * 144 + 12].tobytes() == pri[3:].tobytes()[:12]
    jobs = np.array([(0, 0, 1), (-1, 1, 1), (n, 1, 1), (1, -1, 0), (1, n, 0), (2, 0, 1), (3, 2, 0), (1, 3, 1)], np.int32)
    dst = np.full((n, 15), -4.0, np.float32)
    bias, pose_R, pose_t, want = fm.recover(sc["graph"], sc["cal"], jobs, dst)
    d_dst, d_bias = _padded(torch, dev, np.full(15 * n, -4.0, np.float32), np.float32(-2.5)), _padded(torch, dev, np.full(6 * len(jobs), -4.0, np.float32), np.float32(-2.5))
    d_R, d_t = _padded(torch, dev, np.full(9 * len(jobs), NAN), -1.5), _padded(torch, dev, np.full(3 * len(jobs), NAN), -1.5)
    imu.graph_recover_device(d.graph, _calib(sc["cal"]), _up(torch, dev, jobs), len(jobs), d_dst[1], n, d_bias[1], d.result, d_R[1], d_t[1])
    torch.cuda.synchronize()
    assert want.tolist() == [3, 4, 1, 0, 0, 0, 0, 0] and np.array_equal(d.res(), want)
    assert all(_guards_intact(x[0], f) for x, f in ((d_dst, np.float32(-2.5)), (d_bias, np.float32(-2.5)), (d_R, -1.5), (d_t, -1.5)))
    _same_bits("recover dst", d_dst[1].cpu().numpy(), dst.reshape(-1))
    _same_bits("recover bias", d_bias[1].cpu().numpy(), bias.reshape(-1))
    _same_bits("recover T_cw", np.concatenate([d_R[1].cpu().numpy(), d_t[1].cpu().numpy()]), np.concatenate([pose_R.reshape(-1), pose_t.reshape(-1)]))


def test_one_chain_on_one_stream_with_one_wait():
    """prior information -> init -> edge information -> linearise -> oplus with a fixed dx from the test -> linearise (mode 1) ->
    recover -> orbi_set_bias_device, all enqueued on one stream before the single wait; every stage is compared with the model fed the
    same dx.  Teacher-forced: no accept / reject decision is taken anywhere.  After the oplus the bias vertices are not float-
    representable, and the float intermediates still equal the model's bit for bit: the cast to float is there."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    n_edges = 5
    sc = _chain_scene(n_edges)
    if "one_chain" not in _cache:
        g = sc["graph"].copy()
        dx = np.random.RandomState(17).normal(0, 1.0, (g.n, 15)) * np.array([1e-3] * 3 + [1e-3] * 3 + [1e-3] * 3 + [1e-4] * 3 + [1e-3] * 3)
        graphs = []
        for _ in range(3):                                           # three updates: the third renormalises the rotations
            res = fm.oplus(g, dx)
            graphs.append(g.copy())
        assert not g.iter[(g.fixed & 1) == 0].any() and (g.bg.astype(np.float32).astype(np.float64) != g.bg).any()
        assert not np.array_equal(fm.float_deltas(sc["recs"][1], g.bg[1], g.ba[1])[0], fm.float_deltas(sc["recs"][1], sc["graph"].bg[1], sc["graph"].ba[1])[0])
        out = fm.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], sc["priors"], sc["pjobs"], fm.HUBER_DELTA, mode=1)
        jobs = np.array([(s, s, fm.RECOVER_POSE if s % 2 else 0) for s in range(g.n)], np.int32)
        dst = sc["src"].copy()
        bias, pose_R, pose_t, rres = fm.recover(g, sc["cal"], jobs, dst)
        _cache["one_chain"] = dict(dx=dx, graphs=graphs, ores=res, out=out, jobs=jobs, dst=dst, bias=bias, rres=rres)
    m = _cache["one_chain"]
    d = _Dev(torch, dev, sc, n_priors=2, n_pjobs=3)
    n = d.n
    src, init_jobs, pi_jobs, pjobs, dx, jobs = (_up(torch, dev, a) for a in (sc["src"], sc["init_jobs"], sc["prior_info_jobs"], sc["pjobs"], m["dx"], m["jobs"]))
    ids = _up(torch, dev, np.arange(n, dtype=np.int32))
    d_dst, d_bias = _padded(torch, dev, sc["src"], np.float32(-2.5)), _padded(torch, dev, np.full(6 * n, -4.0, np.float32), np.float32(-2.5))
    d_R, d_t = _padded(torch, dev, np.full(9 * n, NAN), -1.5), _padded(torch, dev, np.full(3 * n, NAN), -1.5)
    first = {k: torch.empty_like(getattr(d, k)) for k in ("err", "chi2", "total", "chi2_prior", "H_diag", "H_off", "b", "J", "flt", "result")}
    stages = []
    st = _stream(torch, dev, "explicit")
    cal = _calib(sc["cal"])
    imu.prior_information_device(d.priors, 2, d.bank, d.cap, pi_jobs, 2, d.result, src, n, stream=st)
    imu.graph_init_device(d.graph, d.bank, d.cap, src, n, init_jobs, n, d.result, stream=st)
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
    d.linearize(sc, fm.HUBER_DELTA, 0, pjobs, 3, 2, st)
    for k, t in first.items():
        t.copy_(getattr(d, k))                                   # device-to-device on the same stream: no wait
    for _ in range(3):
        imu.graph_oplus_device(d.graph, dx, d.it, d.result, stream=st)
        stages.append({k: getattr(d, k).clone() for k in ("Rwb", "twb", "v", "bg", "ba", "it", "result")})
    d.linearize(sc, fm.HUBER_DELTA, 1, pjobs, 3, 2, st)
    lin_res = d.result.clone()
    imu.graph_recover_device(d.graph, cal, jobs, n, d_dst[1], n, d_bias[1], d.result, d_R[1], d_t[1], stream=st)
    rec_res = d.result.clone()
    imu.set_bias_device(cal, d.bank, d.pool, d.cap, d.cap_meas, ids, d_bias[1], n, d.result, stream=st)
    set_res = d.result.clone()
    d.finish()                                                       # the one wait
    # linearise (mode 0) at the initial estimate
    later = {k: getattr(d, k).clone() for k in first}
    for k, t in first.items():
        getattr(d, k).copy_(t)
    _assert_linear("one chain: linearise", d, sc["out"], 0, 3)
    # the three updates
    for k, (got, want) in enumerate(zip(stages, m["graphs"])):
        _close("one chain: oplus %d Rwb" % k, got["Rwb"].cpu().numpy(), want.Rwb, (3, 3))
        for name in ("twb", "v", "bg", "ba"):
            _close("one chain: oplus %d %s" % (k, name), got[name].cpu().numpy(), getattr(want, name), None)
        assert np.array_equal(got["it"].cpu().numpy(), want.iter) and np.array_equal(got["result"].cpu().numpy(), m["ores"])
    fixed = sc["graph"].fixed
    assert np.array_equal(stages[2]["bg"].cpu().numpy().reshape(-1, 3)[(fixed & 4) != 0], sc["graph"].bg[(fixed & 4) != 0])   # fixed vertices did not move
    # computeError at the updated estimate; H, b and J are as the first linearisation left them
    for k in ("err", "chi2", "total", "chi2_prior", "flt"):
        getattr(d, k).copy_(later[k])
    d.result.copy_(lin_res)
    _assert_linear("one chain: mode 1", d, m["out"], 1, 3)
    assert all(torch.equal(later[k], first[k]) for k in ("H_diag", "H_off", "b", "J"))
    # recover and set_bias
    assert np.array_equal(rec_res.cpu().numpy(), m["rres"]) and m["rres"][0] == n
    assert _guards_intact(d_dst[0], np.float32(-2.5)) and _guards_intact(d_bias[0], np.float32(-2.5)) and _guards_intact(d_R[0], -1.5) and _guards_intact(d_t[0], -1.5)
    got_dst, got_bias = d_dst[1].cpu().numpy().reshape(n, 15), d_bias[1].cpu().numpy().reshape(n, 6)
    # the recovered floats are roundings of doubles held to 1e-9: equal to the model's up to one float ulp, and mostly equal
    _same_floats("one chain: recover dst", got_dst, m["dst"])
    _same_floats("one chain: recover bias", got_bias, m["bias"])
    pose = np.array([bool(j[2] & fm.RECOVER_POSE) for j in m["jobs"]])
    got_R, got_t = d_R[1].cpu().numpy().reshape(n, 9), d_t[1].cpu().numpy().reshape(n, 3)
    assert np.isnan(got_R[~pose]).all() and np.isnan(got_t[~pose]).all() and pose.any() and (~pose).any()
    _, want_R, want_t, _ = fm.recover(_graph_from(got_dst, pose, m["graphs"][2]), sc["cal"], m["jobs"], got_dst.copy())
    _same_bits("one chain: T_cw", np.concatenate([got_R[pose].reshape(-1), got_t[pose].reshape(-1)]), np.concatenate([want_R[pose].reshape(-1), want_t[pose].reshape(-1)]))
    # setNewBias with the recovered biases: the bank equals the model's given the same biases
    bank = _pack(sc["recs"])
    sres = im.run_set_bias(sc["cal"], bank, np.arange(n), got_bias)
    assert np.array_equal(set_res.cpu().numpy(), sres) and sres[0] == n
    assert d.bank.cpu().numpy().tobytes() == bank.pack()[0].tobytes()


def _graph_from(dst, pose, g):
    """the model graph with the poses the device recovered (floats widened), so that T_cw is judged given those floats"""
    o = g.copy()
    for s in np.nonzero(pose)[0]:
        o.Rwb[s], o.twb[s] = dst[s, :9].reshape(3, 3).astype(np.float64), dst[s, 9:12].astype(np.float64)
    return o
