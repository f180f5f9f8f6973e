"""fullInertialOptimize's shared-bias graph on the MI355X (include/orbfi.h) against tests/full_inertial_model.py.  Every stage is
teacher-forced: it gets uploaded inputs and is compared with the model on those same inputs, every output starts from NaN (or a
marker) and sits between guard elements.  The float intermediates and every counter and index: bit for bit.  Every double output:
within 1e-9 of the model relative to the largest entry of its own block -- the bar of the sibling tests.  Model outputs are computed
once per scene and shared.  The largest deviation met is printed per output."""
import numpy as np
import pytest

import factors_model as fm
import full_inertial_model as fim
from test_factors_gpu import _Dev, _assert_graph, _calib, _close as _close3, _same_bits
from test_projection_queries_gpu import _stream, _up
from test_vw_gpu import _Win, _close

pytestmark = pytest.mark.gpu

NAN = float("nan")
_cache = {}


def _scene(n_kf, fix_first=True):
    key = (n_kf, fix_first)
    if key not in _cache:
        sc = fim.stage_scene(n_kf, fix_first)
        sc["info"], sc["walk"], _ = fm.edge_information(sc["recs"], sc["edges"])
        sc["lin"] = {mode: fim.inertial_linearize(sc, sc["graph"], mode) for mode in (0, 1)}
        _cache[key] = sc
    return _cache[key]


class _Fi:
    """a scene's device memory: tests/test_factors_gpu.py's for the inertial side, tests/test_vw_gpu.py's for the window, on ONE graph, and
    what orbfi.h adds -- the three off-diagonal entries and blocks of an edge, the two priors' chi2"""

    def __init__(self, torch, dev, sc, graph=None, edges=None, info=None):
        from monoorbslam3_amd import full_inertial
        self.torch, self.dev, self.sc, self.fi = torch, dev, sc, full_inertial
        sc_i = sc if edges is None else dict(sc, edges=edges)
        self.i = i = _Dev(torch, dev, sc_i, sc["graph"] if graph is None else graph)
        self.w = w = _Win(torch, dev, sc, sc["graph"] if graph is None else graph)
        w.graph, w.fixed = i.graph, i.fixed
        ne = max(i.ne, 1)
        self.work = i._pad("fi work", np.full(fim.EDGE_WORK * ne, NAN), -1.5)
        self.chi2 = i._pad("fi chi2", np.full(ne, NAN), -1.5)
        self.chi2_prior = i._pad("fi chi2_prior", np.full(2, NAN), -1.5)
        self.H_off = i._pad("fi H_off", np.full(675 * ne, NAN), -1.5)
        self.off_edges = i._pad("fi off_edges", np.full(12 * ne, -77, np.int32), -3)
        w.edges, w.n_iedges = self.off_edges, 3 * i.ne
        i.info.copy_(_up(torch, dev, np.asarray(sc["info"] if info is None else info, np.float64).reshape(-1)))

    def linearize(self, mode, stream=None, null=None, **over):
        i, sc = self.i, self.sc
        z = (mode != 0) if null is None else null
        a = dict(bias_state=sc["bias_state"], prior_rec=sc["prior_rec"], prior_g=sc["prior_g"], prior_a=sc["prior_a"])
        a.update(over)
        self.fi.linearize_device(i.graph, i.bank, i.cap, sc["cal"]["gravity"], i.edges, i.ne, i.info, a["bias_state"], a["prior_rec"], a["prior_g"], a["prior_a"],
                                 self.work, i.err, self.chi2, self.chi2_prior, i.total, i.result, mode=mode, d_H_diag=None if z else i.H_diag,
                                 d_b=None if z else i.b, d_off_edges=None if z else self.off_edges, d_H_off=None if z else self.H_off, d_float=i.flt, stream=stream)

    def iteration(self, lam, stream, wait):
        """one whole iteration of the chain, with or without a wait behind every call"""
        i, w, torch = self.i, self.w, self.torch
        from monoorbslam3_amd import imu
        calls = [lambda: self.linearize(0, stream), lambda: w.linearize(0, H_diag=i.H_diag, b=i.b, stream=stream), lambda: w.lam.fill_(lam),
                 lambda: w.reduce(H_diag=i.H_diag, H_off=self.H_off, b=i.b, stream=stream), lambda: w.solve(b=i.b, stream=stream), lambda: w.backsub(stream=stream),
                 lambda: imu.graph_oplus_device(i.graph, w.dx, i.it, i.result, stream=stream), lambda: self.linearize(1, stream),
                 lambda: w.linearize(1, points=w.points_out, stream=stream)]
        for c in calls:
            c()
            if wait:
                torch.cuda.synchronize()
        torch.cuda.synchronize()

    def get(self, key, shape=None):
        t = getattr(self, key) if hasattr(self, key) else getattr(self.i, key)
        a = t.cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def everything(self):
        keys = ("Rwb", "twb", "v", "bg", "ba", "it", "err", "total", "H_diag", "b", "flt", "result", "chi2", "chi2_prior", "H_off", "off_edges", "work")
        out = {k: self.get(k).tobytes() for k in keys}
        out.update({"w " + k: self.w.get(k).tobytes() for k in ("S", "rhs", "dx", "out", "xl", "points_out", "out_points", "Hll", "bl", "Hlp", "total", "chi2")})
        return out

    def finish(self):
        self.i.finish()
        self.w.finish()


def _off_edges(d):
    return d.get("off_edges").view(fm.EDGE) if d.i.ne else np.zeros(0, fm.EDGE)


def _assert_fi(what, d, o, mode):
    ne = d.i.ne
    _same_bits(what + " float dR dV dP", d.get("flt", (-1, 15))[:ne], o["flt"])
    _close3(what + " err", d.get("err")[:9 * ne], o["err"], None)
    _close3(what + " chi2", d.get("chi2")[:ne], o["chi2"], ())
    _close3(what + " chi2_prior", d.get("chi2_prior"), o["chi2_prior"], ())
    _close3(what + " total", d.get("total"), o["total"], ())
    assert np.array_equal(d.i.res(), o["result"]), (what, d.i.res(), o["result"])
    if mode != 0:
        assert np.isnan(d.get("H_diag")).all() and np.isnan(d.get("b")).all() and np.isnan(d.get("H_off")).all() and (d.get("off_edges") == -77).all(), what
        return
    _close3(what + " H_diag", d.get("H_diag"), o["H_diag"], (15, 15))
    _close3(what + " b", d.get("b"), o["b"], None)
    _close3(what + " H_off", d.get("H_off")[:675 * ne], o["H_off"], (15, 15))
    assert np.array_equal(_off_edges(d)[:3 * ne], o["off_edges"]), what
    Hd = d.get("H_diag", (-1, 15, 15))
    _close3(what + " H_diag symmetric", Hd, np.transpose(Hd, (0, 2, 1)), (15, 15))


# ---- the stages ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_first", [True, False])
@pytest.mark.parametrize("n_kf", [2, 3, 5, 31])
def test_every_stage_equals_the_model(n_kf, fix_first):
    """2 key frames: one edge, no interior state; 3: one interior state, whose two (s, b) entries add in the reduce; 5; 31: 480 unknowns,
    the limit.  The job lists, the vertices, both modes of the linearisation, the reduce behind it, the solve's fixed dof, the recovery."""
    import torch
    from monoorbslam3_amd import full_inertial, imu
    dev = torch.device("cuda", 0)
    sc = _scene(n_kf, fix_first)
    what = "%d key frames%s" % (n_kf, ", the first fixed" if fix_first else "")
    g, ne, n = sc["graph"], n_kf - 1, n_kf + 1
    # the job lists from the window assembly's, then the vertices from them
    start = fm.Graph(n)
    start.fixed[:] = 0xEE
    d = _Fi(torch, dev, sc, graph=start)
    i, w = d.i, d.w
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        getattr(i, k).fill_(NAN)
    win_init = np.stack([np.arange(n_kf)] * 3, 1).astype(np.int32)                       # (state, state row, record) of an all-key-frame window
    win_edges = sc["edges"].copy()
    win_edges["flags"] = fm.EDGE_WALKS
    mj = fim.jobs(win_init, win_edges, sc["recover_jobs"], n_kf, fix_first, len(sc["src"]), len(sc["recs"]))
    assert np.array_equal(mj["fixed"], g.fixed) and np.array_equal(mj["init"], sc["init_jobs"]) and np.array_equal(mj["edges"], sc["edges"]) and mj["prior_rec"] == sc["prior_rec"]
    init_out = i._pad("init_out", np.full(3 * n, -77, np.int32), -3)
    rec_out = i._pad("rec_out", np.full(3 * n_kf, -77, np.int32), -3)
    edges_out = i._pad("edges_out", np.full(4 * max(ne, 1), -77, np.int32), -3)
    prior_rec = i._pad("prior_rec", np.full(1, -77, np.int32), -3)
    fixed = i._pad("fixed out", np.full(n, 0xEE, np.uint8), 0xA5)
    full_inertial.jobs_device(_up(torch, dev, win_init), _up(torch, dev, win_edges), _up(torch, dev, sc["recover_jobs"]), n_kf, fix_first, len(sc["src"]), i.cap,
                              fixed, init_out, edges_out, rec_out, prior_rec, i.result)
    assert np.array_equal(i.res(), mj["result"]) and np.array_equal(fixed.cpu().numpy(), g.fixed), what
    assert np.array_equal(init_out.cpu().numpy().reshape(-1, 3), mj["init"]) and np.array_equal(rec_out.cpu().numpy().reshape(-1, 3), mj["recover"]), what
    assert np.array_equal(edges_out.cpu().numpy()[:4 * ne].view(fm.EDGE), mj["edges"]) and prior_rec.cpu().numpy()[0] == mj["prior_rec"], what
    i.fixed.copy_(fixed)
    imu.graph_init_device(i.graph, i.bank, i.cap, _up(torch, dev, sc["src"]), len(sc["src"]), init_out, n, i.result)
    assert i.res().tolist() == [n, 0, 0, 0, 0, 0, 0, 0], what
    _assert_graph(what + " init", i, g)
    assert not i.get("bg", (n, 3))[:n_kf].any() and not i.get("ba", (n, 3))[:n_kf].any() and i.get("bg", (n, 3))[n_kf].all(), what
    # mode 0, then the reduce and the solve behind it
    d.linearize(0)
    _assert_fi(what + " mode 0", d, sc["lin"][0], 0)
    it = sc["first"]
    w.linearize(0, H_diag=i.H_diag, b=i.b)
    w.lam.fill_(1.0)
    w.reduce(H_diag=i.H_diag, H_off=d.H_off, b=i.b)
    assert np.array_equal(w.get("result"), it["reduce"]["result"]), (what, w.get("result"))
    N = 15 * n
    blocks = lambda S: np.asarray(S).reshape(n, 15, n, 15).transpose(0, 2, 1, 3)  # noqa: E731
    _close(what + ": S", blocks(w.get("S", (N, N))), blocks(it["reduce"]["S"]), 2)
    _close(what + ": rhs", w.get("rhs", (n, 15)), it["reduce"]["rhs"].reshape(n, 15), 1)
    base = fim.dense(sc["lin"][0], g.fixed, len(sc["recs"]), 1.0)[0]
    Sd, vis = w.get("S", (N, N)), it["reduce"]["S"] - base
    _close(what + ": the base", blocks(np.where(vis == 0, Sd, 0.0)), blocks(np.where(vis == 0, base, 0.0)), 2)   # where the Schur complement adds nothing
    w.solve(b=i.b)
    assert w.get("result").tolist() == [1, 0, 0, 0, 0, 0, 0, 0], what
    dx = w.get("dx", (n, 15))
    fx = np.stack([fm.dof_fixed(f) for f in g.fixed])
    assert not dx[fx].any() and dx[~fx].all() and np.isfinite(dx).all(), what
    assert dx[n_kf, 9:].all() and not dx[:n_kf, 9:].any() and (not dx[0, :9].any()) == fix_first, what
    # mode 1 on fresh NaN
    d1 = _Fi(torch, dev, sc)
    d1.linearize(1, stream=_stream(torch, dev, "explicit"))
    d1.finish()
    _assert_fi(what + " mode 1", d1, sc["lin"][1], 1)
    # the recovery of the model's updated graph
    g1 = it["graph"]
    d2 = _Fi(torch, dev, sc, graph=g1)
    dst0 = np.random.RandomState(3).normal(0, 1, (len(sc["src"]), 15)).astype(np.float32)
    dst = d2.i._pad("dst", dst0.reshape(-1).copy(), np.float32(-2.5))
    bias = d2.i._pad("bias", np.full(6 * n_kf, NAN, np.float32), np.float32(-2.5))
    pR, pt = d2.i._pad("pose_R", np.full(9 * n_kf, NAN), -1.5), d2.i._pad("pose_t", np.full(3 * n_kf, NAN), -1.5)
    jobs = sc["recover_jobs"].copy()
    jobs[:, 2] = 0                                              # the flags say no pose: this recovery writes it all the same
    full_inertial.recover_device(d2.i.graph, _calib(sc["cal"]), n_kf, _up(torch, dev, jobs), n_kf, dst, len(dst0), bias, d2.i.result, pR, pt)
    want = dst0.copy()
    mb, mR, mt, mres = fim.recover(g1, sc["cal"], n_kf, jobs, want)
    assert np.array_equal(d2.i.res(), mres) and mres[0] == n_kf, what
    _same_bits(what + " recovered states", dst.cpu().numpy().reshape(-1, 15), want)
    _same_bits(what + " recovered bias", bias.cpu().numpy().reshape(-1, 6), mb)
    _same_bits(what + " T_cw", np.concatenate([pR.cpu().numpy(), pt.cpu().numpy()]), np.concatenate([mR.reshape(-1), mt.reshape(-1)]))
    assert (mb == mb[0]).all() and mb[0].all(), what
    for x in (d, d2):
        x.finish()


# ---- distrust ----------------------------------------------------------------------------------------------------------------------------------
def test_distrusted_edges_priors_and_jobs_write_zeros_and_nothing_outside():
    """an edge with a state out of range, one naming the carrier, one with i == j, one whose information was refused, prior_rec out of
    range, a duplicate destination in the recovery"""
    import torch
    from monoorbslam3_amd import full_inertial
    dev = torch.device("cuda", 0)
    sc = _scene(5)
    n_kf, b = 5, 5
    edges = np.concatenate([sc["edges"], np.array([(1, 9, 0, 0), (2, b, 1, 0), (3, 3, 2, 0), (-1, 2, 0, 0), (0, 1, 99, 0)], fm.EDGE)])
    info = np.concatenate([sc["info"], sc["info"][[0, 1, 2, 0, 0]]])
    info[2] = 0.0                                               # what orbi_edge_information_device leaves for a refused record
    for prior_rec in (sc["prior_rec"], len(sc["recs"]), -1):
        o = fim.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], edges, info, b, prior_rec, sc["prior_g"], sc["prior_a"])
        assert o["result"].tolist()[:4] == [3, 5, 0, 1] and o["result"][4:6].tolist() == ([2, 0] if prior_rec == sc["prior_rec"] else [0, 2])
        d = _Fi(torch, dev, sc, edges=edges, info=info)
        d.linearize(0, prior_rec=prior_rec)
        d.finish()
        _assert_fi("distrusted, prior_rec %d" % prior_rec, d, o, 0)
        bad = o["status"] != 0
        assert bad.sum() == 6 and not d.get("err", (-1, 9))[bad].any() and not d.get("chi2")[bad].any() and not d.get("flt", (-1, 15))[bad].any()
        assert not d.get("H_off", (-1, 3, 225))[bad].any() and not d.get("off_edges", (-1, 3, 4))[bad].any()
        if prior_rec != sc["prior_rec"]:
            assert not d.get("chi2_prior").any() and d.get("H_diag", (-1, 15, 15))[b, 9:, 9:].any()
    # the recovery: a destination named twice, a state and a destination out of range
    jobs = np.array([(0, 0, 1), (1, 0, 1), (7, 2, 1), (2, 9, 1), (3, 3, 1)], np.int32)
    d = _Fi(torch, dev, sc)
    dst0 = np.random.RandomState(4).normal(0, 1, (len(sc["src"]), 15)).astype(np.float32)
    dst = d.i._pad("dst", dst0.reshape(-1).copy(), np.float32(-2.5))
    bias = d.i._pad("bias", np.full(6 * len(jobs), NAN, np.float32), np.float32(-2.5))
    full_inertial.recover_device(d.i.graph, _calib(sc["cal"]), b, _up(torch, dev, jobs), len(jobs), dst, len(dst0), bias, d.i.result)
    d.finish()
    want = dst0.copy()
    mb, _, _, mres = fim.recover(sc["graph"], sc["cal"], b, jobs, want)
    assert mres.tolist()[:4] == [2, 2, 1, 0] and np.array_equal(d.i.res(), mres)
    _same_bits("recovered states", dst.cpu().numpy().reshape(-1, 15), want)
    _same_bits("recovered bias", bias.cpu().numpy().reshape(-1, 6), mb)
    assert not mb[1:4].any() and mb[0].all() and np.array_equal(want[1], dst0[1]) and np.array_equal(want[2], dst0[2])


def test_the_job_lists_distrust_their_indices():
    import torch
    from monoorbslam3_amd import full_inertial
    dev = torch.device("cuda", 0)
    sc = _scene(5)
    n_kf, n_src, cap = 5, len(sc["src"]), len(sc["recs"])
    win_init = np.stack([np.arange(n_kf)] * 3, 1).astype(np.int32)
    win_init[1, 1], win_init[4, 2] = n_src, cap                   # a state row and the LAST key frame's record out of range
    win_edges = sc["edges"].copy()
    win_edges["i"][0], win_edges["rec"][2], win_edges["j"][3] = -3, cap, n_kf
    m = fim.jobs(win_init, win_edges, sc["recover_jobs"], n_kf, True, n_src, cap)
    assert m["result"].tolist()[:2] == [4, 5] and m["prior_rec"] == -1 and m["init"][5].tolist() == [5, 4, -2] and m["init"][1].tolist() == [1, -1, -1]
    d = _Fi(torch, dev, sc)
    i = d.i
    out = [i._pad("fixed out", np.full(n_kf + 1, 0xEE, np.uint8), 0xA5), i._pad("init_out", np.full(3 * (n_kf + 1), -77, np.int32), -3),
           i._pad("edges_out", np.full(4 * (n_kf - 1), -77, np.int32), -3), i._pad("rec_out", np.full(3 * n_kf, -77, np.int32), -3), i._pad("prior_rec", np.full(1, -77, np.int32), -3)]
    full_inertial.jobs_device(_up(torch, dev, win_init), _up(torch, dev, win_edges), _up(torch, dev, sc["recover_jobs"]), n_kf, True, n_src, cap, *out, i.result)
    d.finish()
    got = [t.cpu().numpy() for t in out]
    assert np.array_equal(i.res(), m["result"]) and np.array_equal(got[0], m["fixed"]) and np.array_equal(got[1].reshape(-1, 3), m["init"])
    assert np.array_equal(got[2].view(fm.EDGE), m["edges"]) and np.array_equal(got[3].reshape(-1, 3), m["recover"]) and got[4][0] == -1


# ---- repeatability and streams -------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_both_streams_give_the_same_bytes():
    """one whole iteration enqueued on an explicit stream and on NULL with one wait gives the bytes of the same calls with a wait behind each"""
    import torch
    from inertial_loop import _chain_stream
    dev = torch.device("cuda", 0)
    sc = _scene(5)
    runs = {}
    for kind, wait in (("waits", True), ("again", True), ("explicit", False), ("null", False)):
        d = _Fi(torch, dev, sc)
        st = _chain_stream(torch, dev, "null" if kind == "null" else "explicit")
        d.iteration(1.0, st, wait)
        d.finish()
        runs[kind] = d.everything()
    for kind in ("again", "explicit", "null"):
        for k, v in runs["waits"].items():
            assert runs[kind][k] == v, (kind, k)
