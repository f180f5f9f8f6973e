"""The steps of the IMU initialisation on the device (include/orbii.h) and the map rescale (include/orbm.h) against tests/imu_init_model.py
on an MI355X: every stage teacher-forced, distrusted input, one trial as a chain on one stream with one wait, the closed loop with every
trial audited, and the whole step on a small device-resident map.  Every array starts from NaN / -9 padding with guard elements."""
import numpy as np
import pytest

import factors_model as fm
import imu_init_model as mm
import imu_model as im
import inertial_loop as il
import vw_model as wm
from test_factors_gpu import _calib, _pack, _same_bits
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up

pytestmark = pytest.mark.gpu

BAR = il.BAR
NAN = float("nan")
# Rwg of the prior goes through asin, sinf and cosf.  Each entry of ExpSO3f is 1 or 0 plus two terms of magnitude <= 1, each a product of
# two or three correctly rounded float operations on sinf(d) / d and (1 - cosf(d)) / d2; a one-ulp difference of asin (the device's
# against glibc's, rounded to float) moves d by one float ulp.  Four float ulps of 1 (4 * 2^-23 = 4.8e-7) bound the entry; the largest
# deviation the test has printed on an MI355X is 0 (asin rounded to float agreed on every scene).
RWG_BAR = 4 * 2.0 ** -23
_worst = {}


def _rel(what, got, want, bar=BAR):
    """doubles: the largest deviation, as a share of the output's largest entry, is at most `bar`"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    scale = np.abs(want).max() if want.size else 0.0
    dev = float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max() if got.size else 0.0)
    _worst[what] = max(_worst.get(what, 0.0), dev)
    print("%-14s largest deviation %.3g of the output's largest entry (the worst so far %.3g)" % (what, dev, _worst[what]))
    assert dev <= bar, (what, dev)


class _Init:
    """a scene's device memory: the pose table, the state rows, the bank, the prior slots, the graph and every output, padded.  The tables
    have two rows more than the scene has key frames, filled with -9: nobody may touch them."""

    def __init__(self, torch, dev, sc, kind, jobs=None, state=None, priors=None):
        from monoorbslam3_amd import imu, imu_init, vw
        self.torch, self.dev, self.imu, self.ii, self.vw, self.sc, self.kind = torch, dev, imu, imu_init, vw, sc, kind
        n = self.n = sc["n_kf"]
        self.ne, self.N = n - 1, mm.system_size(n)
        self.n_pose = self.n_src = self.n_priors = n + 2
        bank, pool = _pack(sc["recs"]).pack()
        self.cap, self.cap_meas, self.bank, self.pool = len(bank), pool.shape[1], _up(torch, dev, bank), _up(torch, dev, pool)
        self.pads = {}
        self.pose_R = _up(torch, dev, np.concatenate([sc["pose_R"], np.full((2, 9), NAN)]))
        self.pose_t = _up(torch, dev, np.concatenate([sc["pose_t"], np.full((2, 3), NAN)]))
        self.state = self._pad("state", self.state_table(sc["state"] if state is None else state), np.float32(-2.5))
        self.priors = self._pad("priors", np.frombuffer(self.prior_table(priors).tobytes(), np.uint8), 0xA5)
        self.jobs = _up(torch, dev, np.asarray(sc["jobs"] if jobs is None else jobs, np.int32))
        self.edges = _up(torch, dev, sc["edges"])
        f64 = lambda k, m: self._pad(k, np.full(m, NAN, np.float64), -1.5)  # noqa: E731
        self.v, self.shared = f64("v", 3 * n), f64("shared", 16)
        self.Rwb, self.twb, self.Oc, self.Pcb = f64("Rwb", 9 * n), f64("twb", 3 * n), f64("Oc", 3 * n), f64("Pcb", 3 * n)
        self.it = self._pad("it", np.full(1, -9, np.int32), -3)
        self.graph = imu_init.Graph.make(self.v, self.shared, self.it, self.Rwb, self.twb, self.Oc, self.Pcb, n)
        self.Rwg = f64("Rwg", 9)
        self.info, self.walk = f64("info", 81 * self.ne), f64("walk", 18 * self.ne)
        self.work, self.err, self.chi2 = f64("work", mm.EDGE_WORK * self.ne), f64("err", 9 * self.ne), f64("chi2", self.ne)
        self.chi2_prior, self.total = f64("chi2_prior", 2), f64("total", 1)
        self.H, self.b, self.S, self.rhs = f64("H", self.N * self.N), f64("b", self.N), f64("S", self.N * self.N), f64("rhs", self.N)
        self.dx, self.out, self.lam = f64("dx", self.N), f64("out", 3), f64("lam", 1)
        self.flt = self._pad("flt", np.full(15 * self.ne, -9.0, np.float32), np.float32(-2.5))
        self.bias = self._pad("bias", np.full(6 * n, -9.0, np.float32), np.float32(-2.5))
        self.summary = self._pad("summary", np.full(mm.SUMMARY, -9.0, np.float32), np.float32(-2.5))
        self.result = self._pad("result", np.full(8, 77, np.int32), -6)
        self.cal, self.ib = _calib(sc["cal"]), imu_init.Bias.make(sc["initial_bias"])
        self.saved = [f64("saved v", 3 * n), f64("saved shared", 16), self._pad("saved it", np.full(1, -9, np.int32), -3)]

    def state_table(self, state):
        return np.concatenate([np.asarray(state, np.float32), np.full((2, 15), -9.0, np.float32)])

    def prior_table(self, priors=None):
        t = np.zeros(self.n_priors, fm.PRIOR)
        for k in t.dtype.names:
            t[k] = -9.0
        if priors is not None:
            t[:len(priors)] = priors
        return t

    def _pad(self, key, a, fill):
        self.pads[key] = (_padded(self.torch, self.dev, a, fill), fill)
        return self.pads[key][0][1]

    def get(self, key, shape=None):
        a = getattr(self, key).cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def res(self):
        return self.result.cpu().numpy().copy()

    def priors_np(self):
        return np.frombuffer(self.priors.cpu().numpy().tobytes(), fm.PRIOR)

    def put_graph(self, g):
        """teacher forcing: the model's vertices into the device graph"""
        self.v.copy_(_up(self.torch, self.dev, g.v.reshape(-1)))
        self.shared.copy_(_up(self.torch, self.dev, g.shared))
        self.it.fill_(int(g.iter))

    def finish(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))
        for key, ((whole, _), fill) in self.pads.items():
            assert _guards_intact(whole, fill), key

    # ---- the calls
    def prior(self, st=None):
        self.ii.prior_device(self.pose_R, self.pose_t, self.n_pose, self.state, self.n_src, self.bank, self.cap, self.priors, self.n_priors, self.jobs,
                             self.n, self.Rwg, self.result, stream=st)

    def init(self, Rwg, scale, st=None):
        self.ii.graph_init_device(self.graph, self.cal, self.pose_R, self.pose_t, self.n_pose, self.state, self.n_src, self.jobs, self.ib, self.result,
                                  d_Rwg=Rwg, scale=scale, stream=st)

    def information(self, st=None):
        self.imu.edge_information_device(self.bank, self.cap, self.edges, self.ne, self.info, self.walk, self.result, stream=st)

    def linearize(self, pg, pa, mode, st=None):
        self.ii.linearize_device(self.graph, self.bank, self.cap, self.sc["cal"]["gravity"], self.edges, self.info, self.ib, pg, pa, self.kind, self.work,
                                 self.err, self.chi2, self.chi2_prior, self.total, self.result, mode=mode, d_H=None if mode else self.H,
                                 d_b=None if mode else self.b, d_float=self.flt, stream=st)

    def damp(self, st=None):
        self.ii.damp_device(self.n, self.kind, self.H, self.b, self.lam, self.S, self.rhs, self.out, self.result, stream=st)

    def solve(self, st=None):
        self.vw.solve_device(self.N // 15, self.S, self.rhs, self.b, self.lam, self.dx, self.out, self.result, stream=st)

    def oplus(self, st=None):
        self.ii.oplus_device(self.graph, self.kind, self.dx, self.result, stream=st)

    def recover(self, st=None):
        self.ii.recover_device(self.graph, self.jobs, self.state, self.n_src, self.priors, self.n_priors, self.bias, self.summary, self.result, stream=st)

    def push(self):
        for s, t in zip(self.saved, (self.v, self.shared, self.it)):
            s.copy_(t)

    def pop(self):
        for s, t in zip(self.saved, (self.v, self.shared, self.it)):
            t.copy_(s)

    def estimate(self):
        return dict(v=self.get("v", (self.n, 3)).copy(), shared=self.get("shared").copy(), iter=self.get("it").copy())


def _assert_linear(d, o, mode):
    n, ne, N = d.n, d.ne, d.N
    assert np.array_equal(d.res(), o["result"]), (d.res(), o["result"])
    _rel("err", d.get("err"), o["err"])
    _rel("chi2", d.get("chi2"), o["chi2"])
    _rel("chi2_prior", d.get("chi2_prior"), o["chi2_prior"])
    _rel("total", d.get("total"), o["total"])
    _same_bits("flt", d.get("flt", (ne, 15)), o["flt"])
    if mode == 0:
        H = d.get("H", (N, N))
        _rel("H", H, o["H"])
        _rel("b", d.get("b"), o["b"])
        fixed = ~mm.dof_free(n, d.kind)
        assert np.array_equal(H[fixed][:, fixed], np.eye(int(fixed.sum()))) and not H[fixed][:, ~fixed].any() and not d.get("b")[fixed].any()
        zero = o["H"] == 0
        assert not H[zero].any(), "entries that no edge touches are exactly zero"


PG, PA = 1e6, 1e12
STAGE_SHAPES = [(2, mm.KIND_GS), (3, mm.KIND_G), (6, mm.KIND_GS), (6, mm.KIND_G), (17, mm.KIND_GS), (66, mm.KIND_GS), (66, mm.KIND_G)]


@pytest.mark.parametrize("n_kf,kind", STAGE_SHAPES)
def test_every_stage_equals_the_model(n_kf, kind):
    """n_kf 2: one edge, N = 15 without padding; 3: N = 18 padded to 30; 6: a workgroup of four edge waves plus one; 17: N = 60 exact; 66:
    65 edges, N = 210.  Records of 2, 3, 8, 40 and 100 samples in turn, every second one with a non-zero delta_bias.  Each stage is given
    the model's inputs of that stage."""
    import torch
    dev = torch.device("cuda:0")
    scale = 1.05 if kind == mm.KIND_GS else 1.0
    sc = mm.make_scene(n_kf, seed=20 + n_kf, tilt=0.1, scale=scale)
    d = _Init(torch, dev, sc, kind)
    # the prior
    m_state, m_priors = d.state_table(sc["state"]), d.prior_table()
    m_Rwg, m_res = mm.prior(sc["pose_R"], sc["pose_t"], m_state, sc["recs"], m_priors, sc["jobs"])
    d.prior()
    assert np.array_equal(d.res(), m_res) and m_res[mm.R_DONE] == n_kf and not m_res[mm.R_REFUSED]
    _same_bits("state", d.get("state", (-1, 15)), m_state)
    assert d.priors_np().tobytes() == m_priors.tobytes()
    dev_Rwg = np.abs(d.get("Rwg") - m_Rwg).max()
    print("Rwg of the prior: largest deviation %.3g (the bar %.3g)" % (dev_Rwg, RWG_BAR))
    assert dev_Rwg <= RWG_BAR and np.array_equal(d.get("Rwg"), d.get("Rwg").astype(np.float32).astype(np.float64))
    # the graph, from the scene's own tilted start
    g = mm.Graph(n_kf)
    m_res = mm.graph_init(g, sc["cal"], sc["pose_R"], sc["pose_t"], m_state, sc["jobs"], sc["initial_bias"], sc["Rwg0"], scale)
    d.Rwg.copy_(_up(torch, dev, sc["Rwg0"]))
    d.init(d.Rwg, scale)
    assert np.array_equal(d.res(), m_res)
    for k in ("v", "Rwb", "twb"):
        _same_bits(k, d.get(k), getattr(g, k).reshape(-1))
    _rel("Oc", d.get("Oc"), g.Oc)
    _rel("Pcb", d.get("Pcb"), g.Pcb)
    assert np.array_equal(d.get("shared"), g.shared) and d.get("it")[0] == 0
    d.Oc.copy_(_up(torch, dev, g.Oc.reshape(-1))), d.Pcb.copy_(_up(torch, dev, g.Pcb.reshape(-1)))
    # the information (an existing call), then both modes of the linearisation, twice: the same launch gives the same bytes
    d.information()
    info = fm.edge_information(sc["recs"], sc["edges"])[0]
    _rel("info", d.get("info"), info)
    d.info.copy_(_up(torch, dev, info.reshape(-1)))
    o = mm.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], info, sc["initial_bias"], PG, PA, kind, 0)
    d.linearize(PG, PA, 0)
    _assert_linear(d, o, 0)
    first = {k: d.get(k).tobytes() for k in ("err", "chi2", "chi2_prior", "total", "H", "b", "flt", "work")}
    d.linearize(PG, PA, 0)
    for k, v in first.items():
        assert d.get(k).tobytes() == v, "%s differs between two launches on the same input" % k
    d.err.fill_(NAN), d.chi2.fill_(NAN), d.total.fill_(NAN)
    d.linearize(PG, PA, 1)
    _assert_linear(d, mm.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], info, sc["initial_bias"], PG, PA, kind, 1), 1)
    assert d.get("H").tobytes() == first["H"] and d.get("b").tobytes() == first["b"], "mode 1 neither reads nor writes d_H and d_b"
    # the damped copy and the solve, from the model's system
    lam = 1e3
    d.H.copy_(_up(torch, dev, o["H"].reshape(-1))), d.b.copy_(_up(torch, dev, o["b"])), d.lam.fill_(lam)
    S, rhs, h_max = mm.damp(o["H"], o["b"], lam, n_kf, kind)
    d.damp()
    assert d.res()[mm.R_DONE] == 1
    _same_bits("S", d.get("S"), S.reshape(-1))
    _same_bits("rhs", d.get("rhs"), rhs)
    assert d.get("out")[1] == h_max and np.isnan(d.get("out")[[0, 2]]).all()
    dx, (m_scale, _), m_res = wm.solve(S, rhs, o["b"], lam)
    d.solve()
    assert np.array_equal(d.res(), m_res) and m_res[mm.R_DONE] == 1
    _rel("dx", d.get("dx"), dx)
    _rel("d_out[0]", d.get("out")[0:1], [m_scale])
    # three updates, so that the third normalises the gravity direction
    d.dx.copy_(_up(torch, dev, dx.reshape(-1)))
    for step in range(3):
        m_res = mm.oplus(g, dx.reshape(-1), kind)
        d.oplus()
        assert np.array_equal(d.res(), m_res)
        _rel("v", d.get("v"), g.v)
        _rel("shared", d.get("shared"), g.shared)
        assert d.get("it")[0] == g.iter == (step + 1) % 3
        d.put_graph(g)
    # the recovery, from the model's vertices
    m_bias, m_summary, m_res = mm.recover(g, sc["jobs"], m_state, m_priors)
    d.recover()
    assert np.array_equal(d.res(), m_res) and m_res[mm.R_DONE] == n_kf
    _same_bits("state", d.get("state", (-1, 15)), m_state)
    assert d.priors_np().tobytes() == m_priors.tobytes()
    _same_bits("bias", d.get("bias", (n_kf, 6)), m_bias)
    _same_bits("summary", d.get("summary"), m_summary)
    d.finish()


def test_the_limit_of_157_key_frames():
    """N = 480, the limit: the linearisation, the damped copy and one solve"""
    import torch
    dev = torch.device("cuda:0")
    n_kf, kind = mm.MAX_KF, mm.KIND_GS
    sc = _limit_scene()
    d = _Init(torch, dev, sc, kind)
    d.put_graph(sc["graph"])
    for k in ("Rwb", "twb", "Oc", "Pcb"):
        getattr(d, k).copy_(_up(torch, dev, getattr(sc["graph"], k).reshape(-1)))
    info = fm.edge_information(sc["recs"], sc["edges"])[0]
    d.info.copy_(_up(torch, dev, info.reshape(-1)))
    o = mm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], info, sc["initial_bias"], PG, PA, kind, 0)
    d.linearize(PG, PA, 0)
    _assert_linear(d, o, 0)
    assert d.N == 480
    lam = 1e3
    d.H.copy_(_up(torch, dev, o["H"].reshape(-1))), d.b.copy_(_up(torch, dev, o["b"])), d.lam.fill_(lam)
    S, rhs, h_max = mm.damp(o["H"], o["b"], lam, n_kf, kind)
    d.damp()
    _same_bits("S", d.get("S"), S.reshape(-1))
    assert d.get("out")[1] == h_max
    dx, (m_scale, _), m_res = wm.solve(S, rhs, o["b"], lam)
    d.solve()
    assert np.array_equal(d.res(), m_res) and m_res[mm.R_DONE] == 1
    _rel("dx", d.get("dx"), dx)
    d.finish()


_cache = {}


def _limit_scene():
    if "limit" not in _cache:
        _cache["limit"] = mm.make_scene(mm.MAX_KF, seed=5, sample_counts=(2, 3, 8), tilt=0.1, scale=1.05)
    return _cache["limit"]


def test_distrusted_jobs_are_dropped_and_counted():
    """an out-of-range pose row and prior slot (job 2), a duplicated state row (job 3 names job 1's) and a record of -1 on a key frame that
    is not the last (job 4): each is dropped and counted, the chain closes over the jobs kept, and nothing is written outside the outputs
    of those -- the whole tables are compared"""
    import torch
    dev = torch.device("cuda:0")
    n_kf, kind = 6, mm.KIND_GS
    sc = mm.make_scene(n_kf, seed=31, tilt=0.1, scale=1.05)
    jobs = sc["jobs"].copy()
    jobs[2, 0], jobs[2, 3] = n_kf + 5, -5
    jobs[3, 1] = jobs[1, 1]
    jobs[4, 2] = -1
    d = _Init(torch, dev, sc, kind, jobs=jobs)
    m_state, m_priors = d.state_table(sc["state"]), d.prior_table()
    m_Rwg, m_res = mm.prior(sc["pose_R"], sc["pose_t"], m_state, sc["recs"], m_priors, jobs)
    assert list(m_res[:4]) == [3, 2, 1, 0]
    d.prior()
    assert np.array_equal(d.res(), m_res)
    _same_bits("state", d.get("state", (-1, 15)), m_state)
    assert d.priors_np().tobytes() == m_priors.tobytes()
    assert np.abs(d.get("Rwg") - m_Rwg).max() <= RWG_BAR
    g = mm.Graph(n_kf)
    m_res = mm.graph_init(g, sc["cal"], sc["pose_R"], sc["pose_t"], m_state, jobs, sc["initial_bias"], None, 1.0)
    assert list(m_res[:2]) == [5, 1]
    d.init(None, 1.0)
    assert np.array_equal(d.res(), m_res)
    for k in ("v", "Rwb", "twb"):
        _same_bits(k, d.get(k), getattr(g, k).reshape(-1))
    _rel("Oc", d.get("Oc"), g.Oc)
    assert np.array_equal(d.get("shared"), g.shared)
    # an edge whose record is out of range and one whose information was refused take no part
    edges = sc["edges"].copy()
    edges["rec"][1] = len(sc["recs"]) + 3
    d.edges.copy_(_up(torch, dev, edges))
    info = fm.edge_information(sc["recs"], sc["edges"])[0]
    info[3] = 0.0
    d.info.copy_(_up(torch, dev, info.reshape(-1)))
    g.v[:] = np.random.RandomState(1).normal(0, 0.5, g.v.shape)
    d.put_graph(g)
    d.Oc.copy_(_up(torch, dev, g.Oc.reshape(-1))), d.Pcb.copy_(_up(torch, dev, g.Pcb.reshape(-1)))
    o = mm.linearize(g, sc["recs"], sc["cal"]["gravity"], edges, info, sc["initial_bias"], PG, PA, kind, 0)
    assert list(o["result"][:4]) == [3, 1, 0, 1]
    d.linearize(PG, PA, 0)
    _assert_linear(d, o, 0)
    assert not d.get("err", (-1, 9))[[1, 3]].any() and not d.get("chi2")[[1, 3]].any()
    m_bias, m_summary, m_res = mm.recover(g, jobs, m_state, m_priors)
    assert list(m_res[:3]) == [4, 1, 1]
    d.recover()
    assert np.array_equal(d.res(), m_res)
    _same_bits("state", d.get("state", (-1, 15)), m_state)
    assert d.priors_np().tobytes() == m_priors.tobytes()
    _same_bits("bias", d.get("bias", (n_kf, 6)), m_bias)
    d.finish()


def test_gravity_already_along_minus_z_is_the_identity_and_counted():
    """|v| == 0: the reference divides by zero; the device gives Rwg = I, counts ORBI_R_REFUSED and writes the velocities all the same"""
    import torch
    dev = torch.device("cuda:0")
    sc = mm.make_scene(3, seed=2)
    state = sc["state"].copy()
    state[:, :9] = np.eye(3, dtype=np.float32).reshape(9)
    for r in sc["recs"]:                                                  # Rwb * dVu = (0, 0, z): the direction is +-z exactly
        r.dV[:2], r.JVg[:2], r.JVa[:2] = 0, 0, 0
    d = _Init(torch, dev, sc, mm.KIND_GS, state=state)
    m_state, m_priors = d.state_table(state), d.prior_table()
    m_Rwg, m_res = mm.prior(sc["pose_R"], sc["pose_t"], m_state, sc["recs"], m_priors, sc["jobs"])
    assert m_res[mm.R_REFUSED] == 1 and m_res[mm.R_DONE] == 3
    d.prior()
    assert np.array_equal(d.res(), m_res) and np.array_equal(d.get("Rwg"), np.eye(3).reshape(9))
    _same_bits("state", d.get("state", (-1, 15)), m_state)
    d.finish()


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_one_trial_is_a_chain_on_one_stream_with_one_wait(stream_kind):
    """damp -> the ordered Cholesky -> push -> oplus -> linearize mode 1, enqueued without a wait, then ONE read-back; a rejected trial's
    pop restores v, shared and iter byte for byte"""
    import torch
    dev = torch.device("cuda:0")
    name = "5 GS"
    n_kf, kind, pg, pa, lam = mm.LOOPS[name]
    sc = mm.loop_scene(name)
    be = mm.loop_backend(name)
    be.linearize()
    ok, m_scale, m_res, g1 = be.trial_outputs(lam)
    m_total = be._lin(g1, 1)["total"][0]
    d = _Init(torch, dev, sc, kind)
    st = il._chain_stream(torch, dev, stream_kind)
    d.Rwg.copy_(_up(torch, dev, sc["Rwg0"]))
    d.init(d.Rwg, sc["graph"].scale, st)
    d.information(st)
    d.linearize(pg, pa, 0, st)
    d.lam.fill_(lam)
    d.damp(st)
    d.solve(st)
    res = d.result.clone()
    d.push()
    d.oplus(st)
    d.linearize(pg, pa, 1, st)
    s = torch.cat([d.total, d.out[0:1]]).cpu().numpy()                   # the one wait
    assert ok and np.array_equal(res.cpu().numpy(), m_res)
    _rel("trial total", s[0:1], [m_total])
    _rel("trial d_out[0]", s[1:2], [m_scale])
    _rel("trial v", d.get("v"), g1.v)
    _rel("trial shared", d.get("shared"), g1.shared)
    assert d.get("it")[0] == g1.iter == 1
    d.pop()
    est = d.estimate()
    assert est["v"].tobytes() == sc["graph"].v.tobytes() and est["shared"].tobytes() == sc["graph"].shared.tobytes() and est["iter"][0] == 0
    d.finish()


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------------
class DeviceInit:
    """tests/inertial_loop.py's back-end interface over the chain of include/orbii.h on the device, per trial
      *d_lambda <- lam; orbii_damp_device; the ordered Cholesky; push; orbii_oplus_device; orbii_linearize_device (mode 1)
    and ONE read-back: the total, d_out[0] and the solve's d_result.  With audit=True the estimate is also read back around every trial:
    the model evaluates that one trial from the device's estimate with the same lambda, and a pop is held to the bytes before the push."""

    def __init__(self, torch, dev, sc, kind, pg, pa, Rwg, scale, stream_kind="explicit", audit=False, bar=BAR, d=None, st=None):
        self.torch, self.sc, self.kind, self.pg, self.pa, self.audit, self.bar = torch, sc, kind, pg, pa, audit, bar
        self.d = d or _Init(torch, dev, sc, kind)
        self.st = st or il._chain_stream(torch, dev, stream_kind)       # torch's current stream too: the fills, copies and read-backs follow it
        self.refused = self.n_trials = 0
        if Rwg is not None:
            self.d.Rwg.copy_(_up(torch, dev, Rwg))
        self.d.init(self.d.Rwg, scale, self.st)
        self.d.information(self.st)

    def linearize(self):
        self.d.linearize(self.pg, self.pa, 0, self.st)
        return float(self.d.total.cpu().numpy()[0])

    def largest_diagonal(self):
        self.d.lam.fill_(0.0)
        self.d.damp(self.st)
        return float(self.d.out[1:2].cpu().numpy()[0])

    def _model_trial(self, before, lam):
        g = self.sc["graph"].copy()
        g.v, g.shared, g.iter = before["v"].copy(), before["shared"].copy(), int(before["iter"][0])
        be = mm.ModelInit(self.sc, self.kind, self.pg, self.pa, graph=g)
        be.linearize()
        ok, scale, res, g1 = be.trial_outputs(lam)
        return ok, scale, res, g1, float(be._lin(g1, 1)["total"][0])

    def trial(self, lam):
        d, st, torch = self.d, self.st, self.torch
        if self.audit:
            self.before = d.estimate()
        d.lam.fill_(lam)
        d.damp(st)
        d.solve(st)
        res = d.result.clone()
        d.push()
        d.oplus(st)
        d.linearize(self.pg, self.pa, 1, st)
        s = torch.cat([d.total, d.out[0:1]]).cpu().numpy()               # the two scalars
        res = res.cpu().numpy()
        ok = bool(res[mm.R_DONE] == 1 and res[mm.R_REFUSED] == 0)
        self.n_trials, self.refused, self.t = self.n_trials + 1, self.refused + (not ok), float(s[0])
        if self.audit:                                                   # EVERY trial: the four outputs the policy reads
            m_ok, m_scale, m_res, g1, m_total = self._model_trial(self.before, lam)
            what = "trial %d " % (self.n_trials - 1)
            assert ok == m_ok and np.array_equal(res, m_res), what
            _rel(what + "total", s[0:1], [m_total], self.bar)
            assert abs(s[1] - m_scale) <= self.bar * (abs(m_scale) + 1e-3), what     # relative to computeScale + 1e-3, what the policy divides by
            est = d.estimate()
            _rel(what + "v", est["v"], g1.v, self.bar)
            _rel(what + "shared", est["shared"], g1.shared, self.bar)
            assert est["iter"][0] == g1.iter
        return ok, float(s[1]), 0.0

    def totals(self):
        return self.t, 0.0

    def accept(self):
        pass                                                             # the graph was updated in place

    def reject(self):
        self.d.pop()
        if self.audit:
            after = self.d.estimate()
            for k in after:
                assert after[k].tobytes() == self.before[k].tobytes(), "trial %d was rejected and %s does not hold the bytes it held before it" % (self.n_trials - 1, k)

    def estimate(self):
        return self.d.estimate()


@pytest.mark.parametrize("name", list(mm.LOOPS))
def test_the_closed_loop_on_the_device(name):
    """inertial_loop.optimize over the device back-end, every trial audited against the model's evaluation of that one trial at 4 x the
    recorded spread of the final total (never below 1e-9); the final estimate against the unperturbed model loop at 4 x the recorded
    spread per output; the total non-increasing over accepted trials; iter = accepted updates mod 3.  Decisions are NOT compared
    (tests/test_imu_init_cpu.py says why)."""
    import torch
    from test_imu_init_cpu import MEASURED_SPREAD, final_total, model_run, split
    dev = torch.device("cuda:0")
    n_kf, kind, pg, pa, lam0 = mm.LOOPS[name]
    sc = mm.loop_scene(name)
    spread = MEASURED_SPREAD[name]
    be = DeviceInit(torch, dev, sc, kind, pg, pa, sc["Rwg0"], sc["graph"].scale, audit=True, bar=max(BAR, 4 * spread["total"]))
    r = il.optimize(be, mm.LOOP_ITERATIONS, user_lambda_init=lam0)
    ref = model_run(name)
    tr = r["trace"]
    print("%s: device %s, model %s" % (name, il.decisions([r])[0], il.decisions([ref])[0]))
    assert be.n_trials == len(tr) and be.refused == 0 and r["accepted"] >= 3
    if pg == 0:
        assert tr[0][2] == il.TAU * float(be.d.out[1:2].cpu().numpy()[0]) > 0       # the default lambda init, from d_out[1]
    accepted = [t[4] for t in tr if t[-1]]
    assert all(b <= a for a, b in zip([tr[0][3]] + accepted, accepted))
    est = be.estimate()
    assert est["iter"][0] == r["accepted"] % 3
    got, want = split(est), split(ref["estimate"])
    for o in ("v", "bg", "ba", "Rwg", "scale"):
        _rel("final " + o, got[o], want[o], max(BAR, 4 * spread[o]))
    assert abs(final_total(r) - final_total(ref)) <= max(BAR, 4 * spread["total"]) * final_total(ref)
    be.d.finish()


# ---- the whole step on a small device-resident map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [65, 1025])
def test_the_whole_step_on_a_device_resident_map(n_points):
    """prior -> init -> information -> the caller's loop -> recover -> orbi_set_bias_device -> orbi_prior_information_device -> the rescale ->
    rebuild + refresh over all rows, on one stream with one wait at the end besides the loop's scalars.  Held to the models applied to the
    device's own estimate: every state row, prior slot, bias and record, d_pose_R / d_pose_t and every point row bit for bit from the same
    d_summary, the refreshed normals and distance ranges.  A second rescale with a d_summary whose scale is 0.05 leaves every table as it
    is and counts the refusal."""
    import torch
    import observations_model as om
    import refresh_model as rm
    from monoorbslam3_amd import imu, matcher
    dev = torch.device("cuda:0")
    n_kf, kind = 6, mm.KIND_GS
    sc = mm.make_scene(n_kf, seed=3, sample_counts=(100,))               # a scene whose model loop ends above min_scale (asserted below)
    mp = mm.make_map(sc, n_points)
    cap, stride = mp["cap_points"], mp["stride"]
    cap_obs = int((mp["slots"] >= 0).sum()) + 40
    d = _Init(torch, dev, sc, kind)
    st = il._chain_stream(torch, dev, "explicit")
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    res = {k: torch.full((8,), 77, dtype=torch.int32, device=dev) for k in ("set_bias", "prior", "rescale", "build", "refresh", "again")}
    t = dict(n=_up(torch, dev, mp["n"]), bad=_up(torch, dev, mp["bad"]), slots=_up(torch, dev, mp["slots"]), valid=_up(torch, dev, mp["valid"]),
             points=_up(torch, dev, mp["points"]), ref_kf=_up(torch, dev, mp["ref_kf"]), kf_imu=_up(torch, dev, mp["kf_imu"]), n_points=_up(torch, dev, mp["n_points"]),
             obs_off=z(cap + 1, torch.int32), obs_kf=z(cap_obs, torch.int32), obs_kp=z(cap_obs, torch.int32), sel=_up(torch, dev, np.arange(cap, dtype=np.int32)),
             pose_R=d.pose_R, pose_t=d.pose_t, state=d.state, priors=d.priors, summary=d.summary, **{k: _up(torch, dev, v) for k, v in mp["table"].items()})
    kps, desc = [_up(torch, dev, k) for k in mp["kps"]], [_up(torch, dev, k) for k in mp["kf_desc"]]
    kft = matcher.KfTable.make(d.pose_R[:9 * n_kf], d.pose_t[:3 * n_kf], t["bad"], kps, desc, t["n"])
    m = matcher.ORBMatcher()
    # ---- the chain
    d.prior(st)
    be = DeviceInit(torch, dev, sc, kind, PG, PA, None, 1.0, d=d, st=st)  # the graph from the prior's d_Rwg, which stays on the device
    r = il.optimize(be, mm.LOOP_ITERATIONS, user_lambda_init=1e3)
    d.recover(st)
    ids = _up(torch, dev, np.arange(n_kf, dtype=np.int32))
    imu.set_bias_device(d.cal, d.bank, d.pool, d.cap, d.cap_meas, ids, d.bias, n_kf, res["set_bias"], stream=st)
    pjobs = np.array([[k, k - 1, -1] for k in range(1, n_kf)], np.int32)
    imu.prior_information_device(d.priors, d.n_priors, d.bank, d.cap, _up(torch, dev, pjobs), n_kf - 1, res["prior"], stream=st)
    m.ApplyScaleRotationDevice(d.cal, dict(t, result=res["rescale"]), n_kf, d.n_src, d.n_priors, cap, True, stream=st)
    m.BuildObservationsDevice(dict(t, result=res["build"]), n_kf, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft, dict(t, result=res["refresh"]), cap, cap, cap_obs, float(rm.MAX_SCALE_FACTOR), stream=st)
    torch.cuda.synchronize()                                             # the one wait behind the loop
    g = lambda x: x.cpu().numpy().copy()  # noqa: E731
    held = {k: g(v) for k, v in t.items()}
    held.update(bank=g(d.bank), pool=g(d.pool), bias=g(d.bias), Rwg=g(d.Rwg), **{"result " + k: g(v) for k, v in res.items()})
    est = d.estimate()
    assert r["accepted"] >= 3 and be.refused == 0
    # ---- the models: the prior, then the tail on the device's own estimate
    m_state, m_priors = d.state_table(sc["state"]), d.prior_table()
    m_Rwg, _ = mm.prior(sc["pose_R"], sc["pose_t"], m_state, sc["recs"], m_priors, sc["jobs"])
    assert np.abs(held["Rwg"] - m_Rwg).max() <= RWG_BAR
    graph = mm.Graph(n_kf)
    mm.graph_init(graph, sc["cal"], sc["pose_R"], sc["pose_t"], m_state, sc["jobs"], sc["initial_bias"], held["Rwg"], 1.0)
    ref = mm.ModelInit(sc, kind, PG, PA, graph=graph)
    ref_run = il.optimize(ref, mm.LOOP_ITERATIONS, user_lambda_init=1e3)
    assert ref_run["accepted"] >= 3 and ref.refused == 0 and ref.g.scale >= 0.1 and abs(est["shared"][15] - ref.g.scale) < 1e-3
    graph.v, graph.shared, graph.iter = est["v"].copy(), est["shared"].copy(), int(est["iter"][0])
    m_bias, m_summary, _ = mm.recover(graph, sc["jobs"], m_state, m_priors)
    bank = im.Bank(len(sc["recs"]), max(max(len(x.meas) for x in sc["recs"]), 1))
    bank.recs = [x.copy() for x in sc["recs"]]
    bres = im.run_set_bias(sc["cal"], bank, np.arange(n_kf), m_bias)
    pres, _ = fm.prior_information(m_priors, bank.recs, None, pjobs)
    assert bres[0] == n_kf and pres[fm.R_DONE] == n_kf - 1
    assert held["result set_bias"].tobytes() == np.asarray(bres, np.int32).tobytes() and held["result prior"].tobytes() == np.asarray(pres, np.int32).tobytes()
    pose_R = np.concatenate([sc["pose_R"], np.full((2, 9), NAN)])
    pose_t = np.concatenate([sc["pose_t"], np.full((2, 3), NAN)])
    points = mp["points"].copy()
    rres = mm.apply_scale_rotation(sc["cal"], pose_R[:n_kf], pose_t[:n_kf], mp["bad"], mp["kf_imu"], m_state, m_priors, points, mp["valid"], cap, m_summary, True)
    assert list(rres[:5]) == [n_kf, 0, 0, 0, n_points] and np.array_equal(held["result rescale"], rres)
    _same_bits("summary", held["summary"], m_summary)
    _same_bits("bias", held["bias"].reshape(n_kf, 6), m_bias)
    _same_bits("state", held["state"].reshape(-1, 15), m_state)
    assert np.frombuffer(held["priors"].tobytes(), fm.PRIOR).tobytes() == m_priors.tobytes()
    b_bytes, p_bytes = bank.pack()
    assert held["bank"].tobytes() == b_bytes.tobytes() and held["pool"].tobytes() == p_bytes.tobytes()
    assert held["pose_R"].tobytes() == pose_R.reshape(-1).tobytes() and held["pose_t"].tobytes() == pose_t.reshape(-1).tobytes()
    _same_bits("points", held["points"].reshape(-1, 3), points)
    assert (points[mp["valid"] != 0] != mp["points"][mp["valid"] != 0]).any() and (m_state[:n_kf] != sc["state"]).any()
    off, okf, okp, ores = om.build(mp["n"], mp["bad"], mp["slots"], stride, mp["valid"], cap, 1 << 30)
    assert held["obs_off"].tobytes() == off.tobytes() and held["obs_kf"][:len(okf)].tobytes() == okf.tobytes() and held["result build"].tobytes() == ores.tobytes()
    rs = dict(n=mp["n"], bad=mp["bad"], pose_R=pose_R[:n_kf], pose_t=pose_t[:n_kf], kps=mp["kps"], kf_desc=mp["kf_desc"], points=points, valid=mp["valid"],
              obs_off=off, obs_kf=okf, obs_kp=okp, ref_kf=mp["ref_kf"], **mp["table"])
    fresh = rm.refresh(rs, np.arange(cap), cap)
    assert np.array_equal(held["result refresh"], fresh["result"]) and fresh["result"][0] == n_points
    assert np.array_equal(held["normals"].reshape(-1, 3), fresh["normals"])           # by value: -0 equals +0
    for k in ("min_dist", "max_dist"):
        assert held[k].view(np.uint32).tobytes() == fresh[k].view(np.uint32).tobytes(), k
    # ---- a scale below min_scale: nothing but d_result is written
    small = m_summary.copy()
    small[9] = 0.05
    d.summary.copy_(_up(torch, dev, small))
    m.ApplyScaleRotationDevice(d.cal, dict(t, result=res["again"]), n_kf, d.n_src, d.n_priors, cap, True)
    torch.cuda.synchronize()
    assert list(g(res["again"])) == [0, 0, 0, 1, 0, 0, 0, 0]
    for k in ("pose_R", "pose_t", "state", "priors", "points"):
        assert g(t[k]).tobytes() == held[k].tobytes(), k
    d.finish()
