"""fullInertialOptimize's Levenberg-Marquardt loop, closed: TEST CODE ONLY.  include/orbfi.h ships the stages of one iteration and leaves
the loop to the caller; tests/inertial_loop.py has the policy (g2o's, as oracle/ba_ref.py restates it) and the shape of a back-end; this
file adds the pair of back-ends of this graph shape, model and device, the driver that follows Optimize.cpp:250 and :397-398, and the
scenes a loop can be judged on.  Both branches: beInit (one bias pair in a carrier state, orbfi_linearize_device) and !beInit (a bias
pair per key frame with walks and no priors: existing calls only, orbi_linearize_device with Huber 4.1134)."""
import numpy as np

import factors_model as fm
import full_inertial_model as fim
import inertial_loop as il
import vw_model as wm


def full_inertial(be, iterations=fim.ITERATIONS):
    """Optimize::fullInertialOptimize (Optimize.cpp:239-442): the user lambda init 1e-5 (:250), optimize(iteration) (:397-398); nothing is
    classified"""
    return [il.optimize(be, iterations, user_lambda_init=fim.USER_LAMBDA_INIT)]


# ---- the model back-end ---------------------------------------------------------------------------------------------------------------------------
class ModelFull(il.ModelWindow):
    """the chain of include/orbfi.h in numpy: inertial_loop.ModelWindow with this graph's inertial side and its three entries per edge"""

    def linearize(self):
        self.oi = fim.inertial_linearize(self.sc, self.g)
        self.ov = self._vis(self.g, self.P, 0, H_diag=self.oi["H_diag"], b=self.oi["b"])
        return self.oi["total"][1] + self.ov["total"][1]

    def _reduce(self, lam):
        sc, g, oi, ov = self.sc, self.g, self.oi, self.ov
        edges, H_off = fim.reduce_edges(sc, oi)
        return wm.reduce(sc["n_solve"], g.fixed, edges, len(sc["recs"]), ov["H_diag"], H_off, ov["b"], lam, ov["point_off"], sc["edge_state"], ov["Hll"], ov["bl"],
                         ov["Hlp"], len(sc["w"]))

    def trial(self, lam):
        sc, g, ov, noise = self.sc, self.g, self.ov, self.noise
        ns, ne = sc["n_solve"], len(sc["w"])
        rd = self._reduce(lam)
        dx, (scale, _), res = wm.solve(rd["S"], rd["rhs"], ov["b"][:ns], lam)
        dx = noise(dx)
        bs = wm.backsub(ns, ov["point_off"], sc["edge_state"], ov["Hlp"], rd["Hll_inv"], ov["bl"], dx, lam, self.P, ne)
        g1 = g.copy()
        fm.oplus(g1, dx)
        il._noisy_graph(noise, g1, g)
        P1 = noise(bs["points_out"])
        ok = bool(res[wm.R_DONE] == 1)
        self.refused += not ok
        self.t = dict(g=g1, P=P1, dx=dx, ok=ok, totals=(float(noise(fim.inertial_linearize(sc, g1, 1)["total"][1])), float(noise(self._vis(g1, P1, 1)["total"][1]))))
        return ok, float(noise(scale)), float(noise(bs["scale"]))


# ---- the device back-end ----------------------------------------------------------------------------------------------------------------------------
class DeviceFull(il._Device):
    """the chain of include/orbfi.h on the device, per trial
      *d_lambda <- lam; orbvw_reduce_device (d_off_edges, d_H_off); orbvw_solve_device; orbvw_backsub_device (live points -> the other buffer);
      push; orbi_graph_oplus_device; orbfi_linearize_device (mode 1); orbvw_linearize_device (mode 1, on the other buffer)
    and ONE read-back: the two robustified totals, d_out[0], d_out_points[0] and the solve's d_result.  With the scene's per_state the
    inertial side is orbi_linearize_device and the reduce takes its edges: the !beInit branch."""

    def __init__(self, torch, dev, sc, stream_kind="explicit", audit=False):
        from monoorbslam3_amd import imu, vw
        from test_full_inertial_gpu import _Fi
        self.torch, self.sc, self.imu, self.vw, self.per_state = torch, sc, imu, vw, sc["per_state"]
        self.f = f = _Fi(torch, dev, sc)
        self.w = f.w
        if self.per_state:
            f.w.edges, f.w.n_iedges = f.i.edges, f.i.ne
        self._init_state(f.i, audit)
        self.kf_bias_zero = []
        self.pts, self.cur = [f.w.points, f.w.points_out], 0
        self.st = il._chain_stream(torch, dev, stream_kind)
        imu.edge_information_device(f.i.bank, f.i.cap, f.i.edges, f.i.ne, f.i.info, f.i.walk, f.i.result, stream=self.st)

    def _inertial(self, mode):
        if self.per_state:
            self.f.i.linearize(self.sc, fim.HUBER_DELTA, mode, stream=self.st)
        else:
            self.f.linearize(mode, self.st)

    def linearize(self):
        i, w = self.d, self.w
        self._inertial(0)
        w.linearize(0, points=self.pts[self.cur], H_diag=i.H_diag, b=i.b, stream=self.st)
        t = self.torch.cat([i.total[1:2], w.total[1:2]]).cpu().numpy()
        return t[0] + t[1]

    def trial(self, lam):
        i, w, st, torch = self.d, self.w, self.st, self.torch
        a, b = self.pts[self.cur], self.pts[1 - self.cur]
        w.lam.fill_(lam)
        w.reduce(H_diag=i.H_diag, H_off=i.H_off if self.per_state else self.f.H_off, b=i.b, stream=st)
        w.solve(b=i.b, stream=st)
        res = w.result.clone()
        self.vw.backsub_device(w.ns, w.np_, w.ne, w.point_off, w.edge_state, w.Hlp, w.Hll_inv, w.bl, w.dx, w.lam, a, w.xl, b, w.out_points, w.result, stream=st)
        self._push()
        self.imu.graph_oplus_device(i.graph, w.dx, i.it, i.result, stream=st)
        self._inertial(1)
        w.linearize(1, points=b, stream=st)
        s = torch.cat([i.total[1:2], w.total[1:2], w.out[0:1], w.out_points[0:1]]).cpu().numpy()       # the four scalars
        res = res.cpu().numpy()
        ok = bool(res[wm.R_DONE] == 1 and res[wm.R_REFUSED] == 0)
        assert ok or res[wm.R_REFUSED] == 1, res
        self.n_trials, self.refused, self.t = self.n_trials + 1, self.refused + (not ok), (float(s[0]), float(s[1]))
        if self.audit:
            self.dx_zero.append(not w.get("dx").any())
            n_kf = self.sc["n_kf"]                                   # the key frames have no bias vertices: their bg, ba stay zero at every trial
            self.kf_bias_zero.append(self.per_state or not (i.bg[:3 * n_kf].any().item() or i.ba[:3 * n_kf].any().item()))
        return ok, float(s[2]), float(s[3])

    def accept(self):
        self.cur = 1 - self.cur

    def estimate(self):
        return dict(self._graph_arrays(), points=self.pts[self.cur].cpu().numpy().reshape(-1, 3).copy())

    def finish(self):
        self.f.finish()


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (how the scene is built, the driver's keywords).  The keywords of inertial_loop.LOOP_WINDOW: 100-sample records, depths of 2 to
# 6 m, every point seen by at least 3 states; the records as inertialOptimize leaves them (one bias for all: the state this optimiser
# starts from) and measurements with a fifth or a twentieth of the stage scenes' pixel noise.  With lambda starting at 1e-5 against an
# inertial information of 1e14 the route of a noisier scene is chaotic: a 1e-9 stage error changes a decision within some fifty trials,
# and such a scene cannot carry a comparison.  Both branches, with and without key frame 0 fixed, fewer and more points than a
# wave, loops that end through max_trials and one that uses all 100 iterations.  Of the seeds 1 to 13 only 1 gives every point three
# observers among 4 key frames with no fixed one beside them, 1 and 11 among 3, none among 5.  The per-state scene has the lower pixel
# noise: at 0.2 its loop walks 100 iterations along a valley of the points and the model's own spread of the final points is 98% of the
# largest coordinate, a comparison that cannot fail; at 0.05 that spread is 1e-7.
SCENES = {
    "full 4 63": (dict(n_kf=4, n_points=63, seed=1, pixel_noise=0.05), dict(iterations=100)),
    "full 3 65 free": (dict(n_kf=3, n_points=65, seed=1, fix_first=False, pixel_noise=0.2), dict(iterations=100)),
    "per-state 3 63": (dict(n_kf=3, n_points=63, seed=1, per_state=True, pixel_noise=0.05), dict(iterations=100)),
}
# the scenes of the whole step on a device-resident map (chain_map below): name -> (map points, the driver's keywords).  Six key frames and
# 65 or 1025 points, the sizes of the whole-step test of tests/test_imu_init_gpu.py; a few iterations; every point seen by at least 2
# states (among six key frames no seed gives every point three observers)
CHAIN_KF = 6
CHAIN_SCENES = {
    "chain 6 65": (65, dict(iterations=4)),
    "chain 6 1025": (1025, dict(iterations=4)),
}
# the scenes that reach their minimum: behind inertial_loop.flat_from() their sequence is rounding and only the estimate is compared
CONVERGED = ("full 3 65 free", "per-state 3 63")
_scenes, _runs, _maps = {}, {}, {}


def scene(name):
    if name in CHAIN_SCENES:
        return chain_map(name)["fs"]
    if name not in _scenes:
        how = dict(SCENES[name][0])
        kw = {k: v for k, v in il.LOOP_WINDOW.items() if k != "fixed_offset"}
        _scenes[name] = fim.scene(how.pop("n_kf"), how.pop("n_points"), common_bias=True, **dict(kw, **how))
    return _scenes[name]


def model_backend(name, noise=None):
    return ModelFull(scene(name), noise)


def device_backend(torch, dev, name, stream_kind="explicit", audit=False):
    return DeviceFull(torch, dev, scene(name), stream_kind, audit)


def run(name, be):
    return dict(rounds=full_inertial(be, **dict(SCENES, **CHAIN_SCENES)[name][1]), estimate=be.estimate(), refused=be.refused)


def model_run(name):
    """the unperturbed model loop of a scene, computed once and shared: nobody changes it"""
    if name not in _runs:
        _runs[name] = run(name, model_backend(name))
    return _runs[name]


# ---- the whole step on a map ----------------------------------------------------------------------------------------------------------------------------
def chain_map(name):
    """a CHAIN_SCENES scene laid out as a map (inertial_window_model.map_from_window_scene: shuffled key-frame slots, table rows, state rows,
    records and prior slots; two more key frames in the table that see nothing and are in no window), computed once and shared:
      map, csr   what the assembly reads            a     the model assembly with all six key frames as its window, oldest first
      jobs       full_inertial_model.jobs on it     fs    the shared-bias scene that assembly and those jobs describe, for the model loop
    The jobs' vertices ARE the scene's: orbi_graph_init_device's model on the map's state rows and d_init_out gives fs's graph bit for bit."""
    if name not in _maps:
        import inertial_window_model as iw
        import local_ba_model as lm
        n_points = CHAIN_SCENES[name][0]
        ws = wm.window_scene(CHAIN_KF, 0, n_points, seed=1, sample_counts=(100,) * (CHAIN_KF - 1), depth=il.LOOP_WINDOW["depth"], min_obs=2, pixel_noise=0.05)
        mp = iw.map_from_window_scene(fim.with_common_bias(ws))
        csr = lm.fresh_csr(mp)
        a = iw.problem(mp, csr)
        iw.reproduces(mp, a)
        edges = np.zeros(CHAIN_KF - 1, fm.EDGE)
        for c, key in enumerate(("i", "j", "rec", "flags")):
            edges[key] = a["inertial_edges"][:, c]
        jobs = fim.jobs(a["init_jobs"], edges, a["recover_jobs"], CHAIN_KF, True, mp["n_src"], mp["cap_bank"])
        fs = fim.of_window_scene(iw.window_scene_of(mp, a))
        assert jobs["result"].tolist() == [CHAIN_KF + 1, 0, 0, 0, 0, 0, 0, 0] and jobs["prior_rec"] == fs["prior_rec"] == mp["kf_imu"][mp["window"][-1], 1]
        assert jobs["edges"].tobytes() == fs["edges"].tobytes() and jobs["fixed"].tobytes() == fs["graph"].fixed.tobytes()
        g = fm.Graph(CHAIN_KF + 1)
        assert fm.graph_init(g, fs["recs"], mp["src"], jobs["init"])[fim.R_DONE] == CHAIN_KF + 1
        for k in il.STATE:
            assert getattr(g, k).tobytes() == getattr(fs["graph"], k).tobytes(), k
        _maps[name] = dict(map=mp, csr=csr, a=a, jobs=jobs, fs=fs)
    return _maps[name]


def chain_tail(cm, est, recs):
    """everything behind the loop (include/orbfi.h, "The chain") in the models, applied to an estimate `est` (the dict a back-end's
    estimate() gives; the device's own): inertial_window_model.tail with orbfi_recover_device in the place of orbi_graph_recover_device and
    nothing classified.  recs: the records (changed in place by set_bias).  -> dict of every array the tail writes"""
    import imu_model as im
    import inertial_window_model as iw
    import local_ba_model as lm
    mp, csr, a, fs = cm["map"], cm["csr"], cm["a"], cm["fs"]
    g = fs["graph"].copy()
    for k in il.STATE:
        setattr(g, k, np.array(est[k], np.float64))
    src = mp["src"].copy()
    bias, pose_R, pose_t, rres = fim.recover(g, fs["cal"], fs["bias_state"], cm["jobs"]["recover"], src)
    res = a["result"]
    prob = dict(a, pose_kf=a["state_kf"], result=np.array([res[iw.W_STATES], res[iw.W_POINTS], res[iw.W_EDGES], res[iw.W_SOLVE]] + [0] * 12, np.int32))
    applied = lm.apply(mp, csr, prob, pose_R, pose_t, np.asarray(est["points"], np.float64), np.zeros(len(a["edge_state"]), np.uint8))
    bank = im.Bank(len(recs), max(max(len(r.meas) for r in recs), 1))
    bank.recs = recs
    bres = im.run_set_bias(fs["cal"], bank, a["bias_ids"], bias)
    priors = mp["priors"].copy()
    pres, _ = fm.prior_information(priors, bank.recs, src, a["prior_info_jobs"])
    flat, vres = iw.velocity_prior(np.frombuffer(priors.tobytes(), np.float32).reshape(-1, 36), src, a["recover_jobs"], a["prior_jobs"])
    return dict(applied, src=src, bias=bias, est_pose_R=pose_R, est_pose_t=pose_t, bank=bank, priors=np.frombuffer(flat.tobytes(), fm.PRIOR).copy(),
                results=dict(recover=rres, apply=applied["result"], set_bias=bres, prior_information=pres, velocity_prior=vres))
