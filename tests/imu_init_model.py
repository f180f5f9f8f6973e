"""Plain numpy restatement of include/orbii.h (the steps of the IMU initialisation) and of include/orbm.h's section "The map rescaled and
rotated on the device": the prior of LocalMapping::initializeIMU (reference modules/Frontend/LocalMapping.cpp:391-407), the graph of
Optimize::inertialOptimize (modules/Backend/Optimize.cpp:93-205), EdgeInertialGS / EdgeInertialG (G2oTypes.cpp:71-246) with the two
EdgePriori3D, the dense system, its damped copy, the four oplusImpl, the recovery and Map::applyScaleRotation (Map.cpp:96-124).  The
parts the reference computes in float are float32 from imu_model; everything behind the cast is float64 in the orders the header fixes:
no `@`, every sum over k written as elementwise operations in ascending k.  The model back-end of the closed loop (inertial_loop.optimize)
and the seeded scenes live here too.  No part of the library is used here."""
import math

import numpy as np

import factors_model as fm
import imu_model as im

MAX_KF = 157
EDGE_WORK = 240
KIND_GS, KIND_G = 0, 1
SHARED_BG, SHARED_BA, SHARED_RWG, SHARED_SCALE = 0, 3, 6, 15
SUMMARY = 10
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_POINTS = 0, 1, 2, 3, 4
JPG_QUIRK_LINE = 236            # G2oTypes.cpp: EdgeInertialG::linearizeOplus writes -JPg into the accelerometer-bias block of ep
F32, F64 = np.float32, np.float64
I3 = np.eye(3)


def system_size(n_kf):
    return 15 * ((9 + 3 * n_kf + 14) // 15)


def dof_free(n_kf, kind):
    """bool [N]: the dof that are vertices' (the rest are identity rows and columns)"""
    free = np.arange(system_size(n_kf)) < 9 + 3 * n_kf
    if kind == KIND_G:
        free[8] = False
    return free


class Graph:
    def __init__(self, n):
        self.n = n
        self.v = np.zeros((n, 3))
        self.shared = np.zeros(16)
        self.shared[SHARED_RWG:SHARED_RWG + 9] = I3.reshape(9)
        self.shared[SHARED_SCALE] = 1.0
        self.iter = 0
        self.Rwb = np.tile(I3, (n, 1, 1))
        self.twb, self.Oc, self.Pcb = (np.zeros((n, 3)) for _ in range(3))

    def copy(self):
        o = Graph(self.n)
        for k in ("v", "shared", "Rwb", "twb", "Oc", "Pcb"):
            setattr(o, k, getattr(self, k).copy())
        o.iter = self.iter
        return o

    bg = property(lambda self: self.shared[0:3])
    ba = property(lambda self: self.shared[3:6])
    Rwg = property(lambda self: self.shared[6:15].reshape(3, 3))
    scale = property(lambda self: self.shared[15])


def _pose_f32(pose_R, pose_t, row):
    return np.asarray(pose_R[row], F64).astype(F32).reshape(3, 3), np.asarray(pose_t[row], F64).astype(F32)


# ---- the prior ---------------------------------------------------------------------------------------------------------------------------
def prior(pose_R, pose_t, state, recs, priors, jobs):
    """orbii_prior_device.  state: float32 [n_src, 15] and priors: PRIOR array, both changed in place.  Returns (Rwg [9] f64, result)."""
    jobs = np.asarray(jobs).reshape(-1, 4)
    n, res = len(jobs), np.zeros(8, np.int32)
    seen_rows, seen_slots, kept = set(), set(), []
    for k, (pr, sr, rec, sl) in enumerate(jobs):
        ok = 0 <= pr < len(pose_R) and 0 <= sr < len(state) and 0 <= sl < len(priors) and (-1 if k == n - 1 else 0) <= rec < len(recs)
        if not ok:
            res[R_RANGE] += 1
        elif sr in seen_rows or sl in seen_slots:
            res[R_DUPLICATE] += 1
        else:
            kept.append(k)
        seen_rows.add(int(sr)), seen_slots.add(int(sl))                  # an earlier job counts, dropped or not
    res[R_DONE] = len(kept)
    O, RdV, dts = {}, {}, {}
    for k in kept:
        pr, sr, rec, _ = jobs[k]
        R, t = _pose_f32(pose_R, pose_t, pr)
        O[k] = im.mv(-(R.T), t)
        if rec >= 0:
            RdV[k] = im.mv(state[sr, :9].reshape(3, 3), recs[rec].updated_deltas()[1])
            dts[k] = recs[rec].delta_t
    dirv, velo = np.zeros(3, F32), {}
    for a, b in zip(kept[:-1], kept[1:]):
        dirv = dirv - RdV[a]
        velo[a] = (O[b] - O[a]) / dts[a]
    if len(kept) >= 2:
        velo[kept[-1]] = velo[kept[-2]]
    for k, v in velo.items():
        state[jobs[k][1], 12:15] = v
        priors[jobs[k][3]]["velo_priori"] = v
    nrm = im.norm3(dirv)
    if nrm > 0:
        dirv = dirv / nrm
    v = np.array([dirv[1], -dirv[0], 0], F32)
    nv = im.norm3(v)
    if nv == 0:
        res[R_REFUSED] = 1
        return I3.reshape(9).copy(), res
    theta = F32(math.asin(float(nv)))
    w = (theta * v) / nv
    return im.exp_and_right_jacobian(w)[0].astype(F64).reshape(9), res


# ---- the graph ---------------------------------------------------------------------------------------------------------------------------
def graph_init(graph, cal, pose_R, pose_t, state, jobs, initial_bias, Rwg=None, scale=1.0):
    """orbii_graph_init_device"""
    res = np.zeros(8, np.int32)
    tcb = cal["tcb"].astype(F64)
    for k, (pr, sr, _, _) in enumerate(np.asarray(jobs).reshape(-1, 4)):
        if not (0 <= pr < len(pose_R) and 0 <= sr < len(state)):
            res[R_RANGE] += 1
            graph.Rwb[k], graph.twb[k], graph.v[k], graph.Oc[k], graph.Pcb[k] = I3, 0, 0, 0, 0
            continue
        R, t = (x.astype(F64) for x in _pose_f32(pose_R, pose_t, pr))
        f = np.asarray(state[sr], F32).astype(F64)
        graph.Rwb[k], graph.twb[k], graph.v[k] = f[:9].reshape(3, 3), f[9:12], f[12:15]
        graph.Oc[k], graph.Pcb[k] = im.mv(-(R.T), t), im.mv(R.T, tcb)
        res[R_DONE] += 1
    graph.shared[0:6] = np.asarray(initial_bias, F32).astype(F64)
    graph.shared[6:15] = I3.reshape(9) if Rwg is None else np.asarray(Rwg, F64).reshape(9)
    graph.shared[15], graph.iter = scale, 0
    return res


# ---- the edge ----------------------------------------------------------------------------------------------------------------------------
def edge(graph, rec, e, gravity, kind, jacobian=True, quirk=True):
    """computeError and linearizeOplus of the edge between key frames e and e + 1: (err [9], J [9, 15] in the local order [v1, bg, ba, v2,
    gravity, scale] or None, float (dR, dV, dP) [15]).  quirk=False puts -JPa where kind G has -JPg (for the finite-difference test only)."""
    dRf, dVf, dPf, dbgf = fm.float_deltas(rec, graph.bg, graph.ba)
    dR, dV, dP, dbg = dRf.astype(F64), dVf.astype(F64), dPf.astype(F64), dbgf.astype(F64)
    JRg, JVg, JVa, JPg, JPa = (getattr(rec, k).astype(F64) for k in ("JRg", "JVg", "JVa", "JPg", "JPa"))
    dt, G, s, Rwg = F64(rec.delta_t), F64(F32(gravity)), graph.scale, graph.Rwg
    gs = kind == KIND_GS
    g = Rwg[:, 2] * (-G)
    R1, R2, v1, v2 = graph.Rwb[e], graph.Rwb[e + 1], graph.v[e], graph.v[e + 1]
    Rb1w = R1.T
    eR = im.mm(im.mm(dR.T, Rb1w), R2)
    er = fm.log_so3(eR)
    grav = ((0.5 * g) * dt) * dt
    if gs:
        O1, O2, P1, P2 = graph.Oc[e], graph.Oc[e + 1], graph.Pcb[e], graph.Pcb[e + 1]
        ev = im.mv(Rb1w, s * (v2 - v1) - g * dt) - dV
        ep = im.mv(Rb1w, ((((s * O2 + P2) - s * O1) - P1) - (s * v1) * dt) - grav) - dP
    else:
        ev = im.mv(Rb1w, (v2 - v1) - g * dt) - dV
        ep = im.mv(Rb1w, ((graph.twb[e + 1] - graph.twb[e]) - v1 * dt) - grav) - dP
    err = np.concatenate([er, ev, ep])
    flt = np.concatenate([dRf.reshape(9), dVf, dPf])
    if not jacobian:
        return err, None, flt
    invJ, Jr = fm.inverse_right_jacobian(er), fm.right_jacobian(im.mv(JRg, dbg))
    JG = np.stack([Rwg[:, 1] * G, Rwg[:, 0] * (-G)], 1)
    J = np.zeros((9, 15))
    if gs:
        J[3:6, 0:3], J[6:9, 0:3], J[3:6, 9:12] = (-s) * Rb1w, ((-s) * dt) * Rb1w, s * Rb1w
        J[3:6, 14], J[6:9, 14] = im.mv(s * Rb1w, v2 - v1), im.mv(s * Rb1w, (O2 - O1) - v1 * dt)
    else:
        J[3:6, 0:3], J[6:9, 0:3], J[3:6, 9:12] = -Rb1w, (-dt) * Rb1w, Rb1w
    J[0:3, 3:6] = im.mm(im.mm(im.mm(-invJ, eR.T), Jr), JRg)
    J[3:6, 3:6], J[6:9, 3:6] = -JVg, -JPg
    J[3:6, 6:9], J[6:9, 6:9] = -JVa, (-JPa if gs or not quirk else -JPg)             # G2oTypes.cpp:236
    J[3:6, 12:14], J[6:9, 12:14] = im.mm(-Rb1w, JG) * dt, im.mm((((-0.5) * dt) * dt) * Rb1w, JG)
    return err, J, flt


def local_to_global(e):
    """the global dof of the 15 local dof of edge e"""
    return np.array([9 + 3 * e + c for c in range(3)] + [0, 1, 2, 3, 4, 5] + [9 + 3 * (e + 1) + c for c in range(3)] + [6, 7, 8])


def edge_status(recs, edges, info):
    st = np.zeros(len(edges), np.int32)
    for e, ed in enumerate(edges):
        if not 0 <= int(ed["rec"]) < len(recs):
            st[e] = R_RANGE
        elif info[e, 0] == 0:
            st[e] = R_REFUSED
    return st


def linearize(graph, recs, gravity, edges, info, initial_bias, priori_g, priori_a, kind, mode=0):
    """orbii_linearize_device: a dict of err, chi2, chi2_prior, total, result, flt, status and, in mode 0, H, b, J, work"""
    n, ne = graph.n, graph.n - 1
    N = system_size(n)
    o = dict(err=np.zeros((ne, 9)), chi2=np.zeros(ne), chi2_prior=np.zeros(2), flt=np.zeros((ne, 15), F32), result=np.zeros(8, np.int32),
             status=edge_status(recs, edges[:ne], info))
    if mode == 0:
        o.update(H=np.zeros((N, N)), b=np.zeros(N), J=np.zeros((ne, 9, 15)), work=np.zeros((ne, EDGE_WORK)))
    total = 0.0
    for e in range(ne):
        o["result"][o["status"][e]] += 1
        if o["status"][e]:
            continue
        err, J, flt = edge(graph, recs[int(edges[e]["rec"])], e, gravity, kind, mode == 0)
        Om = info[e].reshape(9, 9)
        We = fm._ordered(Om, err[:, None])[:, 0]
        chi = float(fm._ordered(err[None, :], We[:, None])[0, 0])
        o["err"][e], o["chi2"][e], o["flt"][e] = err, chi, flt
        total = total + chi
        if mode == 0:
            M = fm._ordered(J.T, fm._ordered(Om, J))
            r = -fm._ordered(J.T, We[:, None])[:, 0]
            o["J"][e], o["work"][e, :225], o["work"][e, 225:] = J, M.reshape(225), r
            gi = local_to_global(e)
            o["H"][np.ix_(gi, gi)] = o["H"][np.ix_(gi, gi)] + M          # every entry: its edges in ascending order from zero
            o["b"][gi] = o["b"][gi] + r
    ib = np.asarray(initial_bias, F32).astype(F64)
    for p, w in enumerate((F64(F32(priori_g)), F64(F32(priori_a)))):
        ep = ib[3 * p:3 * p + 3] - graph.shared[3 * p:3 * p + 3]
        o["chi2_prior"][p] = (ep[0] * (w * ep[0]) + ep[1] * (w * ep[1])) + ep[2] * (w * ep[2])
        total = total + o["chi2_prior"][p]
        if mode == 0:
            for d in range(3):
                o["H"][3 * p + d, 3 * p + d] = o["H"][3 * p + d, 3 * p + d] + w
                o["b"][3 * p + d] = o["b"][3 * p + d] + w * ep[d]
    o["total"] = np.array([total])
    if mode == 0:
        fixed = ~dof_free(n, kind)
        o["H"][fixed, :], o["H"][:, fixed], o["b"][fixed] = 0.0, 0.0, 0.0
        o["H"][fixed, fixed] = 1.0
    return o


def damp(H, b, lam, n_kf, kind):
    """orbii_damp_device: (S, rhs, d_out[1])"""
    free = dof_free(n_kf, kind)
    S = H.copy()
    d = np.diag(H)[free]
    S[free, free] = d + lam
    return S, b.copy(), float(max(0.0, d.max()))


def oplus(graph, dx, kind):
    """orbii_oplus_device"""
    dx = np.asarray(dx, F64).reshape(-1)
    n = graph.n
    graph.shared[0:6] = graph.shared[0:6] + dx[0:6]
    N = im.mm(graph.Rwg, fm.exp_so3(np.array([dx[6], dx[7], 0.0])))
    graph.iter += 1
    if graph.iter == 3:
        N, graph.iter = fm.normalize_rotation(N), 0
    graph.shared[6:15] = N.reshape(9)
    if kind == KIND_GS:
        graph.shared[15] = graph.shared[15] * math.exp(dx[8])
    graph.v = graph.v + dx[9:9 + 3 * n].reshape(n, 3)
    res = np.zeros(8, np.int32)
    res[R_DONE] = n + 3 + (kind == KIND_GS)
    return res


def recover(graph, jobs, state, priors):
    """orbii_recover_device.  state, priors: changed in place.  Returns (bias [n, 6] f32, summary [10] f32, result)."""
    res = np.zeros(8, np.int32)
    seen_rows, seen_slots = set(), set()
    for k, (_, sr, _, sl) in enumerate(np.asarray(jobs).reshape(-1, 4)):
        if not (0 <= sr < len(state) and 0 <= sl < len(priors)):
            res[R_RANGE] += 1
        elif sr in seen_rows or sl in seen_slots:
            res[R_DUPLICATE] += 1
        else:
            state[sr, 12:15] = graph.v[k].astype(F32)
            priors[sl]["velo_priori"] = graph.v[k].astype(F32)
            res[R_DONE] += 1
        seen_rows.add(int(sr)), seen_slots.add(int(sl))
    bias = np.tile(graph.shared[0:6].astype(F32), (graph.n, 1))
    return bias, graph.shared[6:16].astype(F32), res


# ---- Map::applyScaleRotation ---------------------------------------------------------------------------------------------------------------
def apply_scale_rotation(cal, pose_R, pose_t, bad, kf_imu, state, priors, points, valid, n_points, summary, be_first, min_scale=0.1):
    """orbm_apply_scale_rotation_device; pose_R [n_kf, 9] / pose_t [n_kf, 3] f64, state f32 [n_src, 15], priors, points f32 [cap, 3] changed
    in place.  Returns the result."""
    res = np.zeros(8, np.int32)
    summary = np.asarray(summary, F32)
    Rwy, s = summary[:9].reshape(3, 3), summary[9]
    if be_first and s < F32(min_scale):
        res[R_REFUSED] = 1
        return res
    Ryw = Rwy.T
    seen_rows, seen_slots = set(), set()
    for k in range(len(pose_R)):
        if bad[k]:
            continue
        R, t = _pose_f32(pose_R, pose_t, k)
        R2, t2 = im.mm(R, Rwy), (t * s if be_first else t)
        pose_R[k], pose_t[k] = R2.reshape(9).astype(F64), t2.astype(F64)
        row, _, slot = (int(x) for x in kf_imu[k])
        if not (0 <= row < len(state) and 0 <= slot < len(priors)):
            res[R_RANGE] += 1
        elif row in seen_rows or slot in seen_slots:
            res[R_DUPLICATE] += 1
        else:
            Rwb, twb = im.imu_pose(cal, pose_R[k], pose_t[k])
            v = im.mv(Ryw, state[row, 12:15].copy())
            v = v * s if be_first else v
            state[row, :9], state[row, 9:12], state[row, 12:15] = Rwb.reshape(9), twb, v
            priors[slot]["velo_priori"] = v
            res[R_DONE] += 1
        seen_rows.add(row), seen_slots.add(slot)
    for p in range(min(max(int(n_points), 0), len(points))):
        if valid[p]:
            x = im.mv(Ryw, points[p].copy())
            points[p] = x * s if be_first else x
            res[R_POINTS] += 1
    return res


# ---- the closed loop's model back-end (tests/inertial_loop.py's interface) ---------------------------------------------------------------------
class ModelInit:
    """the chain of include/orbii.h in numpy: damp -> the ordered Cholesky (vw_model.solve) -> oplus -> linearize mode 1"""

    def __init__(self, sc, kind, priori_g, priori_a, graph=None, noise=None):
        self.sc, self.kind, self.pg, self.pa = sc, kind, priori_g, priori_a
        self.g, self.noise, self.noisy, self.refused = (sc["graph"] if graph is None else graph).copy(), noise or (lambda x: x), noise is not None, 0
        self.info = fm.edge_information(sc["recs"], sc["edges"])[0]

    def _lin(self, g, mode):
        sc = self.sc
        return linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], self.info, sc["initial_bias"], self.pg, self.pa, self.kind, mode)

    def linearize(self):
        self.o = self._lin(self.g, 0)
        return float(self.o["total"][0])

    def largest_diagonal(self):
        return float(self.noise(damp(self.o["H"], self.o["b"], 0.0, self.g.n, self.kind)[2]))

    def trial_outputs(self, lam):
        """one trial from the current linearisation, exact: (ok, d_out[0], the solve's result, the updated graph, its total)"""
        import vw_model as wm
        S, rhs, _ = damp(self.o["H"], self.o["b"], lam, self.g.n, self.kind)
        dx, (scale, _), res = wm.solve(S, rhs, self.o["b"], lam)
        g1 = self.g.copy()
        oplus(g1, self.noise(dx.reshape(-1)), self.kind)
        return bool(res[R_DONE] == 1), scale, res, g1

    def trial(self, lam):
        ok, scale, _, g1 = self.trial_outputs(lam)
        if self.noisy:                                                   # a perturbed loop: the updated vertices through the noise
            g1.v, g1.shared = self.noise(g1.v), self.noise(g1.shared)
        self.refused += not ok
        self.t = dict(g=g1, total=float(self.noise(self._lin(g1, 1)["total"][0])))
        return ok, float(self.noise(scale)), 0.0

    def totals(self):
        return self.t["total"], 0.0

    def accept(self):
        self.g = self.t["g"]

    def reject(self):
        pass

    def estimate(self):
        return dict(v=self.g.v.copy(), shared=self.g.shared.copy(), iter=np.array([self.g.iter], np.int32))


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def camera_pose(cal, src):
    """T_cw = T_cb * T_wb.inverse() of a float32 state row (Frame.cpp:65-71, imu_model.predict's tail): (Rcw 3x3, tcw 3) float32"""
    Rwb, twb = src[:9].reshape(3, 3), src[9:12]
    Rbw = Rwb.T
    return im.mm(cal["Rcb"], Rbw), im.mv(cal["Rcb"], im.mv(-Rbw, twb)) + cal["tcb"]


def make_scene(n_kf, seed=7, sample_counts=fm.SAMPLE_COUNTS, tilt=0.0, scale=1.0, noise=2e-3):
    """n_kf key frames in a chain (factors_model.make_chain: records of 2, 3, 8, 40, 100 samples in turn, every second one with a non-zero
    delta_bias), their pose table, state rows, prior slots and jobs; the graph as orbii_graph_init_device leaves it from a gravity
    direction tilted by `tilt` rad about x and the scale `scale`.  Key frame k: pose row k, state row k, record k, prior slot k."""
    sc = fm.make_chain(n_kf - 1, seed, walks=False, noise=noise, sample_counts=sample_counts)
    cal = sc["cal"]
    poses = [camera_pose(cal, s) for s in sc["src"]]
    sc["pose_R"] = np.stack([p[0].reshape(9) for p in poses]).astype(F64)
    sc["pose_t"] = np.stack([p[1] for p in poses]).astype(F64)
    sc["state"] = sc["src"].copy()
    sc["priors"] = np.zeros(n_kf, fm.PRIOR)
    sc["jobs"] = np.stack([np.arange(n_kf)] * 4, 1).astype(np.int32)
    sc["initial_bias"] = sc["recs"][0].bias.copy()
    sc["Rwg0"] = im.rodrigues(np.array([tilt, 0.0, 0.0])).reshape(9)
    g = Graph(n_kf)
    res = graph_init(g, cal, sc["pose_R"], sc["pose_t"], sc["state"], sc["jobs"], sc["initial_bias"], sc["Rwg0"], scale)
    assert res[R_DONE] == n_kf
    sc["graph"], sc["n_kf"] = g, n_kf
    return sc


# the closed loops: name -> (n_kf, kind, priori_g, priori_a, user lambda init; 0 = the default, tau * the largest diagonal entry)
LOOPS = {
    "5 GS": (5, KIND_GS, 1e6, 1e12, 1e3),
    "10 GS": (10, KIND_GS, 1e6, 1e12, 1e3),
    "10 G": (10, KIND_G, 0.0, 1e12, 0.0),
}
LOOP_ITERATIONS = 200
_loop_scenes = {}


def loop_scene(name):
    """full records (100 samples), the start tilted by 0.2 rad with the scale 1.1 (1 for kind G, which has no scale vertex)"""
    if name not in _loop_scenes:
        n_kf, kind = LOOPS[name][:2]
        _loop_scenes[name] = make_scene(n_kf, seed=7, sample_counts=(100,), tilt=0.2, scale=1.1 if kind == KIND_GS else 1.0)
    return _loop_scenes[name]


def loop_backend(name, noise=None):
    _, kind, pg, pa, _ = LOOPS[name]
    return ModelInit(loop_scene(name), kind, pg, pa, noise=noise)


# ---- a small map for the whole step ----------------------------------------------------------------------------------------------------------
def make_map(sc, n_points, seed=11):
    """a device-resident map around the key frames of a scene of make_scene, as the map-side calls read it: n_points table rows in
    shuffled order, each observed by two to four key frames through their slot arrays, an orbx_kp record and a descriptor per slot, the
    reference key frames and the refresh's table columns.  Key frame k is row k of the pose table, d_kf_imu[k] = (k, k, k)."""
    from projection_model import KP_DTYPE
    rng = np.random.RandomState(seed)
    n_kf = sc["n_kf"]
    stride, cap = n_points + 8, n_points + 10
    rows = rng.permutation(cap)[:n_points]
    slots = np.full((n_kf, stride), -1, np.int32)
    free = [[int(i) for i in rng.permutation(stride)] for _ in range(n_kf)]
    sizes = [F32(31.0) * F32(1.2) ** F32(r) for r in range(8)]
    kps = [np.zeros(stride, KP_DTYPE) for _ in range(n_kf)]
    ref_kf = np.zeros(cap, np.int32)
    for kp in kps:
        kp["size"], kp["class_id"] = sizes[0], -1
    for p in rows:
        seen = sorted(int(k) for k in rng.permutation(n_kf)[:rng.randint(2, 5)])
        ref_kf[p] = seen[0]
        for k in seen:
            i = free[k].pop()
            slots[k, i] = p
            octave = int(rng.randint(0, 8))
            kps[k]["x"][i], kps[k]["y"][i], kps[k]["size"][i], kps[k]["octave"][i] = rng.uniform(0, 640), rng.uniform(0, 480), sizes[octave], octave
    centre = np.mean([im.mv(-(sc["pose_R"][k].reshape(3, 3).T), sc["pose_t"][k]) for k in range(n_kf)], axis=0)
    points = (centre + rng.uniform(-6, 6, (cap, 3))).astype(F32)
    valid = np.zeros(cap, np.uint8)
    valid[rows] = 1
    table = dict(normals=rng.uniform(-1, 1, (cap, 3)).astype(F32), min_dist=rng.uniform(1, 2, cap).astype(F32), max_dist=rng.uniform(20, 30, cap).astype(F32),
                 desc=rng.randint(0, 256, (cap, 32)).astype(np.uint8))
    return dict(n=np.full(n_kf, stride, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=stride, valid=valid, points=points, cap_points=cap,
                kps=kps, kf_desc=[rng.randint(0, 256, (stride, 32)).astype(np.uint8) for _ in range(n_kf)], ref_kf=ref_kf, table=table,
                kf_imu=np.stack([np.arange(n_kf)] * 3, 1).astype(np.int32), n_points=np.array([cap], np.int32))
