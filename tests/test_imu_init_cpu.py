"""tests/imu_init_model.py, the numpy restatement of include/orbii.h and of the map rescale of include/orbm.h, held to what it restates
without a GPU: the analytic Jacobians of both kinds of edge against central differences, the omitted eigenvalue clamp, the prior and the
rescale against independent object-style restatements of the reference's listings, the structure of the dense system, and the closed
model loop with the spread of its final estimate under stage-sized errors."""
import math

import numpy as np
import pytest

import factors_model as fm
import imu_init_model as mm
import imu_model as im
import inertial_loop as il

F32 = np.float32


# ---- the Jacobians ----------------------------------------------------------------------------------------------------------------------------
# measured with this file (largest |analytic - numeric| over the largest |entry| of the column's block, at least 1; steps 1e-6, 1e-3 for
# the six bias dof, which pass through float); asserted at 4 x, the way tests/test_factors_cpu.py sets its bars
MEASURED_FD = {mm.KIND_GS: 9.1e-06, mm.KIND_G: 9.1e-06}
QUIRK_COLUMNS = (6, 7, 8)      # kind G, the accelerometer-bias block of ep: -JPg where -JPa belongs, G2oTypes.cpp:236 (mm.JPG_QUIRK_LINE)


def _fd_column(sc, g, e, kind, c):
    h = 1e-3 if 3 <= c < 9 else 1e-6
    d = np.zeros(mm.system_size(g.n))
    d[mm.local_to_global(e)[c]] = h
    gp, gm = g.copy(), g.copy()
    mm.oplus(gp, d, kind), mm.oplus(gm, -d, kind)
    rec, G = sc["recs"][e], sc["cal"]["gravity"]
    return (mm.edge(gp, rec, e, G, kind, False)[0] - mm.edge(gm, rec, e, G, kind, False)[0]) / (2 * h)


@pytest.mark.parametrize("kind", [mm.KIND_GS, mm.KIND_G])
def test_the_analytic_jacobian_agrees_with_central_differences(kind):
    """all 15 local dof through the vertices' own oplusImpl (14 for kind G, which has no scale vertex).  The three columns of kind G's
    quirk are EXEMPTED BY NAME: there the restated Jacobian is held to the listing (-JPg), and the listing corrected (-JPa) to the
    differences"""
    sc = mm.make_scene(4, seed=3, tilt=0.1, scale=1.05 if kind == mm.KIND_GS else 1.0)
    g, worst = sc["graph"], 0.0
    assert mm.JPG_QUIRK_LINE == 236
    for e in range(3):
        rec = sc["recs"][e]
        J = mm.edge(g, rec, e, sc["cal"]["gravity"], kind)[1]
        Jfixed = mm.edge(g, rec, e, sc["cal"]["gravity"], kind, quirk=False)[1]
        for c in range(15 if kind == mm.KIND_GS else 14):
            col = J[:, c]
            if kind == mm.KIND_G and c in QUIRK_COLUMNS:
                assert np.array_equal(col[6:9], -rec.JPg.astype(np.float64)[:, c - 6]) and not np.array_equal(col, Jfixed[:, c])
                col = Jfixed[:, c]
            worst = max(worst, np.abs(_fd_column(sc, g, e, kind, c) - col).max() / max(1.0, np.abs(col).max()))
        if kind == mm.KIND_GS:
            assert np.array_equal(J, Jfixed)
        else:
            assert not J[:, 14].any()
    print("kind %d: largest deviation %.2g" % (kind, worst))
    assert worst <= 4 * MEASURED_FD[kind]


def test_the_edge_information_clamp_is_a_no_op_on_every_test_record():
    """orbii_linearize_device takes orbi_edge_information_device's d_info, which omits the reference's eigenvalue clamp (G2oTypes.cpp:86-90)"""
    scenes = [mm.make_scene(n, seed=20 + n) for n in (2, 3, 6, 17, 66)] + [mm.loop_scene(k) for k in mm.LOOPS]
    for sc in scenes:
        info, _, res = fm.edge_information(sc["recs"], sc["edges"])
        assert res[fm.R_DONE] == len(sc["edges"])
        for e in range(len(sc["edges"])):
            _, clamped, smallest = fm.clamp_information(info[e].reshape(9, 9))
            assert clamped == 0 and smallest > 1e-12


# ---- the prior against an object-style restatement of LocalMapping.cpp:391-407 --------------------------------------------------------------------
class _KeyFrame:
    """what the listings touch of a KeyFrame, in float32 with numpy's own products"""

    def __init__(self, cal, Rcw, tcw, v, rec):
        self.cal, self.rec, self.v_w, self.velo_priori = cal, rec, v.astype(F32), v.astype(F32)
        self.setPose(Rcw.astype(F32), tcw.astype(F32))

    def setPose(self, Rcw, tcw):                       # KeyFrame.cpp:27-34
        self.Rcw, self.tcw = Rcw, tcw
        self.O_w = (-Rcw.T @ tcw).astype(F32)
        Rwc = Rcw.T
        self.Rwb, self.twb = (Rwc @ self.cal["Rcb"]).astype(F32), (Rwc @ self.cal["tcb"] + (-Rwc @ tcw)).astype(F32)

    def setVelocity(self, velo):                       # KeyFrame.cpp:65-69
        self.v_w = self.velo_priori = velo.astype(F32)


def _key_frames(sc):
    return [_KeyFrame(sc["cal"], sc["pose_R"][k].reshape(3, 3), sc["pose_t"][k], sc["state"][k, 12:15], sc["recs"][k]) for k in range(sc["n_kf"])]


def test_the_prior_agrees_with_an_object_style_restatement():
    for n_kf in (2, 3, 6, 17):
        sc = mm.make_scene(n_kf, seed=20 + n_kf)
        kfs = _key_frames(sc)
        for kf, row in zip(kfs, sc["state"]):          # the scene's T_wb, as getImuPose() returns it
            kf.Rwb = row[:9].reshape(3, 3)
        direction = np.zeros(3, F32)
        for i in range(n_kf - 1):                      # LocalMapping.cpp:394-400
            direction = direction - kfs[i].Rwb @ kfs[i].rec.updated_deltas()[1]
            velo = (kfs[i + 1].O_w - kfs[i].O_w) / kfs[i].rec.delta_t
            kfs[i].setVelocity(velo), kfs[i + 1].setVelocity(velo)
        direction = direction / np.linalg.norm(direction)
        v = np.cross(np.array([0, 0, -1], F32), direction).astype(F32)
        nv = F32(np.linalg.norm(v))
        theta = F32(math.asin(nv))
        Rwg = im.rodrigues((theta * v / nv).astype(np.float64))
        state, priors = sc["state"].copy(), sc["priors"].copy()
        got, res = mm.prior(sc["pose_R"], sc["pose_t"], state, sc["recs"], priors, sc["jobs"])
        assert res[mm.R_DONE] == n_kf and not res[1:4].any()
        for k, kf in enumerate(kfs):                   # a velocity is a difference of two camera centres over dt: a few ulps of the centres
            pair = min(k, n_kf - 2)
            bar = 8 * 2.0 ** -24 * max(np.abs(kfs[pair].O_w).max(), np.abs(kfs[pair + 1].O_w).max()) / float(kfs[pair].rec.delta_t)
            assert np.abs(state[k, 12:15].astype(np.float64) - kf.v_w).max() <= bar and np.array_equal(priors[k]["velo_priori"], state[k, 12:15])
        assert np.array_equal(state[:, :12], sc["state"][:, :12]) and np.array_equal(state[-1, 12:15], state[-2, 12:15])
        assert np.abs(got.reshape(3, 3) - Rwg).max() < 2e-6


# ---- the rescale against an object-style restatement of Map.cpp:96-124 ------------------------------------------------------------------------------
@pytest.mark.parametrize("be_first", [True, False])
def test_the_rescale_agrees_with_an_object_style_restatement(be_first):
    n_kf, n_points = 6, 65
    sc = mm.make_scene(n_kf, seed=26)
    rng = np.random.RandomState(4)
    kfs = _key_frames(sc)
    pts = rng.normal(0, 3, (n_points, 3)).astype(F32)
    valid = (rng.uniform(size=n_points) < 0.8).astype(np.uint8)
    bad = np.zeros(n_kf, np.uint8)
    bad[2] = 1
    Rwy, s = im.rodrigues(np.array([0.2, -0.1, 0.05])).astype(F32), F32(1.7)
    summary = np.concatenate([Rwy.reshape(9), [s]]).astype(F32)
    Ryw = Rwy.T
    want_pts = pts.copy()
    for kf, b in zip(kfs, bad):                        # Map.cpp:100-114 (a bad key frame is not in the map's set)
        if b:
            continue
        kf.setPose(kf.Rcw @ Rwy, kf.tcw * s if be_first else kf.tcw)
        kf.setVelocity(Ryw @ kf.v_w * s if be_first else Ryw @ kf.v_w)
    for p in range(n_points):                          # Map.cpp:116-121
        if valid[p]:
            want_pts[p] = Ryw @ pts[p] * s if be_first else Ryw @ pts[p]
    pose_R, pose_t, state, priors, points = sc["pose_R"].copy(), sc["pose_t"].copy(), sc["state"].copy(), sc["priors"].copy(), pts.copy()
    # the scene's state rows are the float T_wb of its poses up to rounding; the rescale recomputes them from the pose
    kf_imu = np.stack([np.arange(n_kf), np.arange(n_kf), np.arange(n_kf)], 1).astype(np.int32)
    res = mm.apply_scale_rotation(sc["cal"], pose_R, pose_t, bad, kf_imu, state, priors, points, valid, n_points, summary, be_first)
    assert list(res[:5]) == [n_kf - 1, 0, 0, 0, int(valid.sum())]
    for k, kf in enumerate(kfs):
        if bad[k]:
            assert np.array_equal(pose_R[k], sc["pose_R"][k]) and np.array_equal(state[k], sc["state"][k])
            continue
        assert np.allclose(pose_R[k].reshape(3, 3), kf.Rcw, atol=1e-6) and np.allclose(pose_t[k], kf.tcw, rtol=1e-6, atol=1e-6)
        assert np.allclose(state[k, :9].reshape(3, 3), kf.Rwb, atol=1e-6) and np.allclose(state[k, 9:12], kf.twb, rtol=1e-5, atol=1e-5)
        assert np.allclose(state[k, 12:15], kf.v_w, rtol=1e-5, atol=1e-6) and np.array_equal(priors[k]["velo_priori"], state[k, 12:15])
    assert np.allclose(points, want_pts, rtol=1e-5, atol=1e-5) and np.array_equal(points[valid == 0], pts[valid == 0])


def test_a_small_scale_leaves_everything_as_it_is():
    sc = mm.make_scene(3, seed=23)
    pts, valid = np.ones((4, 3), F32), np.ones(4, np.uint8)
    summary = np.concatenate([np.eye(3).reshape(9), [0.05]]).astype(F32)
    kf_imu = np.stack([np.arange(3)] * 3, 1).astype(np.int32)
    args = [a.copy() for a in (sc["pose_R"], sc["pose_t"], np.zeros(3, np.uint8), kf_imu, sc["state"], sc["priors"], pts, valid)]
    res = mm.apply_scale_rotation(sc["cal"], *args, 4, summary, True)
    assert list(res[:5]) == [0, 0, 0, 1, 0]
    for a, b in zip(args, (sc["pose_R"], sc["pose_t"], np.zeros(3, np.uint8), kf_imu, sc["state"], sc["priors"], pts, valid)):
        assert a.tobytes() == b.tobytes()
    res = mm.apply_scale_rotation(sc["cal"], *args, 4, summary, False)   # without be_first the scale is not looked at
    assert list(res[:5]) == [3, 0, 0, 0, 4]


# ---- the dense system --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_kf,kind", [(2, mm.KIND_GS), (3, mm.KIND_G), (6, mm.KIND_GS), (17, mm.KIND_G)])
def test_the_dense_system_has_the_stated_structure(n_kf, kind):
    sc = mm.make_scene(n_kf, seed=20 + n_kf, tilt=0.1, scale=1.05 if kind == mm.KIND_GS else 1.0)
    info = fm.edge_information(sc["recs"], sc["edges"])[0]
    o = mm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], info, sc["initial_bias"], 1e6, 1e12, kind, 0)
    H, b, N = o["H"], o["b"], mm.system_size(n_kf)
    assert H.shape == (N, N) and N % 15 == 0 and N >= 9 + 3 * n_kf > N - 15
    fixed = ~mm.dof_free(n_kf, kind)
    assert fixed.sum() == N - 9 - 3 * n_kf + (kind == mm.KIND_G)
    assert np.array_equal(H[fixed][:, fixed], np.eye(fixed.sum())) and not H[fixed][:, ~fixed].any() and not H[~fixed][:, fixed].any() and not b[fixed].any()
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    for k in range(n_kf):
        for j in range(n_kf):
            blk = H[9 + 3 * k:12 + 3 * k, 9 + 3 * j:12 + 3 * j]
            assert blk.any() == (abs(k - j) <= 1), (k, j)
    # against the plain products of the same Jacobians
    Hd, bd = np.zeros((N, N)), np.zeros(N)
    for e in range(n_kf - 1):
        gi, J, Om = mm.local_to_global(e), o["J"][e], info[e].reshape(9, 9)
        Hd[np.ix_(gi, gi)] += J.T @ Om @ J
        bd[gi] -= J.T @ Om @ o["err"][e]
    for p, w in enumerate((float(F32(1e6)), float(F32(1e12)))):      # the priors' weights are floats
        Hd[3 * p:3 * p + 3, 3 * p:3 * p + 3] += w * np.eye(3)
        bd[3 * p:3 * p + 3] += w * (sc["initial_bias"][3 * p:3 * p + 3].astype(np.float64) - sc["graph"].shared[3 * p:3 * p + 3])
    free = ~fixed
    dH, db = np.abs(H[free][:, free] - Hd[free][:, free]).max() / np.abs(Hd).max(), np.abs(b[free] - bd[free]).max() / np.abs(bd).max()
    print("against the plain products: H %.2g, b %.2g" % (dH, db))
    assert dH <= 1e-12 and db <= 1e-12
    o1 = mm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], info, sc["initial_bias"], 1e6, 1e12, kind, 1)
    assert np.array_equal(o1["err"], o["err"]) and o1["total"][0] == o["total"][0] and "H" not in o1
    S, rhs, h_max = mm.damp(H, b, 7.0, n_kf, kind)
    assert np.array_equal(np.diag(S)[free], np.diag(H)[free] + 7.0) and np.array_equal(np.diag(S)[fixed], np.ones(fixed.sum())) and h_max == np.diag(H)[free].max()
    assert np.array_equal(S - np.diag(np.diag(S)), H - np.diag(np.diag(H))) and np.array_equal(rhs, b)


# ---- the closed model loop ------------------------------------------------------------------------------------------------------------------------
RUNS = 8
OUTPUTS = ("v", "bg", "ba", "Rwg", "scale", "total")
# the largest deviation of the final estimate of eight loops whose every trial output is perturbed by 1 + 1e-9 N(0, 1) (inertial_loop.Noise,
# sigma = inertial_loop.BAR) from the unperturbed loop: per output as a share of the output's largest entry, the final total relative.
# Measured with this file; a fresh measurement is held to within 2 x of these, either way.  tests/test_imu_init_gpu.py reads them.
MEASURED_SPREAD = {
    "5 GS": {"v": 9.13e-08, "bg": 8.88e-07, "ba": 4.66e-09, "Rwg": 6.78e-07, "scale": 1.44e-06, "total": 3.20e-08},
    "10 GS": {"v": 2.92e-09, "bg": 2.51e-08, "ba": 3.93e-09, "Rwg": 4.54e-09, "scale": 3.78e-09, "total": 4.86e-09},
    "10 G": {"v": 3.97e-09, "bg": 1.65e-07, "ba": 1.56e-09, "Rwg": 3.71e-09, "scale": 4.41e-09, "total": 4.73e-08},
}
_cache = {}


def split(est):
    s = est["shared"]
    return dict(v=est["v"], bg=s[0:3], ba=s[3:6], Rwg=s[6:15], scale=s[15:16])


def model_run(name):
    """the unperturbed model loop of a scene, computed once and shared: nobody changes it"""
    if ("run", name) not in _cache:
        be = mm.loop_backend(name)
        r = il.optimize(be, mm.LOOP_ITERATIONS, user_lambda_init=mm.LOOPS[name][4])
        _cache[("run", name)] = dict(r, estimate=be.estimate(), refused=be.refused)
    return _cache[("run", name)]


def final_total(r):
    return min([t[4] for t in r["trace"] if t[-1]] + [r["trace"][0][3]])


def _dev(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def measure(name):
    if ("spread", name) not in _cache:
        ref = model_run(name)
        spread = dict.fromkeys(OUTPUTS, 0.0)
        for k in range(RUNS):
            be = mm.loop_backend(name, il.Noise(1000 + k))
            r = il.optimize(be, mm.LOOP_ITERATIONS, user_lambda_init=mm.LOOPS[name][4])
            a, b = split(be.estimate()), split(ref["estimate"])
            for o in OUTPUTS[:-1]:
                spread[o] = max(spread[o], _dev(a[o], b[o]))
            spread["total"] = max(spread["total"], abs(final_total(r) - final_total(ref)) / final_total(ref))
        _cache[("spread", name)] = spread
    return _cache[("spread", name)]


@pytest.mark.parametrize("name", list(mm.LOOPS))
def test_the_model_loop_is_admissible_and_its_spread_is_what_is_written(name):
    """THE CONDITION ON A SCENE: its unperturbed model loop accepts at least three trials, reduces the total at least tenfold and refuses no
    solve.  A scene that fails this is changed, never the condition.  The accept / reject SEQUENCE is not compared: the float cast of the
    bias vertices makes the cost a step function and the sequence leaves the unperturbed one under stage-sized errors; the final estimate
    does not."""
    n_kf, kind, pg, pa, lam0 = mm.LOOPS[name]
    r = model_run(name)
    tr = r["trace"]
    print("    %s: %d iterations, %d trials, %d accepted, total %.4g -> %.4g, %s" % (name, r["iterations"], len(tr), r["accepted"], tr[0][3], final_total(r),
                                                                                   il.decisions([r])[0]))
    assert r["accepted"] >= 3 and final_total(r) <= tr[0][3] / 10 and r["refused"] == 0 and all(t[7] for t in tr)
    o0 = mm.loop_backend(name)._lin(mm.loop_scene(name)["graph"], 0)
    assert tr[0][2] == (lam0 if pg != 0 else il.TAU * mm.damp(o0["H"], o0["b"], 0.0, n_kf, kind)[2]) > 0    # Optimize.cpp:104-105
    accepted = [t[4] for t in tr if t[-1]]
    assert all(b <= a for a, b in zip([tr[0][3]] + accepted, accepted)), "the total is non-increasing over accepted trials"
    assert r["estimate"]["iter"][0] == r["accepted"] % 3
    g0 = mm.loop_scene(name)["graph"]
    if kind == mm.KIND_GS:
        assert abs(r["estimate"]["shared"][15] - 1.0) < abs(g0.scale - 1.0) / 5        # the scene was built at scale 1 with gravity along -z
    else:
        assert r["estimate"]["shared"][15] == g0.scale == 1.0
    assert abs(r["estimate"]["shared"][14] - 1.0) < abs(g0.Rwg[2, 2] - 1.0) / 5
    spread = measure(name)
    print('    "%s": {%s},' % (name, ", ".join('"%s": %.2e' % (k, v) for k, v in spread.items())))
    assert name in MEASURED_SPREAD, "no figures written for this scene"
    for k, v in spread.items():                        # both sides: a figure written too large would widen the GPU test's bars
        w = MEASURED_SPREAD[name][k]
        assert (v == 0 and w == 0) or w / 2 <= v <= 2 * w, (name, k, v, w)
