"""tests/full_inertial_model.py and tests/full_inertial_loop.py judged without a GPU: the shared-bias edge's analytic Jacobian against
central differences, the dense system against factors_model's per-state system folded onto one bias pair, one iteration against an
object-style restatement of Optimize.cpp:239-398 that solves ONE dense system, the structure of the outputs, and the condition a loop
scene must meet before a device loop may be compared with it, with the figures the GPU test's bars come from."""
import numpy as np
import pytest

import factors_model as fm
import full_inertial_loop as fl
import full_inertial_model as fim
import inertial_loop as il
import vi_model as vm
from test_factors_cpu import _Edge, _hat, _jr, _log
from test_inertial_loop_cpu import RUNS, TRIAL, _rel, trial_deviation
from test_vw_cpu import _EdgeMono

_cache = {}
# measured with this file (largest |analytic - numeric| over the largest |entry| of the 9 x 30 Jacobian; steps 1e-6, 1e-3 for the bias
# dof, which pass through a cast to float), on the edges of 2, 8 and 40 samples of the 5-key-frame scene.  The bar is 4 x that.
MEASURED_FD = {2: 3.61e-06, 8: 1.45e-05, 40: 3.53e-05}
# the model's step in the dense system of the restatement (5 key frames, 40 points, lambda 1): the longdouble residual |A x - b|_inf /
# (|A|_inf |x|_inf), computeScale against the dense solve's (relative) and the step against np.linalg.solve's (of its largest entry; the
# inertial information is 1e14 times lambda, so two backward-stable solves agree no better).  The bars are 4 x.
# Measured with key frame 0 fixed: residual 3.54e-19, computeScale 3.78e-13, step 1.55e-12; with every key frame free (the gauge is held by lambda
# alone): 2.14e-17, 5.99e-10, 1.04e-04.
MEASURED_RESIDUAL, MEASURED_SCALE, MEASURED_STEP = {True: 3.54e-19, False: 2.14e-17}, {True: 3.78e-13, False: 5.99e-10}, {True: 1.55e-12, False: 1.04e-04}


def _scene(n_kf=5, fix_first=True):
    key = (n_kf, fix_first)
    if key not in _cache:
        _cache[key] = fim.stage_scene(n_kf, fix_first)
    return _cache[key]


# ---- the analytic Jacobian against central differences ---------------------------------------------------------------------------------------
def _perturbed_error(sc, e, col, h):
    """the edge's error with column col of its Jacobian stepped: 0..8 state i, 9..14 the carrier's bias pair, 15..23 state j"""
    g = sc["graph"].copy()
    g.fixed[:] = 0
    i, j, b = int(sc["edges"][e]["i"]), int(sc["edges"][e]["j"]), sc["bias_state"]
    dx = np.zeros((g.n, 15))
    dx[i if col < 9 else b if col < 15 else j, col % 15] = h
    fm.oplus(g, dx)
    return fm.inertial_edge(sc["recs"][int(sc["edges"][e]["rec"])], fim._SharedBias(g, b), i, j, sc["cal"]["gravity"], False)[0]


@pytest.mark.parametrize("n_samples", [2, 8, 40])
def test_the_shared_bias_jacobian_agrees_with_central_differences(n_samples):
    sc = _scene()
    e = fm.SAMPLE_COUNTS.index(n_samples) if n_samples != 40 else 3
    assert len(sc["recs"][int(sc["edges"][e]["rec"])].meas) == n_samples
    J = fim.inertial_linearize(sc, sc["graph"])["J"][e]
    num = np.zeros((9, 30))
    for col in range(24):
        h = 1e-3 if 9 <= col < 15 else 1e-6
        num[:, col] = (_perturbed_error(sc, e, col, h) - _perturbed_error(sc, e, col, -h)) / (2 * h)
    assert not J[:, 24:].any() and J[:, 9:15].any()
    worst = np.abs(J - num).max() / np.abs(J).max()
    print("samples %d: analytic vs central differences %.3g of the largest entry" % (n_samples, worst))
    assert worst <= 4 * MEASURED_FD[n_samples]


# ---- against the per-state model, folded ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_kf,fix_first", [(2, True), (3, False), (5, True), (31, True)])
def test_the_dense_system_is_the_per_state_system_folded_onto_one_bias_pair(n_kf, fix_first):
    """factors_model's linearisation of the same chain without walks, every state's bias set to the shared value: its Hessian and
    right-hand side, folded by P^T H P with P sending the one bias to every state's bias dof, are this model's dense system.  1e-12, the
    project's bar for two restatements.  The priors are weighted 0 here: the per-state model has none."""
    sc = _scene(n_kf, fix_first)
    g, b = sc["graph"], sc["bias_state"]
    per = fm.Graph(n_kf)
    for k in ("Rwb", "twb", "v"):
        getattr(per, k)[:] = getattr(g, k)[:n_kf]
    per.bg[:], per.ba[:] = g.bg[b], g.ba[b]
    per.fixed[0] = fim.FIRST_FIXED if fix_first else 0
    info = sc["info"]
    o = fm.linearize(per, sc["recs"], sc["cal"]["gravity"], sc["edges"], info, np.zeros((len(info), 18)), None, None, fim.HUBER_DELTA, 0)
    H, rhs = np.zeros((15 * n_kf, 15 * n_kf)), o["b"].reshape(-1)
    for s in range(n_kf):
        H[15 * s:15 * s + 15, 15 * s:15 * s + 15] = o["H_diag"][s]
    for e, ed in enumerate(sc["edges"]):
        i, j = int(ed["i"]), int(ed["j"])
        H[15 * i:15 * i + 15, 15 * j:15 * j + 15] += o["H_off"][e]
        H[15 * j:15 * j + 15, 15 * i:15 * i + 15] += o["H_off"][e].T
    P = np.zeros((15 * n_kf, 9 * n_kf + 6))
    for s in range(n_kf):
        P[15 * s:15 * s + 9, 9 * s:9 * s + 9] = np.eye(9)
        P[15 * s + 9:15 * s + 15, 9 * n_kf:] = np.eye(6)
    mine = fim.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], info, b, sc["prior_rec"], 0.0, 0.0)
    A = np.zeros((15 * (n_kf + 1), 15 * (n_kf + 1)))
    for s in range(n_kf + 1):
        A[15 * s:15 * s + 15, 15 * s:15 * s + 15] = mine["H_diag"][s]
    for e, ed in enumerate(mine["off_edges"]):
        i, j = int(ed["i"]), int(ed["j"])
        A[15 * i:15 * i + 15, 15 * j:15 * j + 15] += mine["H_off"][e]
        A[15 * j:15 * j + 15, 15 * i:15 * i + 15] += mine["H_off"][e].T
    keep = np.concatenate([np.concatenate([np.arange(9) + 15 * s for s in range(n_kf)]), 15 * n_kf + 9 + np.arange(6)])
    rest = np.setdiff1d(np.arange(15 * (n_kf + 1)), keep)
    assert not A[rest].any() and not A[:, rest].any() and not mine["b"].reshape(-1)[rest].any()
    dev_H, dev_b = _rel(A[keep][:, keep], P.T @ H @ P), _rel(mine["b"].reshape(-1)[keep], P.T @ rhs)
    print("%d key frames: H %.3g, b %.3g of the largest entry" % (n_kf, dev_H, dev_b))
    assert dev_H <= 1e-12 and dev_b <= 1e-12
    np.testing.assert_array_equal(mine["chi2"], o["chi2"][:, 0])


# ---- the object-style restatement ------------------------------------------------------------------------------------------------------------------
def _dense_step(sc, lam):
    """Optimize.cpp:239-398 with objects and matrices: a VertexPose and a velocity per key frame (:257-266), ONE gyro and ONE acc bias
    vertex (:282-291), EdgeInertial with Huber 4.1134 on them (:296-351), the two EdgePriori3D (:353-364), every point with its EdgeMono
    (:369-394); ONE Hessian over all of it, lambda on the diagonal, np.linalg.solve"""
    g, n_kf, m, cal = sc["graph"], sc["n_kf"], sc["n_points"], sc["cal"]
    b = 15 * n_kf                                               # the carrier's block: the bias pair at dof 9..14 of it
    n = 15 * (n_kf + 1) + 3 * m
    fixed = np.concatenate([np.concatenate([fm.dof_fixed(f) for f in g.fixed]), np.zeros(3 * m, bool)])
    G = np.array([0, 0, -float(np.float32(cal["gravity"]))])
    bg, ba = g.bg[n_kf], g.ba[n_kf]
    edges = []
    for ed in sc["edges"]:
        i, j, r = int(ed["i"]), int(ed["j"]), sc["recs"][int(ed["rec"])]
        dRf, dVf, dPf, dbgf = fm.float_deltas(r, bg, ba)
        dR, dV, dP, dbg = (x.astype(float) for x in (dRf, dVf, dPf, dbgf))
        JRg, JVg, JVa, JPg, JPa = (getattr(r, k).astype(float) for k in ("JRg", "JVg", "JVa", "JPg", "JPa"))
        dt, R1, R2 = float(r.delta_t), g.Rwb[i], g.Rwb[j]
        eR = dR.T @ R1.T @ R2
        er = _log(eR)
        a = R1.T @ (g.v[j] - g.v[i] - G * dt)
        c = R1.T @ (g.twb[j] - g.twb[i] - g.v[i] * dt - 0.5 * G * dt * dt)
        invJ, Z = _jr(er, True), np.zeros((3, 3))
        blocks = [np.block([[-invJ @ R2.T @ R1, Z], [_hat(a), Z], [_hat(c), -np.eye(3)]]), np.vstack([Z, -R1.T, -R1.T * dt]),
                  np.vstack([-invJ @ eR.T @ _jr(JRg @ dbg) @ JRg, -JVg, -JPg]), np.vstack([Z, -JVa, -JPa]),
                  np.block([[invJ, Z], [Z, Z], [Z, R1.T @ R2]]), np.vstack([Z, R1.T, Z])]
        info = np.linalg.inv(r.C.astype(float)[:9, :9])
        edges.append(_Edge([15 * i, 15 * i + 6, b + 9, b + 12, 15 * j, 15 * j + 6], np.concatenate([er, a - dV, c - dP]), blocks, (info + info.T) / 2, fim.HUBER_DELTA))
    prior = sc["recs"][sc["prior_rec"]].updated_bias.astype(float)
    edges.append(_Edge([b + 9], prior[:3] - bg, [-np.eye(3)], float(np.float32(sc["prior_g"])) * np.eye(3)))
    edges.append(_Edge([b + 12], prior[3:] - ba, [-np.eye(3)], float(np.float32(sc["prior_a"])) * np.eye(3)))
    H, rhs = np.zeros((n, n)), np.zeros(n)
    for ed in edges:
        ed.add_to(H, rhs, fixed)
    total = sum(ed.chi2() if ed.delta <= 0 or ed.chi2() <= ed.delta ** 2 else 2 * np.sqrt(ed.chi2()) * ed.delta - ed.delta ** 2 for ed in edges)
    for e in range(len(sc["w"])):
        s, l = int(sc["edge_state"][e]), int(sc["edge_point"][e])
        edge = _EdgeMono(cal, sc["cam"], g.Rwb[s], g.twb[s], sc["points"][l], sc["z"][e], sc["w"][e])
        err = edge.error()
        chi2 = err @ edge.info @ err
        rho1 = vm.HUBER_MONO / np.sqrt(chi2) if chi2 > vm.HUBER_MONO ** 2 else 1.0
        Jp, Jl = edge.jacobians()
        J = np.zeros((2, n))
        if not fixed[15 * s]:
            J[:, 15 * s:15 * s + 6] = Jp
        J[:, 15 * (n_kf + 1) + 3 * l:15 * (n_kf + 1) + 3 * l + 3] = Jl
        H += J.T @ (rho1 * edge.info) @ J
        rhs -= J.T @ (rho1 * edge.info) @ err
    keep = ~fixed
    A = H[keep][:, keep] + lam * np.eye(keep.sum())
    x = np.zeros(n)
    x[keep] = np.linalg.solve(A, rhs[keep])
    return A, rhs[keep], keep, x, float(x @ (lam * x + np.where(keep, rhs, 0.0))), total


@pytest.mark.parametrize("fix_first", [True, False])
def test_reduce_solve_backsub_equal_one_dense_solve_of_the_restatement(fix_first):
    sc = _scene(5, fix_first)
    it = sc["first"]                                            # lambda 1
    A, rhs, keep, x_np, scale_np, total = _dense_step(sc, 1.0)
    x = np.concatenate([it["dx"].reshape(-1), it["backsub"]["xl"].reshape(-1)])
    assert not x[~keep].any() and keep.sum() == 9 * (5 - fix_first) + 6 + 3 * sc["n_points"]
    L = np.longdouble
    resid = float(np.abs(A.astype(L) @ x[keep].astype(L) - rhs.astype(L)).max() / (np.abs(A).sum(1).max() * np.abs(x).max()))
    step = float(np.abs(x - x_np).max() / np.abs(x_np).max())
    scale = it["scale"] + it["backsub"]["scale"]
    rel = abs(scale - scale_np) / abs(scale_np)
    print("fix_first %s: residual %.3g, step %.3g, computeScale %.10g against %.10g (%.3g), inertial total %.3g" %
          (fix_first, resid, step, scale, scale_np, rel, abs(total - it["inertial"]["total"][1]) / total))
    assert abs(total - it["inertial"]["total"][1]) <= 1e-12 * total
    assert resid <= 4 * MEASURED_RESIDUAL[fix_first] and step <= 4 * MEASURED_STEP[fix_first] and rel <= 4 * MEASURED_SCALE[fix_first]


# ---- structure ---------------------------------------------------------------------------------------------------------------------------------------
def test_masks_symmetry_huber_and_the_priors():
    sc = _scene(5, True)
    g, b, o = sc["graph"], sc["bias_state"], fim.inertial_linearize(_scene(5, True), _scene(5, True)["graph"])
    fx = np.stack([fm.dof_fixed(f) for f in g.fixed])
    assert fx[0].all() and fx[1:5, 9:].all() and not fx[1:5, :9].any() and fx[b, :9].all() and not fx[b, 9:].any()
    for s in range(g.n):                                        # the fixed masks zero exactly their rows and columns
        H = o["H_diag"][s]
        assert not H[fx[s]].any() and not H[:, fx[s]].any() and not o["b"][s][fx[s]].any() and np.diag(H)[~fx[s]].all() and o["b"][s][~fx[s]].all(), s
    A, rhs, mask, _, dropped = fim.dense(o, g.fixed, len(sc["recs"]), 0.0)
    assert dropped == 0 and np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max() and not rhs[mask].any()
    for e, ed in enumerate(sc["edges"]):
        M = o["M"][e]
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max() and not M[24:].any()
        assert (not M[:9].any()) == (int(ed["i"]) == 0), e    # key frame 0 is fixed: its rows of the form are zero
    d2 = fim.HUBER_DELTA ** 2                                  # both Huber branches, in the scenes the GPU stages run on too
    assert (_scene(3)["first"]["inertial"]["chi2"] > d2).all() and o["total"][1] < o["total"][0]
    for n_kf in fim.STAGE_COMMON_BIAS:
        c = _scene(n_kf)["first"]["inertial"]["chi2"]
        assert (c > d2).any() and (c <= d2).any(), (n_kf, c)
    # the priors: zero at the start, non-zero after a bias step; their weight is the double of the float
    assert not o["chi2_prior"].any() and o["result"].tolist() == [4, 0, 0, 0, 2, 0, 0, 0]
    g1 = g.copy()
    dx = np.zeros((g.n, 15))
    dx[:, 9:] = [1e-3, -2e-3, 3e-3, 1e-2, 2e-2, -1e-2]
    fm.oplus(g1, dx)
    assert not g1.bg[:5].any() and not g1.ba[:5].any()          # "no such vertex": only the carrier's pair moves
    o1 = fim.linearize(g1, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], b, sc["prior_rec"], 1e6, 1e12, mode=1)
    assert o1["chi2_prior"][0] == pytest.approx(1e6 * 14e-6, rel=1e-9) and o1["chi2_prior"][1] == pytest.approx(float(np.float32(1e12)) * 6e-4, rel=1e-9)
    assert float(np.float32(1e12)) != 1e12
    p0 = fim.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], b, sc["prior_rec"], 0.0, 0.0)
    alone = fim.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"][:0], sc["info"][:0], b, sc["prior_rec"], 1e6, 1e12)
    assert np.array_equal(alone["H_diag"][b], np.diag([0.0] * 9 + [1e6] * 3 + [float(np.float32(1e12))] * 3)) and not alone["H_diag"][:b].any()
    out = fim.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], b, len(sc["recs"]))
    assert out["result"][4:6].tolist() == [0, 2] and np.array_equal(out["H_diag"], p0["H_diag"])


# ---- the closed loop ---------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = il.STATE + ("points", "total", "lam") + TRIAL
# Measured with `pytest tests/test_full_inertial_cpu.py -s -k spread`, which prints these lines: tests/test_inertial_loop_cpu.py's figures
# (RUNS model loops whose every trial output is multiplied by 1 + 1e-9 N(0, 1) against the unperturbed loop) for the scenes of
# tests/full_inertial_loop.py, those of the whole step on a map included.  The test holds a fresh measurement to within 2 x of these, either way.
MEASURED_SPREAD = {
    "full 4 63": {"Rwb": 3.04e-09, "twb": 2.43e-09, "v": 4.88e-09, "bg": 1.76e-09, "ba": 2.73e-09, "points": 6.40e-09, "total": 3.62e-07, "lam": 0.00e+00, "trial lam": 0.00e+00, "trial total": 1.04e-05, "trial scale": 1.14e-03},
    "full 3 65 free": {"Rwb": 5.72e-05, "twb": 1.90e-04, "v": 2.91e-04, "bg": 4.65e-07, "ba": 2.68e-09, "points": 9.58e-04, "total": 1.41e-05, "lam": None, "trial lam": 1.48e-04, "trial total": 9.15e-04, "trial scale": 3.69e-03},
    "per-state 3 63": {"Rwb": 3.31e-09, "twb": 7.84e-10, "v": 7.72e-09, "bg": 3.31e-09, "ba": 7.22e-08, "points": 9.61e-08, "total": 3.97e-08, "lam": None, "trial lam": 2.06e-03, "trial total": 1.62e-05, "trial scale": 2.22e-03},
    "chain 6 65": {"Rwb": 2.59e-09, "twb": 6.05e-09, "v": 7.32e-09, "bg": 3.90e-09, "ba": 2.07e-09, "points": 2.18e-08, "total": 1.71e-06, "lam": 0.00e+00, "trial lam": 0.00e+00, "trial total": 2.02e-04, "trial scale": 5.73e-03},
    "chain 6 1025": {"Rwb": 2.92e-09, "twb": 3.64e-09, "v": 4.91e-09, "bg": 2.17e-08, "ba": 1.58e-09, "points": 1.91e-08, "total": 9.55e-08, "lam": 2.96e-04, "trial lam": 2.96e-04, "trial total": 1.36e-05, "trial scale": 4.10e-04},
}


def measure(name):
    if name not in _cache:
        ref = fl.model_run(name)
        conv = name in fl.CONVERGED
        spread, runs = dict.fromkeys(OUTPUTS, 0.0), []
        last = lambda x: min([t[4] for t in x["rounds"][-1]["trace"] if t[-1]] + [x["rounds"][-1]["trace"][0][3]])  # noqa: E731
        for k in range(RUNS):
            r = fl.run(name, fl.model_backend(name, il.Noise(1000 + k)))
            runs.append(r)
            for o in il.STATE + ("points",):
                spread[o] = max(spread[o], _rel(r["estimate"][o], ref["estimate"][o]))
            spread["total"] = max(spread["total"], abs(last(r) - last(ref)) / last(ref))
            spread["lam"] = None if conv else max(spread["lam"], abs(r["rounds"][-1]["lam"] - ref["rounds"][-1]["lam"]) / ref["rounds"][-1]["lam"])
            for x, y in zip(r["rounds"], ref["rounds"]):
                flat = il.flat_from(y["trace"]) if conv else len(y["trace"])
                for a, b in zip(x["trace"][:flat], y["trace"][:flat]):
                    for key, dev in zip(TRIAL, trial_deviation(a, b)):
                        spread[key] = max(spread[key], dev)
        _cache[name] = (runs, spread)
    return _cache[name]


@pytest.mark.parametrize("name", list(fl.SCENES) + list(fl.CHAIN_SCENES))
def test_the_loop_scene_is_stable_and_the_spread_is_what_is_written(name):
    """THE CONDITION ON A SCENE, tests/test_inertial_loop_cpu.py's: a stage error of the size the stage tests allow (1e-9) in every trial
    output changes no decision, and no decision hangs on a rho below 1e-3; behind flat_from() a scene that reaches its minimum is exempt
    and only the estimate is compared.  A scene that fails this is changed, never the condition."""
    ref = fl.model_run(name)
    y = ref["rounds"][0]
    tr = y["trace"]
    best = min([t[4] for t in tr if t[-1]] + [tr[0][3]])
    print(name, il.decisions(ref["rounds"]), "iterations", y["iterations"], "robustified total %.10g -> %.10g, lambda %.3g" % (tr[0][3], best, y["lam"]))
    assert best < tr[0][3] and y["accepted"] >= 2 and ref["refused"] == 0
    flat = il.flat_from(tr)
    assert flat == len(tr) or name in fl.CONVERGED, (name, flat, [t[6] for t in tr])
    runs, spread = measure(name)
    for r in runs:
        x = r["rounds"][0]
        cut = flat if name in fl.CONVERGED else len(tr)
        assert il.decisions([x])[0][:cut] == il.decisions([y])[0][:cut], name
        if name not in fl.CONVERGED:
            assert x["iterations"] == y["iterations"] and len(x["trace"]) == len(tr)
    sc = fl.scene(name)
    if not sc["per_state"]:                                     # all key-frame states' bias dof stay zero, whatever the loop did
        assert not ref["estimate"]["bg"][:sc["n_kf"]].any() and not ref["estimate"]["ba"][:sc["n_kf"]].any()
        assert ref["estimate"]["bg"][sc["n_kf"]].tobytes() != sc["graph"].bg[sc["n_kf"]].tobytes()
    print('    "%s": {%s},' % (name, ", ".join('"%s": %s' % (k, "None" if v is None else "%.2e" % v) for k, v in spread.items())))
    assert name in MEASURED_SPREAD, "no figures written for this scene"
    for k, v in spread.items():
        w = MEASURED_SPREAD[name][k]
        assert (v is None and w is None) or w / 2 <= v <= 2 * w, (name, k, v, w)


@pytest.mark.parametrize("name", list(fl.CHAIN_SCENES))
def test_the_whole_step_in_the_models(name):
    """the model chain the GPU test of the whole step is held to: the assembly with all key frames as its window and full_inertial_model.jobs
    on it describe the shared-bias scene the model loop runs on (chain_map asserts the lists and the vertices bit for bit); behind the loop
    every key frame behind the fixed first one and every point moves, every record and every chained prior slot holds the ONE bias, and the
    oldest key frame's velo_priori is its recovered velocity"""
    cm = fl.chain_map(name)
    mp, a, fs = cm["map"], cm["a"], cm["fs"]
    n_kf = fl.CHAIN_KF
    assert a["result"][:4].tolist() == [n_kf, fl.CHAIN_SCENES[name][0], len(fs["w"]), n_kf] and fs["n_solve"] == n_kf + 1 and len(mp["n"]) == n_kf + 2
    est = fl.model_run(name)["estimate"]
    tail = fl.chain_tail(cm, est, [r.copy() for r in fs["recs"]])
    assert [int(v[0]) for v in tail["results"].values()] == [n_kf, 0, n_kf, n_kf - 1, 1] and tail["results"]["apply"][4] == len(a["point_row"])
    moved = [(tail["pose_R"][k] != mp["pose_R"][k]).any() or (tail["pose_t"][k] != mp["pose_t"][k]).any() for k in mp["window"]]
    assert all(moved[1:]) and (tail["points"][a["point_row"]] != mp["points"][a["point_row"]]).any(1).all()
    one = np.concatenate([est["bg"][n_kf], est["ba"][n_kf]]).astype(np.float32)
    assert (tail["bias"] == one).all() and one.tobytes() != fs["recs"][fs["prior_rec"]].updated_bias.tobytes()
    assert all(tail["bank"].recs[rec].updated_bias.tobytes() == one.tobytes() for rec in a["bias_ids"])
    assert tail["priors"][a["prior_jobs"][0, 1]]["velo_priori"].tobytes() == tail["src"][a["recover_jobs"][0, 1], 12:15].tobytes()
    assert all(tail["priors"][slot]["bias_priori"].tobytes() == one.tobytes() for slot in a["prior_info_jobs"][:, 0])
