"""tests/vw_model.py alone, without the library: the two EdgeMono Jacobians against central differences, the reduce -> solve -> backsub
path against an independent object-style restatement that solves ONE dense system over all unknowns, the window scenes' own
conditions, and the structure of the outputs (fixed states, symmetry, the distrusted edge lists, a singular point)."""
import numpy as np
import pytest

import factors_model as fm
import vi_model as vm
import vw_model as wm

_cache = {}
# central differences with h = 1e-6 against the analytic Jacobians, relative to the largest entry of the edge's Jacobian: measured
# 2.84e-8 (pose) and 1.06e-9 (point) for Pinhole, 3.24e-8 and 4.56e-9 for Kannala-Brandt over the 63- / 65-point scenes; the bars are 4 x
JACOBIAN_BAR = {0: (1.14e-7, 4.24e-9), 1: (1.30e-7, 1.83e-8)}
# the model's step in the dense system of the restatement, measured on the Pinhole (5 + 3 states, 65 points, lambda 1) and the
# Kannala-Brandt (2 + 1 states, 65 points, lambda 10) scene: the longdouble residual |A x - b|_inf / (|A|_inf |x|_inf) 2.33e-17 and 3.49e-17;
# computeScale against the dense solve's 7.91e-12 and 1.54e-12 relative; the step itself against np.linalg.solve's 1.34e-3 and 7.25e-4 of its
# largest entry -- the inertial information is 1e14 times lambda, so two backward-stable solves agree no better.  The bars are 4 x.
RESIDUAL_BAR, STEP_BAR, SCALE_BAR = {0: 9.32e-17, 1: 1.40e-16}, {0: 5.36e-3, 1: 2.90e-3}, {0: 3.17e-11, 1: 6.16e-12}


def _scene(*shape):
    if shape not in _cache:
        _cache[shape] = wm.window_scene(*shape)
    return _cache[shape]


def _lin(sc, g=None, points=None, mode=0, **over):
    g = sc["graph"] if g is None else g
    a = {k: over.get(k, sc[k]) for k in ("edge_state", "edge_point", "z", "w")}
    H, b = (np.zeros((g.n, 15, 15)), np.zeros((g.n, 15))) if mode == 0 else (None, None)
    return wm.linearize(g, sc["cal"], sc["cam"], sc["n_solve"], sc["points"] if points is None else points, a["edge_state"], a["edge_point"], a["z"], a["w"],
                        over.get("active"), mode=mode, H_diag=over.get("H0", H), b=over.get("b0", b))


# ---- the Jacobians ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n_points", [(0, 63), (1, 65)])
def test_both_jacobians_against_central_differences(model, n_points):
    sc = _scene(2, 1, n_points, 1, model)
    o = _lin(sc)
    st, h = sc["edge_state"], 1e-6
    ne = len(st)
    num_p, num_l = np.zeros((ne, 2, 6)), np.zeros((ne, 2, 3))
    for k in range(6):
        side = []
        for sign in (1.0, -1.0):
            g = sc["graph"].copy()
            dx = np.zeros((g.n, 15))
            dx[:sc["n_solve"], k] = sign * h
            fm.oplus(g, dx)
            side.append(_lin(sc, g, mode=1)["err"])
        num_p[:, :, k] = (side[0] - side[1]) / (2 * h)
    for k in range(3):
        side = []
        for sign in (1.0, -1.0):
            P = sc["points"].copy()
            P[:, k] += sign * h
            side.append(_lin(sc, points=P, mode=1)["err"])
        num_l[:, :, k] = (side[0] - side[1]) / (2 * h)
    free = st < sc["n_solve"]
    assert free.any() and (~free).any() and not o["Jp"][~free].any()
    dev_p = (np.abs(num_p - o["Jp"])[free].max((1, 2)) / np.abs(o["Jp"][free]).max((1, 2))).max()
    dev_l = (np.abs(num_l - o["Jl"]).max((1, 2)) / np.abs(o["Jl"]).max((1, 2))).max()
    print("model %d: pose Jacobian %.3g, point Jacobian %.3g of the edge's largest entry" % (model, dev_p, dev_l))
    assert dev_p <= JACOBIAN_BAR[model][0] and dev_l <= JACOBIAN_BAR[model][1]


# ---- the independent restatement ------------------------------------------------------------------------------------------------------------
class _EdgeMono:
    """G2oTypes.cpp:59-69 as an object with matrices: computeError, linearizeOplus"""

    def __init__(self, cal, cam, Rwb, twb, Pw, z, inv_sigma2):
        self.cam, self.z, self.info = cam, z, inv_sigma2 * np.eye(2)
        self.Rcb, self.tcb = cal["Rcb"].astype(np.float32).astype(float), cal["tcb"].astype(np.float32).astype(float)
        self.tbc = (-(cal["Rcb"].astype(np.float32).T) @ cal["tcb"].astype(np.float32)).astype(float)      # ImuCalib holds T_bc in float
        self.Rcw = self.Rcb @ Rwb.T
        self.tcw = self.tcb - self.Rcw @ twb
        self.Pc = self.Rcw @ Pw + self.tcw

    def error(self):
        return self.z - np.array(vm.project(self.cam, *self.Pc))

    def jacobians(self):
        Jproj = vm.proj_jacobian(self.cam, *self.Pc)
        Pb = self.Rcb.T @ self.Pc + self.tbc
        hat = np.array([[0, -Pb[2], Pb[1]], [Pb[2], 0, -Pb[0]], [-Pb[1], Pb[0], 0]])
        return np.hstack([-Jproj @ self.Rcb @ hat, Jproj @ self.Rcb]), -Jproj @ self.Rcw


def _dense_step(sc, lam):
    """ONE Hessian over the 15 n_solve + 3 m unknowns: the inertial part from factors_model (tests/test_factors_cpu.py holds it), every
    used EdgeMono added as J^T (w Omega) J, the fixed dof removed, lambda on the diagonal, np.linalg.solve"""
    g, ns, m = sc["graph"], sc["n_solve"], sc["n_points"]
    oi = vm.inertial_linearize(sc, g)
    n = 15 * ns + 3 * m
    H, b = np.zeros((n, n)), np.zeros(n)
    A, rhs, fx, _, _ = vm.assemble(g.fixed[:ns], sc["edges"], len(sc["recs"]), oi["H_diag"][:ns], oi["H_off"], oi["b"][:ns], 0.0)
    H[:15 * ns, :15 * ns], b[:15 * ns] = A, rhs
    for e in range(len(sc["w"])):
        s, l = int(sc["edge_state"][e]), int(sc["edge_point"][e])
        edge = _EdgeMono(sc["cal"], sc["cam"], g.Rwb[s], g.twb[s], sc["points"][l], sc["z"][e], sc["w"][e])
        err = edge.error()
        chi2 = err @ edge.info @ err
        rho1 = vm.HUBER_MONO / np.sqrt(chi2) if chi2 > vm.HUBER_MONO ** 2 else 1.0
        Jp, Jl = edge.jacobians()
        J = np.zeros((2, n))
        if s < ns and not int(g.fixed[s]) & fm.FIX_POSE:
            J[:, 15 * s:15 * s + 6] = Jp
        J[:, 15 * ns + 3 * l:15 * ns + 3 * l + 3] = Jl
        H += J.T @ (rho1 * edge.info) @ J
        b -= J.T @ (rho1 * edge.info) @ err
    keep = np.concatenate([~fx, np.ones(3 * m, bool)])
    Hk, bk = H[keep][:, keep], b[keep]
    x = np.zeros(n)
    x[keep] = np.linalg.solve(Hk + lam * np.eye(keep.sum()), bk)
    return Hk + lam * np.eye(keep.sum()), bk, keep, x, float(x @ (lam * x + np.where(keep, b, 0.0)))


@pytest.mark.parametrize("shape,lam", [((5, 3, 65, 1, 0), 1.0), ((2, 1, 65, 1, 1), 10.0)])
def test_reduce_solve_backsub_equal_one_dense_solve(shape, lam):
    sc = _scene(*shape)
    it = sc["first"] if lam == 1.0 else wm.iterate(sc, lam)
    A, b, keep, x_np, scale_np = _dense_step(sc, lam)
    x = np.concatenate([it["dx"].reshape(-1), it["backsub"]["xl"].reshape(-1)])
    assert not x[~keep].any()
    L = np.longdouble
    resid = float(np.abs(A.astype(L) @ x[keep].astype(L) - b.astype(L)).max() / (np.abs(A).sum(1).max() * np.abs(x).max()))
    step = float(np.abs(x - x_np).max() / np.abs(x_np).max())
    scale = it["scale"] + it["backsub"]["scale"]
    rel = abs(scale - scale_np) / abs(scale_np)
    print("%s: residual %.3g, step %.3g, computeScale %.10g against %.10g (%.3g)" % (shape, resid, step, scale, scale_np, rel))
    assert resid <= RESIDUAL_BAR[shape[4]] and step <= STEP_BAR[shape[4]] and rel <= SCALE_BAR[shape[4]]


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 0, 1, 1, 0), (2, 1, 63, 1, 0), (5, 3, 65, 1, 0), (3, 2, 1025, 1, 0), (4, 1, 20, 1, 0), (2, 1, 65, 1, 1)])
def test_the_window_scenes_hold_what_they_are_meant_to_hold(shape):
    """window_scene asserts its own conditions (both Huber branches, both sides of 5.991, a point with one observation, no pivot refused
    at lambda 1, an iteration that gains); here also its shape and that the gain is in the visual part too"""
    sc = _scene(*shape)
    n_solve, n_fixed, n_points = shape[:3]
    g, it = sc["graph"], sc["first"]
    assert g.n == n_solve + n_fixed and len(sc["points"]) == n_points and (g.fixed[:n_solve] == 0).all() and (g.fixed[n_solve:] == 15).all()
    assert np.array_equal(sc["points"], sc["points"].astype(np.float32).astype(np.float64)) and (np.diff(sc["edge_point"]) >= 0).all()
    assert len(sc["edges"]) == n_solve - 1 and (sc["edges"]["flags"] == fm.EDGE_WALKS).all() and sc["pjobs"]["mask"][0] & fm.PRIOR_ACC_GYRO_INFO
    assert it["visual1"]["total"][1] < it["visual"]["total"][1] and it["after"] < it["before"]
    assert it["visual"]["result"].tolist() == [len(sc["w"]), 0, 0, 0, 0, 0, 0, 0]


# ---- structure ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_fixed_state_receives_no_block_and_s_is_symmetric():
    sc = _scene(5, 3, 65, 1, 0)
    g = sc["graph"].copy()
    g.fixed[1] = fm.FIX_POSE
    rng = np.random.RandomState(4)
    H0 = rng.normal(0, 1.0, (g.n, 15, 15))
    H0, b0 = H0 + H0.transpose(0, 2, 1), rng.normal(0, 1.0, (g.n, 15))
    o = _lin(sc, g, H0=H0, b0=b0)
    st = sc["edge_state"]
    for s in range(g.n):
        touched = s < 5 and s != 1
        assert np.array_equal(o["H_diag"][s], H0[s]) != touched and np.array_equal(o["b"][s], b0[s]) != touched, s
        assert np.array_equal(o["H_diag"][s][6:], H0[s][6:]) and np.array_equal(o["H_diag"][s][:, 6:], H0[s][:, 6:]) and np.array_equal(o["b"][s][6:], b0[s][6:])
        assert o["Hlp"][st == s].any() == touched and (st == s).any()
    assert o["Hll"].any(1).all() and np.array_equal(o["Hll"].reshape(-1, 3, 3), o["Hll"].reshape(-1, 3, 3).transpose(0, 2, 1))
    oi = vm.inertial_linearize(sc, g)
    Hs = (o["H_diag"] + o["H_diag"].transpose(0, 2, 1)) / 2
    r = wm.reduce(5, g.fixed, sc["edges"], len(sc["recs"]), Hs, oi["H_off"], o["b"], 2.0, o["point_off"], st, o["Hll"], o["bl"], o["Hlp"], len(st))
    S = r["S"]
    assert np.array_equal(S, S.T)
    fx = vm.dof_fixed(g.fixed[:5])
    assert fx[15:21].all() and np.array_equal(S[fx][:, fx], np.eye(6)) and not S[fx][:, ~fx].any() and not r["rhs"][fx].any()
    base = vm.assemble(g.fixed[:5], sc["edges"], len(sc["recs"]), Hs[:5], oi["H_off"], o["b"][:5], 2.0)[0]
    changed = (S != base).reshape(5, 15, 5, 15)
    assert not changed[:, 6:].any() and not changed[:, :, :, 6:].any() and not changed[1].any() and not changed[:, :, 1].any()
    assert changed[0, :6, 0, :6].all() and changed[0, :6, 2, :6].any()


def test_distrusted_edge_lists_follow_the_headers_rules():
    sc = _scene(2, 1, 63, 1, 0)
    es, ep = sc["edge_state"].copy(), sc["edge_point"].copy()
    off, eff = wm.point_ranges([5, 3, -2, 70, 9, 9, 1 << 30], 10)
    assert eff.tolist() == [5, 5, 5, 9, 9, 9, 9] and off.tolist() == [0, 0, 0, 0, 0, 0, 3, 3, 3, 3, 7]
    es[[3, 50]] = [3, -1]
    k = int(np.nonzero(ep[1:] == ep[:-1])[0][-1])
    es[k + 1] = es[k]
    o = _lin(sc, edge_state=es)
    assert o["result"][:4].tolist() == [len(es) - 3, 2, 1, 0] and o["status"][[3, 50, k + 1]].tolist() == [wm.R_RANGE, wm.R_RANGE, wm.R_DUPLICATE]
    drop = o["status"] != 0
    assert not o["err"][drop].any() and not o["chi2"][drop].any() and not o["Hlp"][drop].any() and o["err"][~drop].all()
    extra = 257 - int((ep == 62).sum())
    long = dict(edge_state=np.concatenate([es, np.arange(extra, dtype=np.int32) % 3]), edge_point=np.concatenate([ep, np.full(extra, 62, np.int32)]),
                z=np.concatenate([sc["z"], np.tile(sc["z"][-1:], (extra, 1))]), w=np.concatenate([sc["w"], np.tile(sc["w"][-1:], extra)]))
    o2 = _lin(sc, **long)
    assert o2["result"][wm.R_REFUSED] == 1 and (o2["status"] == wm.R_REFUSED).sum() == 257 and not o2["Hll"][62].any() and not o2["bl"][62].any()
    assert np.array_equal(o2["Hll"][:62], o["Hll"][:62]) and o2["result"][wm.R_DONE] == o["result"][wm.R_DONE] - ((o["status"] == 0) & (ep == 62)).sum()


def test_lambda_0_with_a_point_seen_once_is_singular_and_the_step_leaves_it_alone():
    """H_ll of a point with one observation has rank 2: its determinant is 0 up to rounding, and the header's rule (not > 0) skips
    those whose rounding leaves it <= 0; with lambda > 0 none is skipped"""
    sc = _scene(2, 1, 63, 1, 0)
    o, oi = sc["first"]["visual"], sc["first"]["inertial"]
    st, ne = sc["edge_state"], len(sc["w"])
    single = np.bincount(sc["edge_point"], minlength=63) == 1
    r = wm.reduce(2, sc["graph"].fixed, sc["edges"], len(sc["recs"]), o["H_diag"], oi["H_off"], o["b"], 0.0, o["point_off"], st, o["Hll"], o["bl"], o["Hlp"], ne)
    sk = r["skipped"]
    assert sk.any() and single[sk].all() and r["result"][wm.R_POINT_SINGULAR] == sk.sum() and not r["Hll_inv"][sk].any() and not r["tl"][sk].any()
    dx = np.random.RandomState(5).normal(0, 1e-3, (2, 15))
    bs = wm.backsub(2, o["point_off"], st, o["Hlp"], r["Hll_inv"], o["bl"], dx, 0.0, sc["points"], ne)
    assert np.array_equal(bs["points_out"][sk], sc["points"][sk]) and not bs["xl"][sk].any() and bs["xl"][~sk].any(1).all()
    assert bs["result"].tolist() == [63 - sk.sum(), 0, 0, 0, 0, 0, sk.sum(), 0]
    assert not wm.reduce(2, sc["graph"].fixed, sc["edges"], len(sc["recs"]), o["H_diag"], oi["H_off"], o["b"], 1e-9, o["point_off"], st, o["Hll"], o["bl"], o["Hlp"],
                         ne)["skipped"].any()
