"""The model of the visual edges on the inertial graph and of the damped step (tests/vi_model.py) judged without a GPU: the analytic
2 x 6 Jacobian against central differences through the body-frame update, the whole linearisation against an independent
object-style restatement (a CameraImuPose object with all four members, dense `@` products, one dense Hessian), the fixed mask, both
Huber branches, what the header's one canonicalisation changes, the ordered Cholesky against the equations with the normwise
backward-error bound, the fixed dof, the refusal, and one teacher-forced iteration."""
import numpy as np
import pytest

import factors_model as fm
import imu_model as im
import vi_model as vm

_cache = {}


def _scene(n_edges, model):
    key = (n_edges, model)
    if key not in _cache:
        _cache[key] = vm.pose_full_scene(n_edges, model=model)
    return _cache[key]


def _visual(sc, graph, mode=0, H_diag=None, b=None, active=None, delta=vm.HUBER_MONO):
    n = graph.n
    return vm.linearize(graph, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], sc["n_edges"], sc["points"], sc["z"], sc["w"], active, delta,
                        vm.CHI2_MONO, mode, np.zeros((n, 15, 15)) if H_diag is None else H_diag, np.zeros((n, 15)) if b is None else b)


# ---- the analytic Jacobian against central differences ---------------------------------------------------------------------------------
# measured with this file (largest |analytic - numeric| over the largest |entry| of the 2 x 6 Jacobians of 64 edges; step 1e-6 through
# factors_model.oplus, the body-frame update): Pinhole 6.2e-08, Kannala-Brandt 4.6e-08.  The bar is 4 x that.
MEASURED_FD = {0: 6.2e-08, 1: 4.6e-08}


def _errors_at(sc, dof, h):
    g = sc["graph"].copy()
    g.fixed[:] = 0
    dx = np.zeros((g.n, 15))
    dx[1, dof] = h
    fm.oplus(g, dx)
    Rcw, tcw, _, _ = vm.derive_pose(sc["cal"], g.Rwb[1], g.twb[1])
    return vm.edge_errors(sc["cam"], Rcw, tcw, sc["points"], sc["z"], sc["w"])[1]


@pytest.mark.parametrize("model", [0, 1])
def test_the_analytic_jacobian_agrees_with_central_differences(model):
    sc = _scene(64, model)
    g = sc["graph"]
    Rcw, tcw, Rcb, tbc = vm.derive_pose(sc["cal"], g.Rwb[1], g.twb[1])
    Pc, _, _ = vm.edge_errors(sc["cam"], Rcw, tcw, sc["points"], sc["z"], sc["w"])
    J = vm.edge_jacobian(sc["cam"], Rcb, tbc, Pc)
    h = 1e-6
    num = np.stack([(_errors_at(sc, dof, h) - _errors_at(sc, dof, -h)) / (2 * h) for dof in range(6)], 2)
    worst = np.abs(J - num).max() / np.abs(J).max()
    print("model %d: analytic vs central differences %.3g of the largest entry" % (model, worst))
    assert worst <= 4 * MEASURED_FD[model]


# ---- an independent object-style restatement ----------------------------------------------------------------------------------------------
class CameraImuPose:
    """G2oTypes.h:29-71 with its four members; the camera pose derived as update() derives it"""

    def __init__(self, cal, Rwb, twb):
        self.R_cb, self.t_cb = cal["Rcb"].astype(np.float64), cal["tcb"].astype(np.float64)
        T_bc_R = cal["Rcb"].astype(np.float32).T
        self.R_bc, self.t_bc = T_bc_R.astype(np.float64), (-T_bc_R @ cal["tcb"].astype(np.float32)).astype(np.float64)
        self.R_wb, self.t_wb = np.array(Rwb), np.array(twb)
        self.R_cw = self.R_cb @ self.R_wb.T
        self.t_cw = self.t_cb - self.R_cw @ self.t_wb

    def world_to_camera(self, Pw):
        return self.R_cw @ Pw + self.t_cw

    def imu_rotation_jacobian(self, Pc):
        x, y, z = self.R_bc @ Pc + self.t_bc
        return self.R_cb @ np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])

    def imu_translation_jacobian(self):
        return -self.R_cb


def _obj_project(cam, Pc):
    X, Y, Z = Pc
    if cam["model"] == 0:
        return np.array([cam["fx"] * X / Z + cam["cx"], cam["fy"] * Y / Z + cam["cy"]])
    rho = np.hypot(X, Y)
    th = np.arctan2(rho, Z)
    th_d = th * (1 + sum(k * th ** (2 * i + 2) for i, k in enumerate(cam["k"])))
    return np.array([cam["fx"] * th_d * X / rho + cam["cx"], cam["fy"] * th_d * Y / rho + cam["cy"]])


def _obj_proj_jacobian(cam, Pc):
    X, Y, Z = Pc
    if cam["model"] == 0:
        return np.array([[cam["fx"] / Z, 0, -cam["fx"] * X / Z ** 2], [0, cam["fy"] / Z, -cam["fy"] * Y / Z ** 2]])
    k = cam["k"]
    r2, d2 = X * X + Y * Y, X * X + Y * Y + Z * Z
    r = np.sqrt(r2)
    th = np.arctan2(r, Z)
    f = th * (1 + sum(kk * th ** (2 * i + 2) for i, kk in enumerate(k)))
    fd = 1 + sum((2 * i + 3) * kk * th ** (2 * i + 2) for i, kk in enumerate(k))
    A = fd * Z / (r2 * d2)
    B = f / r ** 3
    return np.diag([cam["fx"], cam["fy"]]) @ np.array([[A * X * X + B * Y * Y, (A - B) * X * Y, -fd * X / d2], [(A - B) * X * Y, A * Y * Y + B * X * X, -fd * Y / d2]])


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max())


@pytest.mark.parametrize("model", [0, 1])
def test_the_model_agrees_with_an_object_style_restatement(model):
    sc = _scene(400, model)
    g = sc["graph"]
    rng = np.random.RandomState(4)
    active = (rng.uniform(size=400) < 0.8).astype(np.uint8)
    o = _visual(sc, g, active=active)
    pose = CameraImuPose(sc["cal"], g.Rwb[1], g.twb[1])
    H, b, tot = np.zeros((6, 6)), np.zeros(6), np.zeros(2)
    err, chi2 = np.zeros((400, 2)), np.zeros(400)
    d = vm.HUBER_MONO
    for e in range(400):
        Pc = pose.world_to_camera(sc["points"][e])
        err[e] = sc["z"][e] - _obj_project(sc["cam"], Pc)
        Om = np.eye(2) * sc["w"][e]
        chi2[e] = err[e] @ Om @ err[e]
        if not active[e]:
            continue
        Jp = _obj_proj_jacobian(sc["cam"], Pc)
        J = np.hstack([-Jp @ pose.imu_rotation_jacobian(Pc), -Jp @ pose.imu_translation_jacobian()])
        rho, rw = (2 * np.sqrt(chi2[e]) * d - d * d, d / np.sqrt(chi2[e])) if chi2[e] > d * d else (chi2[e], 1.0)
        H += J.T @ (rw * Om) @ J
        b -= J.T @ (rw * Om) @ err[e]
        tot += (chi2[e], rho)
    worst = max(_rel(o["err"], err), _rel(o["chi2"], chi2), _rel(o["total"][0], tot), _rel(o["H_diag"][1, :6, :6], H), _rel(o["b"][1, :6], b))
    print("model %d: the model against the object-style restatement %.3g" % (model, worst))
    assert worst <= 1e-12
    assert np.array_equal(o["H_diag"][1], o["H_diag"][1].T) and not o["H_diag"][0].any() and not o["H_diag"][1, 6:].any() and not o["b"][1, 6:].any()


def test_the_fixed_mask_and_both_huber_branches():
    """a fixed pose adds nothing to H and b and still writes its errors, chi2 and totals; the scene holds edges on both sides of
    huber_delta^2 and of 5.991; without the kernel the robustified total is the plain one"""
    sc = _scene(400, 0)
    g = sc["graph"]
    free = _visual(sc, g)
    fixed_graph = g.copy()
    fixed_graph.fixed[1] |= fm.FIX_POSE
    H0, b0 = np.random.RandomState(1).normal(size=(2, 15, 15)), np.random.RandomState(2).normal(size=(2, 15))
    fx = _visual(sc, fixed_graph, H_diag=H0, b=b0)
    assert np.array_equal(fx["H_diag"], H0) and np.array_equal(fx["b"], b0)
    for k in ("err", "chi2", "total", "result"):
        assert np.array_equal(fx[k], free[k]), k
    added = _visual(sc, g, H_diag=H0, b=b0)
    mask = np.zeros((2, 15, 15), bool)
    mask[1, :6, :6] = True
    assert np.array_equal(added["H_diag"][~mask], H0[~mask]) and (added["H_diag"][mask] != H0[mask]).all()      # exactly its rows and columns
    assert np.array_equal(added["b"][0], b0[0]) and np.array_equal(added["b"][1, 6:], b0[1, 6:]) and (added["b"][1, :6] != b0[1, :6]).all()
    c2 = free["chi2"]
    assert (c2 > vm.HUBER_MONO ** 2).any() and (c2 <= vm.HUBER_MONO ** 2).any() and (c2 > vm.CHI2_MONO).any() and (c2 <= vm.CHI2_MONO).any()
    assert free["total"][0, 1] < free["total"][0, 0]
    plain = _visual(sc, g, delta=0.0)
    assert plain["total"][0, 0] == plain["total"][0, 1] == free["total"][0, 0]
    cls = _visual(sc, g, mode=2)
    assert np.array_equal(cls["active"], (c2 <= vm.CHI2_MONO).astype(np.uint8)) and cls["n_inliers"][0] == (c2 <= vm.CHI2_MONO).sum()
    assert np.array_equal(_visual(sc, g, mode=1)["total"], free["total"])


@pytest.mark.parametrize("model", [0, 1])
def test_the_canonicalisation_is_measured(model):
    """The reference keeps the frame's FLOAT T_cw = T_cb * T_wb.inverse() (Frame.cpp:65-71) until the first update; the header always
    derives the camera pose in double from (R_wb, t_wb).  What that changes at the first linearisation, printed (DESIGN.md quotes it):
    measured 400 edges, Pinhole: errors by at most 7.2e-5 px, chi2 by at most 9.5e-8 of the largest chi2, the robustified total by 7.7e-9
    of itself; Kannala-Brandt: 2.6e-5 px, 6.5e-8, 9.3e-9.  Both poses come from the same float T_wb, so the difference is float rounding
    of T_cw alone; it must stay far below the pixel noise (kp.size >= 31 px here)."""
    sc = _scene(400, model)
    g, cal = sc["graph"], sc["cal"]
    f = np.float32
    Rwb, twb = sc["src"][1][:9].reshape(3, 3).astype(f), sc["src"][1][9:12].astype(f)
    assert np.array_equal(Rwb.astype(np.float64), g.Rwb[1])                   # the graph starts from these floats
    Rcb, tcb = cal["Rcb"].astype(f), cal["tcb"].astype(f)
    Rcw_f = im.mm(Rcb, Rwb.T)
    tcw_f = im.mv(Rcb, im.mv(-Rwb.T, twb)) + tcb
    assert Rcw_f.dtype == f and tcw_f.dtype == f
    Rcw, tcw, _, _ = vm.derive_pose(cal, g.Rwb[1], g.twb[1])
    _, e0, c0 = vm.edge_errors(sc["cam"], Rcw_f.astype(np.float64), tcw_f.astype(np.float64), sc["points"], sc["z"], sc["w"])
    _, e1, c1 = vm.edge_errors(sc["cam"], Rcw, tcw, sc["points"], sc["z"], sc["w"])
    t0, t1 = vm.huber(c0, vm.HUBER_MONO)[0].sum(), vm.huber(c1, vm.HUBER_MONO)[0].sum()
    de, dc, dt = np.abs(e0 - e1).max(), np.abs(c0 - c1).max() / c1.max(), abs(t0 - t1) / t1
    print("model %d: float T_cw against the derived one: errors %.3g px, chi2 %.3g of the largest, robustified total %.3g of itself" % (model, de, dc, dt))
    assert de < 1e-2 and dc < 1e-4


# ---- the damped step ------------------------------------------------------------------------------------------------------------------------
def _tracker_system(inertial_only=False):
    """the assembled system of poseFullOptimize (state 0: velocity and biases free; state 1: pose and velocity free -- 18 free dof) or of
    poseInertialOptimize (both poses fixed, no visual edges -- 12 free dof)"""
    key = ("system", inertial_only)
    if key not in _cache:
        sc = _scene(400, 0)
        g = sc["graph"].copy()
        if inertial_only:
            g.fixed[1] |= fm.FIX_POSE
        oi = vm.inertial_linearize(sc, g)
        ov = _visual(sc, g, H_diag=oi["H_diag"], b=oi["b"])
        assert (~vm.dof_fixed(g.fixed)).sum() == (12 if inertial_only else 18)
        _cache[key] = (sc, g, oi, ov)
    return _cache[key]


@pytest.mark.parametrize("inertial_only", [False, True])
@pytest.mark.parametrize("damped", [False, True])
def test_the_ordered_cholesky_solves_the_equations(inertial_only, damped):
    """|(H + lambda I) dx - b|_inf within 4n(3n + 1) 2^-53 |H + lambda I|_inf |dx|_inf, n the dof count, at lambda = 0 and at tau * max
    H_jj; dx is exactly 0 on the fixed dof; the scale is g2o's"""
    sc, g, oi, ov = _tracker_system(inertial_only)
    _, out0, _ = vm.solve(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], 0.0)
    lam = vm.TAU * out0[1] if damped else 0.0
    dx, out, res = vm.solve(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], lam)
    A, rhs, fx, h_max, dropped = vm.assemble(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], lam)
    assert res.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and dropped == 0 and out[1] == h_max == out0[1] > 0 and out[2] > 0
    x = dx.reshape(-1)
    L = np.longdouble
    resid = float(np.abs(A.astype(L) @ x.astype(L) - rhs.astype(L)).max())
    bound = vm.backward_error_bound(A, x)
    print("inertial only %d, lambda %.3g: backward error %.3g, bound %.3g, smallest pivot %.3g" % (inertial_only, lam, resid, bound, out[2]))
    assert resid <= bound
    assert not x[fx].any() and np.array_equal(x[fx], np.zeros(fx.sum())) and x[~fx].all()
    assert np.isclose(out[0], x @ (lam * x + rhs), rtol=1e-12)
    cond = np.linalg.cond(A)                                                              # and it is the solution numpy finds, as far as the conditioning lets two solvers agree
    print("condition number %.3g" % cond)
    assert np.abs(x - np.linalg.solve(A, rhs)).max() <= 8 * cond * 2.0 ** -53 * np.abs(x).max()


def test_a_free_state_no_edge_touches_is_refused_at_lambda_zero():
    sc, g, oi, ov = _tracker_system()
    fixed = np.concatenate([g.fixed, [0]]).astype(np.uint8)
    H = np.concatenate([ov["H_diag"], np.zeros((1, 15, 15))])
    b = np.concatenate([ov["b"], np.zeros((1, 15))])
    dx, out, res = vm.solve(fixed, sc["edges"], len(sc["recs"]), H, oi["H_off"], b, 0.0)
    assert res.tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and not dx.any() and out[0] == 0 and out[2] == 0
    dx, out, res = vm.solve(fixed, sc["edges"], len(sc["recs"]), H, oi["H_off"], b, 1e-3)   # damped, the same system is solved
    assert res[vm.R_DONE] == 1 and not dx[2].any() and dx[1, :6].all()


def test_edges_on_one_pair_add_up_and_bad_edges_are_skipped():
    sc, g, oi, ov = _tracker_system()
    cap = len(sc["recs"])
    edges = np.array([(0, 1, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 0, 0), (0, 1, cap, 0), (0, 1, 0, 0)], fm.EDGE)
    B = oi["H_off"][0]
    H_off = np.stack([B, 0.5 * B.T, B, B, B, 0.25 * B])
    A, _, fx, _, dropped = vm.assemble(g.fixed, edges, cap, ov["H_diag"], H_off, ov["b"], 0.0)
    assert dropped == 3
    want = (B + 0.5 * B) + 0.25 * B
    free0, free1 = ~fx[:15], ~fx[15:]
    assert np.array_equal(A[:15, 15:][np.ix_(free0, free1)], want[np.ix_(free0, free1)]) and np.array_equal(A[15:, :15], A[:15, 15:].T)


def test_one_teacher_forced_iteration_lowers_the_robust_total():
    """linearise (inertial, then visual on top) -> solve at tau * max H_jj -> oplus -> the errors at the trial point: no decision is
    taken; the total simply has to come out lower on this scene"""
    sc, g, oi, ov = _tracker_system()
    before = oi["total"][1] + ov["total"][0, 1]
    _, out0, _ = vm.solve(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], 0.0)
    dx, out, _ = vm.solve(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], vm.TAU * out0[1])
    trial = g.copy()
    fm.oplus(trial, dx)
    after = vm.inertial_linearize(sc, trial, 1)["total"][1] + _visual(sc, trial, mode=1)["total"][0, 1]
    print("robust total %.6g -> %.6g, scale %.3g" % (before, after, out[0]))
    assert after < before and out[0] > 0
