"""Optional second kernel set (local-BA linearisation).  CPU: the numpy oracle's analytic Jacobians against
numeric differences of the residual under the reference's update rules.  GPU: HIP kernels vs the oracle,
relative tolerance 1e-9 (f64; only the summation order differs)."""
import numpy as np
import pytest

from monoorbslam3_amd import synth

TOL = 1e-9
LM_TOL = 1e-6      # the local BA's poses and points after both LM rounds against oracle/ba_ref.py (relative, in the sense of _close)


def _close(a, b, tol=TOL):
    scale = max(np.abs(b).max(), 1e-30)
    return np.abs(a - b).max() <= tol * scale


def test_jacobians_match_numeric_differences():
    """KAT (10) of SURVEY 8c: J_point = de/dP, J_pose = de/d(delta) with T <- exp(delta) * T (rotation first)"""
    from oracle import ba_ref
    pr = synth.make_ba_problem(4, 40, seed=3)
    lin = ba_ref.linearize(pr["cam"], pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"],
                           pr["edge_point"], pr["edge_z"], pr["edge_inv_sigma2"], 0.0)
    R = pr["pose_R"].reshape(-1, 3, 3)
    h = 1e-6
    for e in range(0, len(pr["edge_pose"]), 7):
        ip, il = pr["edge_pose"][e], pr["edge_point"][e]
        z = pr["edge_z"][e:e + 1]

        def res(Rm, tv, P):
            return ba_ref.residual(pr["cam"], Rm[None], tv[None], P[None], z)[0][0]
        e0 = res(R[ip], pr["pose_t"][ip], pr["points"][il])
        assert np.allclose(e0, lin["error"][e])
        for k in range(3):
            d = np.zeros(3); d[k] = h
            num = (res(R[ip], pr["pose_t"][ip], pr["points"][il] + d) - res(R[ip], pr["pose_t"][ip], pr["points"][il] - d)) / (2 * h)
            assert np.allclose(num, lin["J_point"][e][:, k], rtol=1e-5, atol=1e-6)
        for k in range(6):
            d = np.zeros(6); d[k] = h
            Rp, tp = ba_ref.se3_exp(d)
            Rm, tm = ba_ref.se3_exp(-d)
            num = (res(Rp @ R[ip], Rp @ pr["pose_t"][ip] + tp, pr["points"][il]) -
                   res(Rm @ R[ip], Rm @ pr["pose_t"][ip] + tm, pr["points"][il])) / (2 * h)
            assert np.allclose(num, lin["J_pose"][e][:, k], rtol=1e-5, atol=1e-5)


def test_huber_and_fixed_blocks():
    from oracle import ba_ref
    from monoorbslam3_amd.ba import HUBER_MONO
    pr = synth.make_ba_problem(5, 60, seed=5, n_fixed=2)
    a = ba_ref.linearize(pr["cam"], pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"],
                         pr["edge_point"], pr["edge_z"], pr["edge_inv_sigma2"], HUBER_MONO)
    assert abs(HUBER_MONO ** 2 - 5.991) < 1e-5
    assert (a["chi2"] > 5.991).any() and (a["chi2"] < 5.991).any()      # both Huber branches exercised
    assert np.all(a["H_pp"][:2] == 0) and np.all(a["b_p"][:2] == 0)      # fixed key frames carry no pose blocks
    assert np.abs(a["H_pp"][2:]).max() > 0 and np.abs(a["H_ll"]).max() > 0
    assert np.allclose(a["H_pp"], a["H_pp"].transpose(0, 2, 1)) and np.allclose(a["H_ll"], a["H_ll"].transpose(0, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n_poses,n_points", [(20, 3000), (3, 17)])
def test_gpu_matches_oracle(n_poses, n_points):
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    pr = synth.make_ba_problem(n_poses, n_points, seed=11, n_fixed=min(4, n_poses - 1))
    ref = ba_ref.linearize(pr["cam"], pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"],
                           pr["edge_point"], pr["edge_z"], pr["edge_inv_sigma2"], ba.HUBER_MONO)
    got = ba.linearize(pr["cam"], pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"],
                       pr["edge_point"], pr["edge_z"], pr["edge_inv_sigma2"])
    for k in ("chi2", "error", "H_pp", "b_p", "H_ll", "b_l", "H_lp"):
        assert _close(got[k], ref[k]), k
    if n_points == 3000:
        assert len(pr["edge_pose"]) > 20000
        print("BA linearise: %d edges, %.3f ms on device" % (len(pr["edge_pose"]), got["kernel_ms"]))


# ---------------------------------------------------------------------------------------------------------------
# Levenberg-Marquardt with marginalised points (g2o's OptimizationAlgorithmLevenberg + BlockSolver_6_3)
def _perturbed(n_poses, n_points, seed, outliers=0, rot=0.01, trans=0.05, pts=0.05, camera="pinhole"):
    from oracle import ba_ref
    pr = synth.make_ba_problem(n_poses, n_points, seed=seed, n_fixed=min(2, n_poses - 1), camera=camera)
    rng = np.random.RandomState(seed)
    R = np.array(pr["pose_R"]).reshape(-1, 3, 3).copy()
    t = np.array(pr["pose_t"]).reshape(-1, 3).copy()
    P = np.array(pr["points"]).reshape(-1, 3).copy()
    for i in np.flatnonzero(~np.asarray(pr["pose_fixed"], bool)):
        dR, dt = ba_ref.se3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))
        R[i], t[i] = dR @ R[i], dR @ t[i] + dt
    P += rng.normal(0, pts, P.shape)
    z = np.array(pr["edge_z"]).reshape(-1, 2).copy()
    if outliers:
        bad = rng.choice(len(z), outliers, replace=False)
        z[bad] += rng.uniform(15, 60, (outliers, 2)) * rng.choice([-1, 1], (outliers, 2))
    args = (pr["cam"], R, t, pr["pose_fixed"], P, pr["edge_pose"], pr["edge_point"], z, pr["edge_inv_sigma2"])
    return pr, args


def test_oracle_lm_converges_and_keeps_fixed_poses():
    from oracle import ba_ref
    pr, args = _perturbed(6, 200, 3)
    out = ba_ref.lm_optimize(*args, float(np.sqrt(np.float32(5.991))), 10)
    n_edges = len(pr["edge_pose"])
    assert out["chi2_final"] < 0.15 * out["chi2_initial"]
    assert out["chi2_final"] < 2.5 * n_edges  # 1-px noise at 1/sigma^2 <= 1: about two per edge at most
    fixed = np.asarray(pr["pose_fixed"], bool)
    assert np.array_equal(out["pose_R"][fixed], np.asarray(args[1])[fixed]) and np.array_equal(out["pose_t"][fixed], args[2][fixed])
    # (depth along the viewing rays is weakly constrained with 1-px noise, so the distance to the generating points
    #  is not a criterion; the reprojection error is)
    # rotations stay orthonormal
    assert np.abs(out["pose_R"] @ out["pose_R"].transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


def test_oracle_se3_exp_is_a_rigid_motion():
    from oracle import ba_ref
    for upd in (np.zeros(6), np.array([1e-7, -2e-7, 3e-7, 0.1, 0.2, 0.3]), np.array([0.3, -0.2, 0.1, 1, 2, 3])):
        R, t = ba_ref.se3_exp(upd)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.allclose(ba_ref.se3_exp(np.array([0, 0, 0, 1, 2, 3.0]))[1], [1, 2, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("n_poses,n_points,huber", [(6, 200, True), (6, 200, False), (20, 3000, True), (25, 600, True), (26, 600, True)])
def test_gpu_lm_matches_oracle(chol, n_poses, n_points, huber):
    """Same LM decisions (iteration / trial counts), estimates within 1e-6 relative of the numpy restatement: the two
    differ only in summation order and in the dense Cholesky -- through the LDS-resident solver (the reduced system of up to 23
    free key frames; 25 poses = 23 free ones is its largest case) and through the global-memory one (ORBBA_VAR_CHOL = 1, and
    what 26 poses take either way)."""
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    ba.set_variant("chol", chol)  # read per call
    pr, args = _perturbed(n_poses, n_points, 5)
    delta = ba.HUBER_MONO if huber else 0.0
    ref = ba_ref.lm_optimize(*args, delta, 6)
    got = ba.optimize(*args, huber_delta=delta, iterations=6)
    assert (got["iterations"], got["trials"]) == (ref["iterations"], ref["trials"])
    assert abs(got["chi2_initial"] - ref["chi2_initial"]) <= 1e-9 * ref["chi2_initial"]
    assert abs(got["chi2_final"] - ref["chi2_final"]) <= 1e-6 * ref["chi2_final"]
    assert abs(got["lam"] - ref["lam"]) <= 1e-6 * ref["lam"]
    for k in ("pose_R", "pose_t", "points"):
        assert _close(got[k], ref[k], 1e-6), k
    assert _close(got["chi2"], ref["chi2"], 1e-5)
    assert got["chi2_final"] < 0.2 * got["chi2_initial"]
    if n_points == 3000:
        print("BA LM: %d edges, %d iterations / %d solves, %.2f ms on device" %
              (len(pr["edge_pose"]), got["iterations"], got["trials"], got["device_ms"]))
    ba.set_variant("chol", "lds")


@pytest.mark.gpu
def test_gpu_local_bundle_adjustment_rejects_outliers():
    """Optimize.cpp:892-922 end to end: 40 gross outliers among ~1000 observations are flagged, the rest fit."""
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    pr, args = _perturbed(6, 200, 9, outliers=40)
    ref = ba_ref.local_bundle_adjustment(*args, ba.HUBER_MONO)
    got = ba.local_bundle_adjustment(*args)
    # 40 gross outliers + the ~5 % tail of the 1-px noise beyond chi2 = 5.991
    assert np.array_equal(got["outlier"], ref["outlier"]) and 40 <= got["outlier"].sum() <= 100
    assert abs(got["chi2_final"] - ref["chi2_final"]) <= 1e-6 * ref["chi2_final"]
    for k in ("pose_R", "pose_t", "points"):
        assert _close(got[k], ref[k], LM_TOL), k
    assert got["chi2_final"] < 2.5 * (~got["outlier"]).sum()
    # An edge demoted after the first round stays an outlier even when its residual at the final estimate drops back
    # under 5.991: g2o does not recompute a level-1 edge's error, so e->chi2() at Optimize.cpp:919 is the stale value.
    demoted = ref["first_round"]["chi2"] > 5.991
    back = demoted & (ref["chi2_final_estimate"] <= 5.991)
    assert back.sum() >= 1 and got["outlier"][back].all() and got["outlier"][demoted].all()
    assert _close(got["chi2"][demoted], ref["first_round"]["chi2"][demoted], 1e-5) and (got["chi2"][demoted] > 5.991).all()
    assert _close(got["chi2"], ref["chi2"], 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("scene", ["easy", "first_round_rejects"])
def test_gpu_local_bundle_adjustment_equals_its_composition(scene, chol):
    """orbba_local_bundle_adjustment runs both rounds of Optimize.cpp:892-922 in one arena behind one upload.  What it returns equals,
    BYTE FOR BYTE, the same rounds composed through the public API: optimize(5); the mask !(chi2 > 5.991); optimize(10) without the robust
    kernel on that mask, from the first round's estimates; the first round's chi2 kept for the demoted edges; the outlier rule; iterations
    and trials summed; chi2_initial of the first round.  No tolerance: the same kernels run in the same order on the same index arrays."""
    from monoorbslam3_amd import ba
    if scene == "easy":
        args = _perturbed(4, 40, 3, outliers=4)[1]
    else:
        from test_ba_lm_paths import _local_ba_args
        args = _local_ba_args()
    ba.set_variant("chol", chol)  # read per call
    try:
        got = ba.local_bundle_adjustment(*args)
        r1 = ba.optimize(*args, iterations=5)
        mask = ~(r1["chi2"] > 5.991)
        r2 = ba.optimize(args[0], r1["pose_R"], r1["pose_t"], args[3], r1["points"], *args[5:], huber_delta=0.0, iterations=10, edge_active=mask)
    finally:
        ba.set_variant("chol", "lds")
    chi2 = np.where(mask, r2["chi2"], r1["chi2"])
    print("%s %s: rounds %d / %d and %d / %d, %d demoted, %d outliers" % (scene, chol, r1["iterations"], r1["trials"], r2["iterations"], r2["trials"],
                                                                       (~mask).sum(), got["outlier"].sum()))
    assert (~mask).any() and mask.any()
    if scene == "first_round_rejects":
        assert r1["trials"] > r1["iterations"]
    for k in ("pose_R", "pose_t", "points"):
        assert got[k].tobytes() == r2[k].tobytes(), k
    assert got["chi2"].tobytes() == chi2.tobytes()
    assert np.array_equal(got["outlier"], ~mask | (chi2 > 5.991))
    assert (got["iterations"], got["trials"]) == (r1["iterations"] + r2["iterations"], r1["trials"] + r2["trials"])
    for k, want in (("lam", r2["lam"]), ("chi2_initial", r1["chi2_initial"]), ("chi2_final", r2["chi2_final"])):
        assert np.float64(got[k]).tobytes() == np.float64(want).tobytes(), k


@pytest.mark.gpu
def test_gpu_local_bundle_adjustment_takes_null_outputs():
    """the C call with outlier, r->chi2 and r->pose_R NULL: OK, and pose_t, points and the scalars are the full call's bytes"""
    import ctypes as C
    from monoorbslam3_amd import ba
    _, args = _perturbed(3, 10, 1)
    full = ba.local_bundle_adjustment(*args)
    prob, keep = ba._problem(*args, ba.HUBER_MONO)
    out, res = ba._lm_out(prob)
    res.pose_R = res.chi2 = None
    assert ba._L().orbba_local_bundle_adjustment(C.byref(prob), C.byref(res), None, -1) == 0
    assert out["pose_t"].tobytes() == full["pose_t"].tobytes() and out["points"].tobytes() == full["points"].tobytes()
    assert not out["pose_R"].any() and not out["chi2"].any()      # as passed
    assert (res.iterations, res.trials) == (full["iterations"], full["trials"])
    for k in ("lam", "chi2_initial", "chi2_final"):
        assert np.float64(getattr(res, k)).tobytes() == np.float64(full[k]).tobytes(), k


@pytest.mark.gpu
def test_gpu_lm_argument_errors():
    from monoorbslam3_amd import ba
    pr, args = _perturbed(4, 30, 2)
    all_fixed = list(args)
    all_fixed[3] = np.ones(4, np.uint8)
    with pytest.raises(Exception, match="fixed"):
        ba.optimize(*all_fixed)
    unsorted_edges = list(args)
    unsorted_edges[6] = np.asarray(args[6])[::-1].copy()
    with pytest.raises(Exception, match="grouped by point"):
        ba.optimize(*unsorted_edges)


@pytest.mark.gpu
def test_gpu_ba_entry_points_lease_their_workspace():
    """include/orbba.h, "Threads": every host-pointer BA call leases a stream, a device arena and a page-locked staging block from a
    per-device pool.  A problem without edges (the arena's edge blocks are empty), calls of growing and shrinking size through one
    workspace (the arena grows, a smaller call then runs inside the larger one), and four host threads calling at once (ctypes releases
    the GIL: four leases in flight) -- every answer equals the one the same call gives alone."""
    import threading
    from monoorbslam3_amd import ba
    # no edges: H and b are zero, nothing is read or written out of bounds
    pr, args = _perturbed(3, 10, 1)
    none = list(args)
    none[5] = np.zeros(0, np.int32); none[6] = np.zeros(0, np.int32); none[7] = np.zeros((0, 2)); none[8] = np.zeros(0)
    g = ba.linearize(*none)
    assert not g["H_pp"].any() and not g["b_p"].any() and not g["H_ll"].any() and not g["b_l"].any() and g["chi2"].size == 0
    # small, large, small again: the second small call reuses the grown arena and gives the first one's bytes
    _, small = _perturbed(4, 40, 3)
    _, large = _perturbed(20, 3000, 5)
    a = ba.local_bundle_adjustment(*small)
    big = ba.local_bundle_adjustment(*large)
    b2 = ba.local_bundle_adjustment(*small)
    for k in ("pose_R", "pose_t", "points", "chi2", "outlier"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b2[k]).tobytes(), k
    assert a["iterations"] == b2["iterations"] and big["iterations"] >= 1
    lin = ba.linearize(*large)
    # four threads: two local BAs, a linearisation and a batch of pose optimisations, three rounds each
    cam, R0, t0, off, P, Z, W = _pose_frames([300, 0, 2, 700], 9)
    pose_ref = ba.pose_optimize_batch(cam, R0, t0, off, P, Z, W)
    bad = []

    def run(kind):
        for _ in range(3):
            if kind == 0:
                got = ba.local_bundle_adjustment(*small)
                ok = all(np.asarray(got[k]).tobytes() == np.asarray(a[k]).tobytes() for k in ("pose_R", "pose_t", "points", "chi2", "outlier"))
            elif kind == 1:
                got = ba.local_bundle_adjustment(*large)
                ok = all(np.asarray(got[k]).tobytes() == np.asarray(big[k]).tobytes() for k in ("pose_R", "pose_t", "points", "chi2", "outlier"))
            elif kind == 2:
                got = ba.linearize(*large)
                ok = all(got[k].tobytes() == lin[k].tobytes() for k in ("chi2", "error", "H_pp", "b_p", "H_ll", "b_l", "H_lp"))
            else:
                got = ba.pose_optimize_batch(cam, R0, t0, off, P, Z, W)
                ok = all(np.asarray(got[k]).tobytes() == np.asarray(pose_ref[k]).tobytes() for k in ("pose_R", "pose_t", "inlier", "n_inliers", "chi2"))
            if not ok:
                bad.append(kind)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------
# Optimize::poseOptimize for a batch of frames (a14b)
def _pose_frames(sizes, seed, outlier_frac=0.1, rot=0.01, trans=0.05, depth=(6, 30)):
    """Per frame: a true pose, points in front of it, exact projections + noise of one pixel times the level scale,
    weights 1/scale^2, a share of gross outliers, and a perturbed initial pose (sigmas rot rad / trans m).  depth: the range
    of the points' depths; their lateral spread shrinks with its upper end, so they stay inside the same field of view."""
    from oracle import ba_ref
    cam = (718.856, 718.856, 607.19, 185.22)
    rng = np.random.RandomState(seed)
    R0, t0, P, Z, W, off = [], [], [], [], [], [0]
    for n in sizes:
        Rt, tt = ba_ref.se3_exp(np.concatenate([rng.normal(0, 0.2, 3), rng.normal(0, 1.0, 3)]))
        Pc = np.stack([rng.uniform(-8, 8, n) * depth[1] / 30, rng.uniform(-3, 3, n) * depth[1] / 30, rng.uniform(depth[0], depth[1], n)], 1)
        Pw = (Pc - tt) @ Rt  # Pc = R Pw + t
        scale = 1.2 ** rng.randint(0, 8, n)
        z = np.stack([cam[0] * Pc[:, 0] / Pc[:, 2] + cam[2], cam[1] * Pc[:, 1] / Pc[:, 2] + cam[3]], 1)
        z += rng.normal(0, 1, (n, 2)) * scale[:, None]
        bad = rng.uniform(size=n) < outlier_frac
        z[bad] += rng.uniform(15, 80, (int(bad.sum()), 2)) * rng.choice([-1, 1], (int(bad.sum()), 2))
        dR, dt = ba_ref.se3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))
        R0.append(dR @ Rt); t0.append(dR @ tt + dt)
        P.append(Pw); Z.append(z); W.append(1.0 / (scale * scale)); off.append(off[-1] + n)
    cat = lambda xs, w: np.concatenate(xs) if off[-1] else np.zeros((0, w))  # noqa: E731
    return cam, np.array(R0), np.array(t0), np.array(off, np.int32), cat(P, 3), cat(Z, 2), np.concatenate(W) if off[-1] else np.zeros(0)


def test_oracle_pose_optimize_recovers_pose_and_flags_outliers():
    from oracle import ba_ref
    cam, R0, t0, off, P, Z, W = _pose_frames([400], 3)
    out = ba_ref.pose_optimize(cam, R0[0], t0[0], P, Z, W, float(np.sqrt(np.float32(5.991))))
    chi0 = ba_ref.pose_optimize(cam, R0[0], t0[0], P, Z, W, float(np.sqrt(np.float32(5.991))), rounds=0)["chi2"]
    assert np.median(out["chi2"]) < 0.2 * np.median(chi0)
    assert 0.8 * 400 < out["n_inliers"] < 0.93 * 400  # ~10 % gross outliers + the 5 % tail of the noise
    assert ba_ref.pose_optimize(cam, R0[0], t0[0], P[:2], Z[:2], W[:2], 2.4)["n_inliers"] == 0  # :491


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [3000, 1000, 0])
def test_gpu_pose_optimize_batch_matches_oracle(lds):
    """Optimize.cpp:447-540 for a batch of frames: edges staged in LDS (ORBBA_VAR_POSE_LDS = capacity in edges; 1000: the two larger
    frames of the batch keep reading global memory beside the staged ones; 0: every frame does -- the parity twin)."""
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    ba.set_variant("pose_lds", lds)  # read per call
    sizes = [300, 1500, 2, 0, 64, 257, 2000, 3]
    cam, R0, t0, off, P, Z, W = _pose_frames(sizes, 17)
    got = ba.pose_optimize_batch(cam, R0, t0, off, P, Z, W)
    for f, n in enumerate(sizes):
        sl = slice(off[f], off[f + 1])
        ref = ba_ref.pose_optimize(cam, R0[f], t0[f], P[sl], Z[sl], W[sl], ba.HUBER_MONO)
        assert got["n_inliers"][f] == ref["n_inliers"], f
        if n >= 3:
            assert np.array_equal(got["inlier"][sl], ref["inlier"]), f
        assert _close(got["pose_R"][f], ref["R"], 1e-7) and _close(got["pose_t"][f], ref["t"], 1e-6), f
        if n:
            assert _close(got["chi2"][sl], ref["chi2"], 1e-5), f
    assert got["n_inliers"][2] == 0 and got["n_inliers"][3] == 0
    assert np.array_equal(got["pose_R"][2], R0[2]) and np.array_equal(got["pose_t"][3], t0[3])
    # throughput shape: 256 frames x 1000 correspondences in one launch
    cam, R0, t0, off, P, Z, W = _pose_frames([1000] * 256, 5)
    big = ba.pose_optimize_batch(cam, R0, t0, off, P, Z, W)
    assert (big["n_inliers"] > 800).all()
    print("poseOptimize: 256 frames x 1000 edges in %.3f ms (%.1f us/frame)" % (big["kernel_ms"], big["kernel_ms"] * 1e3 / 256))
    ba.set_variant("pose_lds", 3000)


def test_oracle_lm_reaches_the_same_minimum_as_scipy():
    """Independent check of the restated solver: without the robust kernel the LM loop and scipy's trust-region
    least squares (its own Jacobian by finite differences, its own parameterisation through se3_exp) must end in the
    same minimum of sum w |z - project(R P + t)|^2."""
    from scipy.optimize import least_squares
    from oracle import ba_ref
    pr, args = _perturbed(4, 40, 21)
    cam, R0, t0, fixed, P0, ep, el, z, w = args
    fixed = np.asarray(fixed, bool)
    free = np.flatnonzero(~fixed)
    ep, el, z, w = np.asarray(ep), np.asarray(el), np.asarray(z, np.float64).reshape(-1, 2), np.asarray(w, np.float64)
    ref = ba_ref.lm_optimize(cam, R0, t0, fixed, P0, ep, el, z, w, 0.0, 60)

    def unpack(x):
        R, t = R0.copy(), t0.copy()
        for i, ip in enumerate(free):
            dR, dt = ba_ref.se3_exp(x[6 * i:6 * i + 6])
            R[ip], t[ip] = dR @ R0[ip], dR @ t0[ip] + dt
        return R, t, P0 + x[6 * len(free):].reshape(-1, 3)

    def fun(x):
        R, t, P = unpack(x)
        e, _ = ba_ref.residual(cam, R[ep], t[ep], P[el], z)
        return (np.sqrt(w)[:, None] * e).ravel()

    sol = least_squares(fun, np.zeros(6 * len(free) + P0.size), method="trf", xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=400)
    cost_scipy = float((sol.fun ** 2).sum())
    assert abs(ref["chi2_final"] - cost_scipy) <= 1e-6 * cost_scipy
    R, t, P = unpack(sol.x)
    e_ref, _ = ba_ref.residual(cam, ref["pose_R"][ep], ref["pose_t"][ep], ref["points"][el], z)
    e_sp, _ = ba_ref.residual(cam, R[ep], t[ep], P[el], z)
    assert np.abs(e_ref - e_sp).max() < 1e-3  # same reprojections (the gauge along the fixed poses is pinned by them)


# ---------------------------------------------------------------- the Fisheye camera (modules/Sensor/Fisheye.cpp:35-108)
def test_fisheye_jacobian_matches_numeric_differences():
    """Fisheye::getProjJacobian (Fisheye.cpp:83-108) against central differences of Fisheye::project (:35-49), and the
    edge Jacobians built from it (G2oTypes.cpp:42-46) against differences of the residual."""
    from oracle import ba_ref
    pr = synth.make_ba_problem(4, 60, seed=8, camera="fisheye")
    cam = pr["cam"]
    assert len(cam) == 8 and len(pr["edge_pose"]) > 100
    rng = np.random.RandomState(2)
    Pc = np.stack([rng.uniform(-6, 6, 50), rng.uniform(-6, 6, 50), rng.uniform(2, 9, 50)], 1)   # up to ~70 degrees off axis
    J = ba_ref.proj_jacobian(cam, Pc)
    h = 1e-6
    for k in range(3):
        d = np.zeros(3); d[k] = h
        num = (ba_ref.project(cam, Pc + d) - ba_ref.project(cam, Pc - d)) / (2 * h)
        assert np.allclose(num, J[:, :, k], rtol=1e-6, atol=1e-6)
    lin = ba_ref.linearize(cam, pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"], pr["edge_point"],
                           pr["edge_z"], pr["edge_inv_sigma2"], 0.0)
    R = pr["pose_R"].reshape(-1, 3, 3)
    for e in range(0, len(pr["edge_pose"]), 11):
        ip, il = pr["edge_pose"][e], pr["edge_point"][e]
        z = pr["edge_z"][e:e + 1]
        res = lambda Rm, tv, P: ba_ref.residual(cam, Rm[None], tv[None], P[None], z)[0][0]  # noqa: E731
        for k in range(6):
            d = np.zeros(6); d[k] = h
            Rp, tp = ba_ref.se3_exp(d)
            Rm, tm = ba_ref.se3_exp(-d)
            num = (res(Rp @ R[ip], Rp @ pr["pose_t"][ip] + tp, pr["points"][il]) -
                   res(Rm @ R[ip], Rm @ pr["pose_t"][ip] + tm, pr["points"][il])) / (2 * h)
            assert np.allclose(num, lin["J_pose"][e][:, k], rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_gpu_fisheye_matches_oracle():
    """The three BA entry points with camera_model = 1: linearisation blocks, the LM loop and the batched poseOptimize
    against the numpy oracle (float64; tolerances as for the pinhole tests -- atan / atan2 / sqrt are the device's)."""
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    pr = synth.make_ba_problem(6, 400, seed=4, camera="fisheye")
    cam = pr["cam"]
    args = (cam, pr["pose_R"], pr["pose_t"], pr["pose_fixed"], pr["points"], pr["edge_pose"], pr["edge_point"], pr["edge_z"],
            pr["edge_inv_sigma2"])
    want = ba_ref.linearize(*args, ba.HUBER_MONO)
    got = ba.linearize(*args, ba.HUBER_MONO)
    for k in ("chi2", "error", "H_pp", "b_p", "H_ll", "b_l", "H_lp"):
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert np.abs(got[k] - want[k]).max() <= 1e-9 * scale, k
    # the pinhole path is untouched by the new field: same problem geometry through the pinhole model differs
    pin = ba.linearize(cam[:4], *args[1:], ba.HUBER_MONO)
    assert np.abs(pin["error"] - got["error"]).max() > 1.0
    w_lm = ba_ref.lm_optimize(*args, ba.HUBER_MONO, 5)
    g_lm = ba.optimize(*args, huber_delta=ba.HUBER_MONO, iterations=5)
    assert (g_lm["iterations"], g_lm["trials"]) == (w_lm["iterations"], w_lm["trials"])
    for k in ("pose_R", "pose_t", "points"):
        assert _close(g_lm[k], w_lm[k], 1e-6), k
    assert g_lm["chi2_final"] < g_lm["chi2_initial"]
    # poseOptimize: every pose against the points it observes
    R = pr["pose_R"].reshape(-1, 3, 3)
    off, P, z, w = [0], [], [], []
    for k in range(len(R)):
        sel = np.flatnonzero(pr["edge_pose"] == k)
        P.append(pr["points"][pr["edge_point"][sel]]); z.append(pr["edge_z"][sel]); w.append(pr["edge_inv_sigma2"][sel])
        off.append(off[-1] + len(sel))
    P, z, w = np.concatenate(P), np.concatenate(z), np.concatenate(w)
    t0 = pr["pose_t"] + 0.02
    out = ba.pose_optimize_batch(cam, R, t0, np.array(off, np.int32), P, z, w)
    for k in range(len(R)):
        ref = ba_ref.pose_optimize(cam, R[k], t0[k], P[off[k]:off[k + 1]], z[off[k]:off[k + 1]], w[off[k]:off[k + 1]], ba.HUBER_MONO)
        assert np.abs(out["pose_t"][k] - ref["t"]).max() < 1e-7 and np.abs(out["pose_R"][k] - ref["R"]).max() < 1e-8
        assert out["n_inliers"][k] == ref["n_inliers"]
