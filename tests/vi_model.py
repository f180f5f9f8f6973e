"""Plain numpy restatement of include/orbvi.h: EdgeMonoOnlyPose on the VertexPose of a factors_model.Graph (reference
modules/Backend/G2oTypes.cpp:49-57, G2oTypes.h:41-54), its quadratic form with g2o's Huber rule summed in the order the header fixes
(a thread's edges t, t + 1024, ..., the wave butterfly, the sixteen waves ascending), the inlier classification of
Optimize.cpp:722-735, and the damped step: the assembly of the 15n x 15n system and the ordered Cholesky with its two substitutions.
float64 throughout except t_bc, which is ImuCalib's float Pose::inverse; no `@`, every sum written out in the header's order.  The
graph, oplus and the inertial scenes come from factors_model / imu_model.  The seeded visual scene lives here and asserts that it
holds what it is meant to hold.  No part of the library is used here."""
import numpy as np

import factors_model as fm
import imu_model as im

F64 = np.float64
MAX_STATES = 4
EDGE_WORK = 16
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_NONFINITE = 0, 1, 2, 3, 4
HUBER_MONO = float(np.sqrt(np.float32(5.991)))          # (double)sqrtf(5.991), Optimize.cpp:683
CHI2_MONO = 5.991                                       # Optimize.cpp:728
TAU = 1e-5                                              # g2o's computeLambdaInit
THREADS, WAVES = 1024, 16

PINHOLE = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, model=0, k=(0.0, 0.0, 0.0, 0.0))
FISHEYE = dict(fx=190.978, fy=190.973, cx=254.932, cy=256.897, model=1, k=(0.0034, 0.0007, -0.0020, 0.0002))


# ---- the camera (csrc/orbba_camera.h: the same expressions, Python's precedence is C's) ----------------------------------------------------
def project(cam, X, Y, Z):
    fx, fy, cx, cy, k = cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k"]
    with np.errstate(all="ignore"):
        if cam["model"] == 0:
            return fx * (X / Z) + cx, fy * (Y / Z) + cy
        a, b = X / Z, Y / Z
        r = np.sqrt(a * a + b * b)
        theta = np.arctan(r)
        theta2 = theta * theta
        theta3 = theta * theta2
        theta5 = theta2 * theta3
        theta7 = theta2 * theta5
        theta9 = theta2 * theta7
        theta_d = theta + k[0] * theta3 + k[1] * theta5 + k[2] * theta7 + k[3] * theta9
        return fx * theta_d * a / r + cx, fy * theta_d * b / r + cy


def proj_jacobian(cam, X, Y, Z):
    """[n, 2, 3]"""
    fx, fy, k = cam["fx"], cam["fy"], cam["k"]
    Jp = np.zeros(np.shape(X) + (2, 3))
    with np.errstate(all="ignore"):
        if cam["model"] == 0:
            Jp[..., 0, 0], Jp[..., 0, 2] = fx / Z, -fx * X / (Z * Z)
            Jp[..., 1, 1], Jp[..., 1, 2] = fy / Z, -fy * Y / (Z * Z)
            return Jp
        x2, y2, z2 = X * X, Y * Y, Z * Z
        r2 = x2 + y2
        r = np.sqrt(r2)
        r3 = r2 * r
        theta = np.arctan2(r, Z)
        theta2 = theta * theta
        theta3 = theta2 * theta
        theta4 = theta2 * theta2
        theta5 = theta4 * theta
        theta6 = theta2 * theta4
        theta7 = theta6 * theta
        theta8 = theta4 * theta4
        theta9 = theta8 * theta
        f = theta + theta3 * k[0] + theta5 * k[1] + theta7 * k[2] + theta9 * k[3]
        fd = 1 + 3 * k[0] * theta2 + 5 * k[1] * theta4 + 7 * k[2] * theta6 + 9 * k[3] * theta8
        Jp[..., 0, 0] = fx * (fd * Z * x2 / (r2 * (r2 + z2)) + f * y2 / r3)
        Jp[..., 1, 0] = fy * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3)
        Jp[..., 0, 1] = fx * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3)
        Jp[..., 1, 1] = fy * (fd * Z * y2 / (r2 * (r2 + z2)) + f * x2 / r3)
        Jp[..., 0, 2] = -fx * fd * X / (r2 + z2)
        Jp[..., 1, 2] = -fy * fd * Y / (r2 + z2)
    return Jp


# ---- the pose and the edge ------------------------------------------------------------------------------------------------------------------
def derive_pose(cal, Rwb, twb):
    """(R_cw, t_cw, R_cb, t_bc) in float64 from the body pose: G2oTypes.cpp:23-24; t_bc is the float Pose::inverse of T_cb, widened"""
    Rcb32, tcb32 = cal["Rcb"].astype(np.float32), cal["tcb"].astype(np.float32)
    Rcb, tcb = Rcb32.astype(F64), tcb32.astype(F64)
    Rcw = im.mm(Rcb, np.asarray(Rwb, F64).T)
    tcw = tcb - im.mv(Rcw, np.asarray(twb, F64))
    tbc = im.mv(-(Rcb32.T), tcb32)
    assert tbc.dtype == np.float32
    return Rcw, tcw, Rcb, tbc.astype(F64)


def _rows(R, t, X, Y, Z):
    """R*(X, Y, Z) + t per edge, the product-sum first"""
    return [((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z) + t[i] for i in range(3)]


def edge_errors(cam, Rcw, tcw, P, z, w):
    """computeError: (Pc [3 x n], err [n, 2], chi2 [n])"""
    P = np.asarray(P, F64).reshape(-1, 3)
    Pc = _rows(Rcw, tcw, P[:, 0], P[:, 1], P[:, 2])
    u, v = project(cam, *Pc)
    z = np.asarray(z, F64).reshape(-1, 2)
    ex, ey = z[:, 0] - u, z[:, 1] - v
    with np.errstate(all="ignore"):
        chi2 = np.asarray(w, F64) * (ex * ex + ey * ey)
    return Pc, np.stack([ex, ey], 1), chi2


def edge_jacobian(cam, Rcb, tbc, Pc):
    """linearizeOplus: J [n, 2, 6] = [(-Jp)*(R_cb*Hat(R_bc*Pc + t_bc)), (-Jp)*(-R_cb)]"""
    X, Y, Z = Pc
    Jp = proj_jacobian(cam, X, Y, Z)
    with np.errstate(all="ignore"):
        bx, by, bz = _rows(Rcb.T, tbc, X, Y, Z)
        zero = np.zeros_like(bx)
        Hb = [[zero, -bz, by], [bz, zero, -bx], [-by, bx, zero]]
        M = [[(Rcb[i, 0] * Hb[0][j] + Rcb[i, 1] * Hb[1][j]) + Rcb[i, 2] * Hb[2][j] for j in range(3)] for i in range(3)]
        J = np.zeros(X.shape + (2, 6))
        for r in range(2):
            for c in range(3):
                J[:, r, c] = (-Jp[:, r, 0] * M[0][c] + -Jp[:, r, 1] * M[1][c]) + -Jp[:, r, 2] * M[2][c]
                J[:, r, 3 + c] = (-Jp[:, r, 0] * -Rcb[0, c] + -Jp[:, r, 1] * -Rcb[1, c]) + -Jp[:, r, 2] * -Rcb[2, c]
    return J


def huber(chi2, delta):
    """g2o's RobustKernelHuber per edge: (rho, rho')"""
    chi2 = np.asarray(chi2, F64)
    rho, rw = chi2.copy(), np.ones_like(chi2)
    with np.errstate(all="ignore"):
        out = (chi2 > delta * delta) if delta > 0 else np.zeros(chi2.shape, bool)
        sq = np.sqrt(chi2[out])
        rho[out], rw[out] = (2.0 * sq) * delta - delta * delta, delta / sq
    return rho, rw


def block_sum(C):
    """the sums of a workgroup: C [n, K] per edge (zero rows for edges that do not take part).  Thread t adds its edges t, t + 1024, ...
    in ascending order from zero; the wave butterfly v = v + v[lane ^ o], o = 32 .. 1; the sixteen waves ascending from zero."""
    C = np.asarray(C, F64)
    n, K = C.shape
    trips = (n + THREADS - 1) // THREADS
    pad = np.zeros((max(trips, 1) * THREADS, K))
    pad[:n] = C
    acc = np.zeros((THREADS, K))
    for k in range(trips):
        acc = acc + pad[THREADS * k:THREADS * (k + 1)]
    v = acc.reshape(WAVES, 64, K)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o, :]
    s = np.zeros(K)
    for wv in range(WAVES):
        s = s + v[wv, 0]
    return s


UPPER = [(r, c) for r in range(6) for c in range(r, 6)]


def edge_contributions(J, W, err):
    """[n, 27]: the 21 entries of J^T (W J)'s upper triangle row by row, then the 6 of J^T (W e)"""
    with np.errstate(all="ignore"):
        WJ = W[:, None, None] * J
        we = W[:, None] * err
        cols = [J[:, 0, r] * WJ[:, 0, c] + J[:, 1, r] * WJ[:, 1, c] for r, c in UPPER]
        cols += [J[:, 0, r] * we[:, 0] + J[:, 1, r] * we[:, 1] for r in range(6)]
    return np.stack(cols, 1)


def ranges(edge_off, cap):
    """d_edge_off as the device reads it: clamped to [0, cap], then non-decreasing"""
    return np.maximum.accumulate(np.clip(np.asarray(edge_off, np.int64), 0, cap))


def linearize(graph, cal, cam, group_state, edge_off, cap, P, z, w, active=None, delta=HUBER_MONO, threshold=CHI2_MONO, mode=0, H_diag=None,
              b=None, err=None, chi2=None):
    """orbvi_linearize_device.  H_diag [n, 15, 15], b [n, 15], err [cap, 2], chi2 [cap]: what the arrays hold before the call (copied;
    NaN when not given).  Returns a dict of err, chi2, total, result and, by mode, H_diag, b (0) or active, n_inliers (2)."""
    ng = len(group_state)
    off = ranges(edge_off, cap)
    P, z, w = np.asarray(P, F64).reshape(-1, 3), np.asarray(z, F64).reshape(-1, 2), np.asarray(w, F64)
    o = dict(err=np.full((cap, 2), np.nan) if err is None else np.array(err, F64).reshape(cap, 2),
             chi2=np.full(cap, np.nan) if chi2 is None else np.array(chi2, F64).reshape(cap), result=np.zeros(8, np.int32))
    if mode != 2:
        o["total"] = np.zeros((ng, 2))
    if mode == 0:
        o["H_diag"], o["b"] = np.array(H_diag, F64).reshape(graph.n, 15, 15), np.array(b, F64).reshape(graph.n, 15)
    if mode == 2:
        o["active"] = np.full(cap, 0xEE, np.uint8) if active is None else np.array(active, np.uint8)
        o["n_inliers"] = np.zeros(ng, np.int32)
    seen = set()
    for g, st in enumerate(int(s) for s in group_state):
        lo, hi = int(off[g]), int(off[g + 1])
        dup = st in seen
        seen.add(st)
        if not 0 <= st < graph.n or dup:
            o["result"][R_DUPLICATE if 0 <= st < graph.n else R_RANGE] += 1
            o["err"][lo:hi], o["chi2"][lo:hi] = 0.0, 0.0
            continue
        o["result"][R_DONE] += 1
        Rcw, tcw, Rcb, tbc = derive_pose(cal, graph.Rwb[st], graph.twb[st])
        Pc, e, c2 = edge_errors(cam, Rcw, tcw, P[lo:hi], z[lo:hi], w[lo:hi])
        o["err"][lo:hi], o["chi2"][lo:hi] = e, c2
        finite = np.isfinite(e).all(1) & np.isfinite(c2)
        if mode == 2:
            with np.errstate(all="ignore"):
                inl = ~(c2 > threshold)
            o["active"][lo:hi], o["n_inliers"][g] = inl, inl.sum()
            o["result"][R_NONFINITE] += (~finite).sum()
            continue
        act = np.ones(hi - lo, bool) if active is None else np.asarray(active[lo:hi]) != 0
        o["result"][R_NONFINITE] += (act & ~finite).sum()
        use = act & finite
        rho, rw = huber(c2, delta)
        o["total"][g] = block_sum(np.where(use[:, None], np.stack([c2, rho], 1), 0.0))
        if mode == 0 and not int(graph.fixed[st]) & fm.FIX_POSE:
            J = edge_jacobian(cam, Rcb, tbc, Pc)
            with np.errstate(all="ignore"):
                C = edge_contributions(J, rw * w[lo:hi], e)
            s = block_sum(np.where(use[:, None], C, 0.0))
            for k, (r, c) in enumerate(UPPER):
                o["H_diag"][st, r, c] = o["H_diag"][st, r, c] + s[k]
                if r != c:
                    o["H_diag"][st, c, r] = o["H_diag"][st, c, r] + s[k]
            o["b"][st, :6] = o["b"][st, :6] - s[21:]
            o["J"] = J
    return o


# ---- the damped step -------------------------------------------------------------------------------------------------------------------------
def dof_fixed(fixed):
    return np.concatenate([fm.dof_fixed(f) for f in fixed]) if len(fixed) else np.zeros(0, bool)


def assemble(fixed, edges, cap, H_diag, H_off, b, lam):
    """(H + lambda*I with the fixed dof as identity rows, the right-hand side, the fixed mask, max free H_jj before damping, dropped edges)"""
    n = len(fixed)
    N = 15 * n
    A = np.zeros((N, N))
    H_diag, b = np.asarray(H_diag, F64).reshape(n, 15, 15), np.asarray(b, F64).reshape(N)
    H_off = np.zeros((0, 15, 15)) if H_off is None else np.asarray(H_off, F64).reshape(-1, 15, 15)
    for s in range(n):
        A[15 * s:15 * s + 15, 15 * s:15 * s + 15] = H_diag[s]
    dropped = 0
    for e, ed in enumerate(edges):
        i, j, rec = int(ed["i"]), int(ed["j"]), int(ed["rec"])
        if not (0 <= i < n and 0 <= j < n and i != j and 0 <= rec < cap):
            dropped += 1
            continue
        B = H_off[e]
        A[15 * i:15 * i + 15, 15 * j:15 * j + 15] = A[15 * i:15 * i + 15, 15 * j:15 * j + 15] + B
        A[15 * j:15 * j + 15, 15 * i:15 * i + 15] = A[15 * j:15 * j + 15, 15 * i:15 * i + 15] + B.T
    fx = dof_fixed(fixed)
    A[fx, :], A[:, fx] = 0.0, 0.0
    A[fx, fx] = 1.0
    d = np.diag(A).copy()
    h_max = max([0.0] + [float(v) for v in d[~fx] if v > 0.0])
    A[~fx, ~fx] = d[~fx] + lam
    return A, np.where(fx, 0.0, b), fx, h_max, dropped


def ordered_cholesky_solve(A, rhs):
    """L*L^T in the header's orders: columns ascending, inner sums ascending from zero, one sqrt and one division per column, then the
    forward (ascending) and backward (descending) substitutions.  Returns (x or None when refused, smallest or offending pivot)."""
    N = len(rhs)
    L, r = np.zeros((N, N)), np.zeros(N)
    pivot = np.inf
    for j in range(N):
        s = np.zeros(N)
        for k in range(j):
            s = s + L[:, k] * L[j, k]
        d = A[j, j] - s[j]
        if not d > 0.0 or not np.isfinite(d):
            return None, d
        pivot = min(pivot, d)
        L[j, j] = np.sqrt(d)
        r[j] = 1.0 / L[j, j]
        L[j + 1:, j] = (A[j + 1:, j] - s[j + 1:]) * r[j]
    s, y = np.zeros(N), np.zeros(N)
    for k in range(N):
        y[k] = (rhs[k] - s[k]) * r[k]
        s[k + 1:] = s[k + 1:] + L[k + 1:, k] * y[k]
    s, x = np.zeros(N), np.zeros(N)
    for k in range(N - 1, -1, -1):
        x[k] = (y[k] - s[k]) * r[k]
        s[:k] = s[:k] + L[k, :k] * x[k]
    return x, pivot


def solve(fixed, edges, cap, H_diag, H_off, b, lam):
    """orbvi_solve_device: (dx [n, 15], out [3], result [8])"""
    n = len(fixed)
    A, rhs, fx, h_max, dropped = assemble(fixed, edges, cap, H_diag, H_off, b, lam)
    x, pivot = ordered_cholesky_solve(A, rhs)
    res = np.zeros(8, np.int32)
    res[R_RANGE] = dropped
    if x is None:
        res[R_REFUSED] = 1
        return np.zeros((n, 15)), np.array([0.0, h_max, pivot]), res
    res[R_DONE] = 1
    scale = 0.0
    for j in range(15 * n):
        scale = scale + x[j] * (lam * x[j] + rhs[j])
    return x.reshape(n, 15), np.array([scale, h_max, pivot]), res


def backward_error_bound(A, x):
    """the normwise bound of Cholesky with substitution: 4n(3n + 1) u |A|_inf |x|_inf, u = 2^-53"""
    n = len(x)
    return 4 * n * (3 * n + 1) * 2.0 ** -53 * np.abs(A).sum(1).max() * np.abs(x).max()


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
OUTLIER_SHARE = 0.1


def make_edges(cal, cam, Rwb, twb, n_edges, rng):
    """n_edges map points in front of the camera of the body pose (Rwb, twb), as floats widened, their noisy measurements and weights"""
    model = cam["model"]
    Rcw, tcw, _, _ = derive_pose(cal, Rwb, twb)
    depth = rng.uniform(2.0, 12.0, n_edges)
    span = 0.35 if model == 0 else 0.8
    Pc = np.stack([rng.uniform(-span, span, n_edges) * depth, rng.uniform(-span, span, n_edges) * depth, depth], 1)
    Pw = (Pc - tcw) @ Rcw                                      # R_cw^T (Pc - t_cw): building the scene, not part of the model
    P = Pw.astype(np.float32).astype(F64)
    size = (np.float32(31.0) * np.float32(1.2) ** rng.randint(0, 8, n_edges).astype(np.float32)).astype(np.float32)
    w = (np.float32(1.0) / size / size).astype(F64)
    u, v = project(cam, *_rows(Rcw, tcw, P[:, 0], P[:, 1], P[:, 2]))
    gross = rng.uniform(size=n_edges) < OUTLIER_SHARE
    noise = rng.normal(0.0, 1.0, (n_edges, 2)) * size[:, None].astype(F64) * np.where(gross, 4.0, 1.0)[:, None]
    z = (np.stack([u, v], 1) + noise).astype(np.float32).astype(F64)
    return P, z, w


def pose_full_scene(n_edges, seed=3, model=0, sample_counts=fm.SAMPLE_COUNTS):
    """poseFullOptimize's graph: factors_model.make_tracker_graph (two states, state 0's pose fixed, one record, three priors) and
    n_edges map points seen by state 1.  The points are projected through a pose a little off state 1's (2e-3 rad, 2 cm: something for
    an iteration to gain) and stored as floats widened, like orbba_pose_edges_device leaves them; kp.size = 31 * 1.2^level, inv_sigma2 =
    1.f / size / size, and the pixel noise is size * N(0, 1) per axis, so that chi2 is about chi-square with two degrees of freedom:
    most below huber_delta^2 = 5.991, about 5 % above; OUTLIER_SHARE of the edges get four times the noise.  sample_counts is
    factors_model.make_chain's, for the closed-loop scenes of tests/inertial_loop.py; its default gives the scene above, byte for byte."""
    rng = np.random.RandomState(1000 * seed + 7 * model + 1)
    sc = fm.make_tracker_graph(11, sample_counts)
    cam = FISHEYE if model else PINHOLE
    g = sc["graph"]
    off = g.copy()
    off.fixed[:] = 0
    dx = np.zeros((2, 15))
    dx[1, :6] = np.array([2e-3, -1.5e-3, 1e-3, 0.02, -0.01, 0.015])
    fm.oplus(off, dx)
    P, z, w = make_edges(sc["cal"], cam, off.Rwb[1], off.twb[1], n_edges, rng)
    sc.update(cam=cam, points=P, z=z, w=w, n_edges=n_edges, group_state=np.array([1], np.int32), edge_off=np.array([0, n_edges], np.int32))
    if n_edges >= 400:
        Rcw1, tcw1, _, _ = derive_pose(sc["cal"], g.Rwb[1], g.twb[1])
        _, _, c2 = edge_errors(cam, Rcw1, tcw1, P, z, w)
        above = float((c2 > HUBER_MONO ** 2).mean())
        assert 0.05 < above < 0.35 and (c2 <= HUBER_MONO ** 2).sum() > n_edges // 2, above      # both Huber branches
        assert (c2 > CHI2_MONO).any() and (c2 <= CHI2_MONO).any()                                # both sides of the classification
        sc["share_above"] = above
    return sc


def inertial_linearize(sc, graph, mode=0, pjobs=None):
    """orbi_linearize_device on a scene's graph: factors_model.linearize with the scene's information (computed once per scene)"""
    if "info" not in sc:
        sc["info"], sc["walk"], _ = fm.edge_information(sc["recs"], sc["edges"])
    return fm.linearize(graph, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], sc["priors"], sc["pjobs"] if pjobs is None else pjobs,
                        0.0, mode)
