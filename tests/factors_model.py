"""Plain numpy restatement of include/orbi.h's section "Inertial factors linearised on the device" (include/orbi_factors.h): the
vertices, EdgeInertial / EdgeInertialOnly (reference modules/Backend/G2oTypes.cpp:309-445), EdgeBiasWalk and EdgePriori3D
(G2oTypes.h:324-343, :452-470), their information matrices (G2oTypes.cpp:366-372, Optimize.cpp:1022-1028, KeyFrame.cpp:86-98),
constructQuadraticForm with g2o's Huber rule, CameraImuPose::update (G2oTypes.cpp:10-25) and step 5 of the optimisers.  The parts the
reference computes in float come from imu_model's float32 functions; everything behind the cast is float64, in the orders the header
fixes: no `@`, every sum over k written as elementwise operations in ascending k.  The seeded scenes live here too; each asserts
that it holds what it is meant to hold.  No part of the library is used here."""
import math

import numpy as np

import imu_model as im

FIX_POSE, FIX_VELO, FIX_GYRO, FIX_ACC = 1, 2, 4, 8
EDGE_WALKS = 1
PRIOR_VELO, PRIOR_GYRO, PRIOR_ACC, PRIOR_ACC_GYRO_INFO = 1, 2, 4, 8
RECOVER_POSE = 1
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_PRIOR_DONE, R_PRIOR_RANGE = 0, 1, 2, 3, 4, 5
JACOBI_SWEEPS = 6
HUBER_DELTA = 4.1134          # fullInertialOptimize, Optimize.cpp:322-324

EDGE = np.dtype([("i", "<i4"), ("j", "<i4"), ("rec", "<i4"), ("flags", "<i4")])
PRIOR = np.dtype([("velo_priori", "<f4", 3), ("bias_priori", "<f4", 6), ("velo_info", "<f4", 9), ("gyro_info", "<f4", 9), ("acc_info", "<f4", 9)])
PRIOR_JOB = np.dtype([("state", "<i4"), ("prior", "<i4"), ("mask", "<i4")])
assert EDGE.itemsize == 16 and PRIOR.itemsize == 144 and PRIOR_JOB.itemsize == 12

F64 = np.float64
I3 = np.eye(3)


# ---- double SO(3) (LieAlgeBra.cpp:30-41, 60-70, 84-112, 124-127) ---------------------------------------------------------------------
def sww(s, W):
    """(s*W)*W with the zeros multiplied"""
    return im.mm(s * W, W)


def norm2(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def log_so3(R):
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr == 3:
        return np.zeros(3)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = np.sqrt(norm2(w)), 0.5 * (tr - 1)
    th = math.atan2(sn, cs)
    if abs(th) < 1e-6:
        return w
    return (th * w) / sn


def right_jacobian(v):
    d2 = norm2(v)
    d = np.sqrt(d2)
    if d < 1e-6:
        return I3.copy()
    W = im.hat(v)
    return (I3 - ((1 - math.cos(d)) / d2) * W) + sww((d - math.sin(d)) / (d2 * d), W)


def inverse_right_jacobian(v):
    d2 = norm2(v)
    d = np.sqrt(d2)
    if d < 1e-6:
        return I3.copy()
    W = im.hat(v)
    return (I3 + W / 2) + sww(1 / d2 - (1 + math.cos(d)) / ((2 * d) * math.sin(d)), W)


def normalize_rotation(X):
    """NormalizeRotation in double: the float code's two Newton steps, widened"""
    return im.newton(im.newton(np.asarray(X, F64)))


def exp_so3(w):
    """ExpSO3 in double, which normalises its result"""
    w = np.asarray(w, F64)
    d2 = norm2(w)
    d = np.sqrt(d2)
    W = im.hat(w)
    if d < 1e-6:
        return normalize_rotation((I3 + W) + sww(0.5, W))
    return normalize_rotation((I3 + (math.sin(d) / d) * W) + sww((1 - math.cos(d)) / d2, W))


# ---- the graph --------------------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, n):
        self.n = n
        self.Rwb = np.tile(I3, (n, 1, 1))
        self.twb, self.v, self.bg, self.ba = (np.zeros((n, 3)) for _ in range(4))
        self.fixed = np.zeros(n, np.uint8)
        self.iter = np.zeros(n, np.int32)

    def copy(self):
        o = Graph(self.n)
        for k in ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter"):
            setattr(o, k, getattr(self, k).copy())
        return o


def _dups(keys):
    seen, out = set(), []
    for k in keys:
        out.append(k in seen)
        seen.add(k)
    return out


def graph_init(graph, recs, src, jobs):
    """orbi_graph_init_device.  recs: imu_model float32 Recs; src: float32 [n_src, 15]; jobs: int [n, 3] (state, source, record)"""
    res = np.zeros(8, np.int32)
    dup = _dups([int(j[0]) for j in jobs])
    for k, (st, fr, rec) in enumerate(np.asarray(jobs).reshape(-1, 3)):
        if not (0 <= st < graph.n and 0 <= fr < len(src) and -1 <= rec < len(recs)):
            res[R_RANGE] += 1
        elif dup[k]:
            res[R_DUPLICATE] += 1
        else:
            f = np.asarray(src[fr], np.float32).astype(F64)
            graph.Rwb[st], graph.twb[st], graph.v[st] = f[:9].reshape(3, 3), f[9:12], f[12:15]
            b = recs[rec].updated_bias.astype(F64) if rec >= 0 else np.zeros(6)
            graph.bg[st], graph.ba[st] = b[:3], b[3:]
            res[R_DONE] += 1
    return res


def oplus(graph, dx):
    """orbi_graph_oplus_device: oplusImpl of every vertex that is not fixed"""
    res = np.zeros(8, np.int32)
    dx = np.asarray(dx, F64).reshape(graph.n, 15)
    for s in range(graph.n):
        fx, d = int(graph.fixed[s]), dx[s]
        if not fx & FIX_POSE:
            R = graph.Rwb[s]
            graph.twb[s] = graph.twb[s] + im.mv(R, d[3:6])
            N = im.mm(R, exp_so3(d[0:3]))
            graph.iter[s] += 1
            if graph.iter[s] == 3:
                N, graph.iter[s] = normalize_rotation(N), 0
            graph.Rwb[s] = N
        if not fx & FIX_VELO:
            graph.v[s] = graph.v[s] + d[6:9]
        if not fx & FIX_GYRO:
            graph.bg[s] = graph.bg[s] + d[9:12]
        if not fx & FIX_ACC:
            graph.ba[s] = graph.ba[s] + d[12:15]
        res[R_DONE] += (fx & 15) != 15
    return res


def recover(graph, cal, jobs, dst, with_pose=True):
    """orbi_graph_recover_device.  dst: float32 [n_dst, 15], changed in place.  Returns (bias [n, 6] f32, pose_R [n, 9], pose_t [n, 3], result);
    pose rows of jobs without ORBI_RECOVER_POSE stay NaN (the device leaves them as passed)."""
    jobs = np.asarray(jobs).reshape(-1, 3)
    n = len(jobs)
    res, bias = np.zeros(8, np.int32), np.zeros((n, 6), np.float32)
    pose_R, pose_t = np.full((n, 9), np.nan), np.full((n, 3), np.nan)
    dup = _dups([int(j[1]) for j in jobs])
    f = np.float32
    for k, (st, to, flags) in enumerate(jobs):
        if not (0 <= st < graph.n and 0 <= to < len(dst)):
            res[R_RANGE] += 1
        elif dup[k]:
            res[R_DUPLICATE] += 1
        else:
            dst[to, 12:15] = graph.v[st].astype(f)
            bias[k, :3], bias[k, 3:] = graph.bg[st].astype(f), graph.ba[st].astype(f)
            if flags & RECOVER_POSE:
                R, t = graph.Rwb[st].astype(f), graph.twb[st].astype(f)
                dst[to, :9], dst[to, 9:12] = R.reshape(9), t
                if with_pose:
                    Rcb, tcb = cal["Rcb"].astype(f), cal["tcb"].astype(f)
                    Rbw = R.T
                    pose_R[k], pose_t[k] = im.mm(Rcb, Rbw).reshape(9).astype(F64), (im.mv(Rcb, im.mv(-Rbw, t)) + tcb).astype(F64)
            res[R_DONE] += 1
    return bias, pose_R, pose_t, res


# ---- information ------------------------------------------------------------------------------------------------------------------------
def gauss_jordan_inverse(A):
    """the general inverse by Gauss-Jordan with partial pivoting on [A | I]; None at a zero pivot"""
    n = len(A)
    M = np.concatenate([np.asarray(A, F64), np.eye(n)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))      # the first row of the largest |entry|
        if not abs(M[p, k]) > 0:
            return None
        if p != k:
            M[[k, p]] = M[[p, k]]
        pr = M[k] / M[k, k]
        f = M[:, k].copy()
        M = M - f[:, None] * pr[None, :]
        M[k] = pr
    return M[:, n:]


def cofactor_inverse(X):
    """(inverse, determinant) of a 3x3 by cofactors: X^-1 = cof(X)^T / det"""
    X = np.asarray(X, F64)
    r = lambda a, b: np.roll(X, (-a, -b), (0, 1))  # noqa: E731
    cof = r(1, 1) * r(2, 2) - r(1, 2) * r(2, 1)
    det = (X[0, 0] * cof[0, 0] + X[0, 1] * cof[0, 1]) + X[0, 2] * cof[0, 2]
    with np.errstate(all="ignore"):
        return cof.T / det, det


def clamp_information(info, threshold=1e-12):
    """the reference's eigenvalue clamp (G2oTypes.cpp:368-372), which the device omits.  Returns (clamped matrix, clamped count, smallest eigenvalue)."""
    lam, V = np.linalg.eigh(info)
    low = lam < threshold
    return (V * np.where(low, 0.0, lam)) @ V.T, int(low.sum()), float(lam.min())


def edge_information(recs, edges):
    """orbi_edge_information_device: (info [n, 81], walk_info [n, 18], result)"""
    n = len(edges)
    info, walk, res = np.zeros((n, 81)), np.zeros((n, 18)), np.zeros(8, np.int32)
    for e, ed in enumerate(edges):
        rec = int(ed["rec"])
        if not 0 <= rec < len(recs):
            res[R_RANGE] += 1
            continue
        C = recs[rec].C.astype(F64)
        X = gauss_jordan_inverse(C[:9, :9])
        (wg, dg), (wa, da) = cofactor_inverse(C[9:12, 9:12]), cofactor_inverse(C[12:15, 12:15])
        if X is None or (int(ed["flags"]) & EDGE_WALKS and (dg == 0 or da == 0)):
            res[R_REFUSED] += 1
            continue
        info[e] = ((X + X.T) / 2).reshape(81)
        if dg != 0:
            walk[e, :9] = wg.reshape(9)
        if da != 0:
            walk[e, 9:] = wa.reshape(9)
        res[R_DONE] += 1
    return info, walk, res


def jacobi_eigen(A, sweeps=JACOBI_SWEEPS):
    """cyclic Jacobi on a symmetric 3x3: (eigenvalues, eigenvectors in columns) after a fixed count of sweeps over (0,1), (0,2), (1,2)"""
    A, V = np.array(A, F64), np.eye(3)
    for _ in range(sweeps):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p, q]
            if apq == 0:
                continue
            with np.errstate(over="ignore"):
                th = (A[q, q] - A[p, p]) / (2 * apq)
                t = (-1.0 if th < 0 else 1.0) / (abs(th) + np.sqrt(th * th + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            arp, arq = A[r, p], A[r, q]
            A[p, p], A[q, q] = A[p, p] - t * apq, A[q, q] + t * apq
            A[p, q] = A[q, p] = 0.0
            A[r, p] = A[p, r] = c * arp - s * arq
            A[r, q] = A[q, r] = s * arp + c * arq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(A).copy(), V


def prior_information(priors, recs, src, jobs):
    """orbi_prior_information_device.  priors: PRIOR array, changed in place.  Returns (result, clamped eigenvalue count per job or -1)."""
    res, clamped = np.zeros(8, np.int32), []
    jobs = np.asarray(jobs).reshape(-1, 3)
    dup = _dups([int(j[0]) for j in jobs])
    n_src = 0 if src is None else len(src)
    for k, (slot, rec, st) in enumerate(jobs):
        clamped.append(-1)
        if not (0 <= slot < len(priors) and 0 <= rec < len(recs) and -1 <= st < n_src):
            res[R_RANGE] += 1
            continue
        if dup[k]:
            res[R_DUPLICATE] += 1
            continue
        C = recs[rec].C.astype(F64)
        (gi, dg), (ai, da) = cofactor_inverse(C[9:12, 9:12]), cofactor_inverse(C[12:15, 12:15])
        if dg == 0 or da == 0:
            res[R_REFUSED] += 1
            continue
        A = (C[3:6, 3:6] + C[3:6, 3:6].T) / 2
        lam, V = jacobi_eigen(A)
        low = lam < 1e-12
        clamped[-1] = int(low.sum())
        lam = np.where(low, 0.0, lam)
        velo = (V[:, 0:1] * lam[0] * V[:, 0:1].T + V[:, 1:2] * lam[1] * V[:, 1:2].T) + V[:, 2:3] * lam[2] * V[:, 2:3].T
        p = priors[slot]
        p["velo_info"], p["gyro_info"], p["acc_info"] = velo.reshape(9).astype(np.float32), gi.reshape(9).astype(np.float32), ai.reshape(9).astype(np.float32)
        p["bias_priori"] = recs[rec].updated_bias
        if st >= 0:
            p["velo_priori"] = np.asarray(src[st], np.float32)[12:15]
        res[R_DONE] += 1
    return res, clamped


# ---- the inertial edge -------------------------------------------------------------------------------------------------------------------
def float_deltas(rec, bg, ba):
    """getDeltaRotation / Velocity / Position (Imu.cpp:182-192) of the bias vertices cast to float: float32 (dR, dV, dP, bg - bias.bg)"""
    f = np.float32
    assert rec.D is np.float32
    dbg, dba = np.asarray(bg, F64).astype(f) - rec.bias[:3], np.asarray(ba, F64).astype(f) - rec.bias[3:]
    dE, _ = im.exp_and_right_jacobian(im.mv(rec.JRg, dbg))
    return (im.normalize_rotation(im.mm(rec.dR, dE)), (rec.dV + im.mv(rec.JVg, dbg)) + im.mv(rec.JVa, dba),
            (rec.dP + im.mv(rec.JPg, dbg)) + im.mv(rec.JPa, dba), dbg)


def inertial_edge(rec, graph, i, j, gravity, jacobian=True):
    """computeError and linearizeOplus of EdgeInertial (G2oTypes.cpp:377-445): (err [9], raw J [9, 30] or None, float (dR, dV, dP) [15])"""
    dRf, dVf, dPf, dbgf = float_deltas(rec, graph.bg[i], graph.ba[i])
    dR, dV, dP, dbg = dRf.astype(F64), dVf.astype(F64), dPf.astype(F64), dbgf.astype(F64)
    JRg, JVg, JVa, JPg, JPa = (getattr(rec, k).astype(F64) for k in ("JRg", "JVg", "JVa", "JPg", "JPa"))
    dt, G = F64(rec.delta_t), F64(np.float32(gravity))
    g = np.array([0.0, 0.0, -G])
    R1, R2, t1, t2, v1, v2 = graph.Rwb[i], graph.Rwb[j], graph.twb[i], graph.twb[j], graph.v[i], graph.v[j]
    Rb1w = R1.T
    eR = im.mm(im.mm(dR.T, Rb1w), R2)
    er = log_so3(eR)
    a = im.mv(Rb1w, (v2 - v1) - g * dt)
    c = im.mv(Rb1w, ((t2 - t1) - v1 * dt) - ((0.5 * g) * dt) * dt)
    err = np.concatenate([er, a - dV, c - dP])
    flt = np.concatenate([dRf.reshape(9), dVf, dPf])
    if not jacobian:
        return err, None, flt
    invJ = inverse_right_jacobian(er)
    Jr = right_jacobian(im.mv(JRg, dbg))
    J = np.zeros((9, 30))
    J[0:3, 0:3] = im.mm(im.mm(-invJ, R2.T), R1)
    J[3:6, 0:3], J[6:9, 0:3], J[6:9, 3:6] = im.hat(a), im.hat(c), -I3
    J[3:6, 6:9], J[6:9, 6:9] = -Rb1w, (-Rb1w) * dt
    J[0:3, 9:12] = im.mm(im.mm(im.mm(-invJ, eR.T), Jr), JRg)
    J[3:6, 9:12], J[6:9, 9:12] = -JVg, -JPg
    J[3:6, 12:15], J[6:9, 12:15] = -JVa, -JPa
    J[0:3, 15:18], J[6:9, 18:21], J[3:6, 21:24] = invJ, im.mm(Rb1w, R2), Rb1w
    return err, J, flt


def dof_fixed(fixed):
    """bool [15] of a state's d_fixed byte"""
    fixed = int(fixed)
    return np.array([bool(fixed & FIX_POSE)] * 6 + [bool(fixed & FIX_VELO)] * 3 + [bool(fixed & FIX_GYRO)] * 3 + [bool(fixed & FIX_ACC)] * 3)


def huber(chi2, delta):
    """g2o's RobustKernelHuber: (rho, rho')"""
    if delta > 0 and chi2 > delta * delta:
        s = np.sqrt(chi2)
        return (2 * s) * delta - delta * delta, delta / s
    return chi2, 1.0


def _ordered(A, B):
    """sum over k ascending of A[:, k] B[k, :], starting from zero"""
    s = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        s = s + A[:, k:k + 1] * B[k:k + 1, :]
    return s


def _prior_parts(pj, pr):
    """the (dof base, information, measurement) of the EdgePriori3D a prior job carries"""
    out = []
    mask = int(pj["mask"])
    for v, (info, meas) in enumerate((("velo_info", pr["velo_priori"]), ("gyro_info", pr["bias_priori"][:3]), ("acc_info", pr["bias_priori"][3:]))):
        if mask >> v & 1:
            if v == 2 and mask & PRIOR_ACC_GYRO_INFO:
                info = "gyro_info"
            out.append((v, pr[info].astype(F64).reshape(3, 3), meas.astype(F64)))
    return out


def linearize(graph, recs, gravity, edges, info, walk, priors=None, pjobs=None, delta=0.0, mode=0):
    """orbi_linearize_device: a dict of err, chi2, chi2_prior, total, result, flt and, in mode 0, H_diag, H_off, b, J"""
    ne, n = len(edges), graph.n
    pjobs = np.zeros(0, PRIOR_JOB) if pjobs is None else pjobs
    o = dict(err=np.zeros((ne, 9)), chi2=np.zeros((ne, 3)), chi2_prior=np.zeros((len(pjobs), 3)), flt=np.zeros((ne, 15), np.float32),
             result=np.zeros(8, np.int32), status=np.zeros(ne, np.int32))
    if mode == 0:
        o.update(H_diag=np.zeros((n, 15, 15)), H_off=np.zeros((ne, 15, 15)), b=np.zeros((n, 15)), J=np.zeros((ne, 9, 30)))
    part = {}
    for e, ed in enumerate(edges):
        i, j, rec, flags = (int(ed[k]) for k in ("i", "j", "rec", "flags"))
        if not (0 <= i < n and 0 <= j < n and i != j and 0 <= rec < len(recs)):
            o["status"][e] = R_RANGE
        elif info[e, 0] == 0:
            o["status"][e] = R_REFUSED
        o["result"][o["status"][e]] += 1
        if o["status"][e]:
            continue
        err, J, flt = inertial_edge(recs[rec], graph, i, j, gravity, mode == 0)
        Om = info[e].reshape(9, 9)
        We = _ordered(Om, err[:, None])[:, 0]
        chi = float(_ordered(err[None, :], We[:, None])[0, 0])
        rho1 = huber(chi, delta)[1]
        we = np.zeros((2, 3))
        if flags & EDGE_WALKS:
            for b, est in enumerate((graph.bg, graph.ba)):
                ew = est[j] - est[i]
                we[b] = im.mv(walk[e, 9 * b:9 * b + 9].reshape(3, 3), ew)
                o["chi2"][e, 1 + b] = (ew[0] * we[b, 0] + ew[1] * we[b, 1]) + ew[2] * we[b, 2]
        o["err"][e], o["chi2"][e, 0], o["flt"][e] = err, chi, flt
        if mode != 0:
            continue
        o["J"][e] = J
        fx = np.concatenate([dof_fixed(graph.fixed[i]), dof_fixed(graph.fixed[j])])
        Jm = np.where(fx[None, :], 0.0, J)
        WJ = rho1 * _ordered(Om, Jm)
        M = _ordered(Jm.T, WJ)
        bvec = -_ordered(Jm.T, (rho1 * We)[:, None])[:, 0]
        Hij = M[:15, 15:].copy()
        if flags & EDGE_WALKS:
            for b in range(2):
                if not fx[9 + 3 * b] and not fx[15 + 9 + 3 * b]:
                    Hij[9 + 3 * b:12 + 3 * b, 9 + 3 * b:12 + 3 * b] -= walk[e, 9 * b:9 * b + 9].reshape(3, 3)
        o["H_off"][e] = Hij
        part[e] = (M[:15, :15], M[15:, 15:], bvec, we)
    # prior jobs
    for p, pj in enumerate(pjobs):
        ok = 0 <= pj["state"] < n and 0 <= pj["prior"] < (0 if priors is None else len(priors))
        o["result"][R_PRIOR_DONE if ok else R_PRIOR_RANGE] += 1
        if ok:
            s = int(pj["state"])
            for v, Om, meas in _prior_parts(pj, priors[pj["prior"]]):
                ep = meas - (graph.v, graph.bg, graph.ba)[v][s]
                w = im.mv(Om, ep)
                o["chi2_prior"][p, v] = (ep[0] * w[0] + ep[1] * w[1]) + ep[2] * w[2]
    plain = robust = 0.0
    for e in range(ne):
        c = o["chi2"][e]
        plain, robust = ((plain + c[0]) + c[1]) + c[2], ((robust + huber(c[0], delta)[0]) + c[1]) + c[2]
    for c in o["chi2_prior"].reshape(-1):
        plain, robust = plain + c, robust + c
    o["total"] = np.array([plain, robust])
    if mode != 0:
        return o
    # one state at a time: its edges in ascending order (the inertial part, then the walks), the priors last
    for s in range(n):
        fx = dof_fixed(graph.fixed[s])
        H, b = np.zeros((15, 15)), np.zeros(15)
        for e in sorted(part):
            i, j, flags = int(edges[e]["i"]), int(edges[e]["j"]), int(edges[e]["flags"])
            if s not in (i, j):
                continue
            Hii, Hjj, bvec, we = part[e]
            H, b = H + (Hii if s == i else Hjj), b + (bvec[:15] if s == i else bvec[15:])
            if flags & EDGE_WALKS:
                for k in range(2):
                    sl = slice(9 + 3 * k, 12 + 3 * k)
                    if not fx[9 + 3 * k]:
                        H[sl, sl] = H[sl, sl] + walk[e, 9 * k:9 * k + 9].reshape(3, 3)
                        b[sl] = b[sl] + we[k] if s == i else b[sl] - we[k]
        for pj in pjobs:
            if pj["state"] != s or not 0 <= pj["prior"] < (0 if priors is None else len(priors)):
                continue
            for v, Om, meas in _prior_parts(pj, priors[pj["prior"]]):
                sl = slice(6 + 3 * v, 9 + 3 * v)
                if fx[6 + 3 * v]:
                    continue
                H[sl, sl] = H[sl, sl] + Om
                b[sl] = b[sl] + im.mv(Om, meas - (graph.v, graph.bg, graph.ba)[v][s])
        o["H_diag"][s], o["b"][s] = H, b
    return o


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
SAMPLE_COUNTS = (2, 3, 8, 40, 100)


def make_record(cal, n_samples, seed, bias_step=None, rng=None):
    """a float32 record of n_samples measurements; with bias_step a setNewBias below its re-integration threshold, so delta_bias != 0"""
    bank = im.Bank(1, max(n_samples, 1))
    r = bank.recs[0]
    r.reset(im.random_bias(rng or np.random.RandomState(seed)))
    if n_samples:
        im.prefill(cal, bank, 0, n_samples, seed)
    if bias_step is not None:
        assert not r.set_new_bias(cal, r.bias + np.asarray(bias_step, np.float32))
    return r


def _next_state(cal, rec, src, rng, noise):
    """the state the record predicts from src, disturbed: a residual of the size the optimisers meet"""
    nxt, _, _ = im.predict(cal, rec, src)
    R = nxt[:9].reshape(3, 3).astype(F64) @ im.rodrigues(rng.normal(0, noise, 3))
    return np.concatenate([R.reshape(9), nxt[9:12] + rng.normal(0, noise, 3), nxt[12:15] + rng.normal(0, noise, 3)]).astype(np.float32)


def make_chain(n_edges, seed=7, walks=True, noise=2e-3, cal=None, sample_counts=SAMPLE_COUNTS):
    """n_edges + 1 states in a chain, edge e between states e and e + 1 with record e; sample counts 2, 3, 8, 40, 100 in turn (or
    `sample_counts` in turn: a closed loop needs the baselines of full records, tests/inertial_loop.py), every second
    record with a non-zero delta_bias.  State e + 1 is what record e predicts from state e, disturbed by `noise`, by a thousandth of it
    and not at all in turn, so that the chi2 of the edges lie on both sides of the Huber threshold.  Returns a dict with the float32 source states, the records, the edges, a prior slot per state
    and the graph as orbi_graph_init_device leaves it."""
    rng = np.random.RandomState(seed)
    cal = cal or im.calib()
    recs, src = [], [np.concatenate([im.rodrigues(rng.normal(0, 0.8, 3)).reshape(9), rng.normal(0, 2.0, 3), rng.normal(0, 0.7, 3)]).astype(np.float32)]
    for e in range(n_edges):
        step = np.array([0.002, -0.003, 0.001, 0.03, -0.02, 0.01]) * (1 + 0.5 * (e % 3)) if e % 2 else None
        recs.append(make_record(cal, sample_counts[e % len(sample_counts)], 200 + 31 * seed + e, step, rng))
        src.append(_next_state(cal, recs[-1], src[-1], rng, noise * (1.0, 1e-3, 0.0)[e % 3]))
    recs.append(make_record(cal, 5, 999 + seed, None, rng))          # the last state's own record: its biases come from there
    src = np.stack(src)
    edges = np.zeros(n_edges, EDGE)
    edges["i"], edges["j"], edges["rec"], edges["flags"] = np.arange(n_edges), np.arange(n_edges) + 1, np.arange(n_edges), EDGE_WALKS if walks else 0
    graph = Graph(n_edges + 1)
    jobs = np.stack([np.arange(n_edges + 1)] * 3, 1).astype(np.int32)
    res = graph_init(graph, recs, src, jobs)
    assert res[R_DONE] == n_edges + 1
    if n_edges >= 5:
        assert {len(r.meas) for r in recs[:n_edges]} == set(sample_counts)
    if n_edges >= 2:
        assert not recs[0].delta_bias.any() and recs[1].delta_bias.all()
    return dict(cal=cal, recs=recs, src=src, edges=edges, graph=graph, init_jobs=jobs)


def make_priors(sc, slots):
    """prior slots from the records `slots` of a chain (slot k from record slots[k] and source state slots[k])"""
    pri = np.zeros(len(slots), PRIOR)
    jobs = np.array([[k, s, s] for k, s in enumerate(slots)], np.int32)
    res, clamped = prior_information(pri, sc["recs"], sc["src"], jobs)
    assert res[R_DONE] == len(slots)
    return pri, jobs, clamped


def make_tracker_graph(seed=11, sample_counts=SAMPLE_COUNTS):
    """poseFullOptimize's inertial part (Optimize.cpp:623-660): two states, the first with a fixed pose, the second without bias
    vertices, one edge without walks, the three priors on the first state"""
    sc = make_chain(1, seed, walks=False, sample_counts=sample_counts)
    sc["graph"].fixed[:] = [FIX_POSE, FIX_GYRO | FIX_ACC]
    sc["graph"].bg[1] = sc["graph"].ba[1] = 0.0
    sc["init_jobs"][1, 2] = -1
    sc["priors"], sc["prior_info_jobs"], _ = make_priors(sc, [0])
    sc["pjobs"] = np.array([(0, 0, PRIOR_VELO | PRIOR_GYRO | PRIOR_ACC)], PRIOR_JOB)
    assert len(sc["edges"]) == 1 and sc["edges"]["flags"][0] == 0
    return sc


def make_clamp_record(noise_acc, n_samples=10, seed=5):
    """a record whose velocity covariance C[3:6,3:6] is small enough for setPrioriInformation's clamp to act"""
    cal = im.calib(noise_acc=noise_acc)
    return cal, make_record(cal, n_samples, seed)
