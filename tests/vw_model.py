"""Plain numpy restatement of include/orbvw.h: EdgeMono (reference modules/Backend/G2oTypes.cpp:59-69) on the VertexPose of a
factors_model.Graph and on the map points, with the distrust of the edge lists, the sums in the orders the header fixes, the Schur
complement over the points, the ordered Cholesky solve of the reduced system and the back-substitution.  The pose, the error, the
camera, the pose Jacobian, Huber, the workgroup sum, the assembly of the pose-side system and the ordered Cholesky are vi_model's; the
graph, oplus and the inertial chain are factors_model's.  float64 throughout, no `@` below the scene builder, every sum written out in
the header's order.  The seeded window scene lives here and asserts that it holds what it is meant to hold.  No part of the library
is used here."""
import numpy as np

import factors_model as fm
import vi_model as vm

F64 = np.float64
MAX_SOLVE_STATES, MAX_EDGES, MAX_POINTS, MAX_OBS, EDGE_WORK = 32, 1 << 20, 1 << 18, 256, 24
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_NONFINITE, R_OUTLIER, R_POINT_SINGULAR = 0, 1, 2, 3, 4, 5, 6
HUBER_MONO, CHI2_MONO = vm.HUBER_MONO, vm.CHI2_MONO
SCHUR_THREADS = 256


def point_ranges(edge_point, n_points):
    """(d_point_off [n_points + 1], the point every edge is read as): clamped to [0, n_points - 1], then the running maximum"""
    ep = np.clip(np.asarray(edge_point, np.int64), 0, n_points - 1)
    eff = np.maximum.accumulate(ep) if len(ep) else ep
    return np.searchsorted(eff, np.arange(n_points + 1), side="left").astype(np.int32), eff


def block_sum(C, threads):
    """vi_model.block_sum for a workgroup of `threads` threads: thread t adds its rows t, t + threads, ... ascending from zero, the wave
    butterfly, the waves ascending from zero"""
    if threads == vm.THREADS:
        return vm.block_sum(C)
    C = np.asarray(C, F64)
    n, K = C.shape
    trips = max((n + threads - 1) // threads, 1)
    pad = np.zeros((trips * threads, K))
    pad[:n] = C
    acc = np.zeros((threads, K))
    for k in range(trips):
        acc = acc + pad[threads * k:threads * (k + 1)]
    v = acc.reshape(threads // 64, 64, K)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o, :]
    s = np.zeros(K)
    for wv in range(threads // 64):
        s = s + v[wv, 0]
    return s


def _sum3(p0, p1, p2):
    return (p0 + p1) + p2


def _per_point(off, C):
    """[n_points, K]: the rows of C [n_edges, K] added per point in ascending edge order, from zero"""
    return _per_point_ranges(off[:-1].astype(np.int64), off[1:].astype(np.int64), C)


def _per_point_ranges(lo, hi, C):
    s = np.zeros((len(lo), C.shape[1]))
    for k in range(int((hi - lo).max()) if len(lo) else 0):
        sel = lo + k < hi
        s[sel] = s[sel] + C[(lo + k)[sel]]
    return s


def edge_status(graph, off, edge_state):
    """the status of every edge (0: kept) and the counters of the dropped"""
    st = np.asarray(edge_state, np.int64)
    status, res = np.zeros(len(st), np.int32), np.zeros(8, np.int32)
    for l in range(len(off) - 1):
        lo, hi = int(off[l]), int(off[l + 1])
        if hi - lo > MAX_OBS:
            status[lo:hi] = R_REFUSED
            res[R_REFUSED] += 1
            continue
        seen = set()
        for e in range(lo, hi):
            s = int(st[e])
            if not 0 <= s < graph.n:
                status[e] = R_RANGE
            elif s in seen:
                status[e] = R_DUPLICATE
            seen.add(s)
    for code in (R_DONE, R_RANGE, R_DUPLICATE):
        res[code] = (status == code).sum()
    return status, res


def linearize(graph, cal, cam, n_solve, P, edge_state, edge_point, z, w, active=None, delta=HUBER_MONO, threshold=CHI2_MONO, mode=0, H_diag=None,
              b=None):
    """orbvw_linearize_device.  H_diag [n, 15, 15], b [n, 15]: what the arrays hold before the call (mode 0; copied).  Returns a dict of
    point_off, err, chi2, result and, by mode, total (0, 1), H_diag, b, Hll, bl, Hlp and the Jacobians Jp, Jl (0) or outlier (2)."""
    P, z, w = np.asarray(P, F64).reshape(-1, 3), np.asarray(z, F64).reshape(-1, 2), np.asarray(w, F64).reshape(-1)
    n_points, ne = len(P), len(w)
    st = np.asarray(edge_state, np.int64)
    off, eff = point_ranges(edge_point, n_points)
    status, res = edge_status(graph, off, st)
    kept = status == 0
    err, chi2 = np.zeros((ne, 2)), np.zeros(ne)
    Jp, Jl, free = np.zeros((ne, 2, 6)), np.zeros((ne, 2, 3)), np.zeros(ne, bool)
    for s in np.unique(st[kept]):
        idx = np.nonzero(kept & (st == s))[0]
        Rcw, tcw, Rcb, tbc = vm.derive_pose(cal, graph.Rwb[s], graph.twb[s])
        Pc, e, c2 = vm.edge_errors(cam, Rcw, tcw, P[eff[idx]], z[idx], w[idx])
        err[idx], chi2[idx] = e, c2
        if mode != 0:
            continue
        pj = vm.proj_jacobian(cam, *Pc)
        with np.errstate(all="ignore"):
            for r in range(2):
                for c in range(3):
                    Jl[idx, r, c] = _sum3(-pj[:, r, 0] * Rcw[0, c], -pj[:, r, 1] * Rcw[1, c], -pj[:, r, 2] * Rcw[2, c])
        if s < n_solve and not int(graph.fixed[s]) & fm.FIX_POSE:
            Jp[idx], free[idx] = vm.edge_jacobian(cam, Rcb, tbc, Pc), True
    o = dict(point_off=off, err=err, chi2=chi2, result=res, status=status)
    finite = np.isfinite(err).all(1) & np.isfinite(chi2)
    if mode == 2:
        with np.errstate(all="ignore"):
            o["outlier"] = (kept & (chi2 > threshold)).astype(np.uint8)
        res[R_OUTLIER], res[R_NONFINITE] = o["outlier"].sum(), (kept & ~finite).sum()
        return o
    act = np.ones(ne, bool) if active is None else np.asarray(active)[:ne] != 0
    res[R_NONFINITE] = (kept & act & ~finite).sum()
    used = kept & act & finite
    rho, rw = vm.huber(chi2, delta)
    o["total"] = vm.block_sum(np.where(used[:, None], np.stack([chi2, rho], 1), 0.0))
    o["used"] = used
    if mode != 0:
        return o
    with np.errstate(all="ignore"):
        W = rw * w
        C = np.where(used[:, None], vm.edge_contributions(Jp, W, err), 0.0)
        WJp, WJl, we = W[:, None, None] * Jp, W[:, None, None] * Jl, W[:, None] * err
        Hlp = np.stack([Jl[:, 0, r] * WJp[:, 0, c] + Jl[:, 1, r] * WJp[:, 1, c] for r in range(3) for c in range(6)], 1)
        hl = np.stack([Jl[:, 0, r] * WJl[:, 0, c] + Jl[:, 1, r] * WJl[:, 1, c] for r in range(3) for c in range(r, 3)], 1)
        gl = np.stack([Jl[:, 0, r] * we[:, 0] + Jl[:, 1, r] * we[:, 1] for r in range(3)], 1)
    o["H_diag"], o["b"] = np.array(H_diag, F64).reshape(graph.n, 15, 15), np.array(b, F64).reshape(graph.n, 15)
    for s in range(n_solve):
        if int(graph.fixed[s]) & fm.FIX_POSE:
            continue
        sums = vm.block_sum(np.where((st == s)[:, None], C, 0.0))
        for k, (r, c) in enumerate(vm.UPPER):
            o["H_diag"][s, r, c] = o["H_diag"][s, r, c] + sums[k]
            if r != c:
                o["H_diag"][s, c, r] = o["H_diag"][s, c, r] + sums[k]
        o["b"][s, :6] = o["b"][s, :6] - sums[21:]
    o["Hlp"] = np.where((used & free)[:, None], Hlp, 0.0)
    h = _per_point(off, np.where(used[:, None], hl, 0.0))
    o["Hll"] = h[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
    o["bl"] = 0.0 - _per_point(off, np.where(used[:, None], gl, 0.0))
    o["Jp"], o["Jl"], o["W"] = Jp, Jl, W
    return o


# ---- the Schur complement -----------------------------------------------------------------------------------------------------------------
def point_inverse(Hll, bl, lam):
    """((Hll + lambda I)^-1 by cofactors [n, 9], its product with bl [n, 3]); zero where the determinant is not finite or not > 0"""
    h, bl = np.asarray(Hll, F64).reshape(-1, 9), np.asarray(bl, F64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a, b, c, d, e, f = h[:, 0] + lam, h[:, 1], h[:, 2], h[:, 4] + lam, h[:, 5], h[:, 8] + lam
        c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
        det = _sum3(a * c00, b * c01, c * c02)
        ok = np.isfinite(det) & (det > 0.0)
        i = 1.0 / det
        m = np.stack([c00 * i, c01 * i, c02 * i, c01 * i, (a * f - c * c) * i, (b * c - a * e) * i, c02 * i, (b * c - a * e) * i, (a * d - b * b) * i], 1)
        m = np.where(ok[:, None], m, 0.0)
        tl = np.stack([_sum3(m[:, 3 * r] * bl[:, 0], m[:, 3 * r + 1] * bl[:, 1], m[:, 3 * r + 2] * bl[:, 2]) for r in range(3)], 1)
    return m, np.where(ok[:, None], tl, 0.0)


def _ranges(point_off, cap_edges):
    off = np.clip(np.asarray(point_off, np.int64), 0, cap_edges)
    return off[:-1], np.maximum(off[:-1], off[1:])


def reduce(n_solve, fixed, edges, cap, H_diag, H_off, b, lam, point_off, edge_state, Hll, bl, Hlp, cap_edges):
    """orbvw_reduce_device: a dict of S, rhs, Hll_inv, tl, h_max (d_out[1]), result"""
    fixed = np.asarray(fixed)[:n_solve]
    H_diag, b = np.asarray(H_diag, F64).reshape(-1, 15, 15)[:n_solve], np.asarray(b, F64).reshape(-1, 15)[:n_solve]
    S, rhs, _, h_max, dropped = vm.assemble(fixed, edges, cap, H_diag, H_off, b, lam)
    Hll, Hlp = np.asarray(Hll, F64).reshape(-1, 9), np.asarray(Hlp, F64).reshape(-1, 3, 6)
    n_points = len(Hll)
    inv, tl = point_inverse(Hll, bl, lam)
    skipped = ~(inv != 0.0).any(1)
    h_max = max([h_max] + [float(v) for v in Hll[:, [0, 4, 8]].reshape(-1) if v > h_max])
    st = np.asarray(edge_state, np.int64)
    lo, hi = _ranges(point_off, cap_edges)
    edge_of = np.full((n_solve, n_points), -1, np.int64)
    for l in range(n_points):
        if hi[l] - lo[l] > MAX_OBS:
            continue
        for e in range(int(hi[l]) - 1, int(lo[l]) - 1, -1):
            if 0 <= st[e] < n_solve:
                edge_of[st[e], l] = e
    m = inv.reshape(-1, 3, 3)
    for i in range(n_solve):
        for j in range(i, n_solve):
            if int(fixed[i]) & fm.FIX_POSE or int(fixed[j]) & fm.FIX_POSE:
                continue
            sel = np.nonzero((edge_of[i] >= 0) & (edge_of[j] >= 0) & ~skipped)[0]
            A, B, M = Hlp[edge_of[i][sel]], Hlp[edge_of[j][sel]], m[sel]
            C = np.zeros((n_points, 42))
            with np.errstate(all="ignore"):
                Cm = [[_sum3(M[:, r, 0] * B[:, 0, c], M[:, r, 1] * B[:, 1, c], M[:, r, 2] * B[:, 2, c]) for c in range(6)] for r in range(3)]
                for r in range(6):
                    for c in range(6):
                        C[sel, 6 * r + c] = _sum3(A[:, 0, r] * Cm[0][c], A[:, 1, r] * Cm[1][c], A[:, 2, r] * Cm[2][c])
                    if i == j:
                        C[sel, 36 + r] = _sum3(A[:, 0, r] * tl[sel, 0], A[:, 1, r] * tl[sel, 1], A[:, 2, r] * tl[sel, 2])
            sums = block_sum(C, SCHUR_THREADS)
            for r in range(6):
                for c in range(6):
                    if i == j and r > c:
                        continue
                    p, q = (15 * i + r, 15 * j + c), (15 * j + c, 15 * i + r)
                    S[p] = S[p] - sums[6 * r + c]
                    if p != q:
                        S[q] = S[q] - sums[6 * r + c]
                if i == j:
                    rhs[15 * i + r] = rhs[15 * i + r] - sums[36 + r]
    res = np.zeros(8, np.int32)
    res[R_DONE], res[R_RANGE], res[R_POINT_SINGULAR] = 1, dropped, skipped.sum()
    return dict(S=S, rhs=rhs, Hll_inv=inv, tl=tl, h_max=h_max, result=res, skipped=skipped)


def solve(S, rhs, b, lam):
    """orbvw_solve_device: (dx [n, 15], (d_out[0], d_out[2]), result).  Only the lower triangle of S is read."""
    rhs, b = np.asarray(rhs, F64).reshape(-1), np.asarray(b, F64).reshape(-1)[:len(np.asarray(rhs).reshape(-1))]
    x, pivot = vm.ordered_cholesky_solve(np.asarray(S, F64), rhs)
    res = np.zeros(8, np.int32)
    if x is None:
        res[R_REFUSED] = 1
        return np.zeros((len(rhs) // 15, 15)), (0.0, pivot), res
    res[R_DONE] = 1
    scale = 0.0
    for j in range(len(rhs)):
        scale = scale + x[j] * (lam * x[j] + b[j])
    return x.reshape(-1, 15), (scale, pivot), res


def backsub(n_solve, point_off, edge_state, Hlp, Hll_inv, bl, dx, lam, P, cap_edges):
    """orbvw_backsub_device: a dict of xl, points_out, scale (d_out_points[0]), result"""
    P, bl, inv = np.asarray(P, F64).reshape(-1, 3), np.asarray(bl, F64).reshape(-1, 3), np.asarray(Hll_inv, F64).reshape(-1, 9)
    Hlp, dx, st = np.asarray(Hlp, F64).reshape(-1, 3, 6), np.asarray(dx, F64).reshape(-1, 15), np.asarray(edge_state, np.int64)
    skipped = ~(inv != 0.0).any(1)
    lo, hi = _ranges(point_off, cap_edges)
    on = (st >= 0) & (st < n_solve)
    q = np.zeros((len(st), 3))
    with np.errstate(all="ignore"):
        for r in range(3):
            p = np.zeros(int(on.sum()))
            for c in range(6):
                p = p + Hlp[on, r, c] * dx[st[on], c]
            q[on, r] = p
        hi_used = np.where(hi - lo > MAX_OBS, lo, hi)
        s = _per_point_ranges(lo, hi_used, q)
        r_ = bl - s
        x = np.stack([_sum3(inv[:, 3 * r] * r_[:, 0], inv[:, 3 * r + 1] * r_[:, 1], inv[:, 3 * r + 2] * r_[:, 2]) for r in range(3)], 1)
        x = np.where(skipped[:, None], 0.0, x)
        c_l = _sum3(x[:, 0] * (lam * x[:, 0] + bl[:, 0]), x[:, 1] * (lam * x[:, 1] + bl[:, 1]), x[:, 2] * (lam * x[:, 2] + bl[:, 2]))
    scale = vm.block_sum(np.where(skipped, 0.0, c_l)[:, None])[0]
    res = np.zeros(8, np.int32)
    res[R_DONE], res[R_POINT_SINGULAR] = (~skipped).sum(), skipped.sum()
    return dict(xl=x, points_out=np.where(skipped[:, None], P, P + x), scale=scale, result=res)


# ---- one iteration ---------------------------------------------------------------------------------------------------------------------------
def iterate(sc, lam, graph=None, points=None):
    """one model iteration of the chain of include/orbvw.h from (graph, points): both linearisations, reduce, solve, backsub, oplus and
    the errors at the trial point.  Returns a dict of the stages' outputs; `before` and `after` are the robustified totals."""
    g = sc["graph"] if graph is None else graph
    P = sc["points"] if points is None else points
    ns, ne = sc["n_solve"], len(sc["edge_state"])
    vis = lambda gr, pts, mode, **kw: linearize(gr, sc["cal"], sc["cam"], ns, pts, sc["edge_state"], sc["edge_point"], sc["z"], sc["w"], mode=mode, **kw)  # noqa: E731
    oi = vm.inertial_linearize(sc, g)
    ov = vis(g, P, 0, H_diag=oi["H_diag"], b=oi["b"])
    rd = reduce(ns, g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], lam, ov["point_off"], sc["edge_state"], ov["Hll"],
                ov["bl"], ov["Hlp"], ne)
    dx, (scale, pivot), sres = solve(rd["S"], rd["rhs"], ov["b"][:ns], lam)
    bs = backsub(ns, ov["point_off"], sc["edge_state"], ov["Hlp"], rd["Hll_inv"], ov["bl"], dx, lam, P, ne)
    g1 = g.copy()
    full = np.zeros((g.n, 15))
    full[:ns] = dx
    fm.oplus(g1, full)
    oi1, ov1 = vm.inertial_linearize(sc, g1, 1), vis(g1, bs["points_out"], 1)
    return dict(inertial=oi, visual=ov, reduce=rd, dx=dx, scale=scale, pivot=pivot, solve_result=sres, backsub=bs, graph=g1, inertial1=oi1, visual1=ov1,
                before=oi["total"][1] + ov["total"][1], after=oi1["total"][1] + ov1["total"][1])


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
def window_scene(n_solve, n_fixed, n_points, seed=1, model=0, min_obs=None, depth=(2.0, 12.0), fixed_offset=0.3, outlier_share=vm.OUTLIER_SHARE,
                 pixel_noise=1.0, sample_counts=fm.SAMPLE_COUNTS):
    """localFullBundleAdjustment's graph: factors_model.make_chain with walks (n_solve states, all free), the three priors on state 0 with
    the acc prior weighted by gyro_info (Optimize.cpp:1189), n_fixed fixed key frames appended near the chain's states, and n_points map
    points stored as floats widened, point l in front of solve state l mod n_solve and seen by 1 to 6 of the states that have it in view
    (point 0 by exactly one).  The measurements
    come from poses a little off the graph's (2e-3 rad, 2 cm) and points 2 cm off, with pixel noise kp.size * N(0, 1) per axis and
    vi_model.OUTLIER_SHARE of them four times that: something for an iteration to gain, chi2 on both sides of the Huber threshold.
    The keywords are for the closed-loop scenes of tests/inertial_loop.py; their defaults give the scene above, byte for byte.  min_obs:
    every point (point 0 too) is seen by at least that many states; depth: the range of the points' depths; fixed_offset: how far the
    fixed key frames sit from the chain's states (m); outlier_share and pixel_noise (a factor on kp.size * N(0, 1)): the measurements;
    sample_counts: factors_model.make_chain's."""
    rng = np.random.RandomState(7000 + 100 * seed + 13 * model + n_points)
    sc = dict(fm.make_chain(n_solve - 1, seed=seed, walks=True, sample_counts=sample_counts))
    sc["priors"], sc["prior_info_jobs"], _ = fm.make_priors(sc, [0])
    sc["pjobs"] = np.array([(0, 0, fm.PRIOR_VELO | fm.PRIOR_GYRO | fm.PRIOR_ACC | fm.PRIOR_ACC_GYRO_INFO)], fm.PRIOR_JOB)
    cam = vm.FISHEYE if model else vm.PINHOLE
    chain, n = sc["graph"], n_solve + n_fixed
    g = fm.Graph(n)
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        getattr(g, k)[:n_solve] = getattr(chain, k)
    for f in range(n_fixed):
        one = fm.Graph(1)
        one.Rwb[0], one.twb[0] = chain.Rwb[f % n_solve], chain.twb[f % n_solve]
        fm.oplus(one, np.concatenate([rng.normal(0, 0.03, 3), rng.normal(0, fixed_offset, 3), np.zeros(9)])[None])
        g.Rwb[n_solve + f], g.twb[n_solve + f], g.fixed[n_solve + f] = one.Rwb[0], one.twb[0], 15
    truth = g.copy()
    truth.fixed[:] = 0
    step = np.zeros((n, 15))
    step[:n_solve, :6] = rng.normal(0, 1.0, (n_solve, 6)) * np.array([2e-3] * 3 + [2e-2] * 3)
    fm.oplus(truth, step)
    cal = sc["cal"]
    poses = [vm.derive_pose(cal, truth.Rwb[s], truth.twb[s])[:2] for s in range(n)]
    depth = rng.uniform(depth[0], depth[1], n_points)
    span = 0.3 if model == 0 else 0.6
    Pc = np.stack([rng.uniform(-span, span, n_points) * depth, rng.uniform(-span, span, n_points) * depth, depth], 1)
    anchor = np.arange(n_points) % n_solve
    P = np.stack([(Pc[l] - poses[a][1]) @ poses[a][0] for l, a in enumerate(anchor)]).astype(np.float32).astype(F64)   # building the scene, not part of the model
    Pt = P + rng.normal(0, 0.02, P.shape)
    es, ep, zs, ws = [], [], [], []
    for l in range(n_points):
        cams = [(Rcw @ Pt[l] + tcw) for Rcw, tcw in poses]
        view = [s for s, c in enumerate(cams) if c[2] > 1.0 and abs(c[0]) < 0.9 * c[2] and abs(c[1]) < 0.9 * c[2]]
        assert anchor[l] in view
        if min_obs is None:
            k = 1 if l == 0 else min(int(rng.randint(1, 7)), len(view))
        else:
            k = min(max(int(rng.randint(1, 7)), min_obs), len(view))
        for s in sorted(rng.choice(view, k, replace=False).tolist()):
            size = np.float32(31.0) * np.float32(1.2) ** np.float32(rng.randint(0, 8))
            u, v = vm.project(cam, *cams[s])
            noise = rng.normal(0.0, 1.0, 2) * float(size) * (4.0 if rng.uniform() < outlier_share else 1.0) * pixel_noise
            es.append(s), ep.append(l), ws.append(F64(np.float32(1.0) / size / size))
            zs.append((np.array([u, v]) + noise).astype(np.float32).astype(F64))
    sc.update(graph=g, cam=cam, n_solve=n_solve, n_fixed=n_fixed, n_points=n_points, points=P, edge_state=np.array(es, np.int32),
              edge_point=np.array(ep, np.int32), z=np.array(zs, F64).reshape(-1, 2), w=np.array(ws, F64))
    ne = len(es)
    counts = np.bincount(sc["edge_point"], minlength=n_points)
    assert counts.max() <= 6 and ((counts == 1).any() and counts.min() >= 1 if min_obs is None else counts.min() >= min_obs)
    it = iterate(sc, 1.0)
    c2 = it["visual"]["chi2"]
    if ne >= 100 and pixel_noise >= 1.0 and outlier_share > 0:
        assert (c2 > HUBER_MONO ** 2).sum() >= 3 and (c2 <= HUBER_MONO ** 2).sum() > ne // 2       # both Huber branches
        assert (c2 > CHI2_MONO).any() and (c2 <= CHI2_MONO).any()                               # both sides of the classification
    assert it["solve_result"][R_DONE] == 1 and it["pivot"] > 0 and not it["reduce"]["skipped"].any()   # no pivot refused at lambda = 1
    assert it["after"] < it["before"], (it["before"], it["after"])                              # one iteration gains
    sc["first"] = it
    return sc
