"""Plain numpy restatement of what LocalMapping::createNewMapPoints does with the matches of one key-frame pair (include/orbm.h,
orbm_triangulate_matches_device), written from the reference: LocalMapping.cpp:171-253 (projection matrices, the gates in their
order), TwoViewReconstruction.cpp:689-705 (Triangulate), MapPoint.cpp:16-30, :43-76, :83-91 (constructor, update(), the
...Invariance getters), Pinhole.cpp:34-42 and Fisheye.cpp:52-73 (project / backProject), Pose.cpp:12-14 (camera centre).
`evaluate` runs the formulas in float32 (singular vectors from LAPACK's float SVD) or in float64 (the yardstick); both start from
the poses ROUNDED TO FLOAT, as the reference holds them.  `make_cloud` builds the seeded two-view clouds the test files use.
No part of the library is used here."""
import numpy as np

from projection_model import FISHEYE, KP_DTYPE, N_LEVELS, PINHOLE, SCALE_FACTORS, H, W, _rodrigues

SIGMA2 = (SCALE_FACTORS * SCALE_FACTORS).astype(np.float32)          # ORBExtractor::getSquareSigmas()
MAX_SCALE_FACTOR = SCALE_FACTORS[N_LEVELS - 1]                        # ORBExtractor.h:53-55
RATIO_FACTOR = np.float32(1.5) * SCALE_FACTORS[1]                     # LocalMapping.cpp:156
COS_PARALLAX, CHI2 = 0.99998, 5.991                                   # LocalMapping.cpp:201, :216 (double literals)
# gate codes = index of the counter in d_result; -1 = feature without a match.  1 (overflow) is no gate.
ACCEPTED, FAIL, ILLEGAL, PARALLAX, NEGATIVE, REPROJ, SCALE = 0, 2, 3, 4, 5, 6, 7
GATES = (ILLEGAL, PARALLAX, NEGATIVE, REPROJ, SCALE)
N_FAR, N_NONFINITE = 12, 6                                             # make_cloud: points beyond useful parallax, non-finite key points


def fisheye_scale_table(cam, w=W, h=H):
    """A stand-in for the reference's scale_mat (Fisheye.cpp:21-30: [height][width] floats, read at [(int) y][(int) x] by
    backProject, :71): tan(theta) / theta_d at the pixel's centre-less integer position, theta from the undistorted radius.  Only
    its role matters here -- a caller-supplied table the back-projection multiplies with."""
    fx, fy, cx, cy, k1, k2, k3, k4 = cam
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    td = np.hypot((u - cx) / fx, (v - cy) / fy)
    th = td.copy()
    for _ in range(10):                                               # Newton on theta_d(theta) = td
        th2 = th * th
        f = th * (1 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)))) - td
        df = 1 + th2 * (3 * k1 + th2 * (5 * k2 + th2 * (7 * k3 + th2 * 9 * k4)))
        th = th - f / df
    s = np.where(td > 1e-9, np.tan(th) / np.maximum(td, 1e-9), 1.0)
    return s.astype(np.float32)


def _project(D, cam, X, Y, Z):
    f = lambda v: D(np.float32(v))  # noqa: E731
    fx, fy, cx, cy = (f(v) for v in cam[:4])
    a, b = X / Z, Y / Z
    if len(cam) == 4:                                                 # Pinhole.cpp:34-38
        return fx * a + cx, fy * b + cy
    k = [f(c) for c in cam[4:]]                                       # Fisheye.cpp:52-66
    r = np.sqrt(a * a + b * b)
    theta = np.arctan(r)
    theta2 = theta * theta
    theta3 = theta * theta2
    theta5 = theta2 * theta3
    theta7 = theta2 * theta5
    theta9 = theta2 * theta7
    theta_d = (((theta + k[0] * theta3) + k[1] * theta5) + k[2] * theta7) + k[3] * theta9
    return ((fx * theta_d) * a) / r + cx, ((fy * theta_d) * b) / r + cy


def _back_project(D, cam, scale_table, x, y):
    f = lambda v: D(np.float32(v))  # noqa: E731
    fx, fy, cx, cy = (f(v) for v in cam[:4])
    inv_fx, inv_fy = D(np.float32(1) / np.float32(cam[0])), D(np.float32(1) / np.float32(cam[1]))   # Camera: float inv_fx = 1.f / fx
    xn, yn = (x - cx) * inv_fx, (y - cy) * inv_fy                     # Pinhole.cpp:40-42
    if len(cam) == 8:                                                 # Fisheye.cpp:68-73; the index is kept inside the table
        h, w = scale_table.shape
        xi = np.clip(np.nan_to_num(x, nan=0.0, posinf=w - 1, neginf=0.0), 0, w - 1).astype(np.int64)
        yi = np.clip(np.nan_to_num(y, nan=0.0, posinf=h - 1, neginf=0.0), 0, h - 1).astype(np.int64)
        s = scale_table[yi, xi].astype(D)
        xn, yn = xn * s, yn * s
    return xn, yn


def evaluate(cam, scale_table, R1, t1, R2, t2, kps1, kps2, desc2, matches12, n_points=0, sigma2=SIGMA2,
             max_scale_factor=MAX_SCALE_FACTOR, cos_parallax=COS_PARALLAX, chi2=CHI2, ratio_factor=RATIO_FACTOR, dtype=np.float32):
    """Gate code per feature of key frame 1 (-1 without a match) and, for the accepted matches in ascending feature order, the rows
    the reference's MapPoint constructor would hold: points, normals, min_dist / max_dist (the ...Invariance values), descriptor,
    observation pair; `result` are the eight counters of d_result (overflow left 0); `index` the table row of every accepted
    feature counted from n_points."""
    D = dtype
    with np.errstate(all="ignore"):
        m12 = np.asarray(matches12, np.int64)
        n1 = len(m12)
        idx1 = np.flatnonzero((m12 >= 0) & (m12 < len(kps2)))          # :180
        idx2 = m12[idx1]
        k1, k2 = kps1[idx1], kps2[idx2]
        Rf = [np.asarray(R, np.float64).reshape(3, 3).astype(np.float32).astype(D) for R in (R1, R2)]
        tf = [np.asarray(t, np.float64).reshape(3).astype(np.float32).astype(D) for t in (t1, t2)]
        x1, y1, x2, y2 = (a.astype(D) for a in (k1["x"], k1["y"], k2["x"], k2["y"]))
        xn1, yn1 = _back_project(D, cam, scale_table, x1, y1)          # :183-184
        xn2, yn2 = _back_project(D, cam, scale_table, x2, y2)
        P = [np.concatenate([Rf[v], tf[v][:, None]], 1) for v in (0, 1)]   # :172-174
        A = np.stack([xn1[:, None] * P[0][2] - P[0][0], yn1[:, None] * P[0][2] - P[0][1],
                      xn2[:, None] * P[1][2] - P[1][0], yn2[:, None] * P[1][2] - P[1][1]], 1)   # TwoViewReconstruction.cpp:692-696
        Ph = np.full((len(idx1), 4), np.nan, D)
        ok = np.isfinite(A).all((1, 2))                                # a non-finite matrix gives a non-finite vector (:698-699)
        if ok.any():
            Ph[ok] = np.linalg.svd(A[ok])[2][:, 3, :]
        code = np.zeros(len(idx1), np.int32)
        live = np.ones(len(idx1), bool)

        def gate(mask, c):
            hit = live & mask
            code[hit] = c
            live[hit] = False

        gate(Ph[:, 3] == 0, FAIL)                                      # :700
        Pw = Ph[:, :3] / Ph[:, 3:4]                                    # :703
        gate(~np.isfinite(Pw).all(1), ILLEGAL)                         # LocalMapping.cpp:187
        O = [np.stack([-((Rf[v][0, k] * tf[v][0] + Rf[v][1, k] * tf[v][1]) + Rf[v][2, k] * tf[v][2]) for k in range(3)]) for v in (0, 1)]
        nv, dist = [], []
        for v in (0, 1):                                               # :193-198
            d = Pw - O[v]
            n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            nv.append(d / n[:, None])
            dist.append(n)
        cosp = (nv[0][:, 0] * nv[1][:, 0] + nv[0][:, 1] * nv[1][:, 1]) + nv[0][:, 2] * nv[1][:, 2]
        gate(cosp.astype(np.float64) > cos_parallax, PARALLAX)         # :201 (float against a double literal)
        s2 = np.asarray(sigma2, np.float32).astype(D)
        lv = [np.clip(k["octave"], 0, len(s2) - 1) for k in (k1, k2)]
        err, pcz = [], []
        view = np.zeros(len(idx1), np.int32)                           # the key frame (1 | 2) whose depth / re-projection test rejected
        for v, (x, y) in enumerate(((x1, y1), (x2, y2))):              # :207-234
            pc = [((Rf[v][k, 0] * Pw[:, 0] + Rf[v][k, 1] * Pw[:, 1]) + Rf[v][k, 2] * Pw[:, 2]) + tf[v][k] for k in range(3)]
            view[live] = v + 1
            gate(pc[2] <= 0, NEGATIVE)
            u, w_ = _project(D, cam, pc[0], pc[1], pc[2])
            e = (u - x) * (u - x) + (w_ - y) * (w_ - y)
            gate(e.astype(np.float64) > s2[lv[v]].astype(np.float64) * chi2, REPROJ)   # float * double literal
            err.append(e)
            pcz.append(pc[2])
        dist_ratio = dist[0] / dist[1]                                 # :236-241
        level_ratio = np.sqrt(s2[lv[1]]) / np.sqrt(s2[lv[0]])
        rf = D(np.float32(ratio_factor))
        gate((dist_ratio * rf < level_ratio) | (dist_ratio > level_ratio * rf), SCALE)
        acc = code == ACCEPTED
        span = dist[1] * k2["size"].astype(D)                          # MapPoint.cpp:71, reference key frame = the current one (:18)
        out_code = np.full(n1, -1, np.int32)
        out_code[idx1] = code
        index = np.full(n1, -1, np.int64)
        index[idx1[acc]] = n_points + np.arange(acc.sum())
        res = np.zeros(8, np.int32)
        res[0] = acc.sum()
        for c in (FAIL,) + GATES:
            res[c] = (code == c).sum()
        out = dict(code=out_code, result=res, index=index, feat1=idx1[acc], feat2=idx2[acc], points=Pw[acc],
                   normals=((nv[0] + nv[1]) / D(2))[acc],              # MapPoint.cpp:57-63, :73
                   max_dist=(D(np.float32(1.2)) * span)[acc],          # :88-91
                   min_dist=(D(np.float32(0.8)) * (span / D(np.float32(max_scale_factor))))[acc],   # :72, :83-86
                   desc=np.asarray(desc2)[idx2[acc]], obs=np.stack([idx1[acc], idx2[acc]], 1).astype(np.int32),
                   dist2=dist[1][acc],
                   # intermediates over all matches (row k belongs to feature idx1[k]) the tests reason with
                   all_feat1=idx1, all_code=code, cosp=cosp, err1=err[0], err2=err[1], pcz1=pcz[0], pcz2=pcz[1],
                   view=np.where(live, 0, view), dist_ratio=dist_ratio, level_ratio=level_ratio)
    return out


def apply_to_slots(e, mp1, mp2, has1, has2):
    """What the call leaves in the two key frames' slot arrays and flags (LocalMapping.cpp:245-246)."""
    mp1, mp2, has1, has2 = mp1.copy(), mp2.copy(), has1.copy(), has2.copy()
    rows = e["index"][e["feat1"]]
    mp1[e["feat1"]], mp2[e["feat2"]] = rows, rows
    has1[e["feat1"]], has2[e["feat2"]] = 1, 1
    return mp1, mp2, has1, has2


def run_model(cloud, dtype=np.float32, **over):
    return evaluate(cloud["cam"], cloud["scale_table"], cloud["R1"], cloud["t1"], cloud["R2"], cloud["t2"], cloud["kps1"], cloud["kps2"],
                    cloud["desc2"], cloud["matches12"], n_points=cloud["n_points"], dtype=dtype, **over)


def threshold_band(cloud, e64, which, rel=1e-4):
    """Matches whose float64 gate code changes when ONE threshold (which = 0 the parallax cosine, 1 the chi-square bound, 2
    ratioFactor) moves by +-rel relative (mask over the features of key frame 1)."""
    band = np.zeros(len(e64["code"]), bool)
    for s in (1 + rel, 1 - rel):
        over = [dict(cos_parallax=COS_PARALLAX * s), dict(chi2=CHI2 * s), dict(ratio_factor=float(RATIO_FACTOR) * s)][which]
        band |= run_model(cloud, np.float64, **over)["code"] != e64["code"]
    return band


def make_cloud(fisheye, n, seed, baseline=3.0, mismatched_octaves=False, margin=40):
    """Two posed views of n world points 3 - 80 m deep, both key frames holding one feature per point in shuffled order (plus
    unmatched features); pixel noise of 0.8 px times the level's scale factor (the
    chi-square gate then rejects about 1 % of the right pairings too); about 10 % of the matches pair a feature with
    another point's feature; a few points behind the far plane of useful parallax, a few behind a camera after the wrong pairing,
    and N_NONFINITE key points of key frame 1 with a non-finite x (the `illegal` gate).  mismatched_octaves draws the two octaves
    independently, so that the scale-consistency gate fires."""
    rng = np.random.RandomState(seed)
    camd = FISHEYE if fisheye else PINHOLE
    cam = camd["cam"]
    table = fisheye_scale_table(cam) if fisheye else None
    R1, t1 = _rodrigues(np.array([0.01, -0.02, 0.005])), np.array([0.1, -0.05, 0.02])
    R2 = _rodrigues(np.array([-0.015, 0.03, -0.01]))
    t2 = t1 + np.array([-baseline, 0.06 * baseline, 0.15 * baseline])   # camera 2 to the right of camera 1, a little behind it
    # points in camera 1's frame, through pixels at least `margin` columns inside the image (a wide Fisheye image reaches towards
    # the epipole, where no depth has parallax)
    px, py = rng.uniform(margin, W - margin, n), rng.uniform(40, H - 40, n)
    depth = np.exp(rng.uniform(np.log(3.0), np.log(80.0), n))
    far = rng.choice(n, N_FAR, replace=False)
    depth[far] = rng.uniform(400.0, 2000.0, N_FAR) * baseline          # parallax far below the limit: cos > 0.99998
    fx, fy, cx, cy = cam[:4]
    if fisheye:
        s = table[py.astype(int), px.astype(int)].astype(np.float64)
    else:
        s = 1.0
    Pc1 = np.stack([(px - cx) / fx * s, (py - cy) / fy * s, np.ones(n)], 1) * depth[:, None]
    Pw = (Pc1 - t1) @ R1                                               # R1^T (Pc1 - t1)
    octave1 = rng.randint(0, N_LEVELS, n)
    octave2 = rng.randint(0, N_LEVELS, n) if mismatched_octaves else np.clip(octave1 + rng.randint(-1, 2, n), 0, N_LEVELS - 1)

    def view(R, t, octave):
        pc = Pw @ R.T + t
        u, v = _project(np.float64, cam, pc[:, 0], pc[:, 1], pc[:, 2])
        noise = 0.8 * SCALE_FACTORS[octave].astype(np.float64)
        return u + rng.normal(size=n) * noise, v + rng.normal(size=n) * noise

    u1, v1 = view(R1, t1, octave1)
    u2, v2 = view(R2, t2, octave2)
    n1, n2 = n + n // 5, n + n // 4                                    # features without a partner on both sides
    slot1, slot2 = rng.permutation(n1)[:n], rng.permutation(n2)[:n]

    def record(nk, slot, u, v, octave):
        k = np.zeros(nk, KP_DTYPE)
        k["x"], k["y"] = rng.uniform(0, W, nk), rng.uniform(0, H, nk)
        k["octave"] = rng.randint(0, N_LEVELS, nk)
        k["x"][slot], k["y"][slot], k["octave"][slot] = u, v, octave
        k["x"], k["y"] = np.clip(k["x"], 0, W - 1), np.clip(k["y"], 0, H - 1)
        k["size"] = SCALE_FACTORS[k["octave"]]
        k["angle"] = rng.uniform(0, 360, nk)
        return k

    kps1, kps2 = record(n1, slot1, u1, v1, octave1), record(n2, slot2, u2, v2, octave2)
    partner = np.arange(n)
    wrong = rng.choice(n, n // 10, replace=False)
    partner[wrong] = partner[np.roll(wrong, 1)]                        # still one-to-one, as SearchForTriangulation leaves it
    matches12 = np.full(n1, -1, np.int32)
    matches12[slot1] = slot2[partner]
    bad = slot1[rng.choice(n, N_NONFINITE, replace=False)]
    kps1["x"][bad] = np.resize(np.array([np.inf, np.nan, -np.inf], np.float32), N_NONFINITE)
    desc2 = rng.randint(0, 256, (n2, 32)).astype(np.uint8)
    n_points = 37
    return dict(cam=cam, bounds=camd["bounds"], scale_table=table, R1=R1, t1=t1, R2=R2, t2=t2, kps1=kps1, kps2=kps2, desc2=desc2,
                matches12=matches12, n1=n1, n2=n2, n_points=n_points, fisheye=fisheye)

