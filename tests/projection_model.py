"""Plain numpy restatement of the arithmetic behind the projection-search queries (include/orbm.h, orbm_project_*_device), written
from the reference: Pose::map / Pose.cpp:12-14, Pinhole.cpp:34-47, Fisheye.cpp:52-78, Frame.cpp:129-166 (isInFrustum),
MapPoint.cpp:159-170 (predictScaleLevel), ORBMatcher.cpp:212-229, :355-365, :534-553, Tracking.cpp:403-412.  `evaluate` runs the
same formulas in float32 (the model the device is compared with) or in float64 (the yardstick the model is judged by); both start
from the pose ROUNDED TO FLOAT, as the reference holds it.  `make_cloud` builds the seeded clouds both test files use.
No part of the library is used here."""
import numpy as np

FRAME, FRUSTUM, FUSE = "frame", "frustum", "fuse"
W, H = 752, 480
PINHOLE = dict(cam=(460.0, 460.0, 376.0, 240.0), bounds=(8.0, 744.0, 6.0, 474.0))       # bounds of an undistorted image (Pinhole.cpp:22-25)
FISHEYE = dict(cam=(300.0, 300.0, 376.0, 240.0, 0.0034, 0.0007, -0.0002, 0.00003), bounds=(0.0, float(W), 0.0, float(H)))
N_LEVELS = 8
SCALE_FACTORS = np.cumprod(np.concatenate([[np.float32(1)], np.full(N_LEVELS - 1, np.float32(1.2))])).astype(np.float32)
LOG_SCALE_FACTOR = np.float32(np.log(np.float32(1.2)))       # ORBExtractor.h:109-115: float tables
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
# stated distances from a gate's threshold inside which float32 and float64 may decide differently
TOL_DEPTH_REL, TOL_PIXEL, TOL_DIST_REL, TOL_COS, TOL_LEVEL = 1e-5, 2e-3, 1e-5, 1e-5, 1e-4


def evaluate(form, cam, bounds, R, t, points, valid, kps1=None, normals=None, min_dist=None, max_dist=None, frame_mp=None,
             scale_factors=SCALE_FACTORS, log_scale_factor=LOG_SCALE_FACTOR, th=1.0, view_cos_limit=0.5, dtype=np.float32):
    """Returns the builder's outputs (q_ok, q_xy, q_radius, q_level, q_angle, view_cos, result) plus the intermediates the tests
    reason with (code = the gate that rejected the point, 0 = on; pcz, u, v, dist, dot, vcos, x_level, th_c)."""
    D = dtype
    f = lambda v: D(np.float32(v))  # noqa: E731  (a float parameter of the reference, widened when D is float64)
    with np.errstate(all="ignore"):
        Rf = np.asarray(R, np.float64).reshape(3, 3).astype(np.float32).astype(D)
        tf = np.asarray(t, np.float64).reshape(3).astype(np.float32).astype(D)
        P = np.asarray(points, np.float32).reshape(-1, 3).astype(D)
        n = len(P)
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        pc = [((Rf[k, 0] * x + Rf[k, 1] * y) + Rf[k, 2] * z) + tf[k] for k in range(3)]
        ow = [-((Rf[0, k] * tf[0] + Rf[1, k] * tf[1]) + Rf[2, k] * tf[2]) for k in range(3)]
        fx, fy, cx, cy = (f(v) for v in cam[:4])
        a, b = pc[0] / pc[2], pc[1] / pc[2]
        if len(cam) == 4:
            u, v = fx * a + cx, fy * b + cy
        else:
            k = [f(c) for c in cam[4:]]
            r = np.sqrt(a * a + b * b)
            theta = np.arctan(r)
            theta2 = theta * theta
            theta3 = theta * theta2
            theta5 = theta2 * theta3
            theta7 = theta2 * theta5
            theta9 = theta2 * theta7
            theta_d = (((theta + k[0] * theta3) + k[1] * theta5) + k[2] * theta7) + k[3] * theta9
            u, v = ((fx * theta_d) * a) / r + cx, ((fy * theta_d) * b) / r + cy
        outside = (u < f(bounds[0])) | (u >= f(bounds[1])) | (v < f(bounds[2])) | (v >= f(bounds[3]))
        code = np.zeros(n, np.int32)
        live = np.ones(n, bool)

        def gate(mask, c):
            hit = live & mask
            code[hit] = c
            live[hit] = False

        gate(np.asarray(valid) == 0, 1)
        g = 2
        if form == FRUSTUM:
            fm = np.asarray(frame_mp, np.int64)
            seen = np.zeros(n, bool)
            seen[fm[(fm >= 0) & (fm < n)]] = True
            gate(seen, 2)
            g = 3
        gate(pc[2] < 0, g)
        gate(outside, g + 1)
        out = dict(code=code, pcz=pc[2], u=u, v=v)
        level = np.zeros(n, np.int32)
        angle = np.zeros(n, np.float32)
        vcos = np.zeros(n, D)
        if form == FRAME:
            radius = f(th) * kps1["size"].astype(D)
            level = kps1["octave"].astype(np.int32)
            angle = kps1["angle"].astype(np.float32)
        else:
            N = np.asarray(normals, np.float32).reshape(-1, 3).astype(D)
            mind, maxd = np.asarray(min_dist, np.float32).astype(D), np.asarray(max_dist, np.float32).astype(D)
            ox, oy, oz = x - ow[0], y - ow[1], z - ow[2]
            dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
            dot = (ox * N[:, 0] + oy * N[:, 1]) + oz * N[:, 2]
            gate((dist < mind) | (dist > maxd), g + 2)
            if form == FRUSTUM:
                vcos = dot / dist
                gate(vcos < f(view_cos_limit), g + 3)
                th_c = f(th) * np.where(vcos.astype(np.float64) > 0.998, D(2.5), D(4.0))   # ORBMatcher.cpp:362-364
            else:
                gate(dot < D(0.5) * dist, g + 3)
                th_c = np.full(n, f(th), D)
            sf = np.asarray(scale_factors, np.float32).astype(D)
            x_level = np.log(maxd / dist) / f(log_scale_factor)
            c = np.nan_to_num(np.ceil(x_level), nan=0.0, posinf=len(sf) - 1, neginf=0.0)
            level = np.clip(c, 0, len(sf) - 1).astype(np.int32)
            radius = th_c * sf[level]
            out.update(dist=dist, dot=dot, x_level=x_level, th_c=th_c, sf=sf)
        on = code == 0
        z32 = lambda arr, dt: np.where(on, arr, 0).astype(dt)  # noqa: E731
        out.update(q_ok=on.astype(np.uint8), q_xy=np.stack([z32(u, D), z32(v, D)], 1), q_radius=z32(radius, D), q_level=z32(level, np.int32),
                   q_angle=z32(angle, np.float32), view_cos=z32(vcos, D), vcos=vcos)
        res = np.bincount(code, minlength=8)[:8].astype(np.int32)
        if form == FRUSTUM:
            res[7] = res[3:7].sum()
        out["result"] = res
    return out


def near_threshold(form, cloud, e64):
    """Per gate: the points within the stated distance of its threshold in the float64 evaluation (dict of bool masks)."""
    with np.errstate(all="ignore"):
        P = cloud["points"].astype(np.float64)
        b = cloud["bounds"]
        scale = np.abs(P).sum(1) + np.abs(np.asarray(cloud["t"], np.float64)).max() + 1.0
        m = dict(depth=np.abs(e64["pcz"]) < TOL_DEPTH_REL * scale,
                 image=(np.abs(e64["u"] - b[0]) < TOL_PIXEL) | (np.abs(e64["u"] - b[1]) < TOL_PIXEL) |
                       (np.abs(e64["v"] - b[2]) < TOL_PIXEL) | (np.abs(e64["v"] - b[3]) < TOL_PIXEL))
        if form != FRAME:
            d = e64["dist"]
            m["dist"] = (np.abs(d - cloud["min_dist"]) < TOL_DIST_REL * d) | (np.abs(d - cloud["max_dist"]) < TOL_DIST_REL * d)
            if form == FRUSTUM:
                m["angle"] = np.abs(e64["vcos"] - np.float32(cloud["view_cos_limit"])) < TOL_COS
                m["radius_class"] = np.abs(e64["vcos"] - 0.998) < TOL_COS
            else:
                m["angle"] = np.abs(e64["dot"] - 0.5 * d) < TOL_DIST_REL * d
            xl = e64["x_level"]
            m["level"] = np.isfinite(xl) & (np.abs(xl - np.round(xl)) < TOL_LEVEL)
    return m


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _rays(cam, px, py):
    """unit-depth (Pinhole) or unit-length (Fisheye, distortion ignored) camera-frame directions through pixels"""
    if len(cam) == 4:
        return np.stack([(px - cam[2]) / cam[0], (py - cam[3]) / cam[1], np.ones_like(px)], 1)
    dx, dy = (px - cam[2]) / cam[0], (py - cam[3]) / cam[1]
    th = np.hypot(dx, dy)
    s = np.where(th > 0, np.sin(th) / np.maximum(th, 1e-12), 1.0)
    return np.stack([s * dx, s * dy, np.cos(th)], 1)


N_ON_BOUND = 12   # candidates placed on the image bounds: 3 per bound


def make_cloud(form, fisheye, n, seed):
    """A seeded cloud in which every gate of `form` rejects at least 2 % of the points and at least 30 % pass: invalid entries,
    points behind the camera, outside the image, outside their distance range, seen too obliquely; for the frustum form indices
    already in frame_mp and frame_mp entries outside [0, n); and N_ON_BOUND candidates bisected (in float32, with the model) onto
    the image bounds -- `on_bound` marks those whose model projection lies EXACTLY on a bound."""
    rng = np.random.RandomState(seed)
    camd = FISHEYE if fisheye else PINHOLE
    cam, bounds = camd["cam"], camd["bounds"]
    R = _rodrigues(np.array([0.05, -0.08, 0.03]))
    t = np.array([0.3, -0.2, 0.5])
    kind = rng.choice(3, size=n, p=[0.76, 0.10, 0.14])     # 0 in view, 1 behind the camera, 2 outside the image
    kind[:N_ON_BOUND] = 0
    px = rng.uniform(bounds[0] + 12, bounds[1] - 12, n)
    py = rng.uniform(bounds[2] + 12, bounds[3] - 12, n)
    side = rng.randint(0, 4, n)
    off = rng.uniform(1.0, 60.0, n)
    o = kind == 2
    px = np.where(o & (side == 0), bounds[0] - off, np.where(o & (side == 1), bounds[1] + off, px))
    py = np.where(o & (side == 2), bounds[2] - off, np.where(o & (side == 3), bounds[3] + off, py))
    which = np.arange(N_ON_BOUND) % 4                       # bound of candidate j: min_x, max_x, min_y, max_y
    px[:N_ON_BOUND] = np.where(which == 0, bounds[0], np.where(which == 1, bounds[1], px[:N_ON_BOUND]))
    py[:N_ON_BOUND] = np.where(which == 2, bounds[2], np.where(which == 3, bounds[3], py[:N_ON_BOUND]))
    depth = np.exp(rng.uniform(np.log(2.0), np.log(20.0), n))
    Pc = _rays(cam, px, py) * depth[:, None]
    Pc[kind == 1] *= -1.0
    Pw = ((Pc - t) @ R).astype(np.float32)                  # R^T (Pc - t)
    valid = (rng.uniform(size=n) > 0.05).astype(np.uint8)
    valid[:N_ON_BOUND] = 1
    cloud = dict(form=form, cam=cam, bounds=bounds, R=R, t=t, points=Pw, valid=valid, th=3.0, view_cos_limit=0.5, n=n)
    if form == FRAME:
        kps = np.zeros(n, KP_DTYPE)
        kps["octave"] = rng.randint(0, N_LEVELS, n)
        kps["size"] = SCALE_FACTORS[kps["octave"]]
        kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        kps["x"], kps["y"] = rng.uniform(0, W, n), rng.uniform(0, H, n)
        cloud.update(kps1=kps, th=7.0)
    else:
        Ow = -R.T @ t
        OP = Pw.astype(np.float64) - Ow
        d0 = np.linalg.norm(OP, axis=1)
        xl = rng.uniform(-0.6, 8.6, n)                      # log_1.2(max_dist / dist): < 0 too far, > 8 too close, > 7 clamped
        xl[:N_ON_BOUND] = rng.uniform(0.2, 7.8, N_ON_BOUND)
        max_dist = d0 * 1.2 ** xl
        dirs = OP / d0[:, None]
        e = np.cross(dirs, rng.normal(size=(n, 3)))
        e /= np.linalg.norm(e, axis=1)[:, None]
        alpha = np.radians(rng.uniform(0.0, 75.0, n))       # viewing angle: the limit 0.5 is 60 degrees, 0.998 is 3.6 degrees
        alpha[:N_ON_BOUND] = np.radians(rng.uniform(0.0, 50.0, N_ON_BOUND))
        normals = np.cos(alpha)[:, None] * dirs + np.sin(alpha)[:, None] * e
        cloud.update(normals=normals.astype(np.float32), max_dist=max_dist.astype(np.float32),
                     min_dist=(max_dist / 1.2 ** 8).astype(np.float32))
    if form == FRUSTUM:
        n2 = 2500
        fm = np.full(n2, -1, np.int32)
        held = rng.choice(np.arange(N_ON_BOUND, n), size=int(0.08 * n), replace=False)
        slots = rng.choice(n2, size=len(held) + 40, replace=False)
        fm[slots[:len(held)]] = held
        fm[slots[len(held):]] = np.resize(np.array([-7, n, n + 5, 2 ** 30, -2 ** 31, 2 ** 31 - 1], np.int64), 40).astype(np.int32)
        cloud.update(frame_mp=fm, n2=n2, th=1.0)
    _bisect_onto_bounds(cloud, which)
    return cloud


def model_inputs(cloud):
    keys = ("kps1", "normals", "min_dist", "max_dist", "frame_mp", "th", "view_cos_limit")
    return dict({k: cloud[k] for k in keys if k in cloud})


def run_model(cloud, dtype=np.float32):
    return evaluate(cloud["form"], cloud["cam"], cloud["bounds"], cloud["R"], cloud["t"], cloud["points"], cloud["valid"], dtype=dtype,
                    **model_inputs(cloud))


def _bisect_onto_bounds(cloud, which):
    """Moves candidate j along world x (bounds in u) or y (bounds in v) to the smallest float32 coordinate whose MODEL projection is
    >= its bound; where that projection equals the bound the point lies exactly on it.  A Fisheye candidate whose in-image decision
    does not flip between the model and float64 is pushed half a pixel inside instead: the device's atanf may differ from numpy's
    by an ulp there, and only flipping points are outside the comparison."""
    m = N_ON_BOUND
    axis = np.where(which < 2, 0, 1)
    target = np.asarray(cloud["bounds"], np.float32)[which]
    sub = dict(cloud, points=cloud["points"][:m].copy(), valid=cloud["valid"][:m])
    for k in ("kps1", "normals", "min_dist", "max_dist"):
        if k in cloud:
            sub[k] = cloud[k][:m]
    if "frame_mp" in cloud:
        sub["frame_mp"] = np.zeros(0, np.int32)

    def coord(vals):
        sub["points"][np.arange(m), axis] = vals
        e = run_model(sub)
        return np.where(which < 2, e["u"], e["v"])

    c0 = cloud["points"][np.arange(m), axis].copy()
    span = np.float32(0.05) * (np.abs(c0) + np.float32(1))
    lo, hi = (c0 - span).astype(np.float32), (c0 + span).astype(np.float32)
    at_lo, at_hi = coord(lo), coord(hi)
    assert (at_lo < target).all() and (at_hi >= target).all()
    px_per_unit = (at_hi - at_lo) / (hi - lo)
    for _ in range(64):
        mid = (lo.astype(np.float64) / 2 + hi.astype(np.float64) / 2).astype(np.float32)
        mid = np.where((mid <= lo) | (mid >= hi), lo, mid)
        ge = coord(mid) >= target
        hi = np.where(ge & (mid > lo), mid, hi)
        lo = np.where(~ge, mid, lo)
    got = coord(hi)
    exact = got == target
    if len(cloud["cam"]) == 8:
        e64 = run_model(sub, np.float64)
        img = 4 if cloud["form"] == FRUSTUM else 3          # the image gate's code
        e32 = run_model(sub)
        flips = (e32["code"] == img) != (e64["code"] == img)
        keep = exact & flips
        inward = np.where(which % 2 == 0, 1.0, -1.0) * 0.5   # half a pixel towards the image centre, as a step of the coordinate
        moved = (hi + inward / px_per_unit).astype(np.float32)
        hi = np.where(keep, hi, moved)
        exact = keep
        coord(hi)
    else:
        coord(hi)
    cloud["points"][:m] = sub["points"]
    on = np.zeros(cloud["n"], bool)
    on[:m] = exact
    cloud["on_bound"] = on
    cloud["on_bound_which"] = which
