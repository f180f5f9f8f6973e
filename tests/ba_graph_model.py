"""The second problem builder of the visual bundle adjustment's tests (csrc/orbba.hip) -- TEST INFRASTRUCTURE ONLY, numpy only.

synth.make_ba_problem, which every other BA test draws from, puts the fixed poses first, lets every pose see every point and lists a
point's edges in ascending pose order.  A local BA graph is none of that (Optimize.cpp:826-845, :867-868), and several kernels change
path exactly there.  make_graph starts from the same scene and then
  * keeps edge (pose k, point j) only if |k - centre_j| <= band, centre_j random per point: edge_of is mostly -1, most 6x6 blocks of the
    reduced system are exactly zero, points are left with 0, 1 or 2 observations;
  * puts a few points at depths from 0.6 m to about 400 m in front of a pose: block magnitudes span orders of magnitude;
  * trims chosen poses to an exact edge count (0, 1, 255, 256, 257: k_ba_reduce_pose strides by 256);
  * shuffles the edges inside each point (they stay grouped by point);
  * fixes poses by layout: "every_third" (k % 3 == 1), "reference" (pose 0, then the free ones, then a fixed block at the end, as
    Optimize.cpp:826-845 lists them) or "first" -- the "every_third" graph with its poses RELABELLED so that the fixed ones lead, the
    layout of synth.make_ba_problem: the same graph under another numbering, for the metamorphic checks;
  * rotates and shifts every free pose by se3_exp of a small 6-vector and moves the points, as test_ba._perturbed does: no entry of a
    free R is structurally 0.
Every step draws from a RandomState of its own, so shuffle=False gives the same graph with each point's edges in ascending pose order.

Besides the builder: linearize_ld, a np.longdouble restatement of ba_ref.linearize with its per-edge contributions (explicit elementwise
expressions and add.at, nothing through LAPACK), and dense_step, the damped step solved on the full unmarginalised system -- a second
float64 route to the step the oracle takes through the Schur complement.

GRAPHS records each graph's jitter sensitivity delta in the manner of test_ba_lm_paths.CASES (tests/test_ba_graphs_cpu.py re-measures
it), LOCAL_BA the same for the two graphs that run Optimize.cpp:892-922.

What the device was held to (tests/test_ba_graphs_gpu.py prints these; measured on an MI355X, the larger of the two Cholesky variants).
(a) per edge: the largest row-relative error against the longdouble model, device / float64 oracle, the bar being 4 x the oracle's;
blocks: the largest error / derived bar over the entries (bar 1).  (c): the step's deviation from the dense solve / its bar, and the
bar itself (4 x the larger of the Schur route's deviation and the jitter sensitivity), at lambda0, 1.0 and 1e6 lambda0.

  graph                 delta    (a) chi2             error                H_lp                 H_pp     b_p      H_ll    b_l
  fisheye_16x257_b1     1.1e-13  8.10e-13 / 8.10e-13  4.46e-13 / 4.46e-13  1.15e-14 / 1.26e-14  0.0040   0.0012   0.011   0.043
  reference_24x257_b2   4.2e-12  4.79e-13 / 4.79e-13  4.00e-13 / 4.00e-13  5.03e-14 / 5.03e-14  0.0063   0.077    0.013   0.040
  reference_3x255_b1    1.8e-14  3.37e-13 / 3.37e-13  3.40e-13 / 3.40e-13  1.70e-14 / 2.65e-14  0.00065  0.00086  0.012   0.12
  third_12x256_b1       1.8e-14  3.16e-13 / 3.16e-13  1.95e-13 / 1.95e-13  2.66e-14 / 2.68e-14  0.0030   0.0021   0.012   0.027
  third_35x1025_b3      9.1e-15  5.67e-13 / 5.67e-13  4.61e-13 / 4.61e-13  3.27e-14 / 3.30e-14  0.0015   0.0012   0.0092  0.052
  third_36x300_b2       2.0e-14  4.79e-13 / 4.57e-13  2.61e-13 / 2.94e-13  2.43e-14 / 2.93e-14  0.0048   0.0034   0.0085  0.027
  trim_12x1025_b2       4.9e-15  1.66e-12 / 1.66e-12  1.92e-12 / 1.92e-12  2.77e-14 / 2.77e-14  0.00039  0.0038   0.0029  0.050

  graph                 (c) lambda0: ratio (bar)   1.0: ratio (bar)    1e6 lambda0: ratio (bar)
  fisheye_16x257_b1     0.086 (6.4e-14)            0.109 (7.7e-14)     0.038 (3.6e-15)
  reference_24x257_b2   0.014 (2.4e-13)            0.071 (2.5e-11)     0.042 (3.2e-15)
  reference_3x255_b1    0.052 (1.9e-14)            0.050 (1.2e-12)     0.030 (3.7e-15)
  third_12x256_b1       0.033 (5.6e-14)            0.093 (7.4e-14)     0.042 (3.2e-15)
  third_35x1025_b3      0.034 (7.7e-14)            0.102 (7.3e-14)     0.036 (3.7e-15)
  third_36x300_b2       0.019 (6.3e-14)            0.164 (2.0e-13)     0.036 (3.6e-15)
  trim_12x1025_b2       0.046 (2.8e-14)            0.059 (5.6e-13)     0.042 (3.1e-15)

The per-edge figures of device and oracle mostly coincide: the library is built without contraction, so both round the same
expressions alike, and the worst row of a graph is an edge whose residual is small against its pixel coordinates.  (d): every graph
and both local-BA graphs reproduce the oracle's (iterations, trials) -- 5 / 5, and 15 / 15 over both rounds -- and its outlier flags
(19 and 131); estimates differ by at most 1.6e-10 relative (reference_24x257_b2, local BA), 1.3e-12 elsewhere.
"""
import numpy as np

from monoorbslam3_amd import synth

HUBER = float(np.sqrt(np.float32(5.991)))


# ----------------------------------------------------------------------------------------------------------------- the builder
def _project(cam, pc):
    from oracle import ba_ref
    return ba_ref.project(cam, np.asarray(pc, np.float64).reshape(1, 3))[0]


def _size(camera):
    return (512, 512) if camera == "fisheye" else (1242, 375)


def make_graph(n_poses, n_points, seed, band, layout="every_third", camera="pinhole", shuffle=True, trim=None, lone=(0, 0), n_depth=6,
               tail=4, rot=0.01, trans=0.05, pts=0.05):
    """-> dict(args = (cam, R, t, fixed, P, edge_pose, edge_point, z, w) as ba_ref.lm_optimize takes them, new_of_old = the relabelling
    ("first": new index of each pose of the "every_third" graph; the identity otherwise), edge_order = for each edge its index in the
    unshuffled graph).  trim: {pose of the unrelabelled graph: exact edge count}; lone: (points stripped of every observation, points
    stripped to one), for a camera that sees everything; tail: fixed poses at the end ("reference")."""
    from oracle import ba_ref
    pr = synth.make_ba_problem(n_poses, n_points, seed=seed, n_fixed=0, camera=camera)
    cam = pr["cam"]
    R0 = np.array(pr["pose_R"], np.float64).reshape(-1, 3, 3)
    t0 = np.array(pr["pose_t"], np.float64).reshape(-1, 3)
    P = np.array(pr["points"], np.float64).reshape(-1, 3).copy()
    ep, el = np.asarray(pr["edge_pose"]), np.asarray(pr["edge_point"])
    z, w = np.asarray(pr["edge_z"], np.float64).reshape(-1, 2), np.asarray(pr["edge_inv_sigma2"], np.float64)
    # banded visibility
    rng = np.random.RandomState(seed + 101)
    centre = rng.randint(0, n_poses, n_points)
    keep = np.abs(ep - centre[el]) <= band
    ep, el, z, w = ep[keep], el[keep], z[keep], w[keep]
    # a few points at depths of 0.6 m to about 400 m in front of their centre pose, seen by the poses of their band that they project into
    rng = np.random.RandomState(seed + 202)
    width, height = _size(camera)
    deep = rng.choice(n_points, min(n_depth, n_points), replace=False)
    depths = np.geomspace(0.6, 400.0, len(deep))
    for j, d in zip(deep, depths):
        k0 = centre[j]
        pc = np.array([rng.uniform(-0.2, 0.2) * d, rng.uniform(-0.1, 0.1) * d, d])
        P[j] = R0[k0].T @ (pc - t0[k0])
        gone = el == j
        ep, el, z, w = ep[~gone], el[~gone], z[~gone], w[~gone]
        for k in range(max(0, k0 - band), min(n_poses, k0 + band + 1)):
            q = R0[k] @ P[j] + t0[k]
            if q[2] <= 0.5:
                continue
            uv = _project(cam, q)
            if 0 <= uv[0] < width and 0 <= uv[1] < height:
                sig = np.float32(1.2) ** rng.randint(0, 8)
                ep, el = np.append(ep, k), np.append(el, j)
                z = np.vstack([z, uv + rng.normal(0, 1.0, 2)])
                w = np.append(w, float(np.float32(1.0) / np.float32(sig) / np.float32(sig)))
    order = np.lexsort((ep, el))                                     # grouped by point, ascending pose inside a point
    ep, el, z, w = ep[order], el[order], z[order], w[order]
    # exact edge counts for the chosen poses
    rng = np.random.RandomState(seed + 303)
    keep = np.ones(len(ep), bool)
    for k, count in sorted((trim or {}).items()):
        mine = np.flatnonzero(ep == k)
        assert len(mine) >= count, "pose %d has %d edges, fewer than %d" % (k, len(mine), count)
        keep[rng.choice(mine, len(mine) - count, replace=False)] = False
    seen = np.flatnonzero(np.bincount(el, minlength=n_points) >= 2)
    for n, j in enumerate(rng.choice(seen, lone[0] + lone[1], replace=False)):
        mine = np.flatnonzero((el == j) & keep)
        keep[mine[:len(mine) if n < lone[0] else len(mine) - 1]] = False
    ep, el, z, w = ep[keep], el[keep], z[keep], w[keep]
    # the fixed poses
    fixed = np.zeros(n_poses, np.uint8)
    if layout in ("every_third", "first"):
        fixed[1::3] = 1
    elif layout == "reference":
        fixed[0] = 1
        fixed[n_poses - tail:] = 1
    else:
        raise ValueError(layout)
    # the estimates: every free pose moved generally, the points moved
    rng = np.random.RandomState(seed + 404)
    R, t = R0.copy(), t0.copy()
    for i in np.flatnonzero(fixed == 0):
        dR, dt = ba_ref.se3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))
        R[i], t[i] = dR @ R0[i], dR @ t0[i] + dt
    P = P + rng.normal(0, pts, P.shape)
    # the order of the edges inside each point
    edge_order = np.arange(len(ep))
    if shuffle:
        rng = np.random.RandomState(seed + 505)
        off = np.searchsorted(el, np.arange(n_points + 1))
        for j in range(n_points):
            edge_order[off[j]:off[j + 1]] = off[j] + rng.permutation(off[j + 1] - off[j])
        ep, el, z, w = ep[edge_order], el[edge_order], z[edge_order], w[edge_order]
    # "first": the same graph, fixed poses numbered first
    new_of_old = np.arange(n_poses)
    if layout == "first":
        old_of_new = np.concatenate([np.flatnonzero(fixed == 1), np.flatnonzero(fixed == 0)])
        new_of_old = np.empty(n_poses, int)
        new_of_old[old_of_new] = np.arange(n_poses)
        R, t, fixed = R[old_of_new], t[old_of_new], fixed[old_of_new]
        ep = new_of_old[ep]
    args = (cam, R, t, fixed, P, ep.astype(np.int32), el.astype(np.int32), np.ascontiguousarray(z), np.ascontiguousarray(w))
    return dict(args=args, new_of_old=new_of_old, edge_order=edge_order)


def structure(args):
    """what the structure conditions are asserted from: counts taken from the arrays alone"""
    fixed, P, ep, el = np.asarray(args[3], bool), np.asarray(args[4]).reshape(-1, 3), np.asarray(args[5]), np.asarray(args[6])
    free = np.flatnonzero(~fixed)
    slot = -np.ones(len(fixed), int)
    slot[free] = np.arange(len(free))
    n_obs = np.bincount(el, minlength=len(P))
    n_free_obs = np.bincount(el[~fixed[ep]], minlength=len(P))
    per_pose = np.bincount(ep, minlength=len(fixed))
    seen = np.zeros((len(free), len(P)), bool)
    seen[slot[ep[~fixed[ep]]], el[~fixed[ep]]] = True
    shared = (seen.astype(np.int64) @ seen.T.astype(np.int64)) > 0
    off = np.searchsorted(el, np.arange(len(P) + 1))
    between = 0
    for j in range(len(P)):
        f = fixed[ep[off[j]:off[j + 1]]]
        fr = np.flatnonzero(~f)
        between += bool(len(fr) >= 2 and f[fr[0]:fr[-1]].any())
    return dict(n_free=len(free), n_edges=len(ep), obs0=int((n_obs == 0).sum()), obs1=int((n_obs == 1).sum()), obs2=int((n_obs == 2).sum()),
                fixed_only=int(((n_obs > 0) & (n_free_obs == 0)).sum()), free_edge_counts=per_pose[free], empty_cells=float(1.0 - seen.mean()),
                unshared_pairs=int((~shared).sum() // 2), fixed_between_free=between,
                grouped=bool((np.diff(el) >= 0).all()), free_pose_is_affine=bool(len(set(free - np.arange(len(free)))) == 1))


# ----------------------------------------------------------------------------------------------------------------- the graphs
def _graph(make, delta, promise, iterations=5):
    """make: make_graph's arguments; delta: the recorded jitter sensitivity of lm_optimize(Huber, iterations) on it; promise: what the
    structure test holds it to besides the conditions common to all -- n_free, free_counts (edge counts that some free pose has exactly),
    and sparse = False for a graph too small to have an empty block"""
    return dict(make=make, delta=delta, promise=promise, iterations=iterations)


GRAPHS = {
    # 23 free poses: the largest reduced system in LDS; 1025 points, about 5 500 edges
    "third_35x1025_b3": _graph(dict(n_poses=35, n_points=1025, seed=3, band=3), 9.1e-15, dict(n_free=23, obs=(207, 10, 7), fixed_only=4)),
    # 24 free poses: the first one in global memory
    "third_36x300_b2": _graph(dict(n_poses=36, n_points=300, seed=4, band=2, trim={35: 0}), 2.0e-14,
                              dict(n_free=24, free_counts=(0,), obs=(61, 1, 6), fixed_only=0)),
    # Optimize.cpp:826-845: pose 0 fixed, 19 free ones, 4 fixed ones at the end
    "reference_24x257_b2": _graph(dict(n_poses=24, n_points=257, seed=5, band=2, layout="reference", trim={9: 1}), 4.2e-12,
                                  dict(n_free=19, free_counts=(1,), obs=(50, 0, 4), fixed_only=20)),
    # one free pose between two fixed ones
    "reference_3x255_b1": _graph(dict(n_poses=3, n_points=255, seed=6, band=1, layout="reference", tail=1), 1.8e-14,
                                 dict(n_free=1, sparse=False, obs=(38, 13, 145), fixed_only=2)),
    # free poses with exactly 0, 1, 255, 256 and 257 edges
    "trim_12x1025_b2": _graph(dict(n_poses=12, n_points=1025, seed=7, band=2, trim={11: 0, 3: 1, 5: 255, 6: 256, 8: 257}), 4.9e-15,
                              dict(n_free=8, free_counts=(0, 1, 255, 256, 257), obs=(173, 19, 113), fixed_only=11)),
    "third_12x256_b1": _graph(dict(n_poses=12, n_points=256, seed=8, band=1), 1.8e-14, dict(n_free=8, obs=(41, 5, 38), fixed_only=2)),
    "fisheye_16x257_b1": _graph(dict(n_poses=16, n_points=257, seed=9, band=1, camera="fisheye", lone=(9, 5), trim={15: 0}), 1.1e-13,
                                dict(n_free=11, free_counts=(0,), obs=(9, 16, 39), fixed_only=0)),
}
# Optimize.cpp:892-922 (both rounds) on the "reference" layout and on the 23-free-pose graph: the recorded delta of both rounds
LOCAL_BA = {"reference_24x257_b2": 1.9e-10, "third_35x1025_b3": 3.1e-14}
# the device form against the host form
DEVICE_FORM = ("reference_24x257_b2", "third_36x300_b2", "fisheye_16x257_b1")

_memo = {}


def graph(name, **change):
    """GRAPHS[name] built once, shared, never changed; change: make_graph's arguments to replace (shuffle=False, layout="first")"""
    key = (name, tuple(sorted(change.items())))
    if key not in _memo:
        _memo[key] = make_graph(**dict(GRAPHS[name]["make"], **change))
    return _memo[key]


# ----------------------------------------------------------------------------------------------------------------- the longdouble model
LD = np.longdouble


def _ld(a):
    return np.asarray(a, np.float64).astype(LD)


def _project_ld(cam, X, Y, Z):
    fx, fy, cx, cy = (LD(v) for v in cam[:4])
    if len(cam) == 4:
        return fx * (X / Z) + cx, fy * (Y / Z) + cy
    k = [LD(float(np.float32(v))) for v in cam[4:8]]
    a, b = X / Z, Y / Z
    r = np.sqrt(a * a + b * b)
    th = np.arctan(r)
    th2 = th * th
    thd = th * (1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
    return fx * thd * a / r + cx, fy * thd * b / r + cy


def _proj_jacobian_ld(cam, X, Y, Z):
    """-> the six entries j00 j01 j02 j10 j11 j12 (Pinhole.cpp:49-53, Fisheye.cpp:83-108)"""
    fx, fy = LD(cam[0]), LD(cam[1])
    zero = np.zeros_like(X)
    if len(cam) == 4:
        return fx / Z, zero, -fx * X / (Z * Z), zero, fy / Z, -fy * Y / (Z * Z)
    k = [LD(float(np.float32(v))) for v in cam[4:8]]
    x2, y2, z2 = X * X, Y * Y, Z * Z
    r2 = x2 + y2
    r = np.sqrt(r2)
    r3 = r2 * r
    th = np.arctan2(r, Z)
    th2 = th * th
    f = th * (1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
    fd = 1 + th2 * (3 * k[0] + th2 * (5 * k[1] + th2 * (7 * k[2] + th2 * 9 * k[3])))
    den = r2 * (r2 + z2)
    j00 = fx * (fd * Z * x2 / den + f * y2 / r3)
    j01 = fx * (fd * Z * Y * X / den - f * Y * X / r3)
    j10 = fy * (fd * Z * Y * X / den - f * Y * X / r3)
    j11 = fy * (fd * Z * y2 / den + f * x2 / r3)
    return j00, j01, -fx * fd * X / (r2 + z2), j10, j11, -fy * fd * Y / (r2 + z2)


def linearize_ld(cam, pose_R, pose_t, pose_fixed, points, edge_pose, edge_point, edge_z, edge_inv_sigma2, huber_delta):
    """ba_ref.linearize in np.longdouble (64-bit mantissa: 2^-11 of a float64 rounding), written out entry by entry.  Returns the arrays
    ba_ref.linearize returns and the per-edge CONTRIBUTIONS to the reduced blocks, c_H_pp [E,6,6], c_b_p [E,6], c_H_ll [E,3,3], c_b_l [E,3] -- each the sum of two
    products, one per row of the residual -- and a_*, the sum of those two products' magnitudes."""
    ep, el = np.asarray(edge_pose), np.asarray(edge_point)
    R = _ld(pose_R).reshape(-1, 3, 3)[ep]
    t = _ld(pose_t).reshape(-1, 3)[ep]
    P = _ld(points).reshape(-1, 3)[el]
    z = _ld(edge_z).reshape(-1, 2)
    om = _ld(edge_inv_sigma2)
    n_e = len(ep)
    Pc = [R[:, r, 0] * P[:, 0] + R[:, r, 1] * P[:, 1] + R[:, r, 2] * P[:, 2] + t[:, r] for r in range(3)]
    X, Y, Z = Pc
    u, v = _project_ld(cam, X, Y, Z)
    e = np.stack([z[:, 0] - u, z[:, 1] - v], 1)
    chi2 = om * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    rw = np.ones(n_e, LD)
    if huber_delta > 0:
        d = LD(huber_delta)
        out = chi2 > d * d
        rw[out] = d / np.sqrt(chi2[out])
    W = rw * om
    jp = _proj_jacobian_ld(cam, X, Y, Z)
    Jl = np.zeros((n_e, 2, 3), LD)
    Jq = np.zeros((n_e, 2, 6), LD)
    for r in range(2):
        a, b, c = jp[3 * r], jp[3 * r + 1], jp[3 * r + 2]
        for col in range(3):
            Jl[:, r, col] = -(a * R[:, 0, col] + b * R[:, 1, col] + c * R[:, 2, col])
        Jq[:, r, 0] = b * Z - c * Y
        Jq[:, r, 1] = -a * Z + c * X
        Jq[:, r, 2] = a * Y - b * X
        Jq[:, r, 3], Jq[:, r, 4], Jq[:, r, 5] = -a, -b, -c
    fixed = np.asarray(pose_fixed, bool)[ep]
    free_e = np.where(fixed, LD(0), LD(1))

    # every entry is a two-term sum over the residual's rows; `mag` is the sum of the two terms' magnitudes
    def outer(A, B):
        out, mag = np.zeros((n_e, A.shape[2], B.shape[2]), LD), np.zeros((n_e, A.shape[2], B.shape[2]), LD)
        for i in range(A.shape[2]):
            for j in range(B.shape[2]):
                p0, p1 = W * (A[:, 0, i] * B[:, 0, j]), W * (A[:, 1, i] * B[:, 1, j])
                out[:, i, j], mag[:, i, j] = p0 + p1, np.abs(p0) + np.abs(p1)
        return out, mag

    def against_error(A):
        out, mag = np.zeros((n_e, A.shape[2]), LD), np.zeros((n_e, A.shape[2]), LD)
        for i in range(A.shape[2]):
            p0, p1 = -W * (A[:, 0, i] * e[:, 0]), -W * (A[:, 1, i] * e[:, 1])
            out[:, i], mag[:, i] = p0 + p1, np.abs(p0) + np.abs(p1)
        return out, mag

    c_Hpp, a_Hpp = (v * free_e[:, None, None] for v in outer(Jq, Jq))
    c_bp, a_bp = (v * free_e[:, None] for v in against_error(Jq))
    (c_Hll, a_Hll), (c_bl, a_bl) = outer(Jl, Jl), against_error(Jl)
    Hlp = outer(Jl, Jq)[0] * free_e[:, None, None]
    n_p, n_l = len(np.asarray(pose_fixed)), len(np.asarray(points).reshape(-1, 3))
    H_pp, b_p = np.zeros((n_p, 6, 6), LD), np.zeros((n_p, 6), LD)
    H_ll, b_l = np.zeros((n_l, 3, 3), LD), np.zeros((n_l, 3), LD)
    np.add.at(H_pp, ep, c_Hpp)
    np.add.at(b_p, ep, c_bp)
    np.add.at(H_ll, el, c_Hll)
    np.add.at(b_l, el, c_bl)
    return {"chi2": chi2, "error": e, "H_pp": H_pp, "b_p": b_p, "H_ll": H_ll, "b_l": b_l, "H_lp": Hlp,
            "c_H_pp": c_Hpp, "c_b_p": c_bp, "c_H_ll": c_Hll, "c_b_l": c_bl, "a_H_pp": a_Hpp, "a_b_p": a_bp, "a_H_ll": a_Hll, "a_b_l": a_bl}


def row_error(got, want):
    """the largest error of a row of `got` relative to the largest magnitude in the same row of the longdouble `want` (rows: the last
    axis; a scalar per edge is its own row); a row that is all zero in `want` has to be exactly zero: inf otherwise"""
    want = np.asarray(want, LD)
    got = np.asarray(got, np.float64).astype(LD).reshape(want.shape)
    if want.ndim == 1:
        want, got = want[:, None], got[:, None]
    scale = np.abs(want).max(-1)
    err = np.abs(got - want).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(rel.max()) if rel.size else 0.0


def block_bars(model, edge_pose, edge_point, per_edge_bar, literal=False):
    """The derived bound of every entry of the reduced blocks: (m 2^-53 + per_edge_bar) sum |c|, where the c are the terms that are
    summed into the entry and m is their number.  A float64 sum of m terms in any order is off by at most m - 1 roundings of partial
    sums, none larger than the sum of the magnitudes, and each term is off by the per-edge bar relative to itself.
    The TERMS are the products W J_ri J_rj (W J_ri e_r), two per edge, one per row r of the residual: an edge's own two-term sum is
    no term a float64 route gets to within a relative bound.  Entry (2, 5) of a pose block shows it: the edge's sum is
    W X Y / Z^3 (fx^2 - fy^2), exactly 0 in the model for the pinhole's fx = fy, while ba_ref.linearize leaves 3e-14 there -- with
    the edge's sum taken as the term (literal=True) the float64 oracle itself misses the bound by an infinite ratio on a pose with
    one edge, and by 0.9 of it on the fisheye graph.
    -> {block: (bar, m)}, m shaped to broadcast against the block"""
    ep, el = np.asarray(edge_pose), np.asarray(edge_point)
    out = {}
    for key, index in (("H_pp", ep), ("b_p", ep), ("H_ll", el), ("b_l", el)):
        c = np.abs(model["c_" + key]) if literal else model["a_" + key]
        total = np.zeros(model[key].shape, LD)
        np.add.at(total, index, c)
        m = np.bincount(index, minlength=len(total)).reshape((-1,) + (1,) * (total.ndim - 1)) * (1 if literal else 2)
        out[key] = ((m * LD(2.0) ** -53 + LD(per_edge_bar)) * total, m)
    return out


# ----------------------------------------------------------------------------------------------------------------- the dense step
def dense_step(args, huber_delta, lam):
    """One damped step WITHOUT the Schur complement: the full (6 NF + 3 NL) system [H_pp + lam I, H_pl; H_pl^T, H_ll + lam I] x = b
    from ba_ref.linearize, solved by np.linalg.solve, and the update applied as VertexSE3 / Vertex3D::oplusImpl do.
    -> dict(pose_R, pose_t, points)"""
    from oracle import ba_ref
    cam, R, t, fixed, P, ep, el, z, w = args
    R = np.array(R, np.float64).reshape(-1, 3, 3)
    t = np.array(t, np.float64).reshape(-1, 3)
    P = np.array(P, np.float64).reshape(-1, 3)
    fixed = np.asarray(fixed, bool)
    ep, el = np.asarray(ep), np.asarray(el)
    free = np.flatnonzero(~fixed)
    slot = -np.ones(len(fixed), int)
    slot[free] = np.arange(len(free))
    nf, nl = len(free), len(P)
    lin = ba_ref.linearize(cam, R, t, fixed, P, ep, el, z, w, huber_delta)
    n = 6 * nf + 3 * nl
    H = np.zeros((n, n))
    b = np.zeros(n)
    for i, ip in enumerate(free):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = lin["H_pp"][ip]
        b[6 * i:6 * i + 6] = lin["b_p"][ip]
    for j in range(nl):
        o = 6 * nf + 3 * j
        H[o:o + 3, o:o + 3] = lin["H_ll"][j]
        b[o:o + 3] = lin["b_l"][j]
    for e in np.flatnonzero(slot[ep] >= 0):
        i, o = 6 * slot[ep[e]], 6 * nf + 3 * el[e]
        H[o:o + 3, i:i + 6] += lin["H_lp"][e]
        H[i:i + 6, o:o + 3] += lin["H_lp"][e].T
    H[np.arange(n), np.arange(n)] += lam
    x = np.linalg.solve(H, b)
    for i, ip in enumerate(free):
        dR, dt = ba_ref.se3_exp(x[6 * i:6 * i + 6])
        R[ip], t[ip] = dR @ R[ip], dR @ t[ip] + dt
    P = P + x[6 * nf:].reshape(-1, 3)
    return {"pose_R": R, "pose_t": t, "points": P}


def caller_has_extended_precision():
    """called by whoever compares against linearize_ld, at import: without a 64-bit mantissa the model is float64 compared with itself"""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no extended precision here: the longdouble model proves nothing"

