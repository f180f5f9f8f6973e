"""Plain numpy / Python restatement of include/orbm.h, "Local bundle adjustment on the device-resident map", twice:
  problem / apply                  the ARRAY form the header states (slot arrays, CSR, liveness), the model the device is compared with;
                                   float and double conversions as the header states them
  problem_objects / apply_objects  an independent OBJECT-style restatement of the reference: the three gathering loops and the edge
                                   loop of Optimize::localBundleAdjustment (Optimize.cpp:766-806, :860-889) with BA_local_for_kf /
                                   BA_fixed_for_kf marks on MapPoint / KeyFrame objects, and its tail (:914-950) with
                                   MapPoint::eraseObservation / setBad (observations_model's objects: a point's observations iterated in
                                   ascending key-frame slot, the header's order)
and the seeded scenes the test files use.  No part of the library is used here."""
import numpy as np

import observations_model as om
from projection_model import KP_DTYPE, N_LEVELS, SCALE_FACTORS

MAX_LOCAL = 1024
P_POSES, P_POINTS, P_EDGES, P_LOCAL, P_FIXED, P_REFUSED, P_LOCAL_DROPPED, P_LOCAL_BAD, P_NO_EDGE, P_SECOND, P_CSR_DROPPED = range(11)
A_ERASED, A_POINTS_BAD, A_CLEARED, A_MOVED, A_ROWS, A_CSR_DROPPED, A_MAP_DROPPED, A_POSES = range(8)
REFUSE_POSES, REFUSE_POINTS, REFUSE_EDGES, REFUSE_NO_FREE_POSE, REFUSE_NO_EDGE = 1, 2, 4, 8, 16
PROBLEM_OUT = ("pose_R", "pose_t", "pose_fixed", "ba_points", "edge_pose", "edge_point", "edge_z", "edge_inv_sigma2", "edge_kf", "edge_kp",
               "edge_off", "point_row", "pose_kf")


def _n_slots(sc, k):
    return min(max(int(sc["n"][k]), 0), sc["stride"])


def _state(sc, csr, slots=None):
    return dict(n=sc["n"], stride=sc["stride"], bad=sc["bad"], slots=sc["slots"] if slots is None else slots, obs_off=csr[0], obs_kf=csr[1],
                obs_kp=csr[2])


def _live_entries(st, p):
    """row p's live CSR entries (k, i) in CSR order"""
    out = []
    for j in om._list(st, p):
        k, i = int(st["obs_kf"][j]), int(st["obs_kp"][j])
        if om._entry_ok(st, k, i) and om._live(st, k, i, p):
            out.append((k, i))
    return out


def _csr_dropped(st):
    return sum(not om._entry_ok(st, int(k), int(i)) for k, i in zip(st["obs_kf"], st["obs_kp"]))


# ---- the array form -----------------------------------------------------------------------------------------------------------
def problem(sc, csr, cap_poses=1 << 20, cap_local_points=1 << 20, cap_edges=1 << 20):
    """sc: dict(n, bad, slots [n_kf, stride], stride, valid, points f32, cap_points, pose_R, pose_t f64 [n_kf, 9 / 3], kps (list of
    KP_DTYPE arrays), local, first_kf).  -> dict of the output arrays cut to the counts (None when refused) and result i32 [16]"""
    n_kf, cap, first_kf = len(sc["n"]), sc["cap_points"], sc["first_kf"]
    st = _state(sc, csr)
    result = np.zeros(16, np.int32)
    result[P_CSR_DROPPED] = _csr_dropped(st)
    local = []
    for pos, k in enumerate(int(x) for x in sc["local"]):
        if not 0 <= k < n_kf:
            result[P_LOCAL_DROPPED] += 1
        elif pos > 0 and sc["bad"][k]:
            result[P_LOCAL_BAD] += 1
        elif k in [int(x) for x in sc["local"][:pos]]:
            result[P_LOCAL_DROPPED] += 1
        else:
            local.append(k)
    seen, rows, edges = set(), [], []                                 # edges: (key frame, feature) per point
    for k in local:
        for i in range(_n_slots(sc, k)):
            p = int(sc["slots"][k, i])
            if p < 0 or p >= cap or not sc["valid"][p] or p in seen:
                continue
            seen.add(p)
            mine, have = [], set()
            for k2, i2 in _live_entries(st, p):
                if k2 in have:
                    result[P_SECOND] += 1
                    continue
                have.add(k2)
                mine.append((k2, i2))
            if not mine:
                result[P_NO_EDGE] += 1
                continue
            rows.append(p)
            edges.append(mine)
    fixed = sorted({k for mine in edges for k, _ in mine} - set(local))
    pose_kf = local + fixed
    pose_of = {k: q for q, k in enumerate(pose_kf)}
    n_edges = sum(len(m) for m in edges)
    result[[P_POSES, P_POINTS, P_EDGES, P_LOCAL, P_FIXED]] = len(pose_kf), len(rows), n_edges, len(local), len(fixed)
    free = len(local) - (first_kf in local)
    result[P_REFUSED] = (REFUSE_POSES * (len(pose_kf) > cap_poses) | REFUSE_POINTS * (len(rows) > cap_local_points)
                         | REFUSE_EDGES * (n_edges > cap_edges) | REFUSE_NO_FREE_POSE * (free < 1) | REFUSE_NO_EDGE * (n_edges < 1))
    out = dict(result=result)
    if result[P_REFUSED]:
        out.update({k: None for k in PROBLEM_OUT})
        return out
    flat = [(k, i, x) for x, mine in enumerate(edges) for k, i in mine]
    ekf, ekp = np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.int32)
    kp = [sc["kps"][k][i] for k, i, _ in flat]
    size = np.array([r["size"] for r in kp], np.float32)
    one = np.float32(1)
    out.update(
        pose_R=sc["pose_R"][pose_kf].astype(np.float32).astype(np.float64), pose_t=sc["pose_t"][pose_kf].astype(np.float32).astype(np.float64),
        pose_fixed=np.array([q >= len(local) or k == first_kf for q, k in enumerate(pose_kf)], np.uint8),
        ba_points=sc["points"][rows].astype(np.float64), edge_pose=np.array([pose_of[e[0]] for e in flat], np.int32),
        edge_point=np.array([e[2] for e in flat], np.int32),
        edge_z=np.array([[r["x"], r["y"]] for r in kp], np.float32).astype(np.float64).reshape(-1, 2),
        edge_inv_sigma2=((one / size) / size).astype(np.float64), edge_kf=ekf, edge_kp=ekp,
        edge_off=np.concatenate([[0], np.cumsum([len(m) for m in edges])]).astype(np.int32), point_row=np.array(rows, np.int32),
        pose_kf=np.array(pose_kf, np.int32))
    return out


def apply(sc, csr, prob, est_R, est_t, est_P, outlier):
    """prob: what `problem` returned; est_*: the optimiser's estimates f64; outlier u8 [n_edges].  -> dict(slots, valid, ref_kf, points,
    pose_R, pose_t, result) after the call, and `found_bad`: outlier edges that found their point bad (not part of d_result)"""
    n_kf, cap, stride = len(sc["n"]), sc["cap_points"], sc["stride"]
    slots, valid, ref_kf, points = sc["slots"].copy(), sc["valid"].copy(), sc["ref_kf"].copy(), sc["points"].copy()
    pose_R, pose_t = sc["pose_R"].copy(), sc["pose_t"].copy()
    st = _state(sc, csr, slots)
    result = np.zeros(8, np.int32)
    result[A_CSR_DROPPED] = _csr_dropped(st)
    n_local, n_edges = int(prob["result"][P_LOCAL]), len(prob["edge_kf"])
    found_bad = 0
    for x, p in enumerate(int(v) for v in prob["point_row"]):
        b, e = int(prob["edge_off"][x]), int(prob["edge_off"][x + 1])
        if p < 0 or p >= cap or b < 0 or e < b or e > n_edges:
            result[A_MAP_DROPPED] += 1
            continue
        for j in range(b, e):
            if not outlier[j]:
                continue
            if not valid[p]:
                found_bad += 1
                break
            k, i = int(prob["edge_kf"][j]), int(prob["edge_kp"][j])
            if not om._entry_ok(st, k, i):
                result[A_MAP_DROPPED] += 1
                continue
            if slots[k, i] != p or sc["bad"][k]:
                continue
            slots[k, i] = -1
            result[A_ERASED] += 1
            left = [(k2, i2) for k2, i2 in _live_entries(st, p) if k2 != k]
            if ref_kf[p] == k and left:
                ref_kf[p] = left[0][0]
                result[A_MOVED] += 1
            if len(left) <= 2:
                valid[p] = 0
                result[A_POINTS_BAD] += 1
                for k2, i2 in left:
                    if slots[k2, i2] == p:                               # an entry listed twice clears its slot once
                        slots[k2, i2] = -1
                        result[A_CLEARED] += 1
        if valid[p]:
            points[p] = est_P[x].astype(np.float32)
            result[A_ROWS] += 1
    for q in range(n_local):
        k = int(prob["pose_kf"][q])
        if not 0 <= k < n_kf:
            result[A_MAP_DROPPED] += 1
            continue
        pose_R[k] = est_R[q].reshape(9).astype(np.float32).astype(np.float64)
        pose_t[k] = est_t[q].astype(np.float32).astype(np.float64)
        result[A_POSES] += 1
    return dict(slots=slots, valid=valid, ref_kf=ref_kf, points=points, pose_R=pose_R, pose_t=pose_t, result=result, found_bad=found_bad)


# ---- the object form ----------------------------------------------------------------------------------------------------------
def _objects(sc):
    world = om._world(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], sc["ref_kf"])
    for kf in world["kfs"]:
        kf.ba_local = kf.ba_fixed = False
    for mp in world["mps"]:
        mp.ba_local = False
    return world


def problem_objects(sc):
    """Optimize.cpp:766-806 and :860-889 on objects; for scenes whose CSR is fresh.  -> (local key frames, fixed key frames in the
    order the reference meets them, local rows, per row the (key frame, feature) of its edges)"""
    world = _objects(sc)
    kfs, n_kf = world["kfs"], len(sc["n"])
    cur = kfs[int(sc["local"][0])]
    local = [cur]
    cur.ba_local = True
    for k in (int(x) for x in sc["local"][1:]):
        if not 0 <= k < n_kf or kfs[k].ba_local:                         # not a key frame; the covisibility graph holds a key frame once
            continue
        if not kfs[k].is_bad:
            kfs[k].ba_local = True                                       # (the reference also marks a bad one, which then has no edge)
            local.append(kfs[k])
    points = []
    for kf in local:
        for mp in kf.map_points:
            if mp is not None and not mp.is_bad and not mp.ba_local:
                mp.ba_local = True
                points.append(mp)
    fixed = []
    for mp in points:
        for k in sorted(mp.observations):
            kf = kfs[k]
            if not kf.is_bad and not kf.ba_local and not kf.ba_fixed:
                kf.ba_fixed = True
                fixed.append(kf)
    edges = [[(k, mp.observations[k][0]) for k in sorted(mp.observations) if not kfs[k].is_bad] for mp in points]
    return [kf.k for kf in local], [kf.k for kf in fixed], [mp.row for mp in points], edges


def apply_objects(sc, prob, est_R, est_t, est_P, outlier):
    """Optimize.cpp:914-950 on objects.  -> what `apply` returns (result without the counts of dropped entries)"""
    world = _objects(sc)
    kfs, mps, cap = world["kfs"], world["mps"], sc["cap_points"]
    result = np.zeros(8, np.int32)
    to_erase = [(int(prob["edge_kf"][j]), int(prob["point_row"][prob["edge_point"][j]])) for j in np.flatnonzero(outlier)]
    found_bad = 0
    for k, p in to_erase:
        mp = mps[p]
        if mp.is_bad:
            found_bad += 1
            continue
        i = mp.observations[k][0]                                        # getFeatureId
        kfs[k].map_points[i] = None                                      # eraseMapPoint
        mp.erase_observation(k, world)
        result[A_ERASED] += 1
    pose_R, pose_t, points = sc["pose_R"].copy(), sc["pose_t"].copy(), sc["points"].copy()
    for q in range(int(prob["result"][P_LOCAL])):
        k = int(prob["pose_kf"][q])
        pose_R[k], pose_t[k] = est_R[q].reshape(9).astype(np.float32), est_t[q].astype(np.float32)
        result[A_POSES] += 1
    for x, p in enumerate(int(v) for v in prob["point_row"]):
        if not mps[p].is_bad:
            points[p] = est_P[x].astype(np.float32)
            result[A_ROWS] += 1
    slots = sc["slots"].copy()
    for k, kf in enumerate(kfs):
        for i, mp in enumerate(kf.map_points):
            if mp is None and 0 <= slots[k, i] < cap:
                slots[k, i] = -1
    valid, ref_kf = sc["valid"].copy(), sc["ref_kf"].copy()
    valid[:cap][[mp.is_bad for mp in mps]] = 0
    ref_kf[:cap] = [mp.ref for mp in mps]
    result[A_POINTS_BAD], result[A_CLEARED], result[A_MOVED] = world["points_bad"], world["cleared"], world["reassigned"]
    # a bad found more than once: every later pair of the same point is counted by the reference's `continue`, the arrays stop at one
    return dict(slots=slots, valid=valid, ref_kf=ref_kf, points=points, pose_R=pose_R, pose_t=pose_t, result=result, found_bad=found_bad)


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------
PINHOLE = (460.0, 460.0, 376.0, 240.0)
FISHEYE = PINHOLE + (-0.02, 0.01, -0.004, 0.001)
SCENES = {
    "first_local": dict(seed=41, first_local=True),
    "first_fixed": dict(seed=42, first_local=False),
}


def _project(cam, Pc):
    """double: Pinhole.cpp:28-32 / Fisheye.cpp:35-49"""
    fx, fy, cx, cy = cam[:4]
    a, b = Pc[0] / Pc[2], Pc[1] / Pc[2]
    if len(cam) == 4:
        return fx * a + cx, fy * b + cy
    k = [float(np.float32(v)) for v in cam[4:]]
    r = np.sqrt(a * a + b * b)
    th = np.arctan(r)
    th_d = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
    return fx * th_d * a / r + cx, fy * th_d * b / r + cy


def make_scene(seed, first_local, cam=PINHOLE, n_kf=8, stride=96, cap_points=200, n_rows=160):
    """8 key frames of 96 slots around the origin looking down +z, 160 rows in front of them seen by two to four key frames each (about
    500 edges: six usable key frames of 92 slots hold no more); key
    points = the projection plus half a pixel, or plus tens of pixels for the engineered outliers.  The roles of the key frames are
    permuted by the seed: cur + three connected ones are local, one connected one is bad, two are fixed (one of them first_kf unless
    first_local), and one sees a few local rows only (a third fixed one).  `expect` names the engineered rows."""
    rng = np.random.RandomState(seed)
    role = [int(x) for x in rng.permutation(n_kf)]
    cur, conn, bad_kf, fix, far = role[0], role[1:4], role[4], role[5:7], role[7]
    first_kf = conn[1] if first_local else fix[0]
    local = [cur, conn[0], n_kf + 3, conn[1], bad_kf, conn[0], conn[2], -1]   # out of range, a bad one, a duplicate
    good = [cur] + conn + fix
    pose_R, pose_t = np.zeros((n_kf, 9)), np.zeros((n_kf, 3))
    for k in range(n_kf):
        w = rng.uniform(-0.05, 0.05, 3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        pose_R[k], pose_t[k] = R.reshape(9), rng.uniform(-0.4, 0.4, 3)
    pose_R, pose_t = pose_R.astype(np.float32).astype(np.float64), pose_t.astype(np.float32).astype(np.float64)
    truth = np.stack([rng.uniform(-3, 3, cap_points), rng.uniform(-2, 2, cap_points), rng.uniform(5, 10, cap_points)], 1)
    points = (truth + rng.normal(0, 0.02, truth.shape)).astype(np.float32)
    kps = []
    for k in range(n_kf):
        kp = np.zeros(stride, KP_DTYPE)
        kp["x"], kp["y"] = rng.uniform(0, 752, stride), rng.uniform(0, 480, stride)
        kp["octave"], kp["class_id"] = rng.randint(0, N_LEVELS, stride), -1
        kp["size"] = SCALE_FACTORS[kp["octave"]]
        kps.append(kp)
    free = [[int(x) for x in rng.permutation(stride - 4)] for _ in range(n_kf)]   # the last four slots stay out: behind d_n
    slots = np.full((n_kf, stride), -1, np.int32)
    ref_kf = np.zeros(cap_points + 4, np.int32)
    rows, expect = [0], {}

    def observe(p, k, off=None):
        i = free[k].pop()
        slots[k, i] = p
        Pc = pose_R[k].reshape(3, 3) @ truth[p] + pose_t[k]
        u, v = _project(cam, Pc)
        du, dv = rng.normal(0, 0.5, 2) if off is None else off
        kps[k]["x"][i], kps[k]["y"][i] = u + du, v + dv
        return i

    def point(observers, outliers=(), ref=None):
        p = rows[0]
        rows[0] += 1
        for k in observers:
            observe(p, k, (rng.choice([-1, 1]) * rng.uniform(40, 60), rng.choice([-1, 1]) * rng.uniform(40, 60)) if k in outliers else None)
        ref_kf[p] = observers[0] if ref is None else ref
        return p

    lo, hi = sorted(good)[0], sorted(good)[1]
    expect["ref_outlier"] = point(good[:5], outliers=[cur], ref=cur)          # its outlier edge names its reference key frame
    expect["falls_to_two"] = point([cur, conn[0], fix[0]], outliers=[conn[0]])
    expect["two_outliers"] = point([lo, hi, [k for k in good if k not in (lo, hi)][0]], outliers=[lo, hi])
    p = point([cur, conn[2], fix[1]])                                         # a row named by two slots of one key frame
    slots[conn[2], free[conn[2]].pop()] = p
    expect["twice"] = p
    invalid = [point([cur, conn[0]]), point([conn[1], fix[0]])]
    expect["only_bad"] = point([bad_kf])                                      # seen by the bad connected key frame alone: not local
    expect["far"] = point([far, fix[0]])                                      # seen by no local key frame
    while rows[0] < n_rows:
        roomy = [k for k in rng.permutation(good) if len(free[k]) > 8]
        ks = [int(k) for k in roomy[:rng.randint(2, 5)]]
        if not set(ks) & set([cur] + conn):
            ks.append(cur)
        if rng.uniform() < 0.15:
            ks.append(bad_kf)
        if rng.uniform() < 0.1:
            ks.append(far)
        point(ks, outliers=ks[:1] if rng.uniform() < 0.1 and len(ks) >= 4 else ())
    n = np.full(n_kf, stride - 4, np.int32)
    n[cur] = stride + 7                                                       # d_n > stride: clamped
    slots[:, stride - 4:] = rng.randint(0, rows[0], (n_kf, 4))                # behind d_n: ignored ...
    slots[cur, stride - 4:] = -1                                              # ... but not in cur
    valid = np.zeros(cap_points + 4, np.uint8)
    valid[:rows[0]] = rng.randint(1, 200, rows[0])
    valid[invalid] = 0
    valid[cap_points:] = 1
    bad = np.zeros(n_kf, np.uint8)
    bad[bad_kf] = 7
    sc = dict(n=n, bad=bad, slots=slots, stride=stride, valid=valid, points=points, cap_points=cap_points, pose_R=pose_R, pose_t=pose_t,
              kps=kps, local=np.array(local, np.int32), first_kf=first_kf, ref_kf=ref_kf, cam=cam, expect=expect, n_rows=rows[0],
              roles=dict(cur=cur, conn=conn, bad=bad_kf, fix=fix, far=far))
    return sc


def fresh_csr(sc):
    return om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30)[:3]


def stale_scene(sc, csr, seed=3):
    """The same scene after edits the CSR does not know: a local key frame's free slot names a valid row the CSR does not list there (no
    edge from it; a row named only so has no edge and is dropped), a listed slot emptied (a stale entry), plus unusable entries put
    into lists and broken offsets.  -> (scene, csr, unusable entries)"""
    rng = np.random.RandomState(seed)
    slots = sc["slots"].copy()
    cur = sc["roles"]["cur"]
    # a valid row without any observation, named now by a free slot of cur: a local point without an edge
    off, kf, kp = [np.asarray(a).copy() for a in csr]
    lists = om.lists_of(off, kf, kp)
    empty = [p for p in range(sc["n_rows"], sc["cap_points"]) if not lists[p]]
    free_slot = int(np.flatnonzero(slots[cur, :sc["stride"] - 4] == -1)[0])
    valid = sc["valid"].copy()
    valid[empty[0]] = 1
    slots[cur, free_slot] = empty[0]
    # stale: a listed observation whose slot now names nothing
    victim = next(p for p in range(10, sc["n_rows"]) if len(lists[p]) >= 4 and valid[p])
    k, i = lists[victim][1]
    slots[k, i] = -1
    junk, n_kf = 0, len(sc["n"])
    for p in rng.permutation(sc["n_rows"])[:30]:
        kind = rng.randint(3)
        entry = [(n_kf + int(rng.randint(0, 99)), 0), (-1 - int(rng.randint(0, 99)), 3), (int(rng.randint(0, n_kf)), sc["stride"] + int(rng.randint(0, 9)))][kind]
        lists[p].insert(int(rng.randint(0, len(lists[p]) + 1)), entry)
        junk += 1
    lengths = [len(v) for v in lists]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    flat = [e for v in lists for e in v]
    kf, kp = np.array([a for a, _ in flat], np.int32), np.array([b for _, b in flat], np.int32)
    off[empty[2]] = -5                                                     # rows without an observation: both lists stay empty
    return dict(sc, slots=slots, valid=valid, expect=dict(sc["expect"], no_edge=empty[0], stale=(victim, k, i))), (off, kf, kp), junk
