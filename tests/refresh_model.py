"""Plain numpy restatement of the refresh of a device-resident map-point table (include/orbm.h, "Map points refreshed on the
device"), written from the reference: MapPoint.cpp:43-76 (update), :83-91 (the ...Invariance getters), :103-152
(computeDescriptor), KeyFrame.cpp:233-242 (the counting loop of updateConnections), KeyFrame.cpp:159-179 (computeSceneMedianDepth),
LocalMapping.cpp:163 (the baseline), Pose.cpp:12-14 (camera centre).  `refresh` and `median_depth` run the header's evaluation
orders in float32 (the model the device is compared with) or in float64 (the yardstick the model is judged by); both start from the
poses ROUNDED TO FLOAT, as the reference holds them.  `make_scene` builds the seeded scenes both test files use.
No part of the library is used here."""
import numpy as np

from projection_model import KP_DTYPE, N_LEVELS, SCALE_FACTORS, _rodrigues

MAX_SCALE_FACTOR = SCALE_FACTORS[N_LEVELS - 1]
MAX_OBS = 1024
DONE, INVALID, NONE, LONG, DROPPED, ALL_BAD, REF_UNSEEN, REF_MISSING = range(8)


def camera_centres(pose_R, pose_t, D=np.float32):
    """O_w_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2), [n_kf][3]"""
    R = np.asarray(pose_R, np.float64).reshape(-1, 3, 3).astype(np.float32).astype(D)
    t = np.asarray(pose_t, np.float64).reshape(-1, 3).astype(np.float32).astype(D)
    return -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])


def hamming(rows):
    """[N][N] distances; as two products of the bit matrices (exact in float: no entry exceeds 256)"""
    bits = np.unpackbits(rows, axis=1).astype(np.float32)
    return (bits @ (1 - bits).T + (1 - bits) @ bits.T).astype(np.int32)


def medoid(rows):
    """MapPoint.cpp:124-146 on the [N][32] rows: the index of the row of least median distance, strict '<' from 256"""
    n = len(rows)
    med = np.sort(hamming(rows), axis=1)[:, (n - 1) // 2]
    best = int(np.argmin(med))                                          # the first of the least
    return best if med[best] < 256 else 0


def medoid_brute(rows):
    """the reference's loops, literally"""
    n = len(rows)
    dist = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            dist[i][j] = dist[j][i] = int(np.unpackbits(rows[i] ^ rows[j]).sum())
    best_median, best = 256, 0
    for i in range(n):
        median = sorted(dist[i])[(n - 1) // 2]
        if median < best_median:
            best_median, best = median, i
    return best


def refresh(sc, sel, cap_points, kf_self=-1, D=np.float32, max_scale_factor=MAX_SCALE_FACTOR):
    """sc: a scene of make_scene.  Returns dict(normals, min_dist, max_dist, desc: the table after the call -- float outputs in D --,
    result i32 [8], covis i32 [n_kf], touched: rows written, n: remaining observations per row (-1 = not looked at), amp: the
    largest sum_i |R_ik t_i| / |Pw - O_k| over a row's observations and its reference key frame)."""
    n_kf = len(sc["n"])
    O = camera_centres(sc["pose_R"], sc["pose_t"], D)
    T = (np.abs(np.asarray(sc["pose_R"]).reshape(-1, 3, 3)) * np.abs(np.asarray(sc["pose_t"]).reshape(-1, 3, 1))).sum(axis=1).max(axis=1)
    out = dict(normals=sc["normals"].astype(D), min_dist=sc["min_dist"].astype(D), max_dist=sc["max_dist"].astype(D), desc=sc["desc"].copy())
    result, covis = np.zeros(8, np.int32), np.zeros(n_kf, np.int32)
    touched, n_left, amp = np.zeros(len(sc["valid"]), bool), np.full(len(sc["valid"]), -1, np.int64), np.zeros(len(sc["valid"]))
    n_obs = len(sc["obs_kf"])
    for p in np.asarray(sel).tolist():
        if p < 0 or p >= cap_points:
            continue
        if not sc["valid"][p]:
            result[INVALID] += 1
            continue
        b, e = int(sc["obs_off"][p]), int(sc["obs_off"][p + 1])
        if b < 0 or e < b or e > n_obs:
            b = e = 0
        k, f = sc["obs_kf"][b:e].astype(np.int64), sc["obs_kp"][b:e].astype(np.int64)
        ok = (k >= 0) & (k < n_kf) & (f >= 0)
        ok[ok] &= f[ok] < sc["n"][k[ok]]
        result[DROPPED] += int((~ok).sum())
        k, f = k[ok], f[ok]
        n = len(k)
        n_left[p] = n
        np.add.at(covis, k[k != kf_self], 1)
        if n == 0:
            result[NONE] += 1
            continue
        if n > MAX_OBS:
            result[LONG] += 1
            continue
        rk = int(sc["ref_kf"][p])
        if rk < 0 or rk >= n_kf:
            result[REF_MISSING] += 1
            continue
        at = np.flatnonzero(k == rk)
        if len(at) == 0 and sc["n"][rk] < 1:
            result[REF_MISSING] += 1
            continue
        result[REF_UNSEEN] += len(at) == 0
        result[DONE] += 1
        touched[p] = True
        Pw = sc["points"][p].astype(D)
        v = Pw[None, :] - O[k]
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where((ln > 0)[:, None], v / ln[:, None], v)
        s = np.add.accumulate(np.concatenate([np.zeros((1, 3), D), d]), axis=0, dtype=D)[-1]   # ((0 + d_0) + d_1) + ...
        out["normals"][p] = s / D(n)
        vr = Pw - O[rk]
        dist = np.sqrt((vr[0] * vr[0] + vr[1] * vr[1]) + vr[2] * vr[2])
        span = dist * D(sc["kps"][rk]["size"][int(f[at[0]]) if len(at) else 0])
        out["max_dist"][p] = D(np.float32(1.2)) * span
        out["min_dist"][p] = D(np.float32(0.8)) * (span / D(max_scale_factor))
        with np.errstate(divide="ignore"):
            amp[p] = max(float((T[k] / ln.astype(np.float64)).max()), float(T[rk] / np.float64(dist)))
        good = sc["bad"][k] == 0
        if not good.any():
            result[ALL_BAD] += 1
            continue
        rows = np.stack([sc["kf_desc"][kk][ff] for kk, ff in zip(k[good].tolist(), f[good].tolist())])
        out["desc"][p] = rows[medoid(rows)]
    out.update(result=result, covis=covis, touched=touched, n=n_left, amp=amp)
    return out


def depth_keys(z):
    """order-preserving uint32 keys of float32 depths (-0 below +0)"""
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def median_depth(pose_R, pose_t, slots, n, stride, points, cap_points, cur=-1, D=np.float32):
    """(median [n_kf], count [n_kf], baseline [n_kf] or None)"""
    R = np.asarray(pose_R, np.float64).reshape(-1, 3, 3).astype(np.float32).astype(D)
    t = np.asarray(pose_t, np.float64).reshape(-1, 3).astype(np.float32).astype(D)
    n_kf = len(R)
    med, cnt = np.full(n_kf, np.nan, D), np.zeros(n_kf, np.int32)
    for k in range(n_kf):
        s = np.asarray(slots).reshape(n_kf, -1)[k, :min(max(int(n[k]), 0), stride)]
        s = s[(s >= 0) & (s < cap_points)]
        P = points[s].astype(D)
        z = ((R[k, 2, 0] * P[:, 0] + R[k, 2, 1] * P[:, 1]) + R[k, 2, 2] * P[:, 2]) + t[k, 2]
        cnt[k] = len(z)
        if len(z) == 0:
            continue
        if D is np.float32:
            key = np.sort(depth_keys(z))[len(z) // 2]
            u = np.uint32(key & 0x7fffffff) if key >> 31 else np.uint32(~key & 0xffffffff)
            med[k] = np.array([u], np.uint32).view(np.float32)[0]
        else:
            med[k] = np.sort(z)[len(z) // 2]
    base = None
    if cur >= 0:
        O = camera_centres(pose_R, pose_t, D)
        v = O[cur][None, :] - O
        base = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return med, cnt, base


# ---- seeded scenes -----------------------------------------------------------------------------------------------------------------
# raw list lengths; 64 | 65: one tile | tiles, 2 | 3: the shortcut; 1026 and 1027 lose two dropped observations: 1024 and 1025 remain
LENGTHS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1024, 1025, 1026, 1027)


def make_scene(seed, n_kf=12, feats=(50, 300), n_rows=400, lengths=LENGTHS, typical=(2, 15), spare_rows=16):
    """Key frames (poses, orbx_kp records, descriptors, bad flags), a point table of n_rows + spare_rows rows whose output fields
    are GARBAGE, CSR observations: the first rows take `lengths`, the rest draw from `typical`; then the rows the edge cases need."""
    rng = np.random.RandomState(seed)
    n = rng.randint(feats[0], feats[1] + 1, n_kf).astype(np.int32)
    pose_R = np.stack([_rodrigues(rng.uniform(-0.3, 0.3, 3) + 1e-3) for _ in range(n_kf)]).reshape(n_kf, 9)
    pose_t = rng.uniform(-2.0, 2.0, (n_kf, 3))
    bad = (rng.uniform(size=n_kf) < 0.25).astype(np.uint8)
    bad[0], bad[1] = 0, 1
    kps, kf_desc = [], []
    pool = rng.randint(0, 256, (24, 32)).astype(np.uint8)               # few distinct rows: ties in the medians
    for k in range(n_kf):
        kp = np.zeros(n[k], KP_DTYPE)
        kp["x"], kp["y"] = rng.uniform(0, 752, n[k]), rng.uniform(0, 480, n[k])
        kp["octave"] = rng.randint(0, N_LEVELS, n[k])
        kp["size"] = np.float32(31) * SCALE_FACTORS[kp["octave"]]
        kp["angle"], kp["response"], kp["class_id"] = rng.uniform(0, 360, n[k]), rng.uniform(20, 90, n[k]), -1
        kps.append(kp)
        d = rng.randint(0, 256, (n[k], 32)).astype(np.uint8)
        if k % 2:
            d = pool[rng.randint(0, len(pool), n[k])]
            flip = rng.uniform(size=n[k]) < 0.5
            d[flip, rng.randint(0, 32, flip.sum())] ^= np.uint8(1) << rng.randint(0, 8, flip.sum()).astype(np.uint8)
        kf_desc.append(np.ascontiguousarray(d))
    cap = n_rows + spare_rows
    points = (rng.uniform(-3, 3, (cap, 3)) + [0, 0, 8]).astype(np.float32)
    valid = (rng.uniform(size=cap) < 0.9).astype(np.uint8) * rng.randint(1, 200, cap).astype(np.uint8)
    valid[:len(lengths)] = 1
    counts = np.concatenate([lengths, rng.randint(typical[0], typical[1] + 1, cap - len(lengths))]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs_kf = rng.randint(0, n_kf, off[-1]).astype(np.int32)
    obs_kp = (rng.uniform(size=off[-1]) * n[obs_kf]).astype(np.int32)
    ref_kf = np.array([obs_kf[off[p] + rng.randint(counts[p])] if counts[p] else 0 for p in range(cap)], np.int32)
    e = len(lengths)                                                    # the edge rows, all valid
    valid[e:e + 8] = 1
    row = lambda p: slice(off[p], off[p + 1])  # noqa: E731
    bad_kfs = np.flatnonzero(bad)
    obs_kf[row(e)] = bad_kfs[rng.randint(0, len(bad_kfs), counts[e])]   # every observer bad: the descriptor stays
    obs_kp[row(e)] = 0
    ref_kf[e] = obs_kf[off[e]]
    obs_kf[row(e + 1)] = rng.randint(0, n_kf - 1, counts[e + 1])        # a reference key frame that is not observed: feature 0
    obs_kp[row(e + 1)] = 0
    ref_kf[e + 1] = n_kf - 1
    ref_kf[e + 2], ref_kf[e + 3] = -1, n_kf                             # no such key frame: untouched
    obs_kf[off[e + 4]], obs_kf[off[e + 4] + 1] = -1, n_kf               # observations that are dropped
    obs_kp[off[e + 5]], obs_kp[off[e + 5] + 1] = -1, n[obs_kf[off[e + 5] + 1]]
    obs_kf[row(e + 6)] = n_kf + 3                                       # all dropped: no usable observation
    k7 = obs_kf[off[e + 7]]                                             # the reference key frame twice: the first observation's feature
    obs_kf[off[e + 7] + 1], obs_kp[off[e + 7] + 1], ref_kf[e + 7] = k7, n[k7] - 1, k7
    for p in range(len(lengths)):                                       # dropped ones inside the long lists, across a chunk border
        if 65 <= counts[p] < 1024 or counts[p] > 1025:
            obs_kf[off[p] + 63], obs_kp[off[p] + 64] = n_kf, -5
    g = np.random.RandomState(seed + 1000)
    return dict(n=n, pose_R=pose_R, pose_t=pose_t, bad=bad, kps=kps, kf_desc=kf_desc, points=points, valid=valid,
                normals=g.uniform(-9, 9, (cap, 3)).astype(np.float32), min_dist=g.uniform(50, 60, cap).astype(np.float32),
                max_dist=g.uniform(70, 80, cap).astype(np.float32), desc=g.randint(0, 256, (cap, 32)).astype(np.uint8), obs_off=off,
                obs_kf=obs_kf, obs_kp=obs_kp, ref_kf=ref_kf, n_rows=n_rows, edge=e)


def make_selection(sc, seed, fraction=0.8):
    """rows of the scene in random order with -1s, rows past the table and duplicates mixed in; the special rows always"""
    rng = np.random.RandomState(seed)
    cap = sc["n_rows"]
    sel = np.flatnonzero(rng.uniform(size=cap) < fraction)
    sel = np.union1d(sel, np.arange(sc["edge"] + 8))
    sel = np.concatenate([sel, rng.randint(0, cap, 30), [-1] * 25, [cap, cap + 3, cap + 1000, -7, 2 ** 31 - 1, -2 ** 31]])
    return rng.permutation(sel).astype(np.int32)
